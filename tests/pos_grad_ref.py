"""Float64 numpy restatement of the rg_pos_grad contract (include/recguru_hip.h), written from the contract, not from kernel output:

    dP[l, e] += sum_b dx[b, l, e] * mask[b*L + l] * keep(seed, drop_p, idx),   idx = (unsigned)(b*L + l) * (unsigned)d + e   for l < L

with keep = 0 or the f32 1/(1-p) of tests/dropmask.py (the mask of the forward embedding stage: dropmask.rowmajor_index with
row = token b*L + l).  A position with mask == 0 contributes nothing whatever its dx row holds (NaN included)."""
import numpy as np

import dropmask


def keep_array(seed, p, B, L, d):
    """[B, L, d] float64 multipliers of the embedding stage's dropout (all ones for p == 0)."""
    if not p:
        return np.ones((B, L, d), dtype=np.float64)
    return dropmask.rowmajor_mask(seed, p, B * L, d).reshape(B, L, d)


def terms(dx, mask, p=0.0, seed=0):
    """[B, L, d] float64 summands dx * mask * keep, exactly zero where mask == 0."""
    dx = np.asarray(dx, dtype=np.float64)
    B, L, d = dx.shape
    m = np.asarray(mask, dtype=np.float64).reshape(B, L, 1)
    live = np.broadcast_to(m != 0, dx.shape)
    return np.where(live, np.where(live, dx, 0.0) * m * keep_array(seed, p, B, L, d), 0.0)


def pos_grad(dx, mask, dP, p=0.0, seed=0):
    """The contract: returns (dP after the call, sum_b |term_b|) in float64; rows >= L of dP unchanged."""
    t = terms(dx, mask, p, seed)
    out = np.array(dP, dtype=np.float64, copy=True)
    L = t.shape[1]
    out[:L] += t.sum(axis=0)
    return out, np.abs(t).sum(axis=0)


def bound(B, prior, abs_sum):
    """Element-wise rounding bound of the two-launch kernel on f32: a chain of at most B + 1 f32 additions (slice sums, slices, the
    add onto dP) plus the roundings of the products dx * mask * inv_keep: (B + 3) * 2^-24 * (|prior| + sum_b |term_b|)."""
    return (B + 3) * 2.0 ** -24 * (np.abs(np.asarray(prior, dtype=np.float64)) + abs_sum)
