"""Host restatement of the device sampler (recguru_amd/csrc/sampler.hip) in numpy integer arithmetic: the counter-based draws,
the uniform draw over a user's allowed items, the alias draw with its rejection loop and fall-back, and batch assembly.  Written
from the contract and the kernel source, not from kernel output, so that the GPU tests can hold every drawn id to it by exact
integer equality (tests/test_sampler_gpu.py), as tests/dropmask.py does for the dropout masks.

The draw contract: draw i of a launch (i = row * n + column of the [B, n] output) is a function of (seed, i) only.
  * uniform: the 64-bit variate r = draw32(seed, 2i) << 32 | draw32(seed, 2i + 1) picks the u-th allowed item,
    u = mulhi64(r, V - m) + 1, m the size of the user's exclusion set;
  * alias: try tr = 0 .. 63 of draw i reads counters c = (64 i + tr) * 2 (the slot, from the high product with the slot count)
    and c + 1 (a 24-bit fraction compared with the f32 acceptance of the slot); the first candidate in 1..V that is not excluded
    wins, and after 64 rejections the uniform draw of index i under seed ^ 0xA5A5A5A5 decides.
All 64 bits of the seed reach the draw: both words are folded into two round keys (draw_key)."""
import numpy as np

import dropmask

U32, U64 = np.uint32, np.uint64
MASK32 = 0xFFFFFFFF
MASK64 = 0xFFFFFFFFFFFFFFFF
FALLBACK_XOR = 0xA5A5A5A5


def draw_key(seed):
    """draw_key (sampler.hip:54-62): k0 is make_drop's fold of the 64-bit seed (rg_common.hip.h:475-479, restated by
    dropmask.DropCfg), k1 a second multiplicative fold of the seed's high word and k0."""
    seed = int(seed) & MASK64
    k0 = dropmask.make_drop(0.0, seed).seed
    s = (((seed >> 32) * 0xC2B2AE3D) & MASK32) ^ ((k0 * 0x27D4EB2F + 0x9E3779B9) & MASK32)
    s ^= s >> 16
    s = (s * 0x85EBCA6B) & MASK32
    s ^= s >> 13
    return k0, s


def draw32(seed, ctr):
    """draw32 (sampler.hip:63-66) of a uint64 counter array: rg_hash(k1, rg_hash(k0, ctr_lo) ^ ctr_hi)."""
    k0, k1 = draw_key(seed)
    ctr = np.asarray(ctr, dtype=U64)
    lo, hi = (ctr & U64(MASK32)).astype(U32), (ctr >> U64(32)).astype(U32)
    return dropmask.rg_hash(k1, dropmask.rg_hash(k0, lo) ^ hi)


def variate64(seed, i, draw=draw32):
    """draw64 (sampler.hip:67-70): counters 2i (high word) and 2i + 1 (low word) of draw index i (uint64 array).  `draw` lets
    a test restate another draw32 under the same counter scheme."""
    i = np.asarray(i, dtype=U64)
    return (draw(seed, U64(2) * i).astype(U64) << U64(32)) | draw(seed, U64(2) * i + U64(1)).astype(U64)


def alias_variates(seed, i, tr, draw=draw32):
    """(h0, h1) of try tr of alias draw i: counters c = (64 i + tr) * 2 and c + 1 (sampler.hip:115-116)."""
    c = (np.asarray(i, dtype=U64) * U64(64) + U64(tr)) * U64(2)
    return draw(seed, c), draw(seed, c + U64(1))


def mulhi64(r, rng):
    """__umul64hi(r, rng): the high 64 bits of the 128-bit product, by 32-bit limbs in uint64 arithmetic."""
    r, g = np.asarray(r, dtype=U64), np.asarray(rng, dtype=U64)
    m, s = U64(MASK32), U64(32)
    a, b, c, d = r >> s, r & m, g >> s, g & m
    ad, bc = a * d, b * c
    mid = ((b * d) >> s) + (ad & m) + (bc & m)
    return a * c + (ad >> s) + (bc >> s) + (mid >> s)


def allowed_ids(excl, V):
    """The allowed items of a user in ascending order, from the definition: 1..V minus the exclusion set."""
    excl = np.asarray(excl, dtype=np.int64)
    return np.setdiff1d(np.arange(1, V + 1, dtype=np.int64), excl)


def nth_allowed(excl, V, u):
    """The u-th (1-based, int array) allowed item (what sampler.hip:72-80 finds by binary search over the sorted exclusions).
    Without exclusions the allowed items are 1..V themselves, which keeps V = 10**12 representable."""
    u = np.asarray(u, dtype=np.int64)
    if len(excl) == 0:
        assert u.min(initial=1) >= 1 and u.max(initial=1) <= V
        return u.copy()
    return allowed_ids(excl, V)[u - 1]


def _rows(excl, excl_off, users):
    """Per distinct user of the batch: (rows of the output that belong to it, its exclusion set)."""
    users = np.asarray(users, dtype=np.int64)
    for usr in np.unique(users):
        yield np.nonzero(users == usr)[0], np.asarray(excl[excl_off[usr]:excl_off[usr + 1]], dtype=np.int64)


def _uniform_rows(ex, rows, n, V, seed):
    i = (rows.astype(U64)[:, None] * U64(n) + np.arange(n, dtype=U64)[None, :])
    u = mulhi64(variate64(seed, i), V - len(ex)).astype(np.int64) + 1
    return i, nth_allowed(ex, V, u)


def uniform_negatives(excl, excl_off, users, n, V, seed):
    """sample_uniform_kernel (sampler.hip:82-97): [B, n] int64."""
    out = np.zeros((len(users), n), dtype=np.int64)
    for rows, ex in _rows(excl, excl_off, users):
        out[rows] = _uniform_rows(ex, rows, n, V, seed)[1]
    return out


def alias_negatives(prob, alias, excl, excl_off, users, n, V, seed, return_fallback=False):
    """sample_alias_kernel (sampler.hip:99-131): [B, n] int64 (and, on request, the bool map of the draws that fell back)."""
    prob, alias = np.asarray(prob, dtype=np.float32), np.asarray(alias, dtype=np.int64)
    slots = U64(len(prob))
    out = np.full((len(users), n), -1, dtype=np.int64)
    fell = np.zeros(out.shape, dtype=bool)
    for rows, ex in _rows(excl, excl_off, users):
        i, fb = _uniform_rows(ex, rows, n, V, (int(seed) & MASK64) ^ FALLBACK_XOR)
        ids = np.full(i.shape, -1, dtype=np.int64)
        for tr in range(64):
            todo = ids < 0
            if not todo.any():
                break
            h0, h1 = alias_variates(seed, i[todo], tr)
            slot = ((h0.astype(U64) * slots) >> U64(32)).astype(np.int64)                  # the high product
            f = (h1 >> U32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)           # 24 bits: exact in f32
            cand = np.where(f < prob[slot], slot, alias[slot])
            ok = (cand >= 1) & (cand <= V) & ~np.isin(cand, ex)
            ids[todo] = np.where(ok, cand, -1)
        out[rows] = np.where(ids < 0, fb, ids)
        fell[rows] = ids < 0
    return (out, fell) if return_fallback else out


def assemble(seqs, users, L_enc, L_dec, eos):
    """assemble_batch_kernel's contract (sampler.hip:16-47), from the host's seq_padding (synthetic.pad_sequences, pinned to the
    reference by tests/test_abi_and_host.py) and the reference's [-L_dec:] cut of the decoder rows (data_loader.py:25-36)."""
    from recguru_amd import synthetic
    enc, dec_in, dec_out = synthetic.pad_sequences([list(seqs[u]) for u in np.asarray(users).tolist()], L_enc, eos)
    return enc, dec_in[:, -L_dec:], dec_out[:, -L_dec:]
