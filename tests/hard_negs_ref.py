"""float64 numpy restatement of the hard-negative contract (include/recguru_hip.h, rg_hard_negs) on top of tests/topk_ref.py: per
position the eligible pool members (not the position's label, not in its sequence's exclusion row), ordered by score descending and
id ascending; ranks skip .. skip + k - 1 go to columns 0 .. k - 1, and a slot the position has no id for, every column >= k and every
position with mask == 0 keep what the output held."""
import numpy as np

import topk_ref as R


def eligible(pool, labels, L, excl_rows=None, table_rows=None):
    """bool [n, C]: pool[c] may be returned for position t -- it is not labels[t], not in the exclusion row of sequence t // L and
    (table_rows given) inside the table.  excl_rows: one id list per sequence, or None."""
    pool = np.asarray(pool, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    el = pool[None, :] != labels[:, None]
    if table_rows is not None:
        el &= ((pool >= 0) & (pool < table_rows))[None, :]
    if excl_rows is not None:
        for t in range(len(labels)):
            el[t] &= ~np.isin(pool, np.asarray(excl_rows[t // L], dtype=np.int64))
    return el


def select(S, pool, el, mask, k, skip, out):
    """(out [n, ld] int64, scores [n, k] float64) after the call: S [n, C] float64 scores of every position against the pool rows, el
    from eligible(), out the buffer as it was before the call (a copy is returned).  scores: -inf wherever no id was written."""
    pool = np.asarray(pool, dtype=np.int64)
    mask = np.asarray(mask).reshape(-1)
    n = S.shape[0]
    out = np.array(out, dtype=np.int64, copy=True)
    sc = np.full((n, k), -np.inf, dtype=np.float64)
    pos, ps = R.topk(S, skip + k, 0, el)
    for t in range(n):
        if mask[t] == 0:
            continue
        for j in range(k):
            p = pos[t, skip + j]
            if p >= 0:
                out[t, j] = pool[p]
                sc[t, j] = ps[t, skip + j]
    return out, sc


def flat_excl(excl_rows, rng=None, gap=3):
    """(values int64, lo int64 [B], hi int64 [B]): the sequences' sorted unique rows laid out one after another in a shuffled order
    with `gap` foreign ids between them -- rows need not be contiguous or in sequence order, unlike a CSR."""
    B = len(excl_rows)
    order = np.arange(B) if rng is None else rng.permutation(B)
    vals, lo, hi = [], np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    at = 0
    for b in order:
        r = np.unique(np.asarray(excl_rows[b], dtype=np.int64))
        vals.append(np.full(gap, -7, dtype=np.int64))
        at += gap
        lo[b], hi[b] = at, at + len(r)
        vals.append(r)
        at += len(r)
    vals.append(np.full(gap, -7, dtype=np.int64))
    return np.concatenate(vals), lo, hi
