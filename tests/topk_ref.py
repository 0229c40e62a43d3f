"""float64 numpy restatement of the full-catalogue scoring contract (include/recguru_hip.h, rg_topk_scores): exact rank, top-K with
the tie rule and exclusion rows, and the derived error bound / rank interval the GPU tests hold the kernel to.  Inputs are rounded
exactly as the tier stores them: to bf16 for the bf16 tier, to f32 for the others."""
import numpy as np
import torch


def round_tier(x, tier):
    """x as the tier's buffers hold it, in float64."""
    t = torch.as_tensor(np.asarray(x, dtype=np.float32))
    if tier == "bf16":
        t = t.to(torch.bfloat16)
    return t.to(torch.float64).numpy()


def scores(h, w):
    """[B, C] float64 scores of already rounded h [B, d] and catalogue rows w [C, d]."""
    return np.asarray(h, np.float64) @ np.asarray(w, np.float64).T


def csr(rows):
    """list of id lists -> (values int64 sorted unique per row, offsets int64 [B + 1])."""
    rows = [np.unique(np.asarray(r, dtype=np.int64)) for r in rows]
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return (np.concatenate(rows) if len(rows) and off[-1] else np.zeros(0, np.int64)), off


def eligible(B, first_row, n_rows, excl_rows=None):
    """bool [B, n_rows]: catalogue id first_row + j is not in user b's exclusion row."""
    el = np.ones((B, n_rows), dtype=bool)
    if excl_rows is not None:
        for b, r in enumerate(excl_rows):
            r = np.asarray(r, dtype=np.int64) - first_row
            r = r[(r >= 0) & (r < n_rows)]
            el[b, r] = False
    return el


def rank(S, target, first_row, el):
    """number of ids i != target[b], not excluded, with S[b, i] > S[b, target[b]] (strictly); the target is never excluded."""
    B, C = S.shape
    out = np.zeros(B, dtype=np.int64)
    for b in range(B):
        t = int(target[b]) - first_row
        m = el[b].copy()
        m[t] = False
        out[b] = int((m & (S[b] > S[b, t])).sum())
    return out


def topk(S, k, first_row, el):
    """(ids [B, k] int64, scores [B, k] float64): the k eligible ids with the highest scores, score descending, ties by ascending
    id; fewer than k eligible: id -1 and score -inf in the trailing slots."""
    B, C = S.shape
    ids = np.full((B, k), -1, dtype=np.int64)
    sc = np.full((B, k), -np.inf, dtype=np.float64)
    for b in range(B):
        j = np.flatnonzero(el[b])
        order = j[np.lexsort((j, -S[b, j]))][:k]
        ids[b, :len(order)] = order + first_row
        sc[b, :len(order)] = S[b, order]
    return ids, sc


def pair_bound(h, w, x3):
    """[B, C] bound on |kernel score - float64 score| derived from the arithmetic, not measured:
         T = ((x3 ? 2^-15 : 0) + 2 d 2^-24) * sum_i |h_i| |w_i|
    first term: what split bf16 operands drop -- x = hi + lo + e with |e| <= 2^-17 |x| (lo's own rounding; hi + lo carries 16+ bits),
    the product hi.hi + hi.lo + lo.hi misses lo.lo (<= 2^-16 |h w|) and the two e terms (<= 2 * 2^-17 |h w|): together <= 2^-15 |h w|;
    second term: f32 accumulation of d products that are exact in f32 (bf16 x bf16), d additions of relative error 2^-24 each on
    partial sums bounded by sum |h_i w_i|, doubled for the matrix unit's internal grouping."""
    d = h.shape[1]
    return ((2.0 ** -15 if x3 else 0.0) + 2.0 * d * 2.0 ** -24) * (np.abs(h) @ np.abs(w).T)


def rank_interval(S, Tb, target, first_row, el):
    """(lo, hi) [B]: #{s > t + 2 T_b} <= rank <= #{s >= t - 2 T_b} over the eligible ids other than the target."""
    B, C = S.shape
    lo = np.zeros(B, dtype=np.int64)
    hi = np.zeros(B, dtype=np.int64)
    for b in range(B):
        t = int(target[b]) - first_row
        m = el[b].copy()
        m[t] = False
        lo[b] = int((m & (S[b] > S[b, t] + 2 * Tb[b])).sum())
        hi[b] = int((m & (S[b] >= S[b, t] - 2 * Tb[b])).sum())
    return lo, hi


def check_topk(ids, sc, S, Tb, k, first_row, el, max_near=5):
    """The random-fixture top-K checks of one call: ids [B, k], sc [B, k] from the kernel against float64 scores S and the per-user
    bound Tb.  Asserts first the condition on the inputs (at most max_near eligible ids within 2 T_b of the reference's k-th score)."""
    B, C = S.shape
    for b in range(B):
        j = np.flatnonzero(el[b])
        kk = min(k, len(j))
        ref = np.sort(S[b, j])[::-1]
        assert int((np.abs(S[b, j] - ref[kk - 1]) <= 2 * Tb[b]).sum()) <= max_near, "input condition: too many near-ties at the cut"
        got = ids[b, :kk] - first_row
        assert np.all(ids[b, kk:] == -1) and np.all(np.isneginf(sc[b, kk:]))
        assert len(set(got.tolist())) == kk and got.min() >= 0 and got.max() < C, "ids distinct and in range"
        assert el[b, got].all(), "an excluded id was returned"
        assert np.all(np.diff(sc[b, :kk]) <= 0), "scores not non-increasing"
        assert np.abs(sc[b, :kk] - S[b, got]).max() <= Tb[b], (b, np.abs(sc[b, :kk] - S[b, got]).max(), Tb[b])
        omitted = np.setdiff1d(j, got)
        if len(omitted):
            assert S[b, omitted].max() <= S[b, got].min() + 2 * Tb[b], "an omitted item outscores a returned one beyond the bound"


def metrics_of(r, k_val):
    """{str(k): (hit, ndcg, mrr)} of a rank vector, by the package's metrics."""
    from recguru_amd import metrics
    return {str(k): (metrics.hit_at_k_batch(r, k), metrics.NDCG_at_k_batch(r, k), metrics.mrr_at_k_batch(r, k)) for k in k_val}
