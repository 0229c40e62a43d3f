"""Helpers of tests/test_logq_gpu.py, and its child process: `logq_worker.py zeros|masked OUT.npz` runs every form of the
per-position item loss the loaded library offers (under RG_DETERMINISTIC=1: forward, atomic backward, training form) twice -- a
baseline and a variant that must not differ from it by a bit -- and saves both sets of outputs.
  zeros   baseline: no biases; variant: all-zero neg_bias and pos_bias
  masked  baseline: clean biases; variant: NaN in pos_bias at the masked positions and in neg_bias at the rows that only masked
          positions' negatives name (ids inside the table everywhere)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

B, L, ROWS = 3, 7, 211
# (d, k): one, two and four register batches (per = 32 / 16 / 8 rows at d = 64 / 128 / 256), exact fills, ragged tails, and the
# online form with a partial 64-row block and with several
SHAPES = [(128, 5), (128, 15), (128, 30), (128, 63), (128, 64), (128, 200), (64, 31), (64, 127), (64, 128), (256, 7), (256, 31), (256, 32)]
CHILD_SHAPES = [(128, 30), (128, 64), (64, 31), (64, 128), (256, 7), (256, 32)]


def problem(d, k, seed, n=B * L, rows=ROWS, reserve=0):
    """h [n, d], table [rows, d], labels, negatives, biases in [-3, 12] (numpy f32 / int64) and a mask.  n = 21: three sequences of
    seven, the middle one wholly masked and five more positions masked in the other two; larger n: one position in five masked.
    reserve > 0: the last `reserve` rows of the table are named by masked positions only (labels and negatives)."""
    rng = np.random.RandomState(seed)
    mask = np.ones(n, dtype=np.float32)
    if n == B * L:
        mask[L:2 * L] = 0
        other = np.concatenate([np.arange(L), np.arange(2 * L, 3 * L)])
        mask[rng.choice(other, 5, replace=False)] = 0
    else:
        mask[rng.rand(n) < 0.2] = 0
    hi = rows - reserve
    h = (0.5 * rng.randn(n, d)).astype(np.float32)
    table = (0.3 * rng.randn(rows, d)).astype(np.float32)
    pos = rng.randint(1, hi, size=n).astype(np.int64)
    neg = rng.randint(1, hi, size=(n, k)).astype(np.int64)
    if reserve:
        dead = mask == 0
        pos[dead] = rng.randint(hi, rows, size=int(dead.sum()))
        neg[dead] = rng.randint(hi, rows, size=(int(dead.sum()), k))
    nb = rng.uniform(-3, 12, size=rows).astype(np.float32)
    pb = rng.uniform(-3, 12, size=n).astype(np.float32)
    return dict(h=h, table=table, pos=pos, neg=neg, mask=mask, nb=nb, pb=pb, d=d, k=k)


def dev(x, dtype=None):
    if x is None:
        return None
    t = torch.as_tensor(x).cuda()
    return t.to(dtype) if dtype is not None else t


def run_forms(p, nb, pb, dtype=torch.float32):
    """Every kernel form at `hip` level -> {name: tensor}: fwd (loss sums, lse), bwd (dh, dE by atomics), binned (dh, dE; not in the
    deterministic library), train (+ scatter where the binned kernels exist): coef, dh, sums, lse, dE."""
    from recguru_amd import hip
    d, k = p["d"], p["k"]
    h, table = dev(p["h"], dtype), dev(p["table"], dtype)
    pos, neg, mask = dev(p["pos"]), dev(p["neg"]), dev(p["mask"])
    nb, pb = dev(nb), dev(pb)
    n, rows = h.shape[0], table.shape[0]
    kw = dict(neg_bias=nb, pos_bias=pb)
    gout = torch.ones(1, device="cuda")
    out = {}
    sums, lse = hip.item_loss_fwd(h, table, pos, neg, mask, k, hip.LOSS_SAMPLED_CE, **kw)
    out["fwd.sums"], out["fwd.lse"] = sums.clone(), lse.clone()
    dE = torch.zeros(rows, d, device="cuda")
    out["bwd.dh"] = hip.item_loss_bwd(h, table, pos, neg, mask, k, hip.LOSS_SAMPLED_CE, lse, sums, gout, dE, -1, **kw)
    out["bwd.dE"] = dE
    binned = bool(hip.item_loss_bwd_binned_supported(n, k, d, rows))
    if binned:
        dE = torch.zeros(rows, d, device="cuda")
        out["binned.dh"] = hip.item_loss_bwd_binned(h, table, pos, neg, mask, k, hip.LOSS_SAMPLED_CE, lse, sums, gout, dE, -1, **kw)
        out["binned.dE"] = dE
    form = hip.item_loss_train_supported(k, d)
    assert form in (1, 2)
    s2 = torch.zeros(2, device="cuda")
    s2[1] = mask.sum()
    lse2 = torch.zeros(n, device="cuda") if form == 2 else None
    coef, dh = hip.item_loss_train(h, table, pos, neg, mask, k, hip.LOSS_SAMPLED_CE, s2, lse=lse2, **kw)
    out["train.coef"], out["train.dh"], out["train.sums"] = coef.view(n, k + 1)[mask != 0], dh, s2
    if form == 2:
        out["train.lse"] = lse2
    if binned:
        dE = torch.zeros(rows, d, device="cuda")
        hip.item_loss_scatter_binned(h, rows, pos, neg, mask, k, coef, gout, dE, -1, lse=lse2, sums=s2 if form == 2 else None)
        out["train.dE"] = dE
    torch.cuda.synchronize()
    return {key: v.float().cpu().numpy() for key, v in out.items()}


def variant_of(p, what):
    """(baseline biases, variant biases) of a child-process mode."""
    if what == "zeros":
        return (None, None), (np.zeros_like(p["nb"]), np.zeros_like(p["pb"]))
    assert what == "masked"
    nb, pb = p["nb"].copy(), p["pb"].copy()
    dead = p["mask"] == 0
    pb[dead] = np.nan
    only_dead = np.ones(len(nb), dtype=bool)
    only_dead[p["neg"][~dead].reshape(-1)] = False
    only_dead[0] = False
    named = np.zeros(len(nb), dtype=bool)
    named[p["neg"][dead].reshape(-1)] = True
    nb[only_dead & named] = np.nan
    assert np.isnan(nb).sum() > 0 and np.isnan(pb).sum() == int(dead.sum())
    return (p["nb"], p["pb"]), (nb, pb)


def pairs(what, shapes):
    """{"<d>.<k>.<a|b>.<form output>": array}: a = baseline, b = variant."""
    res = {}
    for d, k in shapes:
        p = problem(d, k, seed=1000 + d + k, reserve=40 if what == "masked" else 0)
        base, var = variant_of(p, what)
        for tag, (nb, pb) in (("a", base), ("b", var)):
            for key, v in run_forms(p, nb, pb).items():
                res["%d.%d.%s.%s" % (d, k, tag, key)] = v
    return res


if __name__ == "__main__":
    from recguru_amd import hip
    assert hip.DETERMINISTIC and os.path.basename(hip.LIB_PATH) == "librecguru_hip_det.so", "the child compares bits: deterministic library only"
    np.savez(sys.argv[2], **pairs(sys.argv[1], CHILD_SHAPES))
