"""Full-catalogue top-K and exact rank (rg_topk_scores, csrc/topk.hip) against the float64 restatement of tests/topk_ref.py:
an exact integer fixture (tails, slice boundaries, ties, merge), a random fixture under a derived error bound, the existing
candidate-list kernel on the same catalogue, bit invariance across repeats / batch splits in both libraries, the public
recommend / evaluation_full of both model families, and the refused shapes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import topk_ref as R
from parity_util import make_args

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TIERS = ["bf16", "bf16x3", "f32"]


def _set_tier(tier):
    from recguru_amd import ops
    ops.set_compute_dtype({"bf16": torch.bfloat16, "bf16x3": "bf16x3", "f32": torch.float32}[tier])
    return torch.bfloat16 if tier == "bf16" else torch.float32


def _dev(x, dtype=None):
    t = torch.as_tensor(x).cuda()
    return t.to(dtype) if dtype is not None else t


def _call(hip, h, table, k, first_row, n_rows, target=None, rows=None):
    ex = off = None
    if rows is not None:
        v, o = R.csr(rows)
        ex, off = _dev(v), _dev(o)
    ids, sc, rk = hip.topk_scores(h, table, k, first_row, n_rows, target=None if target is None else _dev(target), excl=ex, excl_off=off)
    f = lambda t: None if t is None else t.cpu().numpy()
    return f(ids), f(sc), f(rk)


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact fixture: small integers, every product and sum exact in every tier and in any order
# ---------------------------------------------------------------------------------------------------------------------
def _excl_rows(rng, B, first_row, n_rows, target):
    """random rows; row 0 empty, row 1 holds its own target, the last row also an id just past the catalogue"""
    rows = []
    for b in range(B):
        n = int(rng.integers(0, min(n_rows, 40) + 1))
        r = (first_row + rng.choice(n_rows, size=n, replace=False)).tolist()
        if b == 0:
            r = []
        if b == 1:
            r.append(int(target[b]))
        if b == B - 1 and B > 2:
            r.append(first_row + n_rows)
        rows.append(r)
    return rows


@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("tier", TIERS)
def test_exact_fixture(tier, d):
    from recguru_amd import hip
    dtype = _set_tier(tier)
    rng = np.random.default_rng(1000 + d)
    n = 0
    for B in (1, 5, 37):
        for n_rows in (1, 17, 257, 4099):
            for first_row in (0, 1):
                rows_total = first_row + n_rows + 1                      # one table row past the catalogue, too
                hn = rng.integers(-3, 4, size=(B, d)).astype(np.float32)
                wn = rng.integers(-3, 4, size=(rows_total, d)).astype(np.float32)
                S = R.scores(R.round_tier(hn, tier), R.round_tier(wn[first_row:first_row + n_rows], tier))
                h, table = _dev(hn, dtype), _dev(wn, dtype)
                target = first_row + rng.integers(0, n_rows, size=B)
                for rows in (None, _excl_rows(rng, B, first_row, n_rows, target)):
                    el = R.eligible(B, first_row, n_rows, rows)
                    rk_ref = R.rank(S, target, first_row, el)
                    for K in (1, 10, 128):
                        ids, sc, rk = _call(hip, h, table, K, first_row, n_rows, target, rows)
                        ids_ref, sc_ref = R.topk(S, K, first_row, el)
                        tag = "B=%d n_rows=%d first_row=%d K=%d excl=%s" % (B, n_rows, first_row, K, rows is not None)
                        np.testing.assert_array_equal(ids, ids_ref, err_msg=tag)
                        np.testing.assert_array_equal(sc.astype(np.float64), sc_ref, err_msg=tag)
                        np.testing.assert_array_equal(rk, rk_ref, err_msg=tag)
                        n += 1
                    _, _, rk0 = _call(hip, h, table, 0, first_row, n_rows, target, rows)        # rank only
                    np.testing.assert_array_equal(rk0, rk_ref)
    assert n == 3 * 4 * 2 * 2 * 3


# ---------------------------------------------------------------------------------------------------------------------
# 2. random fixture under the derived bound (topk_ref.pair_bound; nothing here is measured from the kernel)
# ---------------------------------------------------------------------------------------------------------------------
RANDOM_SHAPES = [(37, 4099, 128, 100), (5, 1001, 64, 10), (37, 4099, 256, 100), (16, 100003, 128, 100)]


def random_case(B, C, d, tier, seed=20240):
    """(h f32 [B, d], table f32 [C + 1, d] with the catalogue in rows 1 .. C, targets, exclusion rows, float64 scores, T_b)"""
    rng = np.random.default_rng(seed + B + C + d)
    hn = rng.normal(size=(B, d)).astype(np.float32)
    wn = (0.1 * rng.normal(size=(C + 1, d))).astype(np.float32)
    target = 1 + rng.integers(0, C, size=B)
    rows = [(1 + rng.choice(C, size=int(rng.integers(0, 60)), replace=False)).tolist() for _ in range(B)]
    hr, wr = R.round_tier(hn, tier), R.round_tier(wn[1:], tier)
    S = R.scores(hr, wr)
    Tb = R.pair_bound(hr, wr, tier != "bf16").max(axis=1)
    return hn, wn, target, rows, S, Tb


def check_rank(rk, S, Tb, target, first_row, el, C):
    lo, hi = R.rank_interval(S, Tb, target, first_row, el)
    assert (hi - lo).max() <= 0.005 * C, "input condition: a reference interval wider than 0.5 %% of C (%d)" % (hi - lo).max()
    assert np.all(lo <= rk) and np.all(rk <= hi), (lo, rk, hi)
    return lo, hi


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("B,C,d,K", RANDOM_SHAPES)
def test_random_fixture(B, C, d, K, tier):
    from recguru_amd import hip
    dtype = _set_tier(tier)
    hn, wn, target, rows, S, Tb = random_case(B, C, d, tier)
    h, table = _dev(hn, dtype), _dev(wn, dtype)
    for use_rows in (rows, None):
        el = R.eligible(B, 1, C, use_rows)
        ids, sc, rk = _call(hip, h, table, K, 1, C, target, use_rows)
        check_rank(rk, S, Tb, target, 1, el, C)
        R.check_topk(ids, sc.astype(np.float64), S, Tb, K, 1, el)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the candidate-list kernel over the whole catalogue lands in the same intervals (golden case1 model, f32 tier)
# ---------------------------------------------------------------------------------------------------------------------
def test_against_rank_scores_on_the_golden_model():
    from golden_util import load_case
    from parity_util import batches, build_cross
    from recguru_amd import hip, ops, training
    _set_tier("f32")
    z, ze = load_case("case1"), load_case("eval_case1")
    param, G, _ = build_cross(z)
    G.eval()
    bt = batches(z, "cuda")
    rng = np.random.default_rng(5)
    for dom in "ab":
        C = (param.vocab_size_a if dom == "a" else param.vocab_size_b) - 1
        target = ze["target.%s" % dom]
        h = training._last_rec_state(G, bt[dom][0], bt[dom][1], dom, param, "cuda")
        table = ops.shadow(G.item_table(dom))
        B = h.shape[0]
        cand = np.stack([rng.permutation(np.setdiff1d(np.arange(1, C + 1), [t])) for t in target])
        hr, wr = R.round_tier(h.cpu().numpy(), "f32"), R.round_tier(table[1:C + 1].cpu().numpy(), "f32")
        S = R.scores(hr, wr)
        Tb = R.pair_bound(hr, wr, True).max(axis=1)
        el = R.eligible(B, 1, C)
        _, rk_old = hip.rank_scores(h, table, _dev(target), _dev(cand), want_scores=False)
        _, _, rk_new = _call(hip, h, table, 0, 1, C, target)
        check_rank(rk_old.cpu().numpy(), S, Tb, target, 1, el, C)
        check_rank(rk_new, S, Tb, target, 1, el, C)


# ---------------------------------------------------------------------------------------------------------------------
# 4. bit invariance across repeats and batch splits, in both libraries (fresh child processes: tests/topk_worker.py)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [False, True])
def test_repeat_and_batch_split_invariance(det, tmp_path):
    out = str(tmp_path / "inv.npz")
    env = dict(os.environ, PYTHONPATH=os.path.dirname(HERE))
    env.pop("RG_DETERMINISTIC", None)
    if det:
        env["RG_DETERMINISTIC"] = "1"
    r = subprocess.run([sys.executable, os.path.join(HERE, "topk_worker.py"), out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-4000:]
    z = np.load(out)
    assert (int(z["det_enabled"]) > 0) == det
    for tier in TIERS:
        for name in ("ids", "scores", "rank"):
            one = z["%s.one.%s" % (tier, name)]
            assert one.shape[0] == 37
            np.testing.assert_array_equal(one.view(np.uint8), z["%s.again.%s" % (tier, name)].view(np.uint8), err_msg="%s repeat %s" % (tier, name))
            np.testing.assert_array_equal(one.view(np.uint8), z["%s.split.%s" % (tier, name)].view(np.uint8), err_msg="%s split %s" % (tier, name))


# ---------------------------------------------------------------------------------------------------------------------
# 5. the public interface, both model families
# ---------------------------------------------------------------------------------------------------------------------
def _eval_loader(dom, B):
    """evaluation_2's loader protocol from a two-batch TensorLoader: (validation data, test data, sampled candidates x 2)"""
    from recguru_amd.synthetic import TensorLoader
    out = []
    for (enc_in, dec_in, _), n_items, val, test in TensorLoader(dom, B, "cuda"):
        out.append(((enc_in, dec_in, val), (enc_in, dec_in, test), n_items, n_items))
    assert len(out) == 2
    return out


def _metric_rows(res, k_val, tag):
    return np.array([[res[str(k)][n + "_" + tag][0] for n in ("ht", "ndcg", "mrr")] for k in k_val])


@pytest.mark.parametrize("family", ["cross", "single"])
def test_recommend_and_evaluation_full(family):
    from recguru_amd import auto_training, ops, synthetic, training
    from recguru_amd.config import get_param
    from recguru_amd.models import MyAuto4Rec_c, MyRec
    _set_tier("f32")
    d, H, L, N, V, B, K = 128, 4, 50, 1, 300, 5, 20
    torch.manual_seed(11)
    param = get_param(make_args(d, H, 3, L, V, V, N, B), make_dirs=False)
    if family == "cross":
        M = MyAuto4Rec_c("cuda", param).to(torch.float32).cuda().eval()
        state = lambda e, di: training._last_rec_state(M, e, di, "a", param, "cuda")
        table = lambda: ops.shadow(M.item_table("a"))
        rec = lambda e, di, **kw: training.recommend(M, e, di, K, param, domain="a", device="cuda", **kw)
        evaluate = lambda ld, kv: training.evaluation_full(M, ld, "cuda", param, k_val=kv, domain="a")
    else:
        M = MyRec("cuda", param, None, dec_rec=False, fix_enc=False, sas=False, pos_train=False).to(torch.float32).cuda().eval()

        def state(e, di):
            with torch.no_grad():
                return M.get_embedding(e, di)[:, -1, :].contiguous()
        table = lambda: ops.shadow(M.AutoEnc.src_emb.weight)
        rec = lambda e, di, **kw: auto_training.recommend(M, e, di, K, param, **kw)
        evaluate = lambda ld, kv: auto_training.evaluation_full(M, ld, "cuda", param, k_val=kv)
    dom = synthetic.make_domain(2 * B, V, L, 3, seed=9)
    loader = _eval_loader(dom, B)
    param.eval_steps = 2
    wr = R.round_tier(table()[1:V + 1].cpu().numpy(), "f32")
    lo_all, hi_all = {"eval": [], "test": []}, {"eval": [], "test": []}
    for eval_data, test_data, _, _ in loader:
        enc_in, dec_in = eval_data[0], eval_data[1]
        hr = R.round_tier(state(enc_in, dec_in).cpu().numpy(), "f32")
        S = R.scores(hr, wr)
        Tb = R.pair_bound(hr, wr, True).max(axis=1)
        own = [sorted(set(int(x) for x in row if 0 < x <= V)) for row in enc_in.cpu().numpy()]
        for exclude_seen, rows in ((True, own), (False, None)):
            ids, sc = rec(enc_in, dec_in, exclude_seen=exclude_seen)
            ids, sc = ids.cpu().numpy(), sc.cpu().numpy().astype(np.float64)
            assert ids.shape == (B, K) and ids.min() >= 1 and ids.max() <= V
            if exclude_seen:
                assert all(not set(ids[b].tolist()) & set(own[b]) for b in range(B)), "a seen item was recommended"
            R.check_topk(ids, sc, S, Tb, K, 1, R.eligible(B, 1, V, rows))
        for tag, data in (("eval", eval_data), ("test", test_data)):
            lo, hi = check_rank_interval_only(S, Tb, data[2].cpu().numpy(), V)
            lo_all[tag].append(lo)
            hi_all[tag].append(hi)
    k_val = [1, 5, 10, 30]
    res = evaluate(loader, k_val)
    assert sorted(res) == sorted(str(k) for k in k_val)
    for tag in ("eval", "test"):
        lo, hi = np.concatenate(lo_all[tag]), np.concatenate(hi_all[tag])
        got = _metric_rows(res, k_val, tag)
        best = np.array([R.metrics_of(lo, k_val)[str(k)] for k in k_val])       # lower ranks: higher metrics
        worst = np.array([R.metrics_of(hi, k_val)[str(k)] for k in k_val])
        if np.array_equal(lo, hi):
            np.testing.assert_allclose(got, best, rtol=1e-12, atol=1e-15)
        assert np.all(got <= best + 1e-12) and np.all(got >= worst - 1e-12), (got, best, worst)
    with pytest.raises(NotImplementedError):
        rec(loader[0][0][0], loader[0][0][1], sas=True)


def check_rank_interval_only(S, Tb, target, C):
    """the helper's rank intervals of one batch (evaluation_full excludes nothing); where an interval is not degenerate the metrics
    are held between those of its ends"""
    return R.rank_interval(S, Tb, target, 1, R.eligible(S.shape[0], 1, C))


# ---------------------------------------------------------------------------------------------------------------------
# 6. refused shapes: the package's error with the ABI's message, nothing launched
# ---------------------------------------------------------------------------------------------------------------------
def test_unsupported_shapes_raise():
    from recguru_amd import hip
    h = torch.zeros(4, 128, device="cuda", dtype=torch.bfloat16)
    table = torch.zeros(50, 128, device="cuda", dtype=torch.bfloat16)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match=r"rg_topk_scores failed \(-2\): topk_scores: K must be in \[0, 128\]"):
        hip.topk_scores(h, table, 129, 1, 49)
    h96 = torch.zeros(4, 96, device="cuda", dtype=torch.bfloat16)
    t96 = torch.zeros(50, 96, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match=r"rg_topk_scores failed \(-2\): topk_scores: d must be 64, 128 or 256"):
        hip.topk_scores(h96, t96, 10, 1, 49)
    for bad in (0, 50, -3):
        target = torch.tensor([1, 2, bad, 3], device="cuda")
        with pytest.raises(RuntimeError, match=r"rg_topk_scores failed \(-2\): topk_scores: target\[2\] = %d is outside the catalogue rows \[1, 50\)" % bad):
            hip.topk_scores(h, table, 10, 1, 49, target=target)
    # the refusals launched nothing: the stream is clean and a supported call still answers
    torch.cuda.synchronize()
    ids, sc, rk = hip.topk_scores(h, table, 3, 1, 49, target=torch.tensor([1, 2, 49, 3], device="cuda"))
    assert ids.cpu().tolist() == [[1, 2, 3]] * 4 and rk.cpu().tolist() == [0] * 4 and float(sc.abs().max()) == 0.0
