"""Wide top-K (rg_topk_wide, csrc/topk_wide.hip; 1 <= K <= 1024): the exact integer fixture of test_topk_gpu.py at K = 129, 300 and 1024,
the all-ties worst case of the radix select, bit equality with the shipped kernels (K <= 128 directly, K > 128 through a chain of
K = 128 calls that exclude what they returned), the derived bound of topk_ref.check_topk, repeats / batch splits / both libraries,
the refusals, and recommend(k > 128) of both model families.  The fault word of the workspace is read after every call."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import topk_ref as R
from parity_util import make_args
from test_topk_gpu import TIERS, _dev, _excl_rows, _set_tier, random_case
from test_topk_list_gpu import make_list

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RANDOM_CASES = [(37, 4099, 128), (5, 1001, 64), (37, 4099, 256)]
BIG_CASE = (16, 100003, 128)


# ---------------------------------------------------------------------------------------------------------------------
# helpers (chain_topk is held to topk_ref.topk by tests/test_topk_wide_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------
def chain_topk(call, B, k, chunk, excl_rows=None):
    """The k best as ceil(k / chunk) calls of `chunk`: call(excl_rows) -> (ids [B, chunk], scores [B, chunk]); every call's ids join
    the users' exclusion rows of the next one.  Top-K under a total order: the concatenation is the top-k."""
    rows = [list(r) for r in excl_rows] if excl_rows is not None else [[] for _ in range(B)]
    ids_all, sc_all = [], []
    for _ in range((k + chunk - 1) // chunk):
        ids, sc = call(rows)
        ids_all.append(ids)
        sc_all.append(sc)
        rows = [rows[b] + [int(x) for x in ids[b] if x >= 0] for b in range(B)]
    return np.concatenate(ids_all, axis=1)[:, :k], np.concatenate(sc_all, axis=1)[:, :k]


@functools.lru_cache(maxsize=None)
def _case(B, C, d, tier):
    """test_topk_gpu.random_case, computed once per (shape, tier) and shared: nothing below writes to it"""
    return random_case(B, C, d, tier)


def _csr(excl_rows):
    if excl_rows is None:
        return None, None
    v, o = R.csr(excl_rows)
    return _dev(v), _dev(o)


def _wide(hip, h, table, k, first_row=None, n_rows=None, rows=None, excl_rows=None):
    ex, off = _csr(excl_rows)
    ids, sc = hip.topk_wide(h, table, k, first_row, n_rows, rows=None if rows is None else _dev(rows), excl=ex, excl_off=off)
    fault, levels, kept = hip.topk_wide_state(h.device, h.shape[0])
    assert fault == 0, "fault word %d" % fault
    assert int(levels.min()) >= 1 and int(levels.max()) <= 7 and int(kept.max()) <= 2048
    assert ids.shape == (h.shape[0], k) and ids.dtype == torch.int64 and sc.dtype == torch.float32
    return ids.cpu().numpy(), sc.cpu().numpy()


def _narrow(hip, h, table, k, first_row=None, n_rows=None, rows=None, excl_rows=None):
    ex, off = _csr(excl_rows)
    if rows is None:
        ids, sc, _ = hip.topk_scores(h, table, k, first_row, n_rows, excl=ex, excl_off=off)
    else:
        ids, sc, _ = hip.topk_list(h, table, k, _dev(rows), excl=ex, excl_off=off)
    return ids.cpu().numpy(), sc.cpu().numpy()


def _same(got, want, tag):
    for name, g, w in zip(("ids", "scores"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), "%s: %s differ" % (tag, name)


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact fixture: small integers, every product and sum exact in every tier and in any order; ties everywhere
# ---------------------------------------------------------------------------------------------------------------------
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
                rows_total = first_row + n_rows + 1
                hn = rng.integers(-3, 4, size=(B, d)).astype(np.float32)
                wn = rng.integers(-3, 4, size=(rows_total, d)).astype(np.float32)
                S = R.scores(R.round_tier(hn, tier), R.round_tier(wn[first_row:first_row + n_rows], tier))
                h, table = _dev(hn, dtype), _dev(wn, dtype)
                target = first_row + rng.integers(0, n_rows, size=B)
                for rows in (None, _excl_rows(rng, B, first_row, n_rows, target)):
                    el = R.eligible(B, first_row, n_rows, rows)
                    for K in (129, 300, 1024):
                        ids, sc = _wide(hip, h, table, K, first_row, n_rows, excl_rows=rows)
                        ids_ref, sc_ref = R.topk(S, K, first_row, el)
                        tag = "B=%d n_rows=%d first_row=%d K=%d excl=%s" % (B, n_rows, first_row, K, rows is not None)
                        np.testing.assert_array_equal(ids, ids_ref, err_msg=tag)
                        np.testing.assert_array_equal(sc.astype(np.float64), sc_ref, err_msg=tag)
                        n += 1
    assert n == 3 * 4 * 2 * 2 * 3


# ---------------------------------------------------------------------------------------------------------------------
# 2. the select's worst case: every key ties in its score, the radix refines into the row bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("n,d", [(600, 128), (5000, 64)])          # 5000 > the collect buffer: the row bits decide, seven levels
def test_all_ties(n, d, tier):
    from recguru_amd import hip
    dtype = _set_tier(tier)
    rng = np.random.default_rng(77 + n)
    B = 5
    hn = rng.normal(size=(B, d)).astype(np.float32)
    same = np.repeat(rng.normal(size=(1, d)).astype(np.float32), n + 1, axis=0)
    excl = [sorted(set((1 + rng.choice(n, size=int(rng.integers(0, 50)), replace=False)).tolist() + [n + 1, n + 9])) for _ in range(B)]
    excl[0] = []
    excl[1] = list(range(1, 301))                                    # the 300 lowest ids: the answer starts at 301
    for wn in (np.zeros((n + 1, d), dtype=np.float32), same):
        h, table = _dev(hn, dtype), _dev(wn, dtype)
        for K in (300, 600, 1024):
            for use in (excl, None):
                ids, sc = _wide(hip, h, table, K, 1, n, excl_rows=use)
                for b in range(B):
                    want = np.setdiff1d(np.arange(1, n + 1), use[b] if use is not None else [])[:K]
                    np.testing.assert_array_equal(ids[b, :len(want)], want)
                    assert np.all(ids[b, len(want):] == -1) and np.all(np.isneginf(sc[b, len(want):]))
                    assert np.all(sc[b, :len(want)] == sc[b, 0])
    if n > 2048:
        assert int(hip.topk_wide_state(h.device, B)[1].max()) == 7


# ---------------------------------------------------------------------------------------------------------------------
# 3. K <= 128: the bits of the shipped kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("B,C,d", RANDOM_CASES)
def test_same_bits_as_the_shipped_kernels(B, C, d, tier):
    from recguru_amd import hip
    dtype = _set_tier(tier)
    hn, wn, _, rows, _, _ = _case(B, C, d, tier)
    h, table = _dev(hn, dtype), _dev(wn, dtype)
    rng = np.random.default_rng(31 + C)
    for K in (1, 10, 128):
        for use in (rows, None):
            _same(_wide(hip, h, table, K, 1, C, excl_rows=use), _narrow(hip, h, table, K, 1, C, excl_rows=use), "range K=%d" % K)
    if C == 4099:
        for n_list in (1, 17, 300, 2500):
            lst = make_list(n_list, C + 1, rng)
            for K in (1, 10, 128):
                for use in (rows, None):
                    _same(_wide(hip, h, table, K, rows=lst, excl_rows=use), _narrow(hip, h, table, K, rows=lst, excl_rows=use),
                          "list n=%d K=%d" % (n_list, K))


# ---------------------------------------------------------------------------------------------------------------------
# 4. K > 128: a chain of K = 128 calls of the shipped kernels, no tolerance
# ---------------------------------------------------------------------------------------------------------------------
def _chain_check(hip, h, table, B, C, rows, Ks, lists):
    for K in Ks:
        for use in (rows, None):
            want = chain_topk(lambda ex: _narrow(hip, h, table, 128, 1, C, excl_rows=ex), B, K, 128, use)
            _same(_wide(hip, h, table, K, 1, C, excl_rows=use), want, "range K=%d" % K)
        for lst in lists:
            want = chain_topk(lambda ex: _narrow(hip, h, table, 128, rows=lst, excl_rows=ex), B, K, 128, rows)
            _same(_wide(hip, h, table, K, rows=lst, excl_rows=rows), want, "list n=%d K=%d" % (len(lst), K))


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("B,C,d", RANDOM_CASES)
def test_chain_of_shipped_calls(B, C, d, tier):
    from recguru_amd import hip
    dtype = _set_tier(tier)
    hn, wn, _, rows, _, _ = _case(B, C, d, tier)
    rng = np.random.default_rng(41 + C)
    lists = [make_list(n, C + 1, rng) for n in ((300, 2500) if C == 4099 else (17, 600))]
    _chain_check(hip, _dev(hn, dtype), _dev(wn, dtype), B, C, rows, (300, 1024), lists)


@pytest.mark.parametrize("tier", TIERS)
def test_chain_of_shipped_calls_large_catalogue(tier):
    from recguru_amd import hip
    dtype = _set_tier(tier)
    B, C, d = BIG_CASE
    hn, wn, _, rows, _, _ = _case(B, C, d, tier)
    lists = [make_list(40000, C + 1, np.random.default_rng(43))]
    _chain_check(hip, _dev(hn, dtype), _dev(wn, dtype), B, C, rows, (1024,), lists)


# ---------------------------------------------------------------------------------------------------------------------
# 5. independent of the shipped kernels: the derived bound (topk_ref.pair_bound), max_near an input condition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("B,C,d,Ks", [c + ((1024, 300),) for c in RANDOM_CASES] + [BIG_CASE + ((1024,),)])
def test_derived_bound(B, C, d, Ks, tier):
    from recguru_amd import hip
    dtype = _set_tier(tier)
    hn, wn, _, rows, S, Tb = _case(B, C, d, tier)
    h, table = _dev(hn, dtype), _dev(wn, dtype)
    for K in Ks:
        for use in (rows, None):
            ids, sc = _wide(hip, h, table, K, 1, C, excl_rows=use)
            R.check_topk(ids, sc.astype(np.float64), S, Tb, K, 1, R.eligible(B, 1, C, use), max_near=12)


# ---------------------------------------------------------------------------------------------------------------------
# 6. repeats, batch splits, both libraries (fresh child processes: tests/topk_wide_worker.py)
# ---------------------------------------------------------------------------------------------------------------------
def _worker(det, tmp_path):
    out = str(tmp_path / "wide.npz")
    env = dict(os.environ, PYTHONPATH=os.path.dirname(HERE))
    env.pop("RG_DETERMINISTIC", None)
    if det:
        env["RG_DETERMINISTIC"] = "1"
    r = subprocess.run([sys.executable, os.path.join(HERE, "topk_wide_worker.py"), out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-4000:]
    z = np.load(out)
    assert (int(z["det_enabled"]) > 0) == det
    return z


@pytest.mark.parametrize("det", [False, True])
def test_repeat_and_batch_split_invariance(det, tmp_path):
    from recguru_amd import hip
    z = _worker(det, tmp_path)
    B, C, d, K = 37, 4099, 128, 300
    lst = make_list(2500, C + 1, np.random.default_rng(3))            # the worker's list
    for tier in TIERS:
        dtype = _set_tier(tier)
        hn, wn, _, rows, _, _ = _case(B, C, d, tier)
        h, table = _dev(hn, dtype), _dev(wn, dtype)
        for form in ("range", "list"):
            # this process (the library the suite runs on) against the child's (det: the deterministic library)
            here = _wide(hip, h, table, K, 1, C, excl_rows=rows) if form == "range" else _wide(hip, h, table, K, rows=lst, excl_rows=rows)
            for i, name in enumerate(("ids", "scores")):
                one = z["%s.%s.one.%s" % (tier, form, name)]
                assert one.shape == (B, K)
                for other in ("again", "split"):
                    assert np.array_equal(one.view(np.uint8), z["%s.%s.%s.%s" % (tier, form, other, name)].view(np.uint8)), (tier, form, other, name)
                assert np.array_equal(one.view(np.uint8), here[i].view(np.uint8)), ("this process", tier, form, name)


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals: code and message, nothing launched, no output written, the next call answers
# ---------------------------------------------------------------------------------------------------------------------
def _raw_call(hip, h, table, k, ids, sc, ws, ws_bytes, first_row=0, n_rows=0, rows=None):
    a = hip.TopkWideArgs(h.data_ptr(), table.data_ptr(), first_row, n_rows, None if rows is None else rows.data_ptr(),
                         0 if rows is None else rows.numel(), table.shape[0], None, None, None if ids is None else ids.data_ptr(),
                         None if sc is None else sc.data_ptr(), None if ws is None else ws.data_ptr(), ws_bytes, h.shape[0], h.shape[1], k)
    rc = hip.lib().rg_topk_wide(ctypes.byref(a), hip._full_ce_code(h), hip._stream())
    return rc, hip.lib().rg_last_error().decode()


def test_refusals():
    from recguru_amd import hip
    h = torch.zeros(4, 128, device="cuda", dtype=torch.bfloat16)
    table = torch.zeros(50, 128, device="cuda", dtype=torch.bfloat16)
    good = torch.tensor([3, 7, 49], device="cuda")
    torch.cuda.synchronize()
    pre = r"rg_topk_wide failed \(%d\): topk_wide: "
    for k in (0, 1025):
        with pytest.raises(RuntimeError, match=pre % -2 + r"K must be in \[1, 1024\]"):
            hip.topk_wide(h, table, k, 1, 49)
        with pytest.raises(RuntimeError, match=pre % -2 + r"K must be in \[1, 1024\]"):
            hip.topk_wide(h, table, k, rows=good)
    h96 = torch.zeros(4, 96, device="cuda", dtype=torch.bfloat16)
    t96 = torch.zeros(50, 96, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match=pre % -2 + r"d must be 64, 128 or 256"):
        hip.topk_wide(h96, t96, 300, 1, 49)
    with pytest.raises(RuntimeError, match=pre % -1 + r"rows must be strictly ascending \(rows\[2\] = 5 after 7\)"):
        hip.topk_wide(h, table, 300, rows=torch.tensor([3, 7, 5, 9, 8], device="cuda"))
    with pytest.raises(RuntimeError, match=pre % -1 + r"rows must be strictly ascending \(rows\[1\] = 3 after 3\)"):
        hip.topk_wide(h, table, 300, rows=torch.tensor([3, 3, 5], device="cuda"))
    with pytest.raises(RuntimeError, match=pre % -1 + r"rows\[2\] = 50 is outside the table rows \[0, 50\)"):
        hip.topk_wide(h, table, 300, rows=torch.tensor([3, 7, 50], device="cuda"))
    with pytest.raises(RuntimeError, match=pre % -1 + r"rows\[0\] = -1 is outside the table rows \[0, 50\)"):
        hip.topk_wide(h, table, 300, rows=torch.tensor([-1, 7, 9], device="cuda"))
    # straight at the ABI, with outputs and a workspace of the test's own: both outputs NULL, a workspace one byte short, a bad list
    fn = hip.lib().rg_topk_wide_workspace
    fn.restype = ctypes.c_size_t
    need = int(fn(4, 128, ctypes.c_longlong(49), 300))
    assert need > 0
    ws = torch.full((need,), 0x5A, device="cuda", dtype=torch.uint8)
    ids = torch.full((4, 300), 7, device="cuda", dtype=torch.int64)
    sc = torch.full((4, 300), 7.0, device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    rc, msg = _raw_call(hip, h, table, 300, None, None, ws, need, 1, 49)
    assert rc == -1 and msg == "topk_wide: topk_ids or topk_scores is required", (rc, msg)
    rc, msg = _raw_call(hip, h, table, 300, ids, sc, ws, need - 1, 1, 49)
    assert rc == -1 and msg == "topk_wide: workspace of %d bytes needed, %d given" % (need, need - 1), (rc, msg)
    rc, msg = _raw_call(hip, h, table, 300, ids, sc, None, 0, 1, 49)
    assert rc == -1 and msg.startswith("topk_wide: workspace of"), (rc, msg)
    rc, msg = _raw_call(hip, h, table, 300, ids, sc, ws, need, rows=torch.tensor([3, 9, 9], device="cuda"))
    assert rc == -1 and msg == "topk_wide: rows must be strictly ascending (rows[2] = 9 after 9)", (rc, msg)
    torch.cuda.synchronize()
    assert bool((ids == 7).all()) and bool((sc == 7.0).all()), "a refused call wrote an output"
    body = ws.clone()
    body[128:136] = 0x5A                                             # (the list check's own word)
    assert bool((body == 0x5A).all()), "a refused call wrote more of the workspace than the list check's word"
    # the same arguments, supported: answers
    rc, msg = _raw_call(hip, h, table, 300, ids, None, ws, need, 1, 49)
    torch.cuda.synchronize()
    assert rc == 0 and ids[:, :49].cpu().tolist() == [list(range(1, 50))] * 4 and bool((ids[:, 49:] == -1).all()) and bool((sc == 7.0).all())
    ids2, sc2 = hip.topk_wide(h, table, 4, rows=good)
    assert ids2.cpu().tolist() == [[3, 7, 49, -1]] * 4
    assert sc2.cpu()[:, :3].abs().max() == 0.0 and bool(torch.isneginf(sc2.cpu()[:, 3]).all())
    # the narrow entry points refuse K = 129 as before
    with pytest.raises(RuntimeError, match=r"rg_topk_scores failed \(-2\): topk_scores: K must be in \[0, 128\]"):
        hip.topk_scores(h, table, 129, 1, 49)
    with pytest.raises(RuntimeError, match=r"rg_topk_list failed \(-2\): topk_list: K must be in \[0, 128\]"):
        hip.topk_list(h, table, 129, good)


# ---------------------------------------------------------------------------------------------------------------------
# 8. the public surface, both model families
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["cross", "single"])
def test_recommend_above_128(family):
    from recguru_amd import auto_training, synthetic, training
    from recguru_amd.config import get_param
    from recguru_amd.models import MyAuto4Rec_c, MyRec
    from recguru_amd.synthetic import TensorLoader
    _set_tier("f32")
    d, H, L, N, V, B = 128, 4, 50, 1, 700, 5
    torch.manual_seed(11)
    param = get_param(make_args(d, H, 3, L, V, V, N, B), make_dirs=False)
    if family == "cross":
        M = MyAuto4Rec_c("cuda", param).to(torch.float32).cuda().eval()
        rec = lambda e, di, k, **kw: training.recommend(M, e, di, k, param, domain="a", device="cuda", **kw)
    else:
        M = MyRec("cuda", param, None, dec_rec=False, fix_enc=False, sas=False, pos_train=False).to(torch.float32).cuda().eval()
        rec = lambda e, di, k, **kw: auto_training.recommend(M, e, di, k, param, **kw)
    dom = synthetic.make_domain(2 * B, V, L, 3, seed=9)
    (enc_in, dec_in, _), _, _, _ = next(iter(TensorLoader(dom, B, "cuda")))
    own = [set(int(x) for x in row if 0 < x <= V) for row in enc_in.cpu().numpy()]
    rng = np.random.default_rng(8)
    among_long = rng.permutation(np.arange(1, V + 1))[:500].tolist()
    among_short = rng.permutation(np.arange(1, V + 1))[:200].tolist()
    host = lambda res: tuple(t.cpu().numpy() for t in res)
    for exclude_seen in (True, False):
        for among in (None, among_long):
            narrow = host(rec(enc_in, dec_in, 128, exclude_seen=exclude_seen, among=among))
            for k in (300, 1024):
                ids, sc = host(rec(enc_in, dec_in, k, exclude_seen=exclude_seen, among=among))
                assert ids.shape == (B, k) and sc.shape == (B, k)
                _same((np.ascontiguousarray(ids[:, :128]), np.ascontiguousarray(sc[:, :128])), narrow, "k=%d among=%s" % (k, among is not None))
                members = set(range(1, V + 1)) if among is None else set(among)
                for b in range(B):
                    want = len(members - own[b]) if exclude_seen else len(members)
                    got = ids[b][ids[b] >= 0]
                    assert len(got) == min(k, want) and len(set(got.tolist())) == len(got) and set(got.tolist()) <= members
                    assert np.all(ids[b, len(got):] == -1) and np.all(np.isneginf(sc[b, len(got):]))
                    assert np.all(np.diff(sc[b, :len(got)]) <= 0)
                    if exclude_seen:
                        assert not set(got.tolist()) & own[b], "a seen item was recommended"
        ids, sc = host(rec(enc_in, dec_in, 300, exclude_seen=exclude_seen, among=among_short))          # a list shorter than k
        assert np.all(ids[:, 200:] == -1) and np.all(np.isneginf(sc[:, 200:])) and np.all((ids[:, :100] >= 1))
    with pytest.raises(ValueError, match="1024"):
        rec(enc_in, dec_in, 1025)
    with pytest.raises(ValueError, match="1024"):
        rec(enc_in, dec_in, 1025, among=among_long)
    with pytest.raises(NotImplementedError):
        rec(enc_in, dec_in, 300, sas=True)
