"""Top-K and exact rank over a candidate list shared by the batch (rg_topk_list, csrc/topk.hip).  The list form and the range form
(rg_topk_scores) share one score function, so most checks are bit-exact: a whole-range list against the range call, a subset
against the range call with the complement excluded, additivity over a split list, repeats / batch splits / the deterministic
library; then an exact integer fixture and random fixtures against the float64 restatement of tests/topk_ref.py, the refusals, and
recommend / evaluation_full(among=...) of both model families.  The numpy helpers at the top are checked by tests/test_topk_list_cpu.py."""
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
T_ROWS = 3001                                   # table rows 0 .. 3000
LIST_SIZES = [1, 15, 16, 17, 1040, T_ROWS - 1]   # 1040 = 65 tiles of 16, one more than 64 slices; the last: all rows but row 0
BS = [1, 17, 70]
KS = [0, 1, 10, 128]


# ---------------------------------------------------------------------------------------------------------------------
# numpy helpers (no GPU; tests/test_topk_list_cpu.py holds them to topk_ref on a case enumerated by hand)
# ---------------------------------------------------------------------------------------------------------------------
def make_list(n, table_rows, rng):
    """n strictly ascending table rows: all rows but row 0 when n = table_rows - 1, else random rows (large gaps when n is small)
    that always include the last table row."""
    if n == table_rows - 1:
        return np.arange(1, table_rows, dtype=np.int64)
    rest = rng.choice(table_rows - 1, size=n - 1, replace=False)
    return np.sort(np.concatenate([rest, [table_rows - 1]])).astype(np.int64)


def make_targets(rows, table_rows, B, rng):
    """[B] table rows, alternating between members of the list and rows outside it (where the list leaves any)."""
    outside = np.setdiff1d(np.arange(table_rows), rows)
    tg = rows[rng.integers(0, len(rows), size=B)].copy()
    if len(outside):
        tg[1::2] = outside[rng.integers(0, len(outside), size=len(tg[1::2]))]
    return tg.astype(np.int64)


def make_excl(rows, target, table_rows, rng):
    """per user a random exclusion run over the whole table (members of the list and not); user 0's is empty, user 1's holds its own
    target, the last user's also an id past the table and most of the list (fewer than K eligible ids at any list size)."""
    B = len(target)
    out = []
    for b in range(B):
        r = rng.choice(table_rows, size=int(rng.integers(0, 40)), replace=False).tolist()
        r += rows[rng.integers(0, len(rows), size=int(rng.integers(0, 12)))].tolist()
        if b == 0:
            r = []
        if b == 1:
            r.append(int(target[b]))
        if b == B - 1 and B > 2:
            r += [table_rows, table_rows + 5] + rows[: max(len(rows) - 3, 0)].tolist()
        out.append(sorted(set(r)))
    return out


def complement_excl(excl_rows, rows, first_row, n_rows, B):
    """E_b united with (catalogue minus the list): the exclusion runs under which the range call answers like the list call."""
    comp = np.setdiff1d(np.arange(first_row, first_row + n_rows), rows)
    return [np.union1d(comp, np.asarray(excl_rows[b] if excl_rows is not None else [], dtype=np.int64)) for b in range(B)]


def list_eligible(rows, excl_rows, B):
    """bool [B, n_list]: rows[p] is not in user b's exclusion run."""
    el = np.ones((B, len(rows)), dtype=bool)
    if excl_rows is not None:
        for b in range(B):
            el[b] = ~np.isin(rows, np.asarray(excl_rows[b], dtype=np.int64))
    return el


def list_rank(S_table, rows, target, el):
    """number of list ids i != target[b], eligible, with S_table[b, i] > S_table[b, target[b]] strictly (S_table: [B, table_rows])."""
    out = np.zeros(len(target), dtype=np.int64)
    for b, t in enumerate(target):
        m = el[b] & (rows != t)
        out[b] = int((m & (S_table[b, rows] > S_table[b, t])).sum())
    return out


def list_topk(S_table, rows, k, el):
    """topk_ref.topk over the list's positions, the ids mapped back to table rows (-1 stays)."""
    pos, sc = R.topk(S_table[:, rows], k, 0, el)
    return np.where(pos >= 0, rows[np.maximum(pos, 0)], -1), sc


def positions(ids, rows):
    """returned table rows -> positions in the list (-1 stays); asserts that every returned id is a member."""
    p = np.searchsorted(rows, np.maximum(ids, 0))
    p = np.minimum(p, len(rows) - 1)
    assert np.all((rows[p] == ids) | (ids < 0)), "an id outside the list was returned"
    return np.where(ids >= 0, p, -1)


def list_rank_interval(S_table, Tb, rows, target, el):
    """topk_ref.rank_interval with the target scored wherever it sits in the table."""
    lo = np.zeros(len(target), dtype=np.int64)
    hi = np.zeros(len(target), dtype=np.int64)
    for b, t in enumerate(target):
        m = el[b] & (rows != t)
        s = S_table[b, rows]
        lo[b] = int((m & (s > S_table[b, t] + 2 * Tb[b])).sum())
        hi[b] = int((m & (s >= S_table[b, t] - 2 * Tb[b])).sum())
    return lo, hi


def near_ties_at_cut(S, Tb, k, el):
    """per user the number of eligible ids within 2 T_b of the reference's k-th score: topk_ref.check_topk's input condition"""
    out = np.zeros(S.shape[0], dtype=np.int64)
    for b in range(S.shape[0]):
        j = np.flatnonzero(el[b])
        kk = min(k, len(j))
        if kk == 0:
            continue
        ref = np.sort(S[b, j])[::-1]
        out[b] = int((np.abs(S[b, j] - ref[kk - 1]) <= 2 * Tb[b]).sum())
    return out


def merge_topk(ids1, sc1, ids2, sc2, k):
    """the k best of the union of two results under (score descending, id ascending); -1 slots dropped, then refilled"""
    B = ids1.shape[0]
    ids = np.full((B, k), -1, dtype=np.int64)
    sc = np.full((B, k), -np.inf, dtype=sc1.dtype)
    for b in range(B):
        i = np.concatenate([ids1[b], ids2[b]])
        s = np.concatenate([sc1[b], sc2[b]])
        keep = i >= 0
        i, s = i[keep], s[keep]
        order = np.lexsort((i, -s.astype(np.float64)))[:k]
        ids[b, :len(order)] = i[order]
        sc[b, :len(order)] = s[order]
    return ids, sc


RANDOM_CASES = [(17, 1040, 128, 100), (70, T_ROWS - 1, 64, 10), (17, 17, 256, 10), (1, T_ROWS - 1, 256, 128), (70, 1040, 64, 128)]


def random_list_case(B, n_list, d, tier, seed=4100):
    """(h f32 [B, d], table f32 [T_ROWS, d], rows, target, exclusion runs, float64 scores over the table, T_b over the table)"""
    rng = np.random.default_rng(seed + 7 * B + n_list + d)
    hn = rng.normal(size=(B, d)).astype(np.float32)
    wn = (0.1 * rng.normal(size=(T_ROWS, d))).astype(np.float32)
    rows = make_list(n_list, T_ROWS, rng)
    target = make_targets(rows, T_ROWS, B, rng)
    excl = make_excl(rows, target, T_ROWS, rng)
    hr, wr = R.round_tier(hn, tier), R.round_tier(wn, tier)
    return hn, wn, rows, target, excl, R.scores(hr, wr), R.pair_bound(hr, wr, tier != "bf16").max(axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# device plumbing
# ---------------------------------------------------------------------------------------------------------------------
def _set_tier(tier):
    from recguru_amd import ops
    ops.set_compute_dtype({"bf16": torch.bfloat16, "bf16x3": "bf16x3", "f32": torch.float32}[tier])
    return torch.bfloat16 if tier == "bf16" else torch.float32


def _dev(x, dtype=None):
    t = torch.as_tensor(x).cuda()
    return t.to(dtype) if dtype is not None else t


def _csr_dev(excl_rows):
    if excl_rows is None or isinstance(excl_rows, tuple):          # (a tuple: built already)
        return excl_rows if excl_rows is not None else (None, None)
    v, o = R.csr(excl_rows)
    return _dev(v), _dev(o)


def _host(res):
    return tuple(None if t is None else t.cpu().numpy() for t in res)


def _list_call(hip, h, table, k, rows, target=None, excl_rows=None):
    ex, off = _csr_dev(excl_rows)
    return _host(hip.topk_list(h, table, k, _dev(rows), target=None if target is None else _dev(target), excl=ex, excl_off=off))


def _range_call(hip, h, table, k, first_row, n_rows, target=None, excl_rows=None):
    ex, off = _csr_dev(excl_rows)
    return _host(hip.topk_scores(h, table, k, first_row, n_rows, target=None if target is None else _dev(target), excl=ex, excl_off=off))


def _same(got, want, tag):
    """ids, scores and ranks identical; scores bit for bit"""
    for name, g, w in zip(("ids", "scores", "rank"), got, want):
        assert (g is None) == (w is None), (tag, name)
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, (tag, name)
            np.testing.assert_array_equal(g.view(np.uint8), w.view(np.uint8), err_msg="%s %s" % (tag, name))


def _random_operands(B, d, dtype, rng):
    hn = rng.normal(size=(B, d)).astype(np.float32)
    wn = (0.1 * rng.normal(size=(T_ROWS, d))).astype(np.float32)
    wn[rng.integers(0, T_ROWS, size=400)] = wn[rng.integers(0, T_ROWS, size=400)]          # duplicate rows: exact ties in every tier
    return _dev(hn, dtype), _dev(wn, dtype)


# ---------------------------------------------------------------------------------------------------------------------
# 1. a list that is a whole range answers like the range call, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("tier", TIERS)
def test_whole_range_list_equals_the_range_call(tier, d):
    from recguru_amd import hip
    dtype = _set_tier(tier)
    rng = np.random.default_rng(100 + d)
    for B in BS:
        h, table = _random_operands(B, d, dtype, rng)
        for first, n in ((0, T_ROWS), (1, T_ROWS - 1), (1961, 1040), (T_ROWS - 17, 17), (5, 16), (T_ROWS - 1, 1)):
            rows = np.arange(first, first + n, dtype=np.int64)
            target = first + rng.integers(0, n, size=B)
            for excl in (None, _csr_dev(make_excl(rows, target, T_ROWS, rng))):
                for K in KS:
                    tag = "B=%d first=%d n=%d K=%d excl=%s" % (B, first, n, K, excl is not None)
                    _same(_list_call(hip, h, table, K, rows, target, excl), _range_call(hip, h, table, K, first, n, target, excl), tag)


# ---------------------------------------------------------------------------------------------------------------------
# 2. a subset answers like the range call over the whole table with the complement added to every exclusion run
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("tier", TIERS)
def test_subset_equals_complement_exclusion(tier, d):
    from recguru_amd import hip
    dtype = _set_tier(tier)
    rng = np.random.default_rng(200 + d)
    for B in BS:
        h, table = _random_operands(B, d, dtype, rng)
        for n in LIST_SIZES:
            rows = make_list(n, T_ROWS, rng)
            target = make_targets(rows, T_ROWS, B, rng)          # inside the list and outside it
            for excl in (None, make_excl(rows, target, T_ROWS, rng)):          # user 1's run holds its own target
                ex, off = _csr_dev(complement_excl(excl, rows, 0, T_ROWS, B))
                excl = _csr_dev(excl) if excl is not None else None
                for K in KS:
                    want = _host(hip.topk_scores(h, table, K, 0, T_ROWS, target=_dev(target), excl=ex, excl_off=off))
                    got = _list_call(hip, h, table, K, rows, target, excl)
                    _same(got, want, "B=%d n=%d K=%d excl=%s" % (B, n, K, excl is not None))
                    if K > n:
                        assert np.all(got[0][:, n:] == -1) and np.all(np.isneginf(got[1][:, n:]))


# ---------------------------------------------------------------------------------------------------------------------
# 3. additivity over a split list; repeats, batch splits and the deterministic library change no bit
# ---------------------------------------------------------------------------------------------------------------------
def additivity_case(d=128, B=70, n=1040, seed=300):
    """operands and a list for the additivity / invariance checks (also what tests/topk_list_worker.py runs)"""
    rng = np.random.default_rng(seed + d)
    hn = rng.normal(size=(B, d)).astype(np.float32)
    wn = (0.1 * rng.normal(size=(T_ROWS, d))).astype(np.float32)
    rows = make_list(n, T_ROWS, rng)
    target = make_targets(rows, T_ROWS, B, rng)
    return hn, wn, rows, target, make_excl(rows, target, T_ROWS, rng)


@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("tier", TIERS)
def test_additivity_repeat_and_batch_split(tier, d):
    from recguru_amd import hip
    dtype = _set_tier(tier)
    for n in (17, 1040, T_ROWS - 1):
        hn, wn, rows, target, excl = additivity_case(d, 70, n)
        h, table = _dev(hn, dtype), _dev(wn, dtype)
        for K in (10, 128):
            one = _list_call(hip, h, table, K, rows, target, excl)
            _same(_list_call(hip, h, table, K, rows, target, excl), one, "repeat n=%d K=%d" % (n, K))
            parts = [_list_call(hip, h[b0:b1].contiguous(), table, K, rows, target[b0:b1], excl[b0:b1]) for b0, b1 in ((0, 1), (1, 18), (18, 70))]
            _same(tuple(np.concatenate([p[i] for p in parts]) for i in range(3)), one, "batch split n=%d K=%d" % (n, K))
            for s1, s2 in ((rows[: n // 2], rows[n // 2:]), (rows[0::2], rows[1::2])):          # two halves; two interleaved halves
                a = _list_call(hip, h, table, K, s1, target, excl)
                b = _list_call(hip, h, table, K, s2, target, excl)
                np.testing.assert_array_equal(a[2] + b[2], one[2], err_msg="rank additivity n=%d" % n)
                ids, sc = merge_topk(a[0], a[1], b[0], b[1], K)
                _same((ids, sc, one[2]), one, "top-K of the union n=%d K=%d" % (n, K))


def test_deterministic_library_gives_the_same_bits(tmp_path):
    from recguru_amd import hip
    out = str(tmp_path / "list.npz")
    env = dict(os.environ, PYTHONPATH=os.path.dirname(HERE), RG_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "topk_list_worker.py"), out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-4000:]
    z = np.load(out)
    assert int(z["det_enabled"]) > 0
    for tier in TIERS:
        dtype = _set_tier(tier)
        hn, wn, rows, target, excl = additivity_case()
        one = _list_call(hip, _dev(hn, dtype), _dev(wn, dtype), 100, rows, target, excl)
        _same(tuple(z["%s.%s" % (tier, name)] for name in ("ids", "scores", "rank")), one, "deterministic library, %s" % tier)


# ---------------------------------------------------------------------------------------------------------------------
# 4. exact fixture: small integers, every score exact in every tier; ties across tiles and slices, lower id first
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("tier", TIERS)
def test_exact_fixture(tier, d):
    from recguru_amd import hip
    dtype = _set_tier(tier)
    rng = np.random.default_rng(400 + d)
    pool = rng.integers(-3, 4, size=(9, d)).astype(np.float32)
    for B in BS:
        hn = rng.integers(-3, 4, size=(B, d)).astype(np.float32)
        wn = rng.integers(-3, 4, size=(T_ROWS, d)).astype(np.float32)
        tied = rng.random(T_ROWS) < 0.6
        wn[tied] = pool[rng.integers(0, len(pool), size=int(tied.sum()))]          # 9 distinct rows over 60 % of the table: long tie runs
        wn[-40:] = pool[0]                                                          # ... one across the last tiles and slices of any list
        S = R.scores(R.round_tier(hn, tier), R.round_tier(wn, tier))
        h, table = _dev(hn, dtype), _dev(wn, dtype)
        for n in LIST_SIZES:
            rows = make_list(n, T_ROWS, rng)
            target = make_targets(rows, T_ROWS, B, rng)
            for excl in (None, make_excl(rows, target, T_ROWS, rng)):
                el = list_eligible(rows, excl, B)
                rk_ref = list_rank(S, rows, target, el)
                excl = _csr_dev(excl) if excl is not None else None
                for K in KS:
                    ids, sc, rk = _list_call(hip, h, table, K, rows, target, excl)
                    tag = "B=%d n=%d K=%d excl=%s" % (B, n, K, excl is not None)
                    np.testing.assert_array_equal(rk, rk_ref, err_msg=tag)
                    if K:
                        ids_ref, sc_ref = list_topk(S, rows, K, el)
                        np.testing.assert_array_equal(ids, ids_ref, err_msg=tag)
                        np.testing.assert_array_equal(sc.astype(np.float64), sc_ref, err_msg=tag)


# ---------------------------------------------------------------------------------------------------------------------
# 5. random fixtures under the derived bound (topk_ref.pair_bound; nothing here is measured from the kernel)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("B,n_list,d,K", RANDOM_CASES)
def test_random_fixture(B, n_list, d, K, tier):
    from recguru_amd import hip
    dtype = _set_tier(tier)
    hn, wn, rows, target, excl, S, Tb = random_list_case(B, n_list, d, tier)
    h, table = _dev(hn, dtype), _dev(wn, dtype)
    for use in (excl, None):
        el = list_eligible(rows, use, B)
        ids, sc, rk = _list_call(hip, h, table, K, rows, target, use)
        lo, hi = list_rank_interval(S, Tb, rows, target, el)
        assert np.all(lo <= rk) and np.all(rk <= hi), (lo, rk, hi)
        has = el.any(axis=1)                                     # (check_topk wants an eligible id; a user without one: all -1)
        assert np.all(ids[~has] == -1) and np.all(np.isneginf(sc[~has]))
        R.check_topk(positions(ids, rows)[has], sc.astype(np.float64)[has], S[:, rows][has], Tb[has], K, 0, el[has])


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals: code and message, nothing launched, the next call answers
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from recguru_amd import hip
    h = torch.zeros(4, 128, device="cuda", dtype=torch.bfloat16)
    table = torch.zeros(50, 128, device="cuda", dtype=torch.bfloat16)
    good = torch.tensor([3, 7, 49], device="cuda")
    tg = torch.tensor([1, 2, 49, 3], device="cuda")
    torch.cuda.synchronize()
    pre = r"rg_topk_list failed \(%d\): topk_list: "
    with pytest.raises(RuntimeError, match=pre % -1 + r"rows must be strictly ascending \(rows\[2\] = 5 after 7\)"):
        hip.topk_list(h, table, 3, torch.tensor([3, 7, 5, 9, 8], device="cuda"))
    with pytest.raises(RuntimeError, match=pre % -1 + r"rows must be strictly ascending \(rows\[1\] = 3 after 3\)"):
        hip.topk_list(h, table, 3, torch.tensor([3, 3, 5], device="cuda"), target=tg)
    with pytest.raises(RuntimeError, match=pre % -1 + r"rows\[2\] = 50 is outside the table rows \[0, 50\)"):
        hip.topk_list(h, table, 3, torch.tensor([3, 7, 50], device="cuda"))
    with pytest.raises(RuntimeError, match=pre % -1 + r"rows\[0\] = -1 is outside the table rows \[0, 50\)"):
        hip.topk_list(h, table, 3, torch.tensor([-1, 7, 9], device="cuda"))
    with pytest.raises(RuntimeError, match=pre % -2 + r"n_list must be in \[1, 2\^31\)"):
        hip.topk_list(h, table, 3, torch.zeros(0, device="cuda", dtype=torch.int64))
    with pytest.raises(RuntimeError, match=pre % -2 + r"K must be in \[0, 128\]"):
        hip.topk_list(h, table, 129, good)
    h96 = torch.zeros(4, 96, device="cuda", dtype=torch.bfloat16)
    t96 = torch.zeros(50, 96, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match=pre % -2 + r"d must be 64, 128 or 256"):
        hip.topk_list(h96, t96, 3, good)
    with pytest.raises(RuntimeError, match=pre % -1 + r"rank needs target"):
        hip.topk_list(h, table, 3, good, want_rank=True)
    for bad in (50, -3):
        with pytest.raises(RuntimeError, match=pre % -2 + r"target\[2\] = %d is outside the table rows \[0, 50\)" % bad):
            hip.topk_list(h, table, 3, good, target=torch.tensor([1, 2, bad, 3], device="cuda"))
    # the refusals launched no scoring kernel: the stream is clean and a supported call still answers
    torch.cuda.synchronize()
    ids, sc, rk = hip.topk_list(h, table, 4, good, target=tg)
    assert ids.cpu().tolist() == [[3, 7, 49, -1]] * 4 and rk.cpu().tolist() == [0] * 4
    assert sc.cpu()[:, :3].abs().max() == 0.0 and bool(torch.isneginf(sc.cpu()[:, 3]).all())


# ---------------------------------------------------------------------------------------------------------------------
# 7. the public interface on a catalogue small enough for K to hold the full ranking
# ---------------------------------------------------------------------------------------------------------------------
def _eval_loader(dom, B):
    from recguru_amd.synthetic import TensorLoader
    out = []
    for (enc_in, dec_in, _), n_items, val, test in TensorLoader(dom, B, "cuda"):
        out.append(((enc_in, dec_in, val), (enc_in, dec_in, test), n_items, n_items))
    assert len(out) == 2
    return out


def _filter_full_ranking(ids_full, sc_full, members, k):
    """the full ranking cut down to the members of a list and to k entries, -1 / -inf past them"""
    B = ids_full.shape[0]
    ids = np.full((B, k), -1, dtype=np.int64)
    sc = np.full((B, k), -np.inf, dtype=np.float32)
    for b in range(B):
        keep = np.isin(ids_full[b], members) & (ids_full[b] >= 0)
        ids[b, :min(k, keep.sum())] = ids_full[b][keep][:k]
        sc[b, :min(k, keep.sum())] = sc_full[b][keep][:k]
    return ids, sc


@pytest.mark.parametrize("family", ["cross", "single"])
def test_recommend_and_evaluation_full_among(family):
    from recguru_amd import auto_training, hip, ops, synthetic, training
    from recguru_amd.config import get_param
    from recguru_amd.models import MyAuto4Rec_c, MyRec
    _set_tier("f32")
    d, H, L, N, V, B, K = 128, 4, 50, 1, 97, 5, 10
    torch.manual_seed(12)
    param = get_param(make_args(d, H, 3, L, V, V, N, B), make_dirs=False)
    if family == "cross":
        M = MyAuto4Rec_c("cuda", param).to(torch.float32).cuda().eval()
        state = lambda e, di: training._last_rec_state(M, e, di, "a", param, "cuda")
        table = lambda: ops.shadow(M.item_table("a"))
        rec = lambda e, di, k, **kw: training.recommend(M, e, di, k, param, domain="a", device="cuda", **kw)
        evaluate = lambda ld, kv, **kw: training.evaluation_full(M, ld, "cuda", param, k_val=kv, domain="a", **kw)
        eos = param.vocab_size_a
    else:
        M = MyRec("cuda", param, None, dec_rec=False, fix_enc=False, sas=False, pos_train=False).to(torch.float32).cuda().eval()

        def state(e, di):
            with torch.no_grad():
                return M.get_embedding(e, di)[:, -1, :].contiguous()
        table = lambda: ops.shadow(M.AutoEnc.src_emb.weight)
        rec = lambda e, di, k, **kw: auto_training.recommend(M, e, di, k, param, **kw)
        evaluate = lambda ld, kv, **kw: auto_training.evaluation_full(M, ld, "cuda", param, k_val=kv, **kw)
        eos = param.vocab_size
    assert eos == V + 1 and V <= 128
    dom = synthetic.make_domain(2 * B, V, L, 3, seed=9)
    loader = _eval_loader(dom, B)
    param.eval_steps = 2
    rng = np.random.default_rng(7)
    S_list = np.sort(rng.choice(np.arange(1, V + 1), size=40, replace=False))
    among = rng.permutation(np.concatenate([S_list, S_list[:5]])).tolist()          # unsorted, with repeats: item_list normalises
    ranks = {"eval": [], "test": []}
    for eval_data, test_data, _, _ in loader:
        enc_in, dec_in = eval_data[0], eval_data[1]
        for exclude_seen in (True, False):                                            # (the last `full` is what the ranks are counted from)
            full = _host(rec(enc_in, dec_in, V, exclude_seen=exclude_seen))           # K = V: the full ranking
            got = _host(rec(enc_in, dec_in, K, exclude_seen=exclude_seen, among=among))
            want = _filter_full_ranking(full[0], full[1], S_list, K)
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(got[1].view(np.uint8), want[1].view(np.uint8))
        # among=None makes today's call
        direct = _host(hip.topk_scores(state(enc_in, dec_in), table(), K, 1, V))[:2]
        none = _host(rec(enc_in, dec_in, K, exclude_seen=False, among=None))
        np.testing.assert_array_equal(none[0], direct[0])
        np.testing.assert_array_equal(none[1].view(np.uint8), direct[1].view(np.uint8))
        # ranks among the list, counted from the full ranking (every item with its score, nothing excluded)
        score_of = np.full((B, V + 1), np.nan, dtype=np.float32)
        np.put_along_axis(score_of, full[0], full[1], axis=1)
        assert not np.isnan(score_of[:, 1:]).any()
        for tag, data in (("eval", eval_data), ("test", test_data)):
            tg = data[2].reshape(-1).cpu().numpy()
            ranks[tag].append(np.array([int(((score_of[b, S_list] > score_of[b, tg[b]]) & (S_list != tg[b])).sum()) for b in range(B)]))
    k_val = [1, 5, 10, 30]
    res = evaluate(loader, k_val, among=among)
    assert sorted(res) == sorted(str(k) for k in k_val)
    names = ("ht_eval", "ndcg_eval", "mrr_eval", "ht_test", "ndcg_test", "mrr_test")
    for tag in ("eval", "test"):
        want = R.metrics_of(np.concatenate(ranks[tag]).astype(np.int32), k_val)
        for k in k_val:
            assert sorted(res[str(k)]) == sorted(names) and all(len(res[str(k)][nm]) == 1 for nm in names)
            got = tuple(res[str(k)][nm + "_" + tag][0] for nm in ("ht", "ndcg", "mrr"))
            assert got == want[str(k)], (tag, k, got, want[str(k)])
    with pytest.raises(NotImplementedError):
        rec(loader[0][0][0], loader[0][0][1], K, sas=True, among=among)
    with pytest.raises(NotImplementedError):
        evaluate(loader, k_val, sas=True, among=among)
