"""Hard negatives (rg_hard_negs, csrc/hard_negs.hip): each live position's top-scoring ids of one sampled pool.  An exact integer
fixture and a random fixture under the derived bound against the float64 restatement of tests/hard_negs_ref.py; the kernel the
parent already has (hip.topk_list with label + history as a CSR exclusion) bit for bit; repeats, batch splits, tile placement and
the deterministic library; the model classes; the loader; the refusals."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hard_negs_ref as HR
import topk_ref as R
from parity_util import make_args

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TIERS = ["bf16", "bf16x3", "f32"]
SENT = -77                                     # what the output buffers hold before a call
GUARD = 64                                     # int64 words in front of and behind the output


def _set_tier(tier):
    from recguru_amd import ops
    ops.set_compute_dtype({"bf16": torch.bfloat16, "bf16x3": "bf16x3", "f32": torch.float32}[tier])
    return torch.bfloat16 if tier == "bf16" else torch.float32


@pytest.fixture(autouse=True)
def _restore_tier():
    yield
    from recguru_amd import ops
    ops.set_compute_dtype(torch.bfloat16)


def _dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x)).cuda()
    return t.to(dtype) if dtype is not None else t


def _call(hip, h, table, pool, labels, mask, L, k, skip=0, excl_rows=None, ld=None, flat=None, checked=False, fill=SENT):
    """hip.hard_negs into a guarded, pre-filled buffer -> (out [n, ld], scores [n, k]) numpy; the guard bands are checked here."""
    n = h.shape[0]
    ld = ld or k
    buf = torch.full((2 * GUARD + n * ld,), fill, dtype=torch.int64, device="cuda")
    out = buf[GUARD:GUARD + n * ld].view(n, ld)
    ex = lo = hi = None
    if excl_rows is not None:
        v, l, u = flat if flat is not None else HR.flat_excl(excl_rows)
        ex, lo, hi = _dev(v), _dev(l), _dev(u)
    res, sc = hip.hard_negs(h, table, _dev(pool), _dev(labels), _dev(np.asarray(mask, dtype=np.float32)), L, k, skip=skip, excl=ex,
                            excl_lo=lo, excl_hi=hi, out=out, checked=checked, want_scores=True)
    assert res is out
    b = buf.cpu().numpy()
    assert np.all(b[:GUARD] == fill) and np.all(b[GUARD + n * ld:] == fill), "the guard band around out was written"
    return b[GUARD:GUARD + n * ld].reshape(n, ld).copy(), sc.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact fixture: small integers, every product and sum exact in every tier and any order
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (7, 5), (3, 16), (3, 17)]
POOLS = [1, 17, 257, 1031]
KSKIP = [(1, 0), (7, 3), (30, 98)]
MASKS = ["live", "left", "seq", "tile", "none"]
EXCLS = ["null", "empty", "label", "outside", "all"]
X_ROWS = 2100


def make_mask(kind, B, L, rng):
    m = np.ones((B, L), dtype=np.float32)
    if kind == "left":                                         # left-padded random lengths (length >= 1)
        for b in range(B):
            m[b, :L - int(rng.integers(1, L + 1))] = 0
    elif kind == "seq":                                        # one sequence wholly padded, the others left-padded
        for b in range(B):
            m[b, :L - int(rng.integers(1, L + 1))] = 0
        m[B // 2] = 0
    elif kind == "tile":                                       # a wholly dead 16-row tile (n >= 32), whatever sequences it cuts
        m.reshape(-1)[16:32] = 0
        if B * L < 32:
            m.reshape(-1)[::2] = 0
    elif kind == "none":
        m[:] = 0
    return m.reshape(-1)


def make_excl_rows(kind, B, L, pool, labels, table_rows, rng):
    if kind == "null":
        return None
    rows = []
    for b in range(B):
        r = pool[rng.integers(0, len(pool), size=int(rng.integers(0, 9)))].tolist()
        if kind == "empty" and b % 2 == 0:
            r = []
        if kind == "label":
            r += labels[b * L:(b + 1) * L].tolist()
        if kind == "outside":
            r += np.setdiff1d(rng.integers(0, table_rows, size=20), pool).tolist() + [table_rows, table_rows + 9, 2 ** 40]
        if kind == "all" and b % 2 == 0:
            r = pool.tolist() + [table_rows + 1]
        rows.append(r)
    return rows


@pytest.fixture(scope="module")
def exact_operands():
    rng = np.random.default_rng(5100)
    return {d: (rng.integers(-3, 4, size=(51, d)).astype(np.float32), rng.integers(-3, 4, size=(X_ROWS, d)).astype(np.float32))
            for d in (64, 128, 256)}


@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("tier", TIERS)
def test_exact_fixture(tier, d, exact_operands):
    from recguru_amd import hip
    dtype = _set_tier(tier)
    hn, wn = exact_operands[d]
    table = _dev(wn, dtype)
    rng = np.random.default_rng(5200 + d)
    idx = 0
    for B, L in SHAPES:
        n = B * L
        h = _dev(hn[:n], dtype)
        for C in POOLS:
            pool = np.sort(rng.choice(X_ROWS - 1, size=C, replace=False) + 1).astype(np.int64)
            S = R.scores(hn[:n], wn[pool])
            for k, skip in KSKIP:
                mkind, ekind = MASKS[idx % 5], EXCLS[(idx // 5) % 5]
                ld = k + 5 * (idx % 2)
                idx += 1
                mask = make_mask(mkind, B, L, rng)
                labels = np.where(rng.random(n) < 0.5, pool[rng.integers(0, C, size=n)], rng.integers(0, X_ROWS, size=n)).astype(np.int64)
                rows = make_excl_rows(ekind, B, L, pool, labels, X_ROWS, rng)
                flat = HR.flat_excl(rows, rng) if rows is not None else None
                got, gs = _call(hip, h, table, pool, labels, mask, L, k, skip, rows, ld, flat)
                want, ws = HR.select(S, pool, HR.eligible(pool, labels, L, rows), mask, k, skip, np.full((n, ld), SENT, dtype=np.int64))
                tag = (tier, d, B, L, C, k, skip, ld, mkind, ekind)
                assert np.array_equal(got, want), tag
                assert np.array_equal(gs.astype(np.float64), ws), tag
                if mkind == "none":
                    assert np.all(got == SENT)
    assert idx == 48


# ---------------------------------------------------------------------------------------------------------------------
# 2. random fixture under the derived bound (topk_ref.pair_bound / check_topk); skip against the skip = 0 call
# ---------------------------------------------------------------------------------------------------------------------
RANDOM_CASES = [(7, 23, 1031, 64, 33), (7, 23, 1031, 128, 33), (7, 23, 1031, 256, 33), (3, 50, 4099, 128, 128)]


def random_case(B, L, C, d, tier):
    rng = np.random.default_rng(7100 + B + L + C + d)
    n = B * L
    hn = rng.normal(size=(n, d)).astype(np.float32)
    wn = (0.1 * rng.normal(size=(3 * C, d))).astype(np.float32)
    pool = np.sort(rng.choice(3 * C - 1, size=C, replace=False) + 1).astype(np.int64)
    labels = np.where(np.arange(n) % 3 == 0, pool[rng.integers(0, C, size=n)], rng.integers(1, 3 * C, size=n)).astype(np.int64)
    rows = [pool[rng.choice(C, size=int(rng.integers(0, 60)), replace=False)].tolist() for _ in range(B)]
    mask = make_mask("left", B, L, rng)
    hr, wr = R.round_tier(hn, tier), R.round_tier(wn[pool], tier)
    return hn, wn, pool, labels, rows, mask, R.scores(hr, wr), R.pair_bound(hr, wr, tier != "bf16").max(axis=1)


@pytest.mark.parametrize("B,L,C,d,K", RANDOM_CASES)
@pytest.mark.parametrize("tier", TIERS)
def test_random_fixture_under_the_derived_bound(tier, B, L, C, d, K):
    from recguru_amd import hip
    dtype = _set_tier(tier)
    hn, wn, pool, labels, rows, mask, S, Tb = random_case(B, L, C, d, tier)
    h, table = _dev(hn, dtype), _dev(wn, dtype)
    ids, sc = _call(hip, h, table, pool, labels, mask, L, K, 0, rows, fill=-1)
    live = np.flatnonzero(mask)
    assert np.all(ids[mask == 0] == -1) and len(live) > 16
    el = HR.eligible(pool, labels, L, rows)
    p = np.searchsorted(pool, np.maximum(ids[live], 0))
    assert np.all((pool[np.minimum(p, C - 1)] == ids[live]) | (ids[live] < 0)), "an id outside the pool was returned"
    R.check_topk(np.where(ids[live] >= 0, p, -1), sc[live].astype(np.float64), S[live], Tb[live], K, 0, el[live])
    for s in (1, 20):
        part, ps = _call(hip, h, table, pool, labels, mask, L, K - s, s, rows, fill=-1)
        assert np.array_equal(part, ids[:, s:]) and np.array_equal(ps.view(np.int32), sc[:, s:].view(np.int32)), (tier, s)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the kernel the parent already has: hip.topk_list over every position with (sequence's row + label) as a CSR exclusion
# ---------------------------------------------------------------------------------------------------------------------
def list_case(B=8, L=20, C=300, d=128, seed=7300):
    rng = np.random.default_rng(seed)
    n = B * L
    hn = rng.normal(size=(n, d)).astype(np.float32)
    wn = (0.1 * rng.normal(size=(3 * C, d))).astype(np.float32)
    pool = np.sort(rng.choice(3 * C - 1, size=C, replace=False) + 1).astype(np.int64)
    labels = np.where(np.arange(n) % 2 == 0, pool[rng.integers(0, C, size=n)], rng.integers(1, 3 * C, size=n)).astype(np.int64)
    rows = [pool[rng.choice(C, size=int(rng.integers(0, 60)), replace=False)].tolist() for _ in range(B)]
    rows[1] = pool[:C - 4].tolist()                            # fewer eligible ids than skip + k
    return hn, wn, pool, labels, rows, make_mask("left", B, L, rng)


@pytest.mark.parametrize("tier", TIERS)
def test_against_topk_list(tier):
    from recguru_amd import hip
    dtype = _set_tier(tier)
    hn, wn, pool, labels, rows, mask = list_case()
    L, k, skip = 20, 7, 3
    h, table = _dev(hn, dtype), _dev(wn, dtype)
    got, gs = _call(hip, h, table, pool, labels, mask, L, k, skip, rows, fill=-1)
    v, off = R.csr([rows[t // L] + [int(labels[t])] for t in range(len(labels))])
    ids, sc, _ = hip.topk_list(h, table, skip + k, _dev(pool), excl=_dev(v), excl_off=_dev(off))
    ids, sc = ids.cpu().numpy()[:, skip:], sc.cpu().numpy()[:, skip:]
    live = mask != 0
    assert live.sum() > 40 and np.any(ids[live] == -1) and np.any(ids[live] >= 0)
    assert np.array_equal(got[live], ids[live])
    assert np.array_equal(gs[live].view(np.int32), sc[live].view(np.int32))
    assert np.all(got[~live] == -1)


# ---------------------------------------------------------------------------------------------------------------------
# 4. invariance: repeats, batch splits, tile placement, the deterministic library
# ---------------------------------------------------------------------------------------------------------------------
def invariance_results(hip, tier, dtype):
    """the list case's (ids, scores) at k = 9, skip = 2 -- also what tests/hard_negs_worker.py runs"""
    hn, wn, pool, labels, rows, mask = list_case()
    return _call(hip, _dev(hn, dtype), _dev(wn, dtype), pool, labels, mask, 20, 9, 2, rows, fill=-1)


@pytest.mark.parametrize("tier", TIERS)
def test_repeats_splits_and_tile_placement(tier):
    from recguru_amd import hip
    dtype = _set_tier(tier)
    hn, wn, pool, labels, rows, mask = list_case()
    B, L, k, skip = 8, 20, 9, 2
    base, bs = invariance_results(hip, tier, dtype)
    again, as_ = invariance_results(hip, tier, dtype)
    assert np.array_equal(base, again) and np.array_equal(bs.view(np.int32), as_.view(np.int32))
    table = _dev(wn, dtype)
    # the batch split along B
    for cut in (1, 3):
        parts = []
        for lo, hi in ((0, cut), (cut, B)):
            s = slice(lo * L, hi * L)
            parts.append(_call(hip, _dev(hn[s], dtype), table, pool, labels[s], mask[s], L, k, skip, rows[lo:hi], fill=-1))
        assert np.array_equal(np.concatenate([p[0] for p in parts]), base), (tier, cut)
        assert np.array_equal(np.concatenate([p[1] for p in parts]).view(np.int32), bs.view(np.int32)), (tier, cut)
    # every sequence left-padded by 3 more dead positions: its positions sit in other tiles, at other rows of them
    L2 = L + 3
    pad = lambda x, fill: np.concatenate([np.full((B, 3) + x.shape[1:], fill, dtype=x.dtype), x.reshape((B, L) + x.shape[1:])], axis=1)
    h2 = pad(hn, 1.5).reshape(B * L2, -1)
    got, gs = _call(hip, _dev(h2, dtype), table, pool, pad(labels, 5).reshape(-1), pad(mask, 0).reshape(-1), L2, k, skip, rows, fill=-1)
    keep = np.tile(np.arange(L2) >= 3, B)
    assert np.array_equal(got[keep], base) and np.array_equal(gs[keep].view(np.int32), bs.view(np.int32))
    assert np.all(got[~keep] == -1)


def _worker(tmp_path, mode):
    out = str(tmp_path / ("hn_%s.npz" % mode))
    env = dict(os.environ, PYTHONPATH=os.path.dirname(HERE), RG_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "hard_negs_worker.py"), mode, out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-4000:]
    z = np.load(out)
    assert int(z["det_enabled"]) > 0
    return z


def test_deterministic_library_gives_the_same_bits(tmp_path):
    from recguru_amd import hip
    z = _worker(tmp_path, "kernel")
    for tier in TIERS:
        dtype = _set_tier(tier)
        ids, sc = invariance_results(hip, tier, dtype)
        assert np.array_equal(z[tier + ".ids"], ids) and np.array_equal(z[tier + ".scores"].view(np.int32), sc.view(np.int32)), tier


# ---------------------------------------------------------------------------------------------------------------------
# 5. through the models (the deterministic library, one child process: tests/hard_negs_worker.py `models`)
# ---------------------------------------------------------------------------------------------------------------------
def test_models_take_hard_negatives(tmp_path):
    """Loss and every parameter gradient with n_items = HardNegatives(...) equal, bit for bit in the deterministic library, the run
    where hip.hard_negs is called by hand on the same h and the plain tensor is passed; with k_hard < k the other columns are the
    private draw; no hard negative of a live position is its label or an id of its sequence's exclusion row."""
    z = _worker(tmp_path, "models")
    runs = sorted(set(k.split("|")[0] for k in z.files if "|" in k))
    assert len(runs) == 3 * 5, runs                            # three tiers x (cross recon, cross bpr, single recon, MyRec bpr, k_hard < k)
    for run in runs:
        assert np.array_equal(z[run + "|loss.hard"].view(np.int32), z[run + "|loss.plain"].view(np.int32)), run
        grads = [k for k in z.files if k.startswith(run + "|g.hard.")]
        assert len(grads) > 10
        for g in grads:
            a, b = z[g], z[g.replace("|g.hard.", "|g.plain.")]
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), g
        neg, priv, labels, mask = z[run + "|neg"], z[run + "|private"], z[run + "|labels"], z[run + "|mask"]
        k_hard, L = int(z[run + "|k_hard"]), int(z[run + "|L"])
        live = mask != 0
        assert live.any() and np.array_equal(neg[:, k_hard:], priv[:, k_hard:]), run
        assert np.array_equal(neg[~live], priv[~live]), run
        # the worker's private draw avoids the pool: a hard column is a pool member exactly where the kernel wrote it
        ex, lo, hi, pool = z[run + "|excl"], z[run + "|excl_lo"], z[run + "|excl_hi"], z[run + "|pool"]
        assert not np.isin(priv, pool).any() and not np.isin(neg[:, k_hard:], pool).any() and not np.isin(neg[~live], pool).any()
        written = 0
        for t in np.flatnonzero(live):
            w = neg[t, :k_hard][np.isin(neg[t, :k_hard], pool)]
            written += len(w)
            assert labels[t] not in w and not np.isin(w, ex[lo[t // L]:hi[t // L]]).any(), (run, t)
            assert len(set(w.tolist())) == len(w)
        assert written > live.sum(), run


# ---------------------------------------------------------------------------------------------------------------------
# 6. the loader
# ---------------------------------------------------------------------------------------------------------------------
def _domain():
    from recguru_amd import sampler
    rng = np.random.default_rng(7600)
    V = 900
    seqs = [rng.choice(np.arange(1, V + 1), size=int(rng.integers(3, 14)), replace=False).tolist() for _ in range(24)]
    val = rng.integers(1, V + 1, size=24).tolist()
    test = rng.integers(1, V + 1, size=24).tolist()
    return sampler.DeviceDomain(seqs, val, test, V, "cuda"), V


def test_loader_yields_hard_negatives():
    from recguru_amd import sampler
    from recguru_amd.models import HardNegatives
    dom, V = _domain()
    L, k = 12, 5
    mk = lambda **kw: sampler.DeviceLoader(dom, 8, L, L, V + 1, L * k, seed=3, shuffle=False, **kw)
    plain = list(mk())
    hard = list(mk(hard_negs=257, hard_k=3, hard_skip=2))
    assert len(plain) == len(hard) == 3
    pools = []
    for i, ((seqs, n_items, val, test), (seqs0, n0, val0, test0)) in enumerate(zip(hard, plain)):
        assert isinstance(n_items, HardNegatives) and (n_items.k_hard, n_items.skip) == (3, 2)
        assert torch.is_tensor(n0) and torch.equal(n_items.private, n0)           # the private draw is what it was
        assert all(torch.equal(a, b) for a, b in zip(seqs, seqs0)) and torch.equal(val, val0) and torch.equal(test, test0)
        pool = n_items.pool.cpu().numpy()
        assert pool.ndim == 1 and 1 <= len(pool) <= 257 and np.all(np.diff(pool) > 0) and pool.min() >= 1 and pool.max() <= V
        users = torch.arange(i * 8, (i + 1) * 8, device="cuda")
        assert n_items.excl.data_ptr() == dom.excl.data_ptr()                      # the values are not copied
        assert torch.equal(n_items.excl_lo, dom.excl_off[users]) and torch.equal(n_items.excl_hi, dom.excl_off[users + 1])
        pools.append(pool)
    assert not np.array_equal(pools[0], pools[1])
    # hard_k None: all k; another rank draws another pool; the pool is not the shared-candidates draw of the batch seed itself
    other = next(iter(sampler.DeviceLoader(dom, 4, L, L, V + 1, L * k, seed=3, shuffle=False, rank=1, world=2, hard_negs=257)))[1]
    mine = next(iter(sampler.DeviceLoader(dom, 4, L, L, V + 1, L * k, seed=3, shuffle=False, rank=0, world=2, hard_negs=257)))[1]
    assert other.k_hard == k and not np.array_equal(other.pool.cpu().numpy(), mine.pool.cpu().numpy())
    shared = next(iter(mk(shared_negs=257)))[1]
    assert not np.array_equal(shared.cpu().numpy(), pools[0])
    # and the whole thing feeds the kernel
    from recguru_amd import hip
    _set_tier("f32")
    seqs, n_items, _, _ = hard[0]
    rng = np.random.default_rng(1)
    h = _dev(rng.normal(size=(8 * L, 64)).astype(np.float32))
    table = _dev(rng.normal(size=(V + 2, 64)).astype(np.float32))
    mask = (seqs[2] != 0).float().reshape(-1)
    out, _ = hip.hard_negs(h, table, n_items.pool, seqs[2].reshape(-1), mask, L, 3, skip=2, excl=n_items.excl, excl_lo=n_items.excl_lo,
                           excl_hi=n_items.excl_hi, checked=True)
    out = out.cpu().numpy()
    ex, lo, hi = dom.excl.cpu().numpy(), n_items.excl_lo.cpu().numpy(), n_items.excl_hi.cpu().numpy()
    for t in np.flatnonzero(mask.cpu().numpy()):
        assert np.all(out[t] >= 1) and not np.isin(out[t], ex[lo[t // L]:hi[t // L]]).any() and int(seqs[2].reshape(-1)[t]) not in out[t]


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------------
def _raw(hip, dtype_code=None, **kw):
    """rg_hard_negs itself on a small valid call with fields overridden -> (rc, message, out after the call)"""
    n, L, d, C, k = 34, 17, 64, 40, 4
    t = {"h": torch.ones(n, d, device="cuda"), "table": torch.ones(100, d, device="cuda"), "pool": torch.arange(1, C + 1, device="cuda"),
         "labels": torch.zeros(n, dtype=torch.int64, device="cuda"), "mask": torch.ones(n, device="cuda"),
         "out": torch.full((n, 8), SENT, dtype=torch.int64, device="cuda"), "excl": torch.arange(5, device="cuda"),
         "lo": torch.zeros(2, dtype=torch.int64, device="cuda"), "hi": torch.zeros(2, dtype=torch.int64, device="cuda")}
    live = hip.live_tiles(t["mask"], n)
    f = dict(h=t["h"].data_ptr(), table=t["table"].data_ptr(), table_rows=100, pool=t["pool"].data_ptr(), C=C, labels=t["labels"].data_ptr(),
             mask=t["mask"].data_ptr(), live16=live.data_ptr(), excl=None, excl_lo=None, excl_hi=None, out=t["out"].data_ptr(),
             out_scores=None, n=n, L=L, d=d, k=k, skip=0, ld_out=8, checked=1)
    for name, v in kw.items():
        f[name] = t[v].data_ptr() if isinstance(v, str) else v
    a = hip.HardNegsArgs(**f)
    torch.cuda.synchronize()
    rc = hip.lib().rg_hard_negs(ctypes.byref(a), hip.X3 if dtype_code is None else dtype_code, hip._stream())
    torch.cuda.synchronize()
    return rc, hip.lib().rg_last_error().decode(), t["out"].cpu().numpy()


UNSUPPORTED = [(dict(d=96), "d must be"), (dict(k=0), "k must be"), (dict(skip=-1), "skip must not"), (dict(skip=125), "skip \\+ k"),
               (dict(k=129, ld_out=129), "skip \\+ k"), (dict(C=0), "C must be"), (dict(C=2 ** 31), "C must be"),
               (dict(table_rows=2 ** 31), "table_rows"), (dict(n=2 ** 31 + 16, L=1), "n must be")]
INVALID = [(dict(L=0), "L must be"), (dict(L=16), "multiple of L"), (dict(ld_out=3), "ld_out"), (dict(h=None), "required"),
           (dict(table=None), "required"), (dict(pool=None), "required"), (dict(labels=None), "required"), (dict(mask=None), "required"),
           (dict(live16=None), "required"), (dict(out=None), "required"), (dict(excl="excl"), "excl_lo"),
           (dict(excl="excl", excl_lo="lo"), "excl_lo"), (dict(excl="excl", excl_hi="hi"), "excl_lo")]


def test_refusals_come_before_any_launch():
    import re
    from recguru_amd import hip
    RG_ERR_INVALID, RG_ERR_UNSUPPORTED = _err_codes()
    rc, _, out = _raw(hip)
    assert rc == 0 and np.all(out[:, :4] >= 1) and np.all(out[:, 4:] == SENT)          # the unchanged call works
    for code, cases in ((RG_ERR_UNSUPPORTED, UNSUPPORTED), (RG_ERR_INVALID, INVALID)):
        for kw, text in cases:
            rc, msg, out = _raw(hip, **kw)
            assert rc == code and re.search(text, msg) and msg.startswith("hard_negs:"), (kw, rc, msg)
            assert np.all(out == SENT), kw
    for dt in (hip.F32, 7):
        rc, msg, out = _raw(hip, dtype_code=dt)
        assert rc == RG_ERR_UNSUPPORTED and "dtype" in msg and np.all(out == SENT)
    rc, _, out = _raw(hip, n=0)                                                       # nothing to do is no error
    assert rc == 0 and np.all(out == SENT)


def _err_codes():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "recguru_hip.h")).read()
    import re
    return tuple(int(re.search(r"#define\s+%s\s+\(?(-?\d+)" % nm, hdr).group(1)) for nm in ("RG_ERR_INVALID", "RG_ERR_UNSUPPORTED"))


def test_bad_pools():
    from recguru_amd import hip
    _set_tier("f32")
    rng = np.random.default_rng(7700)
    n, L, d, T = 40, 20, 64, 500
    h, table = _dev(rng.normal(size=(n, d)).astype(np.float32)), _dev(rng.normal(size=(T, d)).astype(np.float32))
    labels, mask = np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.float32)
    good = np.arange(3, 103, dtype=np.int64)
    unsorted = good.copy()
    unsorted[[30, 31]] = unsorted[[31, 30]]
    dup = good.copy()
    dup[50] = dup[49]
    outside = good.copy()
    outside[70:] += T
    negative = good.copy()
    negative[0] = -4
    huge = good.copy()
    huge[99] = 2 ** 32 + 5                                      # its low 32 bits are a table row
    for pool, text in ((unsorted, r"ascending \(pool\[31\] = 33 after 34\)"), (dup, r"ascending \(pool\[50\] = 52 after 52\)"),
                       (outside, r"pool\[70\] = 573 is outside the table rows \[0, 500\)"), (negative, r"pool\[0\] = -4 is outside"),
                       (huge, r"pool\[99\] = 4294967301 is outside")):
        out = torch.full((n, 6), SENT, dtype=torch.int64, device="cuda")
        with pytest.raises(RuntimeError, match=text):
            hip.hard_negs(h, table, _dev(pool), _dev(labels), _dev(mask), L, 6, out=out)
        assert torch.all(out == SENT)
        # the same pool under checked=True: a valid-input contract, but no id outside the table comes back and nothing faults
        got, sc = _call(hip, h, table, pool, labels, mask, L, 6, 0, checked=True)
        assert np.all((got >= 0) & (got < T)), text
        assert np.all(np.isin(got, pool[(pool >= 0) & (pool < T)]))
    # every id outside: nothing eligible, nothing written
    got, sc = _call(hip, h, table, good + T, labels, mask, L, 6, 0, checked=True)
    assert np.all(got == SENT) and np.all(np.isneginf(sc))


def test_shared_list_still_refuses_bpr_and_means_shared_logits():
    from recguru_amd.models import SharedLogits
    s = SharedLogits(None, None, None, torch.arange(4))
    with pytest.raises(NotImplementedError):
        s.bpr(None)
