"""The MFMA GEMM family held to integer fixtures BIT FOR BIT, in the bf16, bf16x3 and f32 tiers (tests/exact_util.py says why
that is possible and lists the cases; tests/test_exact_fixtures_cpu.py proves the fixtures' conditions without a GPU).

Every case asserts, through rg_gemm_nt_plan / rg_gemm_tn_plan on the very arguments that are launched, that the kernel it means
to test is the one that runs: a case that fell back to the generic kernel would prove nothing.  The two epilogues that cannot be
exact (GELU', and the GELU output of DROP_GELU) run on the same fixtures: their accumulator is then known exactly and the only
error left is the function's own, bounded by 4 x the deviation of a float32 restatement (exact_util.DELTA)."""
import contextlib
import ctypes

import pytest
import torch

import exact_util as E

pytestmark = pytest.mark.gpu

TIER_NAME = {"bf16": "bf16", "bf16x3": "x3", "f32": "f32"}
WS_TIERS = ["bf16", "bf16x3"]          # the weight-stationary and whole-tile kernels exist in these two tiers


@contextlib.contextmanager
def tier(name):
    """Switch tiers the way tests/test_x3_gpu.py does: f32 storage + hip.SPLIT_OPERANDS for bf16x3."""
    from recguru_amd import hip
    prev, hip.SPLIT_OPERANDS = hip.SPLIT_OPERANDS, name == "bf16x3"
    try:
        yield hip, E.storage_dtype(name)
    finally:
        hip.SPLIT_OPERANDS = prev


@contextlib.contextmanager
def plans(entry):
    """While active, every call of the library's `entry` (rg_gemm_nt / rg_gemm_tn) made by recguru_amd.hip first asks
    `entry`_plan for the kernel these very arguments launch; yields the list of names."""
    from recguru_amd import hip
    L = hip.lib()
    real, plan, names = getattr(L, entry), getattr(L, entry + "_plan"), []

    def spy(a, dt, stream):
        buf = ctypes.create_string_buffer(128)
        assert plan(a, dt, buf, 128) == 0
        names.append(buf.value.decode())
        return real(a, dt, stream)

    setattr(L, entry, spy)
    try:
        yield names
    finally:
        setattr(L, entry, real)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def assert_bits(out, ref, what):
    """out (GPU) == ref (CPU, already in the output dtype) bit for bit; on failure the count and the first few indices."""
    out = out.detach().cpu()
    assert out.shape == ref.shape and out.dtype == ref.dtype, "%s: %s %s vs %s %s" % (what, out.shape, out.dtype, ref.shape, ref.dtype)
    ne = _bits(out.contiguous()) != _bits(ref.contiguous())
    if bool(ne.any()):
        idx = ne.nonzero()
        first = ", ".join("%s got %r want %r" % (tuple(i.tolist()), float(out[tuple(i.tolist())]), float(ref[tuple(i.tolist())])) for i in idx[:6])
        raise AssertionError("%s: %d of %d elements differ; first: %s" % (what, idx.shape[0], ne.numel(), first))


def assert_within(out, ref, bound, what):
    err = (out.detach().cpu().double() - ref).abs()
    bad = err > bound
    if bool(bad.any()):
        idx = bad.nonzero()
        first = ", ".join("%s err %.3g bound %.3g" % (tuple(i.tolist()), float(err[tuple(i.tolist())]), float(bound[tuple(i.tolist())])) for i in idx[:6])
        raise AssertionError("%s: %d of %d elements outside the bound; first: %s" % (what, idx.shape[0], bad.numel(), first))
    print("%s: largest error / bound = %.3g" % (what, float((err / bound.clamp_min(1e-300)).max())))


def _dev(t, dt):
    return None if t is None else t.to(dt).cuda()


SENTINEL = 768.0          # exact in bf16


def _nt_call(hip, dt, c, f, generic, out=None, **kw):
    """Run case c in the current tier; returns (C, the wider tensor C is a slice of or None, kernel names)."""
    EPI = {"none": hip.EPI_NONE, "add": hip.EPI_ADD, "relu": hip.EPI_RELU, "posmask": hip.EPI_MUL_POSMASK, "gelu_grad": hip.EPI_GELU_GRAD,
           "drop_gelu": hip.EPI_DROP_GELU}
    M, N, K = c["M"], c["N"], c["K"]
    odt = torch.float32 if c["out_f32"] else dt
    A, W, bias, aux = _dev(f["A"], dt), _dev(f["W"], dt), _dev(f["bias"], torch.float32), _dev(f["aux"], dt)
    wide = None
    if c["layout"] == "slices":                    # leading dimensions multiples of 8, column offsets too (16-byte vectors)
        Aw = torch.full((M, K + 24), 3.0, device="cuda", dtype=dt)
        Aw[:, 8:8 + K] = A
        A = Aw[:, 8:8 + K]
        xw = torch.full((M, N + 16), 5.0, device="cuda", dtype=dt)
        xw[:, 8:8 + N] = aux
        aux = xw[:, 8:8 + N]
        wide = torch.full((M, N + 24), SENTINEL, device="cuda", dtype=odt)
        out = wide[:, 16:16 + N]
    elif c["layout"] == "ldc_odd":                 # ldc = N + 4
        wide = torch.full((M, N + 4), SENTINEL, device="cuda", dtype=odt)
        out = wide[:, :N]
    if aux is None and c["epi"] == "relu" and not generic:
        aux = torch.zeros(M, N, device="cuda", dtype=dt)          # the bf16 weight-stationary form wants an aux pointer for every epilogue; ReLU ignores it
    with plans("rg_gemm_nt") as names:
        C = hip.gemm_nt(A, W, bias, out=out, out_f32=c["out_f32"], prologue=hip.PRO_GELU if c["pro"] == "gelu" else hip.PRO_NONE,
                        epilogue=EPI[c["epi"]], aux=aux, debug_ablate=16 if generic else 0, epi_scale=c["epi_scale"],
                        epi_nonzero_scale=c["nz"], drop_p=c["drop_p"], drop_seed=E.DROP_SEED, **kw)
    torch.cuda.synchronize()
    return C, wide, names


def _untouched(wide, c):
    """The columns of the wider output tensor beside C still hold the sentinel."""
    w = wide.detach().cpu().float()
    lo, hi = (16, 16 + c["N"]) if c["layout"] == "slices" else (0, c["N"])
    assert bool((w[:, :lo] == SENTINEL).all()) and bool((w[:, hi:] == SENTINEL).all()), "stores outside C"


def _nt_name(t, N):
    return "gemm_nt_kernel<%s,%d>" % (TIER_NAME[t], 1 if N <= 64 else 2)


def _ws_name(t, K, N):
    code = E.ws_code(t, K, N)
    return "gemm_ws_kernel<%d,%d>" % (code // 10, code % 10)


def _ids(kind):
    return [E.case_id(c) for c in E.CASES[kind]]


# ------------------------------------------------------------------------------------------------ gemm_nt, generic tile kernel
@pytest.mark.parametrize("idx", range(len(E.NT_GENERIC_CASES)), ids=_ids("nt"))
@pytest.mark.parametrize("t", E.TIERS)
def test_gemm_nt_generic_bitwise(idx, t):
    c, f = E.NT_GENERIC_CASES[idx], E.fixture("nt", idx)
    with tier(t) as (hip, dt):
        C, wide, names = _nt_call(hip, dt, c, f, generic=True)
        assert names == [_nt_name(t, c["N"])], names
        ref = E.exact_cast(f["ref"], C.dtype, E.case_id(c))
        assert_bits(C, ref, "gemm_nt %s [%s] %s" % (E.case_id(c), t, names[0]))
        if wide is not None:
            _untouched(wide, c)


def _gelu_grad_check(C, c, f, delta, what):
    g = E.gelu_grad64(f["aux"])
    acc = f["acc"]
    if c["nz"] > 0:
        acc = acc * c["nz"]
        g = g * (f["aux"] != 0)
    ref = acc * g
    assert_within(C, ref, E.inexact_bound(acc, ref, delta, C.dtype), what)
    if c["nz"] > 0:
        assert float(C.detach().cpu().double()[f["aux"] == 0].abs().max()) == 0.0, "%s: aux == 0 must give exactly 0" % what


@pytest.mark.parametrize("idx", range(len(E.NT_GENERIC_GELU_GRAD_CASES)), ids=_ids("nt_gelu_grad"))
@pytest.mark.parametrize("t", E.TIERS)
def test_gemm_nt_generic_gelu_grad_on_an_exact_accumulator(idx, t):
    """EPI_GELU_GRAD (with epi_nonzero_scale) through the vector epilogue, the scalar one (N = 203) and an unaligned ldc: the
    scalar path used to ignore epi_nonzero_scale (unscaled gradients, also where aux == 0).
    Allowed: |acc| * 4 delta + half an ulp, delta = exact_util.DELTA (9.04e-07 measured for the exp2 / rcp form of the bf16 and
    bf16x3 tiers, 1.92e-07 for the tanhf form of the f32 tier)."""
    c, f = E.NT_GENERIC_GELU_GRAD_CASES[idx], E.fixture("nt_gelu_grad", idx)
    with tier(t) as (hip, dt):
        C, wide, names = _nt_call(hip, dt, c, f, generic=True)
        assert names == [_nt_name(t, c["N"])], names
        _gelu_grad_check(C, c, f, E.DELTA["gelu_grad_tanhf" if t == "f32" else "gelu_grad_fast"], "gemm_nt %s [%s]" % (E.case_id(c), t))
        if wide is not None:
            _untouched(wide, c)


# ------------------------------------------------------------------------------------------- gemm_nt, weight-stationary kernel
@pytest.mark.parametrize("idx", range(len(E.WS_CASES)), ids=_ids("ws"))
@pytest.mark.parametrize("t", WS_TIERS)
def test_gemm_ws_bitwise(idx, t, monkeypatch):
    c, f = E.WS_CASES[idx], E.fixture("ws", idx)
    with tier(t) as (hip, dt):
        # bf16x3 at K = 256: the wrapper hands the weights over presplit (the WP = 1 / 2 forms); the in-kernel split is run as well
        for presplit in ((True, False) if (t == "bf16x3" and c["K"] == 256) else (True,)):
            monkeypatch.setattr(hip, "PRESPLIT_WS_X3", presplit)
            C, _, names = _nt_call(hip, dt, c, f, generic=False)
            assert names == [_ws_name(t, c["K"], c["N"])], names
            assert_bits(C, E.exact_cast(f["ref"], C.dtype, E.case_id(c)), "gemm_ws %s [%s] %s presplit=%s" % (E.case_id(c), t, names[0], presplit))


@pytest.mark.parametrize("idx", range(len(E.WS_DROP_GELU_CASES)), ids=_ids("ws_drop_gelu"))
@pytest.mark.parametrize("t", WS_TIERS)
def test_gemm_ws_drop_gelu(idx, t):
    """EPI_DROP_GELU: C = dropout(acc + bias) bit for bit (the factor 2 of p = 0.5 is exact; mask of tests/dropmask.py); the
    second output against float64 gelu(C): |C| * 4 delta + half an ulp, delta = 6.83e-08 measured for the factor sigmoid(2u)."""
    c, f = E.WS_DROP_GELU_CASES[idx], E.fixture("ws_drop_gelu", idx)
    with tier(t) as (hip, dt):
        C2 = torch.full((c["M"], c["N"]), float("nan"), device="cuda", dtype=dt)
        C, _, names = _nt_call(hip, dt, c, f, generic=False, out2=C2)
        assert names == [_ws_name(t, c["K"], c["N"])], names
        what = "gemm_ws %s [%s]" % (E.case_id(c), t)
        assert_bits(C, E.exact_cast(f["ref"], C.dtype, what), what + " C")
        assert float(f["ref"].abs().max()) <= 512                       # the range exact_util.measure_delta covers
        ref2 = E.gelu64(f["ref"])
        assert_within(C2, ref2, E.inexact_bound(f["ref"], ref2, E.DELTA["gelu_fast"], C2.dtype), what + " gelu(C)")


@pytest.mark.parametrize("idx", range(len(E.WS_GELU_GRAD_CASES)), ids=_ids("ws_gelu_grad"))
@pytest.mark.parametrize("t", WS_TIERS)
def test_gemm_ws_gelu_grad_on_an_exact_accumulator(idx, t):
    c, f = E.WS_GELU_GRAD_CASES[idx], E.fixture("ws_gelu_grad", idx)
    with tier(t) as (hip, dt):
        C, _, names = _nt_call(hip, dt, c, f, generic=False)
        assert names == [_ws_name(t, c["K"], c["N"])], names
        _gelu_grad_check(C, c, f, E.DELTA["gelu_grad_fast"], "gemm_ws %s [%s]" % (E.case_id(c), t))


@pytest.mark.parametrize("M,L", E.WS_HEADMAJOR_CASES)
def test_gemm_ws_head_major_bitwise(M, L):
    """headmajor_L (bf16, N = 384): C leaves as q | k | v [3, M / L, 4, L, 32]; L = 24 makes 16-row tiles span two sequences."""
    from recguru_amd import hip
    K, N, dt = 128, 384, torch.bfloat16
    A, W, bias = E.nonzero_ints((M, K), 1, 71), E.nonzero_ints((N, K), 1, 72), E.small_ints((N,), 3, 73, step=2)
    ref = (A @ W.t() + bias).view(M // L, L, 3, 4, 32).permute(2, 0, 3, 1, 4).contiguous()
    with plans("rg_gemm_nt") as names:
        C = hip.gemm_nt(_dev(A, dt), _dev(W, dt), _dev(bias, torch.float32), headmajor_L=L)
    torch.cuda.synchronize()
    assert names == ["gemm_ws_kernel<1,3>"], names
    assert_bits(C, E.exact_cast(ref, dt, "head-major"), "gemm_ws head-major M=%d L=%d" % (M, L))


@pytest.mark.parametrize("K,N,epi,mode", E.WS_LIVE_CASES)
@pytest.mark.parametrize("t", WS_TIERS)
def test_gemm_ws_live_tile_list_bitwise(K, N, epi, mode, t):
    """Rows of the listed 16-row tiles bit for bit; rows of the other tiles -- whose A and aux hold nonzero values that must
    never be read -- as the skip_dead_fill mode promises: zeros (0), untouched NaN poison (1), the bias row (2)."""
    M = E.WS_LIVE_M
    c = E.ws(M, K, N, epi, epi_scale=0.5, seed=40 + mode)
    f = E.build_nt(c)
    mask = E.seq_mask(M, E.WS_LIVE_L, 5)
    live = E.live_rows(mask)
    with tier(t) as (hip, dt):
        gmask = mask.cuda()
        lst = hip.live_tiles(gmask, M)
        out = torch.full((M, N), float("nan"), device="cuda", dtype=dt)
        C, _, names = _nt_call(hip, dt, c, f, generic=False, out=out, live=lst, skip_dead_fill=mode)
        assert names == [_ws_name(t, K, N)], names
        what = "gemm_ws live list %s mode %d [%s]" % (E.case_id(c), mode, t)
        ref = E.exact_cast(f["ref"], dt, what)
        assert_bits(C[live.cuda()], ref[live], what + " listed rows")
        dead = C[(~live).cuda()].detach().cpu()
        if mode == 1:
            assert bool(torch.isnan(dead).all()), what + ": a dead row was written"
        elif mode == 2:
            assert_bits(dead, f["bias"].to(dt)[None, :].expand_as(dead).contiguous(), what + " dead rows = bias")
        else:
            assert_bits(dead, torch.zeros_like(dead), what + " dead rows = 0")


# -------------------------------------------------------------------------------------------------------------------- gemm_tn
def _tn_call(hip, dt, c, f):
    Y, X = _dev(f["Y"], dt), _dev(f["X"], dt)
    dW = f["dW0"].float().cuda()
    cs = torch.zeros(c["N1"], device="cuda") if c["colsum"] else None
    gmask = f["mask"].cuda() if c["listed"] else None
    live = hip.live_tiles(gmask, c["T"]) if c["listed"] else None
    with plans("rg_gemm_tn") as names:
        hip.gemm_tn(Y, X, dW, cs, prologue_x=hip.PRO_GELU if c["fix"] == "gelu" else hip.PRO_NONE, scale=c["scale"], splits=c["splits"],
                    use_tr=c["use_tr"], live=live, partials=c["partials"], colsum_rows=c["colsum_rows"])
    torch.cuda.synchronize()
    return dW, cs, names


def _tn_check(dW, cs, c, f, what):
    assert_bits(dW, E.exact_cast(f["ref"], torch.float32, what), what + " dW")
    if cs is not None:
        assert_bits(cs, E.exact_cast(f["cs_ref"], torch.float32, what), what + " colsum")


@pytest.mark.parametrize("idx", range(len(E.TN_GENERIC_CASES)), ids=_ids("tn"))
@pytest.mark.parametrize("t", E.TIERS)
def test_gemm_tn_generic_bitwise(idx, t):
    c, f = E.TN_GENERIC_CASES[idx], E.fixture("tn", idx)
    with tier(t) as (hip, dt):
        dW, cs, names = _tn_call(hip, dt, c, f)
        assert names == ["gemm_tn_kernel<%s>" % TIER_NAME[t]], names
        _tn_check(dW, cs, c, f, "gemm_tn %s [%s]" % (E.case_id(c), t))


@pytest.mark.parametrize("idx", range(len(E.TN_BIG_CASES)), ids=_ids("tn_big"))
@pytest.mark.parametrize("t", WS_TIERS)
def test_gemm_tn_whole_tile_bitwise(idx, t):
    c, f = E.TN_BIG_CASES[idx], E.fixture("tn_big", idx)
    with tier(t) as (hip, dt):
        dW, cs, names = _tn_call(hip, dt, c, f)
        want = "gemm_tn_dma_kernel<%d,%d>" % (c["N1"], c["N2"]) if t == "bf16" else "gemm_tn_big_kernel<x3,%d,%d>" % (c["N1"], c["N2"])
        assert names == [want], names
        _tn_check(dW, cs, c, f, "gemm_tn %s [%s] %s" % (E.case_id(c), t, names[0]))


@pytest.mark.parametrize("present", E.LAYER_PRESENT)
@pytest.mark.parametrize("listed", [False, True])
@pytest.mark.parametrize("t", WS_TIERS)
def test_gemm_tn_layer_bitwise(present, listed, t, monkeypatch):
    """rg_gemm_tn_layer, slot 0 on the GELU-prologue fixture, with two different deals of the workgroups to the slots."""
    fx = E.fixture("layer", (present, listed))
    with tier(t) as (hip, dt):
        L = hip.lib()
        real, deals = L.rg_gemm_tn_layer, []

        def spy(args, wgs, code, stream):
            deals.append(tuple(wgs))
            return real(args, wgs, code, stream)

        monkeypatch.setattr(L, "rg_gemm_tn_layer", spy)
        for wgs_total, cost in ((hip.LAYER_WGS, hip.LAYER_COST), (120, {False: (0.5, 2.0, 1.0, 1.0), True: (0.5, 2.0, 1.0, 1.0)})):
            monkeypatch.setattr(hip, "LAYER_WGS", wgs_total)
            monkeypatch.setattr(hip, "LAYER_COST", cost)
            probs, outs, keep = [], [], []
            for i, f in enumerate(fx):
                if f is None:
                    probs.append(None)
                    outs.append(None)
                    continue
                N1 = E.LAYER_SHAPES[i][0]
                gmask = f["mask"].cuda() if f["mask"] is not None else None
                keep.append(gmask)
                live = hip.live_tiles(gmask, E.LAYER_T) if gmask is not None else None
                dW, cs = f["dW0"].float().cuda(), torch.zeros(N1, device="cuda")
                probs.append((_dev(f["Y"], dt), _dev(f["X"], dt), dW, cs, live))
                outs.append((dW, cs))
            assert hip.gemm_tn_layer(probs) is True, "rg_gemm_tn_layer refused the set: nothing was launched"
            torch.cuda.synchronize()
            for i, f in enumerate(fx):
                if f is not None:
                    what = "gemm_tn_layer slot %d present=%s listed=%s [%s] wgs=%s" % (i, present, listed, t, deals[-1])
                    assert_bits(outs[i][0], E.exact_cast(f["ref"], torch.float32, what), what + " dW")
                    assert_bits(outs[i][1], E.exact_cast(f["cs_ref"], torch.float32, what), what + " colsum")
        assert len(deals) == 2 and deals[0] != deals[1], deals
