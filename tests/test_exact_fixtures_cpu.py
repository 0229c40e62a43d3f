"""The conditions under which tests/test_exact_gemm_gpu.py may demand bit-for-bit equality, proved on the references themselves
(no GPU): every partial sum below 2^24, every reference value representable in its output dtype, no zero product in the dense
fixture, GELU the identity on the prologue fixture -- zero exceptions each -- and the float32 restatements of the GELU forms
held to the deviations recorded in exact_util.DELTA."""
import math

import pytest
import torch

import exact_util as E

NT_KINDS = ["nt", "nt_gelu_grad", "ws", "ws_drop_gelu", "ws_gelu_grad"]
NT_IDS = [(k, i) for k in NT_KINDS for i in range(len(E.CASES[k]))]
TN_IDS = [(k, i) for k in ("tn", "tn_big") for i in range(len(E.CASES[k]))]


def _out_dtypes(c):
    """Output dtypes a case is run with: f32 where it asks for it (and in the f32 / bf16x3 tiers), bf16 in the bf16 tier."""
    return [torch.float32] if c["out_f32"] else [torch.float32, torch.bfloat16]


def _integers(t):
    return bool((t == t.round()).all())


@pytest.mark.parametrize("kind,idx", NT_IDS, ids=["%s-%s" % (k, E.case_id(E.CASES[k][i])) for k, i in NT_IDS])
def test_gemm_nt_fixture_conditions(kind, idx):
    c = E.CASES[kind][idx]
    f = E.fixture(kind, idx)
    assert f["bound"] < E.LIMIT
    # operands: integers bf16 holds exactly (bf16x3: lo half 0); aux of the GELU' cases: quarters, exact in bf16 too
    for name in ("A", "W", "bias", "aux"):
        t = f[name]
        if t is None:
            continue
        assert torch.equal(t, t.bfloat16().double()), name
        if not (name == "aux" and c["epi"] == "gelu_grad"):
            assert _integers(t), name
    if f["dense"]:
        assert int((f["A"] == 0).sum()) == 0 and int((f["W"] == 0).sum()) == 0           # no product is zero
    if c["fix"] == "selector":
        assert bool(((f["A"] != 0).sum(1) == 1).all())
        assert len(set((f["A"] != 0).double().argmax(1).tolist())) == c["K"]              # k(m) covers every k
    if c["pro"] == "gelu":
        assert set(f["A"].unique().tolist()) <= set(E.GELU_VALUES)
    assert float(f["acc"].abs().max()) <= f["bound"]
    for dt in _out_dtypes(c):
        if c["epi"] == "gelu_grad":
            continue                                         # inexact by nature: held to a tolerance, the accumulator is exact
        E.exact_cast(f["ref"], dt, E.case_id(c))


@pytest.mark.parametrize("kind,idx", TN_IDS, ids=["%s-%s" % (k, E.case_id(E.CASES[k][i])) for k, i in TN_IDS])
def test_gemm_tn_fixture_conditions(kind, idx):
    c = E.CASES[kind][idx]
    f = E.fixture(kind, idx)
    _check_tn(c, f)


def _check_tn(c, f):
    assert f["bound"] < E.LIMIT
    for name in ("Y", "X", "dW0"):
        assert _integers(f[name]) and torch.equal(f[name], f[name].bfloat16().double()), name
    assert math.log2(abs(c["scale"])) == round(math.log2(abs(c["scale"])))
    if f["dense"]:
        assert int((f["Y"] == 0).sum()) == 0 and int((f["X"] == 0).sum()) == 0
    if c["fix"] == "gelu":
        assert set(f["X"].unique().tolist()) <= set(E.GELU_VALUES)
    if c["fix"] == "selector":
        assert bool(((f["Y"] != 0).sum(1) == 1).all())
        assert len(set((f["Y"] != 0).double().argmax(1).tolist())) == min(c["N1"], c["T"])
    if c["colsum_rows"] > 0:
        assert c["colsum_rows"] % 32 != 0 and c["colsum_rows"] < c["T"]                   # strictly inside a 32-row step
    if c["listed"]:
        live = E.live_rows(f["mask"])
        assert 0 < int(live.sum()) < c["T"] and int((f["Y"][~live] == 0).sum()) == 0      # dead rows exist and hold nonzero values
    assert float(f["ref"].abs().max()) <= f["bound"] and float(f["cs_ref"].abs().max()) <= f["bound"]
    E.exact_cast(f["ref"], torch.float32, E.case_id(c))
    E.exact_cast(f["cs_ref"], torch.float32, E.case_id(c))


@pytest.mark.parametrize("listed", [False, True])
@pytest.mark.parametrize("present", E.LAYER_PRESENT)
def test_gemm_tn_layer_fixture_conditions(present, listed):
    for i, f in enumerate(E.fixture("layer", (present, listed))):
        assert (f is None) == (not present[i])
        if f is not None:
            N1, N2, gelu = E.LAYER_SHAPES[i]
            _check_tn(E.tn(E.LAYER_T, N1, N2, fix="gelu" if gelu else "dense", listed=listed and i != 2), f)


@pytest.mark.parametrize("K,N,epi,mode", E.WS_LIVE_CASES)
def test_live_list_fixture_of_the_weight_stationary_cases(K, N, epi, mode):
    mask = E.seq_mask(E.WS_LIVE_M, E.WS_LIVE_L, 5)
    live = E.live_rows(mask)
    assert 0 < int(live.sum()) < E.WS_LIVE_M
    assert bool((live[mask != 0]).all())
    assert mode != 2 or epi == "none"                        # the bias row is promised to EPI_NONE only
    f = E.build_nt(E.ws(E.WS_LIVE_M, K, N, epi, epi_scale=0.5, seed=40 + mode))
    assert f["bound"] < E.LIMIT and int((f["A"] == 0).sum()) == 0
    for dt in (torch.float32, torch.bfloat16):
        E.exact_cast(f["ref"], dt, "live list")
        E.exact_cast(f["bias"], dt, "bias row")


@pytest.mark.parametrize("M,L", E.WS_HEADMAJOR_CASES)
def test_head_major_fixture(M, L):
    assert M >= 4096 and M % L == 0 and L >= 16
    A, W, bias = E.nonzero_ints((M, 128), 1, 71), E.nonzero_ints((384, 128), 1, 72), E.small_ints((384,), 3, 73, step=2)
    E.exact_cast(A @ W.t() + bias, torch.bfloat16, "head-major")


def test_gelu_is_the_identity_on_the_prologue_values():
    """float64 GELU of 0, 8, 16 rounds to the value in bf16 and in f32, and so do the two device forms (float32 restatements)."""
    x = torch.tensor(E.GELU_VALUES, dtype=torch.float64)
    g = E.gelu64(x)
    assert torch.equal(g.float().double(), x) and torch.equal(g.bfloat16().double(), x)
    assert torch.equal(E.gelu_fast32(x).double(), x)
    xf = x.float()
    tanh_form = 0.5 * xf * (1.0 + torch.tanh(torch.tensor(0.7978845608028654, dtype=torch.float32) * (xf + 0.044715 * xf * xf * xf)))
    assert torch.equal(tanh_form.double(), x)


def test_restatements_stay_inside_the_recorded_deviation():
    """exact_util.DELTA is what the GPU test multiplies by 4: the measured deviation of the float32 restatements from float64,
    rounded up -- never below the measurement, and not a loose multiple of it either."""
    got = E.measure_delta()
    for k, v in got.items():
        assert 0.5 * E.DELTA[k] <= v <= E.DELTA[k], (k, v, E.DELTA[k])


def test_half_ulp():
    one = torch.tensor([1.0, 1.5, 2.0, 0.0, 300.0], dtype=torch.float64)
    assert E.half_ulp(one, torch.float32).tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -23, 0.0, 2.0 ** -16]
    assert E.half_ulp(one, torch.bfloat16).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 0.0, 1.0]
