"""Integer fixtures on which the MFMA GEMM family (rg_gemm_nt, rg_gemm_tn, rg_gemm_tn_layer) has to be right BIT FOR BIT, in the
bf16, bf16x3 and f32 tiers alike, and their float64 references.  CPU only: tests/test_exact_fixtures_cpu.py proves the conditions
below where there is no GPU, tests/test_exact_gemm_gpu.py runs the kernels.

Why no tolerance is needed.  bf16 holds the integers up to 256 exactly (bf16x3: the lo half of such an operand is 0), their
products are integers, and f32 adds integers exactly as long as every partial sum stays below 2^24.  Then EVERY order of
accumulation -- MFMA blocks, split-K atomics, partial-sum workspaces, persistent walkers -- gives the same bits, and one dropped
or repeated product moves an output by at least 1 (0.5 after scale = 0.5).  Scales are powers of two.

Three fixtures:
  dense     operands from a NONZERO integer alphabet ({+-1..+-8} where the output is f32, {+-1} where it is bf16), so no product is 0;
  selector  one nonzero (+-1, +-2) per row of A (of Y) at column k(m), against the asymmetric pattern (arange % 61) - 30 of
            test_gemm_nt_identity_asymmetric: C[m, n] = +-W[n, k(m)] names the (n, k) every output element read;
  gelu      X in {0, 8, 16}: tanh-GELU is the identity there to f32 precision (1 + exp2(-71) rounds to 1, tanhf(24.6) is 1), so
            the GELU prologues stay bit-exact.
The cases are data (the *_CASES lists): the CPU test checks each one's conditions, the GPU test runs each one, and a case's
fixture and reference are built once and shared by the tiers (fixture())."""
import functools
import math

import numpy as np
import torch

import dropmask

LIMIT = float(2 ** 24)
GELU_VALUES = (0.0, 8.0, 16.0)
TIERS = ("bf16", "bf16x3", "f32")


def storage_dtype(tier):
    return torch.bfloat16 if tier == "bf16" else torch.float32


# ---------------------------------------------------------------------------------------------------------------- raw draws
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(int(seed))


def nonzero_ints(shape, amax, seed):
    """float64 draws from {+-1 .. +-amax}."""
    g = _gen(seed)
    mag = torch.randint(1, amax + 1, shape, generator=g)
    sgn = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sgn).double()


def small_ints(shape, amax, seed, step=1):
    """float64 draws from step * {-amax .. amax} (zero included: masks need it)."""
    return (torch.randint(-amax, amax + 1, shape, generator=_gen(seed)) * step).double()


def gelu_ints(shape, seed):
    """float64 draws from GELU_VALUES."""
    return (torch.randint(0, 3, shape, generator=_gen(seed)) * 8).double()


def pattern(rows, cols):
    """The asymmetric integer pattern of test_gemm_nt_identity_asymmetric: (arange % 61) - 30."""
    return (torch.arange(rows * cols).reshape(rows, cols) % 61 - 30).double()


def selector(rows, cols):
    """[rows, cols] with ONE nonzero per row: +1, -1, +2, -2 (by row % 4) at column (37 row + 5) % cols; 37 is coprime to every
    width used here, so rows >= cols covers every column.  Returns (matrix, column of each row, value of each row)."""
    assert math.gcd(37, cols) == 1
    r = torch.arange(rows)
    col = (37 * r + 5) % cols
    val = torch.tensor([1.0, -1.0, 2.0, -2.0], dtype=torch.float64)[r % 4]
    m = torch.zeros(rows, cols, dtype=torch.float64)
    m[r, col] = val
    return m, col, val


def seq_mask(M, L, seed):
    """Left-padded row mask [M] (sequences of L positions, the last one cut), with an all-padding and a full sequence."""
    B = (M + L - 1) // L
    lens = torch.randint(0, L + 1, (B,), generator=_gen(seed))
    lens[0], lens[1] = 0, L
    return (torch.arange(L)[None, :] >= (L - lens)[:, None]).float().reshape(-1)[:M].contiguous()


def live_rows(mask):
    """bool [M]: rows of the 16-row tiles that hold a row with mask != 0 (what a live-tile list makes a kernel visit)."""
    M = mask.numel()
    pad = torch.nn.functional.pad(mask, (0, (-M) % 16))
    return (pad.view(-1, 16).sum(1) != 0).repeat_interleave(16)[:M]


# --------------------------------------------------------------------------------------------------------------- exactness
def exact_cast(ref, dt, what=""):
    """ref (float64) in the output dtype; raises unless EVERY value is representable there (the cap is zero exceptions)."""
    out = ref.to(dt)
    bad = int((out.double() != ref).sum())
    assert bad == 0, "%s: %d reference value(s) not representable in %s" % (what, bad, dt)
    return out


def gelu64(x):
    x = x.double()
    return 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_grad64(x):
    x = x.double()
    c = math.sqrt(2 / math.pi)
    t = torch.tanh(c * (x + 0.044715 * x ** 3))
    return 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * c * (1 + 3 * 0.044715 * x * x)


def sigmoid2u64(x):
    """gelu(x) / x = 0.5 (1 + tanh u) = sigmoid(2u): the factor the fast GELU multiplies x with."""
    x = x.double()
    return torch.sigmoid(2 * math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3))


# ---- float32 restatements of rg_common.hip.h gelu_t / gelu_grad_t, one f32 rounding per device operation ------------------
_f = np.float32
_C = _f(0.7978845608028654)
_K1 = _f(-2.0) * _f(1.4426950408889634) * _C
_K3 = _K1 * _f(0.044715)
_G1 = _f(6.0) * _f(0.044715) * _C
_G0 = _f(2.0) * _C


def _fma(a, b, c):
    """fmaf on float32 tensors: the product of two f32 is exact in float64, the sum is rounded once more on the way back (a
    double rounding in ~2^-29 of the cases, half an f32 ulp of an intermediate: far inside the 4x allowance)."""
    return (a.double() * b.double() + c.double()).float()


def _t(v):
    return torch.tensor(float(v), dtype=torch.float32)


def _sig_fast32(x):
    x = x.float()
    e = torch.exp2(x * _fma(x * x, _t(_K3), _t(_K1)))
    return 1.0 / (1.0 + e)


def gelu_fast32(x):
    """gelu_t<false>: x * rcp(1 + exp2(x * fma(x^2, k3, k1)))."""
    return x.float() * _sig_fast32(x)


def gelu_grad32(x, precise):
    """gelu_grad_t<PRECISE> in float32 torch: the tanhf form (f32 tier) or the exp2 / rcp form (bf16, bf16x3)."""
    x = x.float()
    x2 = x * x
    if precise:
        u = _t(_C) * (x + _t(_f(0.044715)) * x * x2)
        t = torch.tanh(u)
        return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * _t(_C) * (1.0 + _t(_f(3.0) * _f(0.044715)) * x2)
    sg = _sig_fast32(x)
    return _fma(x * sg * (1.0 - sg), _fma(x2, _t(_G1), _t(_G0)), sg)


def aux_grid(shape, seed):
    """aux operand of the GELU' cases: k / 4 for k in -16 .. 16 -- exact in bf16, zeros included (epi_nonzero_scale)."""
    return small_ints(shape, 16, seed) / 4


AUX_GRID_VALUES = torch.arange(-16, 17, dtype=torch.float64) / 4

# Largest deviation of the float32 restatement from float64 over the values the tests use (AUX_GRID_VALUES for GELU'; the
# integers -512 .. 512 a DROP_GELU case can store, for the factor gelu(x) / x).  MEASURED with measure_delta() below, rounded up
# in the second digit; tests/test_exact_fixtures_cpu.py holds the restatement to them, the GPU test allows 4 x (v_exp_f32 /
# v_rcp_f32 are ~1-ulp operations where libm is correctly rounded).
DELTA = {
    "gelu_grad_fast": 9.1e-7,       # measured 9.04e-07 (exp2 / rcp form: 1 - sigmoid cancels, f32 constants)
    "gelu_grad_tanhf": 2.0e-7,      # measured 1.92e-07 (tanhf form)
    "gelu_fast": 7.0e-8,            # measured 6.83e-08 (sigmoid(2u) factor of gelu_t<false>)
}


def measure_delta():
    ints = torch.arange(-512, 513, dtype=torch.float64)
    return {
        "gelu_grad_fast": float((gelu_grad32(AUX_GRID_VALUES, False).double() - gelu_grad64(AUX_GRID_VALUES)).abs().max()),
        "gelu_grad_tanhf": float((gelu_grad32(AUX_GRID_VALUES, True).double() - gelu_grad64(AUX_GRID_VALUES)).abs().max()),
        "gelu_fast": float((_sig_fast32(ints).double() - sigmoid2u64(ints)).abs().max()),
    }


def half_ulp(mag, dt):
    """Half a unit in the last place of dtype dt at magnitude mag (float64 tensor, elementwise; 0 at 0)."""
    p = 8 if dt == torch.bfloat16 else 24
    _, e = torch.frexp(mag.abs().double().clamp_min(2.0 ** -120))
    return torch.ldexp(torch.ones_like(mag, dtype=torch.float64), e - p - 1) * (mag != 0)


def inexact_bound(acc, ref, delta, dt):
    """|acc| * 4 delta + half an ulp of the output dtype (taken at |ref| + the first term, so that a result pushed across a
    power of two is still allowed its own rounding)."""
    t = acc.abs() * (4 * delta)
    return t + half_ulp(ref.abs() + t, dt)


# -------------------------------------------------------------------------------------------------------------- gemm_nt
def nt(M, N, K, epi="none", epi_scale=0.0, bias=True, out_f32=True, drop_p=0.0, layout="plain", fix="dense", pro="none",
       nz=0.0, seed=0):
    return dict(kind="nt", M=M, N=N, K=K, epi=epi, epi_scale=epi_scale, bias=bias, out_f32=out_f32, drop_p=drop_p, layout=layout,
                fix=fix, pro=pro, nz=nz, seed=seed)


DROP_SEED = 0x5EED1234ABCD


def build_nt(c):
    """Fixture + float64 reference of a gemm_nt case: dict A, W, bias, aux (float64 CPU tensors holding integers), acc
    (A W^T + bias, exact) and ref (after the epilogue; for gelu_grad / drop_gelu the exact part only), bound (see below)."""
    M, N, K, s = c["M"], c["N"], c["K"], 1000 * c["seed"] + 7
    amax = 8 if c["out_f32"] else 1
    if c["fix"] == "selector":
        A, col, val = selector(M, K)
        W = pattern(N, K)
    else:
        A = gelu_ints((M, K), s + 1) if c["pro"] == "gelu" else nonzero_ints((M, K), amax, s + 1)
        W = nonzero_ints((N, K), amax, s + 2)
    bias = small_ints((N,), 3, s + 3, step=2) if c["bias"] else None       # even: stays an integer under epi_scale = 0.5
    aux = None
    if c["epi"] in ("add", "posmask"):
        aux = small_ints((M, N), 4, s + 4)
    elif c["epi"] == "gelu_grad":
        aux = aux_grid((M, N), s + 4)
    acc = A @ W.t()
    if bias is not None:
        acc = acc + bias
    ref = acc
    if c["epi"] == "add":
        ref = acc + aux
    elif c["epi"] == "relu":
        ref = acc.clamp_min(0)
        if c["drop_p"] > 0:
            ref = ref * torch.from_numpy(dropmask.rowmajor_mask(DROP_SEED, c["drop_p"], M, N))
    elif c["epi"] == "posmask":
        ref = torch.where(aux > 0, acc * (c["epi_scale"] if c["epi_scale"] > 0 else 1.0), torch.zeros_like(acc))
    elif c["epi"] == "drop_gelu":
        if c["drop_p"] > 0:
            ref = acc * torch.from_numpy(dropmask.rowmajor_mask(DROP_SEED, c["drop_p"], M, N))
    # every partial sum of the accumulator, and every epilogue value, is below this
    bound = float(A.abs().max() * W.abs().max()) * K + (float(bias.abs().max()) if bias is not None else 0.0)
    if c["epi"] == "add":
        bound += float(aux.abs().max())
    if c["epi"] in ("relu", "drop_gelu") and c["drop_p"] > 0:
        bound *= 1.0 / (1.0 - c["drop_p"])
    return dict(A=A, W=W, bias=bias, aux=aux, acc=acc, ref=ref, bound=bound, dense=c["fix"] == "dense" and c["pro"] == "none")


# generic tile kernel (debug_ablate = 16 where the shape would otherwise go to the weight-stationary kernel).  Between them:
# K in {32, 96, 128, 160, 256, 384, 640, 1280} (partial-only, full + partial, FULLK; 1, 2, 3, 5, 10 chunks: both exits of the
# double-buffered loop), N in {1, 8, 48, 64, 72, 128, 136, 203} (NTW 1 / 2, clamped columns, vector and scalar epilogue),
# M in {1, 63, 64, 65, 130}, every epilogue with and without bias, f32 and storage-dtype output.
NT_GENERIC_CASES = [
    nt(1, 1, 32, "none", bias=True, out_f32=True),
    nt(63, 8, 96, "add", bias=False, out_f32=True),
    nt(64, 48, 128, "relu", bias=True, out_f32=False),
    nt(65, 64, 160, "posmask", 0.0, bias=False, out_f32=True),
    nt(130, 72, 256, "posmask", 0.5, bias=True, out_f32=True),
    nt(130, 128, 384, "add", bias=True, out_f32=False),
    nt(65, 136, 640, "none", bias=False, out_f32=False),
    nt(130, 203, 1280, "relu", bias=True, out_f32=True),
    nt(64, 203, 128, "add", bias=False, out_f32=False),                    # scalar epilogue with an aux operand, FULLK
    nt(63, 1, 640, "posmask", 0.5, bias=True, out_f32=True),                # scalar epilogue, one column
    nt(130, 203, 96, "posmask", 0.0, bias=False, out_f32=False),
    nt(65, 72, 32, "none", bias=True, out_f32=False),
    nt(130, 136, 96, "relu", bias=True, out_f32=True, drop_p=0.5),          # dropout after ReLU, vector epilogue
    nt(65, 203, 160, "relu", bias=False, out_f32=True, drop_p=0.5),         # ... scalar epilogue
    nt(130, 72, 160, "add", bias=True, out_f32=True, layout="slices"),      # A, aux, out: column slices of wider tensors
    nt(130, 136, 384, "add", bias=False, out_f32=False, layout="slices"),
    nt(65, 64, 128, "add", bias=True, out_f32=True, layout="ldc_odd"),      # ldc % 8 != 0: scalar epilogue at N % 8 == 0
    nt(130, 128, 256, "posmask", 0.5, bias=True, out_f32=False, layout="ldc_odd"),
    nt(130, 128, 384, "none", bias=True, out_f32=True, pro="gelu"),         # GELU prologue, FULLK
    nt(65, 72, 160, "add", bias=False, out_f32=True, pro="gelu"),           # ... partial chunk
    nt(130, 203, 96, "none", bias=False, out_f32=True, fix="selector"),     # M spans 3 row tiles with a tail; every k is hit
    nt(130, 72, 128, "none", bias=True, out_f32=False, fix="selector"),
    nt(200, 136, 160, "add", bias=False, out_f32=True, fix="selector"),
]

# the epilogues that cannot be exact, on an exact accumulator (section 3): vector path, scalar path (N = 203, the fix of this
# change: epi_nonzero_scale), unaligned ldc
NT_GENERIC_GELU_GRAD_CASES = [
    nt(130, 136, 160, "gelu_grad", bias=True, out_f32=True),
    nt(130, 136, 160, "gelu_grad", bias=True, out_f32=False, nz=2.0),
    nt(130, 203, 160, "gelu_grad", bias=True, out_f32=True, nz=2.0),
    nt(65, 203, 128, "gelu_grad", bias=False, out_f32=False),
    nt(65, 64, 128, "gelu_grad", bias=True, out_f32=True, nz=2.0, layout="ldc_odd"),
]


def ws(M, K, N, epi="none", **kw):
    c = nt(M, N, K, epi, out_f32=False, **kw)       # bf16 tier: bf16 output only -> the {+-1} alphabet (bf16x3 writes f32)
    c["kind"] = "ws"
    return c


def ws_code(tier, K, N):
    """Instantiation code rg_gemm_ws_select returns (10 K/128 + N/128 of the template arguments)."""
    nkc, ncb = K // 128, N // 128
    return 10 * nkc + (ncb if (tier == "bf16" and nkc == 1) else 1)


_WS_SHAPES = [(128, 128), (128, 256), (128, 384), (128, 512), (256, 128), (384, 128), (512, 128),      # <1, 1..4>, <2..4, 1>
              (256, 256), (384, 256), (512, 256), (256, 1024), (384, 1024), (512, 1024)]              # column-block grid form
_WS_EPIS = [("none", "add"), ("relu", "posmask")]
# every instantiation with and without an aux operand (a template argument), M = 4096 and 4096 + 77 alternating
WS_CASES = [ws(4096 + 77 * ((i + j) % 2), K, N, _WS_EPIS[i % 2][j], epi_scale=0.5 if (i + j) % 3 == 0 else 0.0, bias=(i + j) % 4 != 3)
            for i, (K, N) in enumerate(_WS_SHAPES) for j in range(2)]
WS_CASES += [ws(4096 + 77, 128, 128, fix="selector"), ws(4096 + 77, 384, 128, "add", fix="selector"), ws(4096 + 77, 512, 256, fix="selector")]
WS_DROP_GELU_CASES = [ws(4096 + 77, 128, 512, "drop_gelu", drop_p=0.0), ws(4096, 256, 256, "drop_gelu", drop_p=0.5),
                      ws(4096 + 77, 128, 128, "drop_gelu", drop_p=0.5)]
WS_GELU_GRAD_CASES = [ws(4096 + 77, 128, 512, "gelu_grad", nz=2.0), ws(4096, 512, 128, "gelu_grad"), ws(4096 + 77, 256, 256, "gelu_grad", nz=2.0)]
WS_HEADMAJOR_CASES = [(4104, 24), (4096, 64)]          # (M, L) at K = 128, N = 384; L = 24: 16-row tiles that span two sequences
# (K, N, epilogue, skip_dead_fill): 0 dead rows come out as zeros, 1 unwritten, 2 the bias row (EPI_NONE)
WS_LIVE_CASES = [(128, 128, "none", 2), (128, 512, "relu", 0), (512, 128, "add", 0), (384, 128, "add", 1), (256, 512, "none", 1),
                 (256, 256, "posmask", 0), (512, 1024, "none", 2)]
WS_LIVE_M, WS_LIVE_L = 4096 + 77, 120


# -------------------------------------------------------------------------------------------------------------- gemm_tn
def tn(T, N1, N2, splits=0, use_tr=1, scale=1.0, colsum=True, colsum_rows=0, fix="dense", partials=True, listed=False, seed=0):
    return dict(kind="tn", T=T, N1=N1, N2=N2, splits=splits, use_tr=use_tr, scale=scale, colsum=colsum, colsum_rows=colsum_rows,
                fix=fix, partials=partials, listed=listed, seed=seed)


def build_tn(c):
    """Fixture + reference of a gemm_tn case: Y, X, dW0 (the nonzero integers dW starts from), ref = dW0 + scale Y^T X and
    cs_ref = scale * column sums of Y (over the first colsum_rows rows if > 0).  With listed=True the rows of the dead 16-row
    tiles hold nonzero values in BOTH operands and are left out of the reference: the list says they are never read."""
    T, N1, N2, s = c["T"], c["N1"], c["N2"], 1000 * c["seed"] + 11
    if c["fix"] == "selector":
        Y, _, _ = selector(T, N1)
        X = pattern(T, N2)
    else:
        Y = nonzero_ints((T, N1), 8, s + 1)
        X = gelu_ints((T, N2), s + 2) if c["fix"] == "gelu" else nonzero_ints((T, N2), 8, s + 2)
    dW0 = small_ints((N1, N2), 5, s + 3)
    mask = seq_mask(T, 120, s + 4) if c["listed"] else None
    Yr = Y * live_rows(mask)[:, None].double() if c["listed"] else Y
    ref = dW0 + c["scale"] * (Yr.t() @ X)
    rows = c["colsum_rows"] if c["colsum_rows"] > 0 else T
    cs_ref = torch.zeros(N1, dtype=torch.float64) + c["scale"] * Yr[:rows].sum(0)      # accumulated into zeros: a zero sum times -2 is +0
    bound = float(Y.abs().max() * X.abs().max()) * T * abs(c["scale"]) + float(dW0.abs().max())
    return dict(Y=Y, X=X, dW0=dW0, mask=mask, ref=ref, cs_ref=cs_ref, bound=bound, dense=c["fix"] == "dense")


# generic 64 x 64 kernel: T in {1, 63, 64, 65, 333, 4101}, splits in {0, 1, 3, 64}, use_tr in {0, 1}, N1 / N2 in
# {8, 64, 72, 128, 640}, scale in {1, 0.5, -2}, colsum with and without colsum_rows strictly inside a 32-row step
TN_GENERIC_CASES = [
    tn(1, 8, 8, splits=0, use_tr=1, scale=1.0),
    tn(63, 64, 72, splits=1, use_tr=0, scale=0.5),
    tn(64, 72, 128, splits=3, use_tr=1, scale=-2.0),
    tn(65, 128, 64, splits=64, use_tr=0, scale=1.0, colsum_rows=37),
    tn(333, 640, 8, splits=0, use_tr=1, scale=0.5, colsum_rows=301),
    tn(4101, 72, 640, splits=3, use_tr=1, scale=1.0),
    tn(4101, 128, 128, splits=64, use_tr=1, scale=-2.0, colsum_rows=4001),
    tn(4101, 8, 72, splits=0, use_tr=0, scale=1.0, colsum=False),
    tn(333, 64, 640, splits=1, use_tr=1, scale=-2.0),
    tn(65, 640, 64, splits=0, use_tr=0, scale=0.5),
    tn(333, 64, 64, splits=3, use_tr=1, fix="gelu"),
    tn(4101, 128, 72, splits=0, use_tr=0, scale=0.5, fix="gelu"),
    tn(333, 72, 136, splits=3, use_tr=1, fix="selector"),                  # ~5 rows t per n1: dW[n1] = sum of +-X[t]
    tn(333, 640, 64, splits=0, use_tr=0, fix="selector"),                  # one t per n1: dW[n1(t)] = +-X[t]
]

# whole-tile kernels (T >= 8192): every native shape, one shape per blocked route (b1 = 512, 384, 256, 128 and 128 x 512),
# partial-sum workspace on and off, live-tile lists, the GELU prologue, the selector
TN_BIG_CASES = [
    tn(8192, 512, 128, scale=0.5, partials=True),
    tn(8192 + 333, 384, 128, scale=1.0, partials=False),
    tn(8192 + 333, 256, 128, scale=-2.0, partials=True),
    tn(8192, 128, 128, scale=1.0, partials=False),
    tn(8192 + 333, 128, 512, scale=0.5, partials=True),
    tn(8192 + 333, 512, 128, scale=1.0, partials=False),
    tn(8192, 128, 512, scale=-2.0, partials=False),
    tn(8192 + 333, 1024, 128, scale=1.0, partials=True),                   # blocks of 512 x 128
    tn(8192, 768, 256, scale=0.5, partials=False),                         # 384 x 128
    tn(8192 + 333, 256, 256, scale=1.0, partials=True),                    # 256 x 128
    tn(8192, 640, 128, scale=-2.0, partials=True),                         # 128 x 128
    tn(8192 + 333, 256, 512, scale=1.0, partials=False),                   # 128 x 512
    tn(8192 + 333, 512, 128, partials=True, listed=True),
    tn(8192 + 333, 128, 512, partials=False, listed=True, fix="gelu"),
    tn(8192, 128, 128, scale=0.5, partials=True, listed=True),
    tn(8192 + 333, 768, 256, partials=True, listed=True),
    tn(8192 + 333, 128, 512, partials=True, fix="gelu"),
    tn(8192, 256, 512, scale=0.5, partials=False, fix="gelu"),
    tn(8192 + 333, 384, 128, partials=True, fix="selector"),
    tn(8192 + 333, 128, 512, partials=False, fix="selector"),
]

# rg_gemm_tn_layer: the `present` subsets of test_gemm_tn_layer_equals_four_products, listed and not
LAYER_SHAPES = ((128, 512, True), (512, 128, False), (384, 128, False), (128, 128, False))      # (N1, N2, GELU prologue) per slot
LAYER_PRESENT = [(1, 1, 1, 1), (1, 1, 0, 0), (0, 0, 1, 1), (1, 0, 1, 0)]
LAYER_T = 8192 + 333


def build_layer(present, listed):
    """Per slot None or the build_tn() dict (scale 1; slot 0 on the GELU fixture; slot 2 never takes the list)."""
    out = []
    for i, (N1, N2, gelu) in enumerate(LAYER_SHAPES):
        if not present[i]:
            out.append(None)
            continue
        out.append(build_tn(tn(LAYER_T, N1, N2, fix="gelu" if gelu else "dense", listed=listed and i != 2, seed=20 + i)))
    return out


@functools.lru_cache(maxsize=4)
def _fixture(key):
    kind, idx = key
    if kind == "layer":
        return build_layer(*idx)
    c = CASES[kind][idx]
    return build_nt(c) if c["kind"] in ("nt", "ws") else build_tn(c)


def fixture(kind, idx):
    """The fixture of case idx of CASES[kind], built once and shared by the tiers (treat it as read-only)."""
    return _fixture((kind, idx))


CASES = {"nt": NT_GENERIC_CASES, "nt_gelu_grad": NT_GENERIC_GELU_GRAD_CASES, "ws": WS_CASES, "ws_drop_gelu": WS_DROP_GELU_CASES,
         "ws_gelu_grad": WS_GELU_GRAD_CASES, "tn": TN_GENERIC_CASES, "tn_big": TN_BIG_CASES}


def case_id(c):
    if c["kind"] in ("nt", "ws"):
        return "M%d-N%d-K%d-%s%s%s%s%s%s" % (c["M"], c["N"], c["K"], c["epi"], "-s%g" % c["epi_scale"] if c["epi_scale"] else "",
                                              "-bias" if c["bias"] else "", "-f32" if c["out_f32"] else "", "-p%g" % c["drop_p"] if c["drop_p"] else "",
                                              "".join("-" + x for x in (c["layout"], c["fix"], c["pro"]) if x not in ("plain", "dense", "none"))
                                              + ("-nz%g" % c["nz"] if c["nz"] else ""))
    return "T%d-%dx%d-sp%d-tr%d-x%g%s%s%s%s" % (c["T"], c["N1"], c["N2"], c["splits"], c["use_tr"], c["scale"],
                                                "-cs%d" % c["colsum_rows"] if c["colsum"] else "-nocs", "" if c["partials"] else "-atomics",
                                                "-listed" if c["listed"] else "", "" if c["fix"] == "dense" else "-" + c["fix"])
