"""The degenerate end of the padding structure, kernel by kernel: wholly padded sequences, live-tile lists of length zero and a
local mask count of zero -- what a data-parallel shard made of users with at most one item hands to the HIP path.  Every value
is held to a float64 restatement on the CPU (f32 tier: inputs as they are; bf16 tier: inputs rounded to bf16 first; bf16x3: the
f32 buffers under hip.SPLIT_OPERANDS, bounds of tests/test_x3_gpu.py); tolerances are the ones tests/test_kernels_gpu.py,
tests/test_x3_gpu.py and tests/test_dropout_masks_gpu.py already use for the same kernel and tier.

Attention length buckets, as read from the launchers of csrc/attention.hip (nkt = 2 * ceil(L / 32) key tiles; launch_fwd,
launch_bwd and both bf16x3 backward branches cut at the same edges; launch_fwd_x / launch_fwd_hm start at nkt <= 4):
    nkt <=  2   L <=  32   covered by L = 12
    nkt <=  4   L <=  64   covered by L = 50   (the x-input and head-major forms also take L = 12 here)
    nkt <=  8   L <= 128   covered by L = 128  (bf16 backward: one-pass form from here to nkt 16)
    nkt <= 14   L <= 224   covered by L = 200  (bf16x3 backward: two-tiles-at-a-time form for 128 < L <= 224)
    nkt <= 16   L <= 256   covered by L = 256  (bf16x3 backward: restaged form from here on)
    nkt <= 26   L <= 416   covered by L = 400  (bf16 backward: eight-wave two-phase form)
The six lengths of the issue reach every bucket; none is added.

List consumers covered with a list of length ZERO and with ONE live row in the ragged final tile (a consumer that is not named
here is not tested at the empty list):
    gemm_nt(live=)                    weight-stationary kernel, epilogues none / add / gelu_grad, K or N = 256 included
    gemm_tn(live=)                    big-shape kernel, with and without PRO_GELU, partial-sum and atomic flush
    gemm_tn_layer                     four products present, list on the slots that take one
    post_attn_fwd(compact=True)       d_model 128 (every tier) and 256 (bf16), save=True / False
    ffn_bwd_data(live=)               data path of the FFN backward, with the LayerNorm backward inside as well
    attn_out_bwd(live=)
    full_ce_fwd(train=True) + full_ce_dw
The list-driven GEMMs have a smallest size (rg_gemm_nt: M >= 4096, rg_gemm_tn / rg_gemm_tn_layer: T >= 8192; a smaller call with
a list is refused, include/recguru_hip.h), so they run at M = 4101 / T = 8197 only; the fused kernels run at M = 203 and 4101.
"""
import contextlib
import math

import pytest
import torch

import dropmask as dm

pytestmark = pytest.mark.gpu

TIERS = ["f32", "bf16", "x3"]
BINNED_SKIP = "the binned table-gradient kernels are not offered by the deterministic library (csrc/rg_det.hip.h)"


def _dt(tier):
    return torch.bfloat16 if tier == "bf16" else torch.float32


@contextlib.contextmanager
def _tier(tier):
    from recguru_amd import hip
    prev, hip.SPLIT_OPERANDS = hip.SPLIT_OPERANDS, tier == "x3"
    try:
        yield
    finally:
        hip.SPLIT_OPERANDS = prev


def rnd(*shape, dt, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dt).cuda()


def tol(dt):                                    # tests/test_kernels_gpu.py tol()
    return dict(rtol=2e-5, atol=2e-5) if dt == torch.float32 else dict(rtol=2e-2, atol=2e-2)


def close(a, b, what, bound=4e-5):              # tests/test_x3_gpu.py close()
    a, b = a.double(), b.double()
    assert a.shape == b.shape, what
    scale = max(float(b.abs().max()), 1e-30)
    err = float((a - b).abs().max()) / scale
    assert err <= bound, "%s: max error %.3g of max |value| (bound %.1g)" % (what, err, bound)


def _cmp(tier, got, ref, what, kind):
    """kind: 'ctx' | 'lse' | 'grad' -- the bound of the existing attention tests for that output and tier."""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert bool(torch.isfinite(got).all()), "%s: not finite" % what
    if tier == "x3":
        close(got, ref, what, 6e-5 if kind == "grad" else 4e-5)
        return
    dt = _dt(tier)
    if kind == "ctx":
        t = tol(dt)
    elif kind == "lse":
        t = dict(rtol=1e-4, atol=1e-3 if dt == torch.float32 else 3e-2)
    else:
        t = dict(rtol=1e-3, atol=1e-4) if dt == torch.float32 else dict(rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(got, ref, msg=lambda m: "%s: %s" % (what, m), **t)


# ======================================================================================================= a. attention
ATTN_L = [12, 50, 128, 200, 256, 400]
PAD = 0


def _attn_ids(L, seed):
    """B = 4: sequence 0 all pad, 1 one live key (the last), 2 full, 3 random left padding."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 50, (4, L), generator=g)
    ids[0] = PAD
    ids[1, : L - 1] = PAD
    ids[3, : int(torch.randint(1, L - 1, (1,), generator=g))] = PAD
    return ids


def _attn64(qkv, ids, causal, H, kmask=None):
    """tests/test_kernels_gpu.py _attn_ref in float64 (optionally with a dropout multiplier [B,H,L,L] on the probabilities)."""
    B, L, P3 = qkv.shape
    P = P3 // 3
    q, k, v = [t.reshape(B, L, H, 32).transpose(1, 2) for t in qkv.split(P, dim=2)]
    s = q @ k.transpose(-1, -2) / math.sqrt(32)
    m = ids.eq(PAD)[:, None, None, :].expand(B, H, L, L)
    if causal:
        m = m | torch.ones(L, L, dtype=torch.bool).triu(1)
    s = s.masked_fill(m, -1e9)
    a = torch.softmax(s, -1)
    if kmask is not None:
        a = a * kmask
    return (a @ v).transpose(1, 2).reshape(B, L, P), torch.logsumexp(s, -1)


_ATTN_REF = {}


def _attn_case(dt, L, H, causal, p=0.0, seed=0):
    """Inputs and the float64 reference of one case, computed once and shared: ctx, lse, and dqkv for the random dctx and for the
    dctx with its dead rows zeroed (the rowmask runs)."""
    key = (dt, L, H, causal, p, seed)
    if key not in _ATTN_REF:
        P = H * 32
        ids = _attn_ids(L, 1000 + L)
        qkv = rnd(4, L, 3 * P, dt=dt, seed=L + H)
        dctx = rnd(4, L, P, dt=dt, seed=7)
        rm = (ids != PAD).to(dt)
        dctx_m = (dctx.cpu() * rm[:, :, None]).contiguous()
        kmask = torch.from_numpy(dm.attn_mask(seed, p, H, L, range(4))) if p > 0 else None
        x = qkv.double().cpu().requires_grad_(True)
        ctx, lse = _attn64(x, ids, causal, H, kmask)
        g_full, = torch.autograd.grad(ctx, x, dctx.double().cpu(), retain_graph=True)
        g_mask, = torch.autograd.grad(ctx, x, dctx_m.double())
        _ATTN_REF[key] = dict(ids=ids.cuda(), qkv=qkv, dctx=dctx, dctx_m=dctx_m.cuda(), rm=(ids != PAD).float().reshape(-1).cuda(),
                              ctx=ctx.detach(), lse=lse.detach(), g_full=g_full, g_mask=g_mask)
    return _ATTN_REF[key]


def _dead_tile_rows(rm, B, L):
    """[B, L] bool: rows of the 16-query tiles (counted within a sequence) that hold no row with rowmask != 0."""
    Lp = (L + 15) // 16 * 16
    r = torch.zeros(B, Lp)
    r[:, :L] = rm.view(B, L).cpu()
    return (r.view(B, -1, 16).amax(2) == 0).repeat_interleave(16, dim=1)[:, :L]


def _check_attn(tier, c, L, H, causal, fwd, bwd, p=0.0, with_lse=True, what=""):
    """fwd(rowmask) -> (ctx, lse | None); bwd(dctx, ctx, lse, rowmask) -> dqkv, or None."""
    ref_ctx, ref_lse = c["ctx"], c["lse"]
    # ---- no rowmask: every row against float64
    ctx, lse = fwd(None)
    _cmp(tier, ctx, ref_ctx, what + "ctx", "ctx")
    if with_lse:
        _cmp(tier, lse, ref_lse, what + "lse", "lse")
    if p == 0.0:
        # sequence 0: every score is -1e9 -- uniform over all L keys, the causal future included (Q3 for the whole sequence)
        v = c["qkv"].double().cpu()[0, :, 2 * H * 32:]
        _cmp(tier, ctx[0], v.mean(0, keepdim=True).expand(L, -1), what + "ctx of the all-pad sequence = mean of its V rows", "ctx")
        if with_lse:
            _cmp(tier, lse[0], torch.full((H, L), -1e9 + math.log(L), dtype=torch.float64), what + "lse of the all-pad sequence", "lse")
    if bwd is not None:
        _cmp(tier, bwd(c["dctx"], ctx, lse, None), c["g_full"], what + "dqkv", "grad")
    # ---- rowmask = (ids != pad): rg_attn_args.rowmask -- rows of skipped tiles are written as ctx = 0, lse = 0; live rows as above
    ctx, lse = fwd(c["rm"])
    live = c["rm"].view(4, L).cpu() != 0
    dead = _dead_tile_rows(c["rm"], 4, L)
    assert bool(dead[0].all()) and int(dead[1].sum()) == (L - 1) // 16 * 16 and not bool(dead[2].any())
    assert bool(torch.isfinite(ctx.float()).all())
    _cmp(tier, ctx.cpu()[live], ref_ctx[live], what + "ctx (rowmask, live rows)", "ctx")
    assert float(ctx.float().cpu()[dead].abs().max()) == 0.0, what + "ctx rows of skipped tiles must be zero"
    if with_lse:
        lt = lse.transpose(1, 2).cpu()
        _cmp(tier, lt[live], ref_lse.transpose(1, 2)[live], what + "lse (rowmask, live rows)", "lse")
        assert float(lt[dead].abs().max()) == 0.0, what + "lse rows of skipped tiles must be zero"
    if bwd is not None:
        _cmp(tier, bwd(c["dctx_m"], ctx, lse, c["rm"]), c["g_mask"], what + "dqkv (rowmask)", "grad")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("L", ATTN_L)
@pytest.mark.parametrize("tier", TIERS)
def test_attn_wholly_padded_sequence(tier, L, H, causal):
    """hip.attn_fwd / attn_bwd, token-major, on a batch with an all-pad sequence (uniform attention over all L keys,
    lse = -1e9 + log L), a sequence with one live key, a full one and a left-padded one; without and with a rowmask."""
    from recguru_amd import hip
    dt = _dt(tier)
    c = _attn_case(dt, L, H, causal)
    with _tier(tier):
        _check_attn(tier, c, L, H, causal,
                    lambda rm: hip.attn_fwd(c["qkv"], c["ids"], PAD, causal, H, rowmask=rm),
                    lambda dctx, ctx, lse, rm: hip.attn_bwd(c["qkv"], dctx, ctx, lse, c["ids"], PAD, causal, H, rowmask=rm))


@pytest.mark.parametrize("tier", TIERS)
def test_attn_wholly_padded_sequence_dropout(tier):
    """The same batch at drop_p = 0.5: the reference multiplies the probabilities by the host restatement of the kernel's mask
    (tests/dropmask.py), so it stays exact -- the all-pad sequence is the kept half of its V rows x 2 / L."""
    from recguru_amd import hip
    L, H, causal, p, seed = 200, 4, True, 0.5, 0x5EED0123
    c = _attn_case(_dt(tier), L, H, causal, p, seed)
    kw = dict(drop_p=p, seed=seed)
    with _tier(tier):
        _check_attn(tier, c, L, H, causal,
                    lambda rm: hip.attn_fwd(c["qkv"], c["ids"], PAD, causal, H, rowmask=rm, **kw),
                    lambda dctx, ctx, lse, rm: hip.attn_bwd(c["qkv"], dctx, ctx, lse, c["ids"], PAD, causal, H, rowmask=rm, **kw), p=p)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("L", ATTN_L)
def test_attn_wholly_padded_sequence_head_major(L, H, causal):
    """The head-major form (bf16: q | k | v [3, B, H, L, 32], K / V tiles by LDS-DMA) on the same batch and reference.  x_masked
    is off, so pad_rows (random bias rows + the zero row) may stand in for nothing but the key range beyond L."""
    from recguru_amd import hip
    dt = torch.bfloat16
    c = _attn_case(dt, L, H, causal)
    qh = c["qkv"].view(4, L, 3, H, 32).permute(2, 0, 3, 1, 4).contiguous()
    pad_rows = torch.cat([rnd(3 * H, 32, dt=dt, seed=3), torch.zeros(1, 32, dtype=dt, device="cuda")], 0).contiguous()
    _check_attn("bf16", c, L, H, causal,
                lambda rm: hip.attn_fwd(qh, c["ids"], PAD, causal, H, rowmask=rm, pad_rows=pad_rows),
                lambda dctx, ctx, lse, rm: hip.attn_bwd(qh, dctx, ctx, lse, c["ids"], PAD, causal, H, rowmask=rm), what="head-major ")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", ATTN_L)
@pytest.mark.parametrize("drop_p", [0.0, 0.5])
def test_attn_wholly_padded_sequence_x_input(L, causal, drop_p):
    """The x-input form (inference, bf16, d_model 128: Q / K / V projected inside the kernel) on the same id pattern.  The reference
    projects in float64 and rounds Q / K / V to bf16, as the kernel's operands are; bound of
    test_attn_fwd_x_equals_projection_plus_attention (2e-2)."""
    from recguru_amd import hip
    H, d, dt = 4, 128, torch.bfloat16
    assert hip.attn_fwd_x_supported(d, dt, drop_p)
    P = H * 32
    seed = 77
    ids = _attn_ids(L, 1000 + L)
    x = rnd(4, L, d, dt=dt, scale=0.8, seed=L)
    w = rnd(3 * P, d, dt=dt, scale=d ** -0.5, seed=2)
    bias = rnd(3 * P, dt=torch.float32, scale=0.2, seed=3)
    qkv = (x.double().cpu() @ w.double().cpu().t() + bias.double().cpu()).to(dt).double()
    kmask = torch.from_numpy(dm.attn_mask(seed, drop_p, H, L, range(4))) if drop_p > 0 else None
    ref, _ = _attn64(qkv, ids, causal, H, kmask)
    rm = (ids != PAD).float().reshape(-1).cuda()
    live = ids != PAD
    dead = _dead_tile_rows(rm, 4, L)
    idc = ids.cuda()
    got = hip.attn_fwd_x(x, w, bias, idc, PAD, causal, H, drop_p=drop_p, seed=seed)
    assert bool(torch.isfinite(got.float()).all())
    torch.testing.assert_close(got.double().cpu(), ref, rtol=2e-2, atol=2e-2)
    got = hip.attn_fwd_x(x, w, bias, idc, PAD, causal, H, drop_p=drop_p, seed=seed, rowmask=rm)
    assert bool(torch.isfinite(got.float()).all())
    torch.testing.assert_close(got.double().cpu()[live], ref[live], rtol=2e-2, atol=2e-2)
    assert float(got.float().cpu()[dead].abs().max()) == 0.0
    # x_masked: the rows of x at positions with rowmask == 0 are zero (their K / V are the bias rows, folded)
    xm = (x * rm.view(4, L, 1).to(dt)).contiguous()
    qkv = (xm.double().cpu() @ w.double().cpu().t() + bias.double().cpu()).to(dt).double()
    ref, _ = _attn64(qkv, ids, causal, H, kmask)
    got = hip.attn_fwd_x(xm, w, bias, idc, PAD, causal, H, drop_p=drop_p, seed=seed, rowmask=rm, x_masked=True)
    assert bool(torch.isfinite(got.float()).all())
    torch.testing.assert_close(got.double().cpu()[live], ref[live], rtol=2e-2, atol=2e-2)
    assert float(got.float().cpu()[dead].abs().max()) == 0.0


# ======================================================================================================= b. single-query kernels
@pytest.mark.parametrize("drop_p", [0.0, 0.5])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_attn_lastq_whole_sequence_is_the_folded_prefix(dt, drop_p):
    """The batch of test_attn_lastq_folds_the_padded_prefix with lens[2] = 0: first_live == L, the whole K / V of that sequence is
    the folded prefix (bias rows) and the NaN holes cover every row of it.  Folded and unfolded kernels against float64."""
    from recguru_amd import hip
    B, L, H, d = 9, 200, 4, 128
    P = H * 32
    seed = 9
    g0 = torch.Generator().manual_seed(29)
    ids = torch.randint(1, 50, (B, L), generator=g0)
    lens = torch.randint(1, L + 1, (B,), generator=g0)
    lens[0], lens[1], lens[2] = L, 2, 0
    for b in range(B):
        ids[b, : L - int(lens[b])] = 0
    rowmask = (ids != 0).float().view(-1).cuda()
    ids = ids.cuda()
    M = B * L
    x = ((torch.randn(B, L, d, generator=g0) * 0.8).cuda() * rowmask.view(B, L, 1)).to(dt).contiguous()
    w = (torch.randn(2 * P, d, generator=g0) / d ** 0.5).to(dt).cuda()
    bkv = (torch.randn(2 * P, generator=g0) * 0.3).cuda()
    kv = hip.gemm_nt(x.view(M, d), w, bkv).view(B, L, 2 * P)
    assert int(hip.first_live(rowmask, B, L)[2]) == L
    # the bias rows as the projection wrote them (bit for bit what the fold substitutes): every row of sequence 2
    assert torch.equal(kv[2], kv[2, :1].expand(L, -1))
    holes = kv.clone()
    holes.view(M, 2 * P)[rowmask == 0] = float("nan")
    assert bool(torch.isnan(holes[2].float()).all())
    q_last = (torch.randn(B, P, generator=g0) * 0.5).cuda().to(dt)
    dctx = (torch.randn(B, P, generator=g0) * 0.5).cuda().to(dt)
    # float64: row L-1, no key masked (pad value 51 does not occur, quirk Q2)
    q64 = q_last.double().cpu().requires_grad_(True)
    kv64 = kv.double().cpu().requires_grad_(True)
    k64, v64 = [t.reshape(B, L, H, 32).transpose(1, 2) for t in kv64.split(P, dim=2)]
    s = (q64.view(B, H, 1, 32) @ k64.transpose(-1, -2)) / math.sqrt(32)
    a = torch.softmax(s, -1)
    if drop_p > 0:
        a = a * torch.from_numpy(dm.attn_mask(seed, drop_p, H, L, range(B)))[:, :, L - 1:L, :]
    ref = (a @ v64).reshape(B, P)
    ref.backward(dctx.double().cpu())
    tf = tol(dt)
    tb = dict(rtol=1e-3, atol=1e-4) if dt == torch.float32 else dict(rtol=5e-2, atol=5e-2)
    tfold = dict(rtol=1e-5, atol=1e-6) if dt == torch.float32 else dict(rtol=1e-2, atol=1e-2)
    outs = {}
    for name, kvin, fold in (("unfolded", kv, {}), ("folded", holes, dict(rowmask=rowmask, bkv=bkv))):
        c = hip.attn_lastq_fwd(q_last, kvin, ids, 51, H, drop_p, seed, **fold)
        dq, dkv = hip.attn_lastq_bwd(q_last, kvin, dctx, ids, 51, H, drop_p, seed, **fold)
        for t in (c, dq, dkv):
            assert bool(torch.isfinite(t.float()).all()), name
        torch.testing.assert_close(c.double().cpu(), ref.detach(), **tf)
        torch.testing.assert_close(dq.double().cpu(), q64.grad, **tb)
        torch.testing.assert_close(dkv.double().cpu(), kv64.grad, **tb)
        outs[name] = (c, dq, dkv)
    for got, want in zip(outs["folded"], outs["unfolded"]):
        torch.testing.assert_close(got.float(), want.float(), **tfold)


@pytest.mark.parametrize("L", [200, 77])
@pytest.mark.parametrize("drop_p", [0.0, 0.5])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_attn_lastq_x_whole_sequence_is_the_folded_prefix(dt, drop_p, L):
    """The x-input single-query kernels (bf16: rg_attn_lastq_x_*, f32 tensors: the exact-f32 rg_attn_lastq_xf_*) on the same kind of
    batch: lens[2] = 0, so first_live == L and every row of x of that sequence is a zero row.  With the first-live index
    (rowmask) and without it, against float64 autograd from x (context, dq, dx on the live rows, dWK, dWV, dbV) and against the
    projection + unfolded single-query kernels; bounds (fractions of the largest element) of
    test_attn_lastq_xf_f32_form_matches_projection_plus_single_query / test_attn_lastq_x_matches_projection_plus_single_query."""
    from recguru_amd import hip
    B, H, d = 9, 4, 128
    P = H * 32
    seed = 9
    assert hip.attn_lastq_x_supported(d, P, H, L, dt)
    g0 = torch.Generator().manual_seed(31 + L)
    ids = torch.randint(1, 50, (B, L), generator=g0)
    lens = torch.randint(1, L + 1, (B,), generator=g0)
    lens[0], lens[1], lens[2] = L, 2, 0
    for b in range(B):
        ids[b, : L - int(lens[b])] = 0
    rowmask = (ids != 0).float().view(-1).cuda().contiguous()
    ids = ids.cuda()
    M = B * L
    assert int(hip.first_live(rowmask, B, L)[2]) == L
    x = ((torch.randn(B, L, d, generator=g0) * 0.8).cuda() * rowmask.view(B, L, 1)).to(dt).contiguous()
    w = (torch.randn(2 * P, d, generator=g0) / d ** 0.5).to(dt).cuda()
    bkv = (torch.randn(2 * P, generator=g0) * 0.3).cuda()
    wk, wv, bk, bv = w[:P].contiguous(), w[P:].contiguous(), bkv[:P].contiguous(), bkv[P:].contiguous()
    q_last = (torch.randn(B, P, generator=g0) * 0.7).cuda().to(dt)
    dctx = (torch.randn(B, P, generator=g0) * 0.5).cuda().to(dt)
    # float64 from the same (tier-rounded) inputs; pad value 51 does not occur: no key is replaced
    x64, w64, b64 = (t.double().cpu().requires_grad_(True) for t in (x, w, bkv))
    q64 = q_last.double().cpu().requires_grad_(True)
    kv64 = (x64.view(M, d) @ w64.t() + b64).view(B, L, 2, H, 32)
    sc = torch.einsum("bhc,blhc->bhl", q64.view(B, H, 32), kv64[:, :, 0]) * 32 ** -0.5
    a = torch.softmax(sc, -1)
    if drop_p > 0:
        a = a * torch.from_numpy(dm.attn_mask(seed, drop_p, H, L, range(B)))[:, :, L - 1, :]
    ref = torch.einsum("bhl,blhc->bhc", a, kv64[:, :, 1]).reshape(B, P)
    ref.backward(dctx.double().cpu())
    # the projection + unfolded single-query kernels
    with _tier("f32"):
        kv = hip.gemm_nt(x.view(M, d), w, bkv).view(B, L, 2 * P)
    c_old = hip.attn_lastq_fwd(q_last, kv, ids, 51, H, drop_p, seed)
    dq_old, dkv_old = hip.attn_lastq_bwd(q_last, kv, dctx, ids, 51, H, drop_p, seed)
    dkv2 = dkv_old.view(M, 2 * P).double()
    old = dict(c=c_old, dq=dq_old, dx=(dkv2 @ w.double()).view(B, L, d), dWv=(dkv2.t() @ x.view(M, d).double())[P:],
               dWk=(dkv2.t() @ x.view(M, d).double())[:P], dbv=dkv2[:, P:].sum(0))
    r64 = dict(c=ref.detach(), dq=q64.grad, dx=x64.grad, dWv=w64.grad[P:], dWk=w64.grad[:P], dbv=b64.grad[P:])
    f32 = dt == torch.float32
    frac = dict(c=2e-5, dq=5e-5, dx=5e-5, dWv=5e-5, dWk=1e-4, dbv=5e-5) if f32 else dict(c=0.02, dq=0.03, dx=0.03, dWv=0.03, dWk=0.04, dbv=0.02)
    rows = (rowmask.view(B, L) != 0).cpu()

    def close(got, want, fr, what):
        got, want = got.double().cpu(), want.double().cpu()
        assert bool(torch.isfinite(got).all()), what
        err, top = float((got - want).abs().max()), float(want.abs().max())
        assert err <= fr * top + (1e-7 if f32 else 1e-6), "%s: max err %.3g of max %.3g" % (what, err, top)

    for rm in (rowmask, None):
        tag = "first-live " if rm is not None else "plain "
        c = hip.attn_lastq_x_fwd(x, q_last, wk, wv, bk, bv, ids, 51, drop_p, seed, rowmask=rm)
        dbv = torch.zeros(P, device="cuda")
        dx, dq, ym_v, xbar, ym_q, dqp = hip.attn_lastq_x_bwd(x, q_last, dctx, wk, wv, bk, bv, ids, 51, dbv, drop_p, seed, rowmask=rm)
        got = dict(c=c, dq=dq, dx=dx, dWv=ym_v.double().t() @ xbar.double(), dWk=ym_q.double().t() @ dqp.double(), dbv=dbv)
        assert bool(torch.isfinite(dx.float()).all()), tag + "dx"
        for k in ("c", "dq", "dx", "dWv", "dWk", "dbv"):
            for name, want in (("float64", r64[k]), ("unfolded kernels", old[k])):
                g_, w_ = (got[k].cpu()[rows], want.cpu()[rows]) if k == "dx" else (got[k], want)
                close(g_, w_, frac[k], "%s%s vs %s" % (tag, k, name))


# ======================================================================================================= c. zero live tiles
def _list_mask(M, which):
    m = torch.zeros(M)
    if which == "last":
        m[M - 1] = 1.0                           # the last row: inside the ragged final tile
    return m.cuda()


def _live(mask, M, which):
    from recguru_amd import hip
    live = hip.live_tiles(mask, M)
    assert int(live[0]) == (0 if which == "zero" else 1)
    return live


def _rows_ok(listed, full, mask, zero_dead=True):
    """Live rows bit-identical to the unlisted call; every other row exactly zero (zero_dead) or still poisoned (unwritten)."""
    lv = mask != 0
    assert torch.equal(listed[lv], full[lv])
    if int((~lv).sum()):
        rest = listed[~lv].float()
        if zero_dead:
            assert float(rest.abs().max()) == 0.0
        else:
            assert bool(torch.isnan(rest).all())


@pytest.mark.parametrize("which", ["zero", "last"])
@pytest.mark.parametrize("K,N,epi", [(128, 512, "gelu_grad"), (512, 128, "add"), (128, 128, "none"), (384, 128, "add"),
                                     (256, 768, "none"), (256, 512, "gelu_grad"), (512, 256, "add")])
def test_zero_live_gemm_nt(K, N, epi, which):
    from recguru_amd import hip
    dt = torch.bfloat16
    M = 4101
    mask = _list_mask(M, which)
    live = _live(mask, M, which)
    A = rnd(M, K, dt=dt, seed=1) * mask[:, None].to(dt)
    W = rnd(N, K, dt=dt, seed=2, scale=0.1)
    aux = rnd(M, N, dt=dt, seed=3) * mask[:, None].to(dt)
    kw = {"gelu_grad": dict(epilogue=hip.EPI_GELU_GRAD, aux=aux), "add": dict(epilogue=hip.EPI_ADD, aux=aux), "none": {}}[epi]
    full = hip.gemm_nt(A, W, **kw)
    t16 = (torch.arange(M, device="cuda") // 16 == (M - 1) // 16) & (mask.sum() > 0)       # rows of the one live tile
    An = A.clone()
    An[~t16] = float("nan")                                                 # rows of the dead tiles are not read
    if "aux" in kw:
        kw["aux"] = aux.clone()
        kw["aux"][~t16] = float("nan")
    out = torch.full((M, N), float("nan"), dtype=dt, device="cuda")
    hip.gemm_nt(An, W, out=out, live=live, **kw)
    _rows_ok(out, full, mask)
    # dead tiles left unwritten: FINITE operands here (zero rows), so that a tile launched from an empty list -- which would store
    # finite values over the NaN pre-fill -- shows; with NaN operands it would store NaN and pass for unwritten
    out = torch.full((M, N), float("nan"), dtype=dt, device="cuda")
    hip.gemm_nt(A, W, out=out, live=live, skip_dead_fill=1, **dict(kw, **({"aux": aux} if "aux" in kw else {})))
    assert torch.equal(out[t16], full[t16]) and bool(torch.isnan(out[~t16].float()).all())


def test_list_gemms_refuse_a_list_below_their_smallest_size():
    """M = 203 of the issue: rg_gemm_nt / rg_gemm_tn do not take a list there (no list-driven kernel below 4096 / 8192 rows) and say
    so with an error instead of ignoring it; the output / accumulator is untouched."""
    from recguru_amd import hip
    dt = torch.bfloat16
    M = 203
    mask = _list_mask(M, "zero")
    live = _live(mask, M, "zero")
    A, W = torch.zeros(M, 128, dtype=dt, device="cuda"), rnd(128, 128, dt=dt, seed=2)
    out = torch.full((M, 128), float("nan"), dtype=dt, device="cuda")
    with pytest.raises(RuntimeError, match="live16"):
        hip.gemm_nt(A, W, out=out, live=live)
    assert bool(torch.isnan(out.float()).all())
    dW0 = rnd(128, 128, dt=torch.float32, seed=5)
    dW = dW0.clone()
    with pytest.raises(RuntimeError, match="live16"):
        hip.gemm_tn(A, rnd(M, 128, dt=dt, seed=3), dW, None, live=live)
    assert torch.equal(dW, dW0)


@pytest.mark.parametrize("which", ["zero", "last"])
@pytest.mark.parametrize("partials", [True, False])
@pytest.mark.parametrize("N1,N2,gelu", [(128, 512, True), (512, 128, False), (128, 128, False), (256, 512, True), (768, 256, False)])
def test_zero_live_gemm_tn(N1, N2, gelu, partials, which):
    from recguru_amd import hip
    dt = torch.bfloat16
    T = 8197
    mask = _list_mask(T, which)
    live = _live(mask, T, which)
    Y = rnd(T, N1, dt=dt, seed=1) * mask[:, None].to(dt)
    X = rnd(T, N2, dt=dt, seed=2)
    X[: T - 16] = float("nan")                                  # rows of dead tiles are never read
    kw = dict(prologue_x=hip.PRO_GELU if gelu else hip.PRO_NONE, partials=partials)
    dW0, cs0 = rnd(N1, N2, dt=torch.float32, seed=5), rnd(N1, dt=torch.float32, seed=6)
    dW, cs = dW0.clone(), cs0.clone()
    hip.gemm_tn(Y, X, dW, cs, live=live, **kw)
    if which == "zero":
        assert torch.equal(dW, dW0) and torch.equal(cs, cs0)
    else:
        Xf = torch.where(torch.isnan(X.float()), torch.zeros_like(X.float()), X.float()).to(dt)
        dW1, cs1 = dW0.clone(), cs0.clone()
        hip.gemm_tn(Y, Xf, dW1, cs1, **kw)                       # unlisted: zero Y rows add exact zeros
        assert torch.equal(dW, dW1) and torch.equal(cs, cs1)
        assert not torch.equal(dW, dW0)


@pytest.mark.parametrize("which", ["zero", "last"])
@pytest.mark.parametrize("tier", ["bf16", "x3"])
def test_zero_live_gemm_tn_layer(tier, which):
    """Four products present, the list on the slots that take one (dWqkv sums every row, as in the training step).  The X and Y rows
    of the dead tiles of the listed slots hold NaN: a tile launched from an empty list, or a read through entry 0 of it, shows.
    'last': bit for bit the unlisted launch on the same operands with those rows zeroed."""
    from recguru_amd import hip
    dt = _dt(tier)
    T = 8197
    mask = _list_mask(T, which)
    live = _live(mask, T, which)
    dead = torch.arange(T, device="cuda") < (T - 1) // 16 * 16         # rows of the dead tiles (every row for the empty list: see below)
    if which == "zero":
        dead[:] = True
    listed, plain, keep = [], [], []
    for i, (N1, N2, pro) in enumerate(hip.LAYER_SLOTS):
        Y = rnd(T, N1, dt=dt, seed=10 + i) * mask[:, None].to(dt)
        X = rnd(T, N2, dt=dt, seed=20 + i)
        dW0, cs0 = rnd(N1, N2, dt=torch.float32, seed=30 + i), rnd(N1, dt=torch.float32, seed=40 + i)
        Yn, Xn = Y.clone(), X.clone()
        if i != 2:
            Yn[dead] = float("nan")
            Xn[dead] = float("nan")
        a_, b_ = (dW0.clone(), cs0.clone()), (dW0.clone(), cs0.clone())
        listed.append((Yn, Xn, a_[0], a_[1], live if i != 2 else None))
        plain.append((Y, X, b_[0], b_[1], None))
        keep.append((dW0, cs0, a_, b_))
    with _tier(tier):
        assert hip.gemm_tn_layer(listed)
        if which == "last":
            assert hip.gemm_tn_layer(plain)
    for i, (dW0, cs0, a_, b_) in enumerate(keep):
        if which == "zero":
            assert torch.equal(a_[0], dW0) and torch.equal(a_[1], cs0), "slot %d" % i
        else:
            assert torch.equal(a_[0], b_[0]) and torch.equal(a_[1], b_[1]), "slot %d" % i
            assert not torch.equal(a_[0], dW0), "slot %d" % i


def _post_attn_operands(M, d, dff, dt):
    f32 = torch.float32
    ctx, x = rnd(M, d, dt=dt, seed=1), rnd(M, d, dt=dt, seed=2)
    ws = (rnd(d, d, dt=dt, seed=3, scale=d ** -0.5), rnd(dff, d, dt=dt, seed=4, scale=d ** -0.5), rnd(d, dff, dt=dt, seed=5, scale=dff ** -0.5))
    bs = (rnd(d, dt=f32, seed=6), rnd(dff, dt=f32, seed=7), rnd(d, dt=f32, seed=8))
    g, be = 1 + 0.1 * rnd(d, dt=f32, seed=9), 0.1 * rnd(d, dt=f32, seed=10)
    return ctx, x, ws, bs, g, be


@pytest.mark.parametrize("which", ["zero", "last"])
@pytest.mark.parametrize("save", [False, True])
@pytest.mark.parametrize("M", [203, 4101])
@pytest.mark.parametrize("d,dff,dt", [(128, 256, torch.bfloat16), (128, 512, torch.bfloat16), (128, 256, torch.float32), (128, 512, torch.float32),
                                      (256, 256, torch.bfloat16), (256, 512, torch.bfloat16)])
def test_zero_live_post_attn_fwd(d, dff, dt, M, save, which, monkeypatch):
    """post_attn_fwd(compact=True) hands the kernel a list from hip.COMPACT_MIN_ROWS rows on; lowered here so that the small
    shapes run list-driven."""
    from recguru_amd import hip
    assert hip.post_attn_supported(d, d, dff, dt, M)
    monkeypatch.setattr(hip, "COMPACT_MIN_ROWS", 0)
    mask = _list_mask(M, which)
    _live(mask, M, which)
    ctx, x, (wo, w1, w2), (bo, b1, b2), g, be = _post_attn_operands(M, d, dff, dt)
    x = x * mask[:, None].to(dt)
    kw = dict(save=save, drop_p=0.5, seed_h1=11, seed_out=12)
    if d == 256:                                 # csrc/fused256.hip takes fragment-packed weights only
        wo, w1, w2 = (hip.cast(w.float(), dt, transpose=hip.CAST_PACK) for w in (wo, w1, w2))
        kw["w_packed"] = True
    a, sa = hip.post_attn_fwd(ctx, x, wo, bo, g, be, w1, b1, w2, b2, g, be, mask, compact=True, **kw)
    b, sb = hip.post_attn_fwd(ctx, x, wo, bo, g, be, w1, b1, w2, b2, g, be, mask, compact=False, **kw)
    _rows_ok(a, b, mask)
    lv = mask != 0
    for name in sa:
        assert bool(torch.isfinite(sa[name].float()).all()), name
        assert torch.equal(sa[name][lv], sb[name][lv]), name
        if name in ("y", "h1") and int((~lv).sum()):
            t16 = torch.arange(M, device="cuda") // 16 == (M - 1) // 16 if which == "last" else torch.zeros(M, dtype=torch.bool, device="cuda")
            assert float(sa[name][~t16].float().abs().max()) == 0.0, name      # rows of the dead tiles


@pytest.mark.parametrize("which", ["zero", "last"])
@pytest.mark.parametrize("M", [203, 4101])
@pytest.mark.parametrize("dff", [256, 512])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_zero_live_ffn_bwd_data(dt, dff, M, which):
    from recguru_amd import hip
    d = 128
    mask = _list_mask(M, which)
    live = _live(mask, M, which)
    mk = mask[:, None].to(dt)
    dl2, dz, h1 = rnd(M, d, dt=dt, seed=1) * mk, rnd(M, d, dt=dt, seed=2) * mk, rnd(M, dff, dt=dt, seed=3) * mk
    W1, W2 = rnd(dff, d, dt=torch.float32, scale=d ** -0.5, seed=5), rnd(d, dff, dt=torch.float32, scale=dff ** -0.5, seed=6)
    W2tp, W1tp = hip.cast(W2, dt, transpose=hip.CAST_TRANSPOSE | hip.CAST_PACK), hip.cast(W1, dt, transpose=hip.CAST_TRANSPOSE | hip.CAST_PACK)
    t16 = (torch.arange(M, device="cuda") // 16 == (M - 1) // 16) & (mask.sum() > 0)       # rows of the one live tile
    dh1, dy = hip.ffn_bwd_data(dl2, dz, h1, W2tp, W1tp, w_packed=True)
    hip.POISON_UNWRITTEN = True
    try:
        dh1_l, dy_l = hip.ffn_bwd_data(dl2, dz, h1, W2tp, W1tp, live=live, w_packed=True)
    finally:
        hip.POISON_UNWRITTEN = False
    assert torch.equal(dy_l[t16], dy[t16]) and torch.equal(dh1_l[t16], dh1[t16])
    assert float(dy_l[~t16].float().abs().max()) == 0.0                                  # dy: zeros; dh1: unwritten
    assert bool(torch.isnan(dh1_l[~t16].float()).all())
    # with the LayerNorm backward inside: dgamma / dbeta are accumulated into
    f32 = torch.float32
    g, be = 1 + 0.1 * rnd(d, dt=f32, seed=7), 0.1 * rnd(d, dt=f32, seed=8)
    z = rnd(M, d, dt=f32, seed=9)
    rstd = 1 / torch.sqrt(z.var(1, unbiased=False) + 1e-8)
    out = (torch.nn.functional.layer_norm(z, (d,), g, be, 1e-8) * mask[:, None]).to(dt)
    dout = rnd(M, d, dt=dt, seed=10) * mk
    dg0, db0 = rnd(d, dt=f32, seed=11), rnd(d, dt=f32, seed=12)
    res = {}
    for name, lv in (("full", None), ("listed", live)):
        dg, db = dg0.clone(), db0.clone()
        hip.POISON_UNWRITTEN = lv is not None
        try:
            res[name] = hip.ffn_bwd_data(None, None, h1, W2tp, W1tp, live=lv, w_packed=True, ln=(dout, out, rstd, g, be, mask, dg, db, 0.0, 0)) + (dg, db)
        finally:
            hip.POISON_UNWRITTEN = False
    _, dy_l, dl2_l, dg_l, db_l = res["listed"]
    _, dy_f, dl2_f, dg_f, db_f = res["full"]
    assert torch.equal(dy_l[t16], dy_f[t16]) and torch.equal(dl2_l[t16], dl2_f[t16])
    assert float(dy_l[~t16].float().abs().max()) == 0.0
    if which == "zero":
        assert torch.equal(dg_l, dg0) and torch.equal(db_l, db0)
    else:
        assert torch.equal(dg_l, dg_f) and torch.equal(db_l, db_f) and not torch.equal(db_l, db0)


@pytest.mark.parametrize("which", ["zero", "last"])
@pytest.mark.parametrize("M", [203, 4101])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_zero_live_attn_out_bwd(dt, M, which):
    from recguru_amd import hip
    d = 128
    f32 = torch.float32
    mask = _list_mask(M, which)
    live = _live(mask, M, which)
    g, be = 1 + 0.1 * rnd(d, dt=f32, seed=1), 0.1 * rnd(d, dt=f32, seed=2)
    z = rnd(M, d, dt=f32, seed=3)
    rstd = 1 / torch.sqrt(z.var(1, unbiased=False) + 1e-8)
    y = torch.nn.functional.layer_norm(z, (d,), g, be, 1e-8).to(dt)
    dy = rnd(M, d, dt=dt, seed=4) * mask[:, None].to(dt)
    Wotp = hip.cast(rnd(d, d, dt=f32, scale=d ** -0.5, seed=5), dt, transpose=hip.CAST_TRANSPOSE | hip.CAST_PACK)
    dg0, db0 = rnd(d, dt=f32, seed=6), rnd(d, dt=f32, seed=7)
    dgf, dbf = dg0.clone(), db0.clone()
    dzf, dcf = hip.attn_out_bwd(dy, y, rstd, g, be, mask, dgf, dbf, Wotp, w_packed=True)
    dg, db = dg0.clone(), db0.clone()
    hip.POISON_UNWRITTEN = True
    try:
        dz, dc = hip.attn_out_bwd(dy, y, rstd, g, be, mask, dg, db, Wotp, live=live, w_packed=True)
    finally:
        hip.POISON_UNWRITTEN = False
    t16 = (torch.arange(M, device="cuda") // 16 == (M - 1) // 16) & (mask.sum() > 0)
    assert torch.equal(dz[t16], dzf[t16]) and torch.equal(dc[t16], dcf[t16])
    assert bool(torch.isnan(dz[~t16].float()).all()) and bool(torch.isnan(dc[~t16].float()).all())     # unwritten by contract
    if which == "zero":
        assert torch.equal(dg, dg0) and torch.equal(db, db0)
    else:
        assert torch.equal(dg, dgf) and torch.equal(db, dbf) and not torch.equal(db, db0)


@pytest.mark.parametrize("which", ["zero", "last"])
@pytest.mark.parametrize("M", [203, 4101])
@pytest.mark.parametrize("d", [128, 256])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_zero_live_full_ce(dt, d, M, which):
    """full_ce_fwd(train=True) + full_ce_dw: sums[1] is the (global) count 7 on entry and must stay; with no live tile the loss sum
    is exactly 0 whatever sums[0] and the partials scratch held, dh is zero on every row and dw is bitwise unchanged.  rg_full_ce_* has
    no unlisted form (live16 is required), so the one-live-row case is held to the same row run alone, not to an unlisted call: loss and dh bit for bit, dw (another
    split of the rows among workgroups) under the bounds test_full_softmax_gpu.py holds a half batch to the whole one with."""
    from recguru_amd import hip
    C = 301
    h = rnd(M, d, dt=dt, scale=0.3, seed=1)
    w = rnd(C, d, dt=dt, seed=2)
    assert hip.full_ce_supported(d, h)
    labels = torch.randint(0, C, (M,), generator=torch.Generator().manual_seed(3)).cuda()
    mask = _list_mask(M, which)
    live = _live(mask, M, which)
    sums = torch.tensor([float("nan"), 7.0], device="cuda")
    lse, dh = hip.full_ce_fwd(h, w, labels, mask, live, sums, train=True)
    assert float(sums[1]) == 7.0
    dw0 = rnd(C, d, dt=torch.float32, seed=4)
    dw = dw0.clone()
    gout = torch.full((1,), 0.7, device="cuda")
    hip.full_ce_dw(h, w, labels, mask, live, lse, sums, gout, dw)
    assert bool(torch.isfinite(dh.float()).all()) and bool(torch.isfinite(dw).all())
    if which == "zero":
        assert float(sums[0]) == 0.0
        assert float(dh.float().abs().max()) == 0.0
        assert torch.equal(dw, dw0)
        return
    # one live row: the same row run alone (n = 1)
    assert float(dh[: M - 1].float().abs().max()) == 0.0
    h1, l1, m1 = h[M - 1:].contiguous(), labels[M - 1:].contiguous(), torch.ones(1, device="cuda")
    live1 = hip.live_tiles(m1, 1)
    s1 = torch.tensor([float("nan"), 7.0], device="cuda")
    lse1, dh1 = hip.full_ce_fwd(h1, w, l1, m1, live1, s1, train=True)
    dw1 = dw0.clone()
    hip.full_ce_dw(h1, w, l1, m1, live1, lse1, s1, gout, dw1)
    assert torch.equal(sums[0], s1[0]) and torch.equal(dh[M - 1:], dh1)       # the loss and dh of a row depend on that row alone
    torch.testing.assert_close(dw, dw1, rtol=1e-5, atol=1e-7)
    assert not torch.equal(dw, dw0)


# ======================================================================================================= d. local count of zero
LOSS_CASES = [(5, 0), (5, 1), (5, 2), (30, 0), (300, 0)]          # (k, mode); k = 300: the online training form


def _loss_inputs(dt, k, ntok, seed=0):
    V, d = 97, 128
    g0 = torch.Generator().manual_seed(k + seed)
    h = rnd(ntok, d, dt=dt, scale=0.3, seed=1 + seed)
    table = rnd(V + 2, d, dt=dt, seed=2)
    pos = torch.randint(1, V + 1, (ntok,), generator=g0).cuda()
    neg = torch.randint(1, V + 1, (ntok, k), generator=g0).cuda()
    return V, d, h, table, pos, neg


def _peer_count(sums):
    """What global_count does on a shard whose peers hold live positions: the all-reduced count replaces the local one."""
    sums[1] = 5.0
    return sums


@pytest.mark.parametrize("k,mode", LOSS_CASES)
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_item_loss_local_count_zero(dt, k, mode):
    """mask all zero, sums[1] = 5 (the global count): loss sum 0, dh exactly zero, dE bitwise its random pre-fill."""
    from recguru_amd import hip
    ntok = 61
    V, d, h, table, pos, neg = _loss_inputs(dt, k, ntok)
    mask = torch.zeros(ntok, device="cuda")
    sums, aux = hip.item_loss_fwd(h, table, pos, neg, mask, k, mode)
    assert float(sums[0]) == 0.0 and float(sums[1]) == 0.0
    _peer_count(sums)
    gout = torch.full((1,), 1.7, device="cuda")
    dE0 = rnd(V + 2, d, dt=torch.float32, seed=9)
    dE = dE0.clone()
    dh = hip.item_loss_bwd(h, table, pos, neg, mask, k, mode, aux, sums, gout, dE)
    assert float(dh.float().abs().max()) == 0.0
    assert torch.equal(dE, dE0)


@pytest.mark.parametrize("k,mode", LOSS_CASES)
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_item_loss_binned_local_count_zero(dt, k, mode):
    from recguru_amd import hip
    if hip.DETERMINISTIC:
        pytest.skip(BINNED_SKIP)
    ntok = 61
    V, d, h, table, pos, neg = _loss_inputs(dt, k, ntok)
    assert hip.item_loss_bwd_binned_supported(ntok, k, d, V + 2)
    mask = torch.zeros(ntok, device="cuda")
    sums, aux = hip.item_loss_fwd(h, table, pos, neg, mask, k, mode)
    _peer_count(sums)
    gout = torch.full((1,), 1.7, device="cuda")
    dE0 = rnd(V + 2, d, dt=torch.float32, seed=9)
    dE = dE0.clone()
    dh = hip.item_loss_bwd_binned(h, table, pos, neg, mask, k, mode, aux, sums, gout, dE)
    assert float(dh.float().abs().max()) == 0.0
    assert torch.equal(dE, dE0)


@pytest.mark.parametrize("k,mode", LOSS_CASES)
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_item_loss_train_local_count_zero(dt, k, mode):
    from recguru_amd import hip
    if hip.DETERMINISTIC:
        pytest.skip(BINNED_SKIP)
    ntok = 61
    V, d, h, table, pos, neg = _loss_inputs(dt, k, ntok)
    form = hip.item_loss_train_supported(k, d)
    assert form == (2 if k == 300 else 1)
    mask = torch.zeros(ntok, device="cuda")
    s2 = _peer_count(torch.zeros(2, device="cuda"))
    lse = torch.full((ntok,), float("nan"), device="cuda") if form == 2 else None
    coef, dh = hip.item_loss_train(h, table, pos, neg, mask, k, mode, s2, lse=lse)
    assert float(s2[0]) == 0.0 and float(s2[1]) == 5.0
    assert float(dh.float().abs().max()) == 0.0
    gout = torch.full((1,), 1.7, device="cuda")
    hip.scale_dev(dh, gout)
    dE0 = rnd(V + 2, d, dt=torch.float32, seed=9)
    dE = dE0.clone()
    hip.item_loss_scatter_binned(h, V + 2, pos, neg, mask, k, coef, gout, dE, **(dict(lse=lse, sums=s2) if form == 2 else {}))
    assert float(dh.float().abs().max()) == 0.0
    assert torch.equal(dE, dE0)


@pytest.mark.parametrize("k,mode", LOSS_CASES)
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_item_loss_live_rows_do_not_depend_on_dead_rows(dt, k, mode):
    """Two all-padding sequences in front of live ones: dh and dE of the batch == those of the live tokens run alone (dh of a row
    depends on that row alone: bitwise; dE under the binned-vs-atomic bounds of test_item_loss)."""
    from recguru_amd import hip
    Ls, nlive = 23, 61
    ntok = 2 * Ls + nlive
    V, d, h, table, pos, neg = _loss_inputs(dt, k, ntok)
    mask = (torch.rand(ntok, generator=torch.Generator().manual_seed(4)) > 0.3).float().cuda()
    mask[: 2 * Ls] = 0.0
    pos[: 2 * Ls] = 0
    s = slice(2 * Ls, ntok)
    cut = lambda t: t[s].contiguous()
    gout = torch.full((1,), 1.7, device="cuda")
    runs = []
    for hh, pp, nn, mm in ((h, pos, neg, mask), (cut(h), cut(pos), cut(neg), cut(mask))):
        n = hh.shape[0]
        sums, aux = hip.item_loss_fwd(hh, table, pp, nn, mm, k, mode)
        dE = torch.zeros(V + 2, d, device="cuda")
        dh = hip.item_loss_bwd(hh, table, pp, nn, mm, k, mode, aux, sums, gout, dE)
        out = [sums, dh, dE]
        if not hip.DETERMINISTIC:
            dE2 = torch.zeros(V + 2, d, device="cuda")
            out += [hip.item_loss_bwd_binned(hh, table, pp, nn, mm, k, mode, aux, sums, gout, dE2), dE2]
            form = hip.item_loss_train_supported(k, d)
            s2 = torch.zeros(2, device="cuda")
            hip.sum_into(mm, s2[1:2])
            lse = torch.empty(n, device="cuda") if form == 2 else None
            coef, dh3 = hip.item_loss_train(hh, table, pp, nn, mm, k, mode, s2, lse=lse)
            hip.scale_dev(dh3, gout)
            dE3 = torch.zeros(V + 2, d, device="cuda")
            hip.item_loss_scatter_binned(hh, V + 2, pp, nn, mm, k, coef, gout, dE3, **(dict(lse=lse, sums=s2) if form == 2 else {}))
            out += [dh3, dE3]
        runs.append(out)
    whole, alone = runs
    assert float(whole[0][1]) == float(alone[0][1]) > 0
    torch.testing.assert_close(whole[0][0], alone[0][0], rtol=1e-5, atol=1e-6)
    for i in range(1, len(whole), 2):
        assert float(whole[i][: 2 * Ls].float().abs().max()) == 0.0
        assert torch.equal(whole[i][s], alone[i])
        torch.testing.assert_close(whole[i + 1], alone[i + 1], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("k,mode", [(5, 0), (5, 1), (5, 2)])
def test_item_loss_single_process_count_zero_matches_the_reference(k, mode):
    """sums[1] left at 0, as in a single process whose whole batch is padding.  The reference divides by mask.sum()
    (oracle/recguru_oracle.py sampled_ce / bpr_loss / bpr_loss_sas): its loss is 0 / 0 = NaN and so is every gradient it returns
    -- recorded here, so nothing can be asserted about the kernels' values: only that the loss is the same 0 / 0 and that no call
    raises or returns an error, in the two-call, the binned and the training form."""
    from oracle import recguru_oracle as O
    from recguru_amd import hip
    dt = torch.float32
    ntok = 61
    V, d, h, table, pos, neg = _loss_inputs(dt, k, ntok)
    mask = torch.zeros(ntok, device="cuda")
    hf, tf = h.cpu().requires_grad_(True), table.cpu().requires_grad_(True)
    lp = (hf * tf[pos.cpu()]).sum(1, keepdim=True)
    ln_ = torch.einsum("td,tkd->tk", hf, tf[neg.cpu()])
    m = mask.cpu()
    if mode == 0:
        ref = O.sampled_ce(torch.cat([lp, ln_], 1).view(1, ntok, 1 + k), m)
    else:
        ref = (O.bpr_loss if mode == 1 else O.bpr_loss_sas)(lp.view(1, ntok), ln_.view(1, ntok, k), m)
    ref.backward()
    assert math.isnan(float(ref)) and bool(torch.isnan(tf.grad).any())       # the reference's own loss and gradient are NaN
    sums, aux = hip.item_loss_fwd(h, table, pos, neg, mask, k, mode)
    assert float(sums[0]) == 0.0 and float(sums[1]) == 0.0 and math.isnan(float(sums[0] / sums[1]))
    gout = torch.ones(1, device="cuda")
    dE = torch.zeros(V + 2, d, device="cuda")
    hip.item_loss_bwd(h, table, pos, neg, mask, k, mode, aux, sums, gout, dE)
    if not hip.DETERMINISTIC:
        dE2 = torch.zeros(V + 2, d, device="cuda")
        hip.item_loss_bwd_binned(h, table, pos, neg, mask, k, mode, aux, sums, gout, dE2)
        s2 = torch.zeros(2, device="cuda")
        coef, dh = hip.item_loss_train(h, table, pos, neg, mask, k, mode, s2)
        assert float(s2[0]) == 0.0 and float(s2[1]) == 0.0
        hip.scale_dev(dh, gout)
        hip.item_loss_scatter_binned(h, V + 2, pos, neg, mask, k, coef, gout, torch.zeros(V + 2, d, device="cuda"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("binned", [False, True])
@pytest.mark.parametrize("what", ["ids", "mask", "both"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_embed_scatter_nothing_live(dt, what, binned):
    """Every id 0 (the skip row) and / or every mask 0: the table gradient is bitwise its pre-fill."""
    from recguru_amd import hip
    if binned and hip.DETERMINISTIC:
        pytest.skip(BINNED_SKIP)
    ntok, d, V = 61, 128, 97
    g0 = torch.Generator().manual_seed(5)
    ids = torch.randint(1, V + 1, (ntok,), generator=g0).cuda()
    mask = (torch.rand(ntok, generator=g0) > 0.3).float().cuda()
    if what in ("ids", "both"):
        ids.zero_()
    if what in ("mask", "both"):
        mask.zero_()
    dx = rnd(ntok, d, dt=dt, scale=0.5, seed=3)
    dE0 = rnd(V + 2, d, dt=torch.float32, seed=9)
    dE = dE0.clone()
    fn = hip.embed_scatter_bwd_binned if binned else hip.embed_scatter_bwd
    fn(dx, ids, mask, dE, skip_row=0, drop_p=0.5, seed=77)
    assert torch.equal(dE, dE0)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_embed_scatter_live_rows_do_not_depend_on_dead_rows(dt):
    from recguru_amd import hip
    Ls, nlive, d, V = 23, 61, 128, 97
    ntok = 2 * Ls + nlive
    g0 = torch.Generator().manual_seed(6)
    ids = torch.randint(1, V + 1, (ntok,), generator=g0).cuda()
    mask = (torch.rand(ntok, generator=g0) > 0.3).float().cuda()
    ids[: 2 * Ls] = 0
    mask[: 2 * Ls] = 0.0
    dx = rnd(ntok, d, dt=dt, scale=0.5, seed=3)
    s = slice(2 * Ls, ntok)
    fns = [hip.embed_scatter_bwd] + ([] if hip.DETERMINISTIC else [hip.embed_scatter_bwd_binned])
    for fn in fns:
        a, b = torch.zeros(V + 2, d, device="cuda"), torch.zeros(V + 2, d, device="cuda")
        fn(dx, ids, mask, a, skip_row=0)                          # (no dropout: its mask is a function of the token index)
        fn(dx[s].contiguous(), ids[s].contiguous(), mask[s].contiguous(), b, skip_row=0)
        assert float(b.abs().max()) > 0
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)   # test_embed_scatter_binned_equals_atomic_form
