"""Every dropout site against the host restatement of the mask contract (tests/dropmask.py).

Each test checks the mask itself exactly -- inputs bounded away from zero, or one-hot operands that expose an internal mask,
so that the kernel's set of zeros must equal the host mask's set of drops element for element -- and the values against a
float64 reference that applies the host mask explicitly.  Seeds differ in their high 32 bits (ops._draw() streams differ there
only).  The last test runs the attention map past the 2^32 wrap of its index space (config-5 scale)."""
import math
import os

import numpy as np
import pytest
import torch

import dropmask as dm

pytestmark = pytest.mark.gpu

SEEDS = [(3 << 32) | 77, (11 << 32) | 77]          # same low half, different high half
F32_TOL = 2e-5


def _dev(m):
    return torch.from_numpy(np.ascontiguousarray(m)).cuda()


def _away_from_zero(shape, seed, dt):
    g = torch.Generator().manual_seed(seed)
    x = (1 + torch.rand(*shape, generator=g)) * torch.where(torch.rand(*shape, generator=g) < 0.5, -1.0, 1.0)
    return x.to(dt).cuda()


def _rnd(*shape, seed=0, scale=1.0, dt=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dt).cuda()


def _close(got, ref, dt, what):
    """The tier's tolerance: f32 2e-5; bf16 as test_kernels_gpu.tol; relative to max |ref| for the bf16x3 tier."""
    got, ref = got.double(), ref.double()
    if dt == "x3":
        err = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
        assert err <= 4e-5, "%s: max error %.3g of max |value|" % (what, err)
    elif dt == torch.float32:
        torch.testing.assert_close(got, ref, rtol=F32_TOL, atol=F32_TOL, msg=lambda m: what + ": " + m)
    else:
        torch.testing.assert_close(got, ref, rtol=2e-2, atol=2e-2, msg=lambda m: what + ": " + m)


def _same_zeros(got, keepmask, what, where=None):
    """got == 0 exactly where the host mask drops (restricted to `where`)."""
    z = (got == 0).cpu().numpy()
    d = (np.asarray(keepmask) == 0)
    if where is not None:
        where = np.asarray(where)
        z, d = z[where], d[where]
    bad = np.flatnonzero(z != d)
    assert bad.size == 0, "%s: %d of %d elements differ from the host mask (first flat positions %s)" % (
        what, bad.size, z.size, bad[:8].tolist())


# ================================================================================================================ anchor
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N", [(37, 41), (129, 77), (64, 256), (333, 40)])   # odd M*N / N % 8 != 0, and N % 8 == 0
@pytest.mark.parametrize("p,seed", [(0.5, SEEDS[0]), (0.3, SEEDS[1]), (0.5, SEEDS[1]), (0.3, SEEDS[0])])
def test_dropout_anchor(dt, M, N, p, seed):
    from recguru_amd import hip
    x = _away_from_zero((M, N), M * N, dt)
    y = x.clone()
    hip.dropout_(y, p, seed)
    k = dm.rowmajor_mask(seed, p, M, N)
    _same_zeros(y, k, "dropout_")
    ref = x.double() * _dev(k)
    _close(y, ref.to(dt) if dt == torch.bfloat16 else ref, dt, "dropout_")


# ================================================================================================================ elementwise
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("p,seed", [(0.5, SEEDS[0]), (0.3, SEEDS[1])])
def test_dropout_gelu_add_drop_ln_ln_bwd(dt, p, seed):
    from recguru_amd import hip
    M, F = 333, 512
    h = _away_from_zero((M, F), 1, dt)
    h0 = h.clone()
    g = hip.dropout_gelu(h, p, seed)
    k = dm.rowmajor_mask(seed, p, M, F)
    _same_zeros(h, k, "dropout_gelu (stored x)")
    hd = h0.double() * _dev(k)
    _close(h, hd.to(dt) if dt == torch.bfloat16 else hd, dt, "dropout_gelu x")
    hs = h.double()
    gr = 0.5 * hs * (1 + torch.tanh(math.sqrt(2 / math.pi) * (hs + 0.044715 * hs ** 3)))
    _close(g, gr, dt, "dropout_gelu gelu")
    for N in (128, 256):
        x = _rnd(M, N, seed=2, dt=dt)
        z = _away_from_zero((M, N), 3, dt)
        gam = 1 + 0.1 * _rnd(N, seed=4)
        bet = 0.1 * _rnd(N, seed=5)
        rm = (torch.arange(M, device="cuda") % 5 != 0).float()
        y, rstd = hip.add_drop_ln(x, z, gam, bet, rm, p, seed)
        kz = _dev(dm.rowmajor_mask(seed, p, M, N))
        ref = torch.nn.functional.layer_norm(x.double() + z.double() * kz, (N,), gam.double(), bet.double(), 1e-8) * rm[:, None].double()
        _close(y, ref, dt, "add_drop_ln N=%d" % N)
        # ln_bwd's dz_drop: dz * mask / (1 - p) in the same index space
        dy = _rnd(M, N, seed=6, dt=dt)
        dgam = torch.zeros(N, device="cuda")
        dbet = torch.zeros(N, device="cuda")
        dz, dzd = hip.ln_bwd(dy, y, rstd, gam, bet, rm, dgam, dbet, drop_p=p, drop_seed=seed)
        live = (dz != 0).cpu().numpy()
        _same_zeros(dzd, kz.cpu().numpy(), "ln_bwd dz_drop N=%d" % N, where=live)
        _close(dzd, (dz.double() * kz).to(dt) if dt == torch.bfloat16 else dz.double() * kz, dt, "ln_bwd dz_drop")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", [320, 40, 37])            # vector epilogue (N % 8 == 0) and the element tail
@pytest.mark.parametrize("p,seed", [(0.2, SEEDS[0]), (0.5, SEEDS[1]), (0.3, SEEDS[1])])
def test_gemm_nt_relu_dropout_epilogue(dt, N, p, seed):
    """EPI_RELU + drop_p on the generic kernel (the unfused discriminator, ops._disc_fwd): a large bias keeps every
    pre-activation positive, so the zeros are the mask."""
    from recguru_amd import hip
    M, K = 133, 64
    A = _rnd(M, K, seed=1, dt=dt)
    W = _rnd(N, K, seed=2, scale=0.05, dt=dt)
    bias = 8 + _rnd(N, seed=3).abs()
    h = hip.gemm_nt(A, W, bias, epilogue=hip.EPI_RELU, drop_p=p, drop_seed=seed)
    k = dm.rowmajor_mask(seed, p, M, N)
    _same_zeros(h, k, "gemm_nt relu+dropout")
    ref = torch.relu(A.double() @ W.double().T + bias.double()) * _dev(k)
    _close(h, ref, dt, "gemm_nt relu+dropout")


@pytest.mark.parametrize("p,seed", [(0.5, SEEDS[0]), (0.3, SEEDS[1])])
def test_gemm_ws_drop_gelu_epilogue(p, seed):
    """EPI_DROP_GELU exists on the bf16 weight-stationary kernel only (the library refuses it elsewhere)."""
    from recguru_amd import hip
    dt = torch.bfloat16
    M, K, N = 4096 + 64 * 3 + 7, 256, 512
    A = _rnd(M, K, seed=1, dt=dt)
    W = _rnd(N, K, seed=2, scale=0.02, dt=dt)
    bias = 4 + _rnd(N, seed=3).abs()                   # pre-activations in [~2, ~8]: away from zero
    g2 = torch.empty(M, N, device="cuda", dtype=dt)
    h = hip.gemm_nt(A, W, bias, epilogue=hip.EPI_DROP_GELU, drop_p=p, drop_seed=seed, out2=g2)
    k = dm.rowmajor_mask(seed, p, M, N)
    _same_zeros(h, k, "gemm_ws drop_gelu C")
    ref = (A.double() @ W.double().T + bias.double()) * _dev(k)
    _close(h, ref, dt, "gemm_ws drop_gelu C")
    hs = h.double()
    _close(g2, 0.5 * hs * (1 + torch.tanh(math.sqrt(2 / math.pi) * (hs + 0.044715 * hs ** 3))), dt, "gemm_ws drop_gelu gelu")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("p,seed", [(0.5, SEEDS[0]), (0.3, SEEDS[1])])
def test_embedding_dropout(dt, d, p, seed):
    """embed_pe_fwd (plain entry, fwd2 with its mirror, fwd_rows under both store policies, fwd_split for f32 tables) and
    embed_scatter_bwd / its binned form: index token * d + feature."""
    from recguru_amd import hip
    B, L, V = 9, 37, 60
    table = (_rnd(V + 2, d, seed=1).abs() + 1).to(dt)
    pe = _rnd(64, d, seed=2, scale=0.1).abs()
    ids = torch.randint(1, V, (B, L), generator=torch.Generator().manual_seed(3)).cuda()
    ids[:, :5] = 0
    mask = (ids != 0).float().reshape(-1)
    ntok = B * L
    k = dm.rowmajor_mask(seed, p, ntok, d)
    kd = _dev(k)
    ref = (table.double()[ids].reshape(ntok, d) + pe.double()[:L].repeat(B, 1)) * mask.double()[:, None] * kd
    live = np.broadcast_to(mask.cpu().numpy()[:, None] != 0, (ntok, d))
    outs = {"rows policy auto": (hip.embed_pe_fwd(table, pe, ids, mask, L, drop_p=p, seed=seed), dt)}
    if d in (128, 256):                              # rg_embed_pe_fwd2's second output
        o, o2 = hip.embed_pe_fwd(table, pe, ids, mask, L, drop_p=p, seed=seed, mirror=True)
        outs["fwd2"], outs["fwd2 mirror"] = (o, dt), (o2, torch.bfloat16)
    for rows in (None, V + 2, 1 << 33):              # plain entry (table size unknown), ordinary / nontemporal stores
        out = torch.full((ntok, d), float("nan"), device="cuda", dtype=dt)
        if rows is None:
            rc = hip.lib().rg_embed_pe_fwd(hip._vp(table), hip._vp(pe), hip._vp(ids), hip._vp(mask), hip._vp(out), hip.c_ll(ntok), L,
                                           d, hip.c_f(p), hip.c_u64(seed), hip.dt_of(table), hip._stream())
        else:
            rc = hip.lib().rg_embed_pe_fwd_rows(hip._vp(table), hip.c_ll(rows), hip._vp(pe), hip._vp(ids), hip._vp(mask), hip._vp(out),
                                                hip.c_ll(ntok), L, d, hip.c_f(p), hip.c_u64(seed), hip.dt_of(table), hip._stream())
        assert rc == 0
        outs["plain" if rows is None else "rows %d" % rows] = (out, dt)
    if dt == torch.float32:
        hi, lo = hip.embed_pe_fwd_split(table, pe, ids, mask, L, drop_p=p, seed=seed)
        outs["split hi + lo"] = (hi.float() + lo.float(), torch.float32)
    for name, (out, tk) in outs.items():
        _same_zeros(out.reshape(ntok, d), k, "embed_pe_fwd %s" % name, where=live)
        _close(out.reshape(ntok, d).float(), ref, tk, "embed_pe_fwd %s" % name)
    dx = _rnd(ntok, d, seed=4, dt=dt)
    refE = torch.zeros(V + 2, d, dtype=torch.float64, device="cuda").index_add_(
        0, ids.view(-1), dx.double() * mask.double()[:, None] * kd)
    dE = torch.zeros(V + 2, d, device="cuda")
    hip.embed_scatter_bwd(dx, ids, mask, dE, drop_p=p, seed=seed)
    tol = dict(rtol=1e-5, atol=1e-4) if dt == torch.float32 else dict(rtol=2e-2, atol=5e-2)
    torch.testing.assert_close(dE.double(), refE, **tol)
    if hip.embed_scatter_binned_supported(ntok, d, V + 2):
        dE2 = torch.zeros(V + 2, d, device="cuda")
        hip.embed_scatter_bwd_binned(dx, ids, mask, dE2, drop_p=p, seed=seed)
        torch.testing.assert_close(dE2.double(), refE, **tol)


@pytest.mark.parametrize("p,seed", [(0.5, SEEDS[0]), (0.3, SEEDS[1]), (0.5, SEEDS[1])])
@pytest.mark.parametrize("B,L,H", [(5, 50, 4), (3, 64, 2), (2, 130, 3)])
def test_cross_drop_scale(p, seed, B, L, H):
    """Row sums of the dropped uniform cross-attention map (attention-map index space), incl. an all-masked row."""
    from recguru_amd import hip
    ids = torch.randint(1, 9, (B, L), generator=torch.Generator().manual_seed(L)).cuda()
    ids[:, : L // 3] = 0
    ids[0, :] = 0
    s = hip.cross_drop_scale(ids, 0, H, p, seed).view(B, L, H).double().cpu().numpy()
    live = (ids != 0).cpu().numpy()
    live[0, :] = True                                        # all masked: uniform over all L keys
    m = dm.attn_mask(seed, p, H, L, range(B))                # [B, H, q, key]
    ref = (m * live[:, None, None, :]).sum(-1) / live.sum(1)[:, None, None]
    np.testing.assert_allclose(s, ref.transpose(0, 2, 1), rtol=1e-5, atol=1e-6)


# ================================================================================================================ fused block
@pytest.mark.parametrize("dt,d,M,dff", [(torch.float32, 128, 203, 512), (torch.bfloat16, 128, 203, 512), (torch.float32, 128, 9000, 512),
                                        (torch.bfloat16, 128, 9000, 512), (torch.bfloat16, 256, 333, 1024)])
@pytest.mark.parametrize("p,seed", [(0.5, SEEDS[0]), (0.3, SEEDS[1])])
def test_post_attn_block_masks(dt, d, M, dff, p, seed):
    """post_attn_fwd(save=True): the saved h1 is the dropped first FFN activation (seed_h1, index row * d_ff + col) and the
    output is LayerNorm(dropout(gelu(h1) W2^T + b2) + y) with the second mask (seed_out, index row * d + col): d = 128
    (fused.hip, incl. the bf16 row-shared hash words at large M) and d = 256 (fused256.hip)."""
    from recguru_amd import hip
    P = d
    assert hip.post_attn_supported(d, P, dff, dt, M)
    s_h1, s_out = seed, seed ^ (5 << 32)
    ctx, x = _rnd(M, P, seed=1, dt=dt), _rnd(M, d, seed=2, dt=dt)
    Wo, W1, W2 = _rnd(d, P, seed=3, scale=P ** -0.5, dt=dt), _rnd(dff, d, seed=4, scale=d ** -0.5, dt=dt), \
        _rnd(d, dff, seed=5, scale=dff ** -0.5, dt=dt)
    bo, b1, b2 = (0.1 * _rnd(n, seed=6 + i) for i, n in enumerate((d, dff, d)))
    g1, g2 = (1 + 0.1 * _rnd(d, seed=10 + i) for i in range(2))
    be1, be2 = (0.1 * _rnd(d, seed=20 + i) for i in range(2))
    rm = (torch.arange(M) % 5 != 2).float().cuda()
    if d == 256:        # fused256.hip takes fragment-packed weights (ops.shadow(pack=True))
        pk = lambda w: hip.cast(w.float().contiguous(), torch.bfloat16, transpose=hip.CAST_PACK)
        out, sv = hip.post_attn_fwd(ctx, x, pk(Wo), bo, g1, be1, pk(W1), b1, pk(W2), b2, g2, be2, rm, save=True, drop_p=p,
                                    seed_h1=s_h1, seed_out=s_out, w_packed=True)
    else:
        out, sv = hip.post_attn_fwd(ctx, x, Wo, bo, g1, be1, W1, b1, W2, b2, g2, be2, rm, save=True, drop_p=p, seed_h1=s_h1,
                                    seed_out=s_out)
    k1 = dm.rowmajor_mask(s_h1, p, M, dff)
    k2 = _dev(dm.rowmajor_mask(s_out, p, M, d))
    live = np.broadcast_to(rm.cpu().numpy()[:, None] != 0, (M, dff))
    _same_zeros(sv["h1"], k1, "post_attn_fwd saved h1 (seed_h1)", where=live)
    F = torch.nn.functional
    y = sv["y"].double()
    h1 = (y @ W1.double().T + b1.double()) * _dev(k1)
    lv = rm != 0
    _close(sv["h1"][lv], h1[lv], dt, "post_attn_fwd h1")
    hs = sv["h1"].double()                                      # the stored (rounded) operand the kernel feeds on
    g = 0.5 * hs * (1 + torch.tanh(math.sqrt(2 / math.pi) * (hs + 0.044715 * hs ** 3)))
    if dt == torch.bfloat16:
        g = g.to(dt).double()
    z2 = (g @ W2.double().T + b2.double()) * k2 + y
    ref = F.layer_norm(z2, (d,), g2.double(), be2.double(), 1e-8) * rm[:, None].double()
    t = dict(rtol=1e-4, atol=1e-4) if dt == torch.float32 else dict(rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(out.double(), ref, **t, msg=lambda m: "post_attn_fwd out (seed_out): " + m)
    # a mask under seed_h1 in place of seed_out gives a different output
    alt = F.layer_norm((g @ W2.double().T + b2.double()) * _dev(dm.rowmajor_mask(s_h1, p, M, d)) + y, (d,), g2.double(),
                       be2.double(), 1e-8) * rm[:, None].double()
    assert float((alt - ref).abs().max()) > 10 * t["atol"]


# ================================================================================================================ attention
def _attn_case(B, L, H, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 50, (B, L), generator=g)
    lens = torch.randint(max(1, L // 3), L + 1, (B,), generator=g)
    lens[0] = L
    rm = (torch.arange(L)[None, :] >= (L - lens)[:, None])
    ids = ids * rm.long()                                    # left padding carries id 0
    return ids.cuda(), rm.float().reshape(-1).cuda()


def _ref64(qkv, ids, pad, causal, H, kmask):
    """float64 attention with an explicit dropout multiplier kmask [B,H,L,L]: ctx, lse (of the undropped scores), A_drop."""
    B, L, P3 = qkv.shape
    P = P3 // 3
    q, k, v = [t.reshape(B, L, H, 32).transpose(1, 2) for t in qkv.split(P, dim=2)]
    s = q @ k.transpose(-1, -2) / math.sqrt(32)
    m = ids.eq(pad)[:, None, None, :].expand(B, H, L, L)
    if causal:
        m = m | torch.ones(L, L, dtype=torch.bool, device=qkv.device).triu(1)
    s = s.masked_fill(m, -1e9)
    a = torch.softmax(s, -1)
    ad = a * kmask
    return (ad @ v).transpose(1, 2).reshape(B, L, P), torch.logsumexp(s, -1), a, ad


def _tier(name):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "x3": torch.float32}[name]


class _Tier:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        from recguru_amd import hip
        self.prev = hip.SPLIT_OPERANDS
        hip.SPLIT_OPERANDS = self.name == "x3"

    def __exit__(self, *a):
        from recguru_amd import hip
        hip.SPLIT_OPERANDS = self.prev


def _tolkey(name):
    return "x3" if name == "x3" else _tier(name)


ATTN_L = [20, 32, 50, 64, 128, 200, 224, 256, 300, 416]   # every key-tile bucket (nkt 2 .. 26) with its upper edge


@pytest.mark.parametrize("tier", ["f32", "bf16", "x3"])
@pytest.mark.parametrize("L", ATTN_L)
@pytest.mark.parametrize("p,seed", [(0.5, SEEDS[0]), (0.3, SEEDS[1])])
def test_attention_masks(tier, L, p, seed):
    """Full attention map, token-major: forward mask through one-hot V chunks (ctx[:, q, c] = A_drop[q, 32 chunk + c]),
    backward mask through one-hot dctx chunks (dV[key, c] = A_drop[32 chunk + c, key]), then ctx / lse / dqkv against float64
    autograd through softmax(...) * host mask.  Causal at every other length, left padding with a row mask."""
    from recguru_amd import hip
    dt = _tier(tier)
    B, H = 2, 2
    P = H * 32
    causal = ATTN_L.index(L) % 2 == 1
    pad = 0 if causal else 51
    ids, rm = _attn_case(B, L, H, L)
    qk = _rnd(B, L, 2 * P, seed=L + 1, dt=dt)
    vr = _rnd(B, L, P, seed=L + 2, dt=dt)
    kmask = dm.attn_mask(seed, p, H, L, range(B))
    km = _dev(kmask)
    qkv = torch.cat([qk, vr], 2).contiguous()
    _, _, a_ref, ad_ref = _ref64(qkv.double(), ids, pad, causal, H, km)
    rows = rm.view(B, L).cpu().numpy() != 0                      # live query rows
    live = (a_ref.cpu().numpy() > 1e-6) & rows[:, None, :, None]
    kw = dict(drop_p=p, seed=seed, rowmask=rm)
    nch = (L + 31) // 32
    tk = _tolkey(tier)
    with _Tier(tier):
        # ---- forward mask, one 32-key chunk at a time
        A = torch.zeros(B, H, L, L, dtype=torch.float64, device="cuda")
        for c in range(nch):
            v = torch.zeros(B, L, H, 32, dtype=dt, device="cuda")
            n = min(32, L - 32 * c)
            v[:, 32 * c: 32 * c + n, :, :n] = torch.eye(n, dtype=dt, device="cuda")[None, :, None, :]
            ctx, _ = hip.attn_fwd(torch.cat([qk, v.reshape(B, L, P)], 2).contiguous(), ids, pad, causal, H, **kw)
            A[:, :, :, 32 * c: 32 * c + n] = ctx.double().view(B, L, H, 32)[..., :n].permute(0, 2, 1, 3)
        _same_zeros(A, kmask, "forward mask", where=live)
        _close(A[torch.from_numpy(live).cuda()], ad_ref[torch.from_numpy(live).cuda()], tk, "forward A_drop")
        # ---- backward mask, one 32-query chunk of dctx at a time
        ctx, lse = hip.attn_fwd(qkv, ids, pad, causal, H, **kw)
        for form in ("one", "two"):
            if form == "two":
                os.environ["RG_ATTN_BWD_TWO_PHASE"] = "1"
            try:
                Ab = torch.zeros(B, H, L, L, dtype=torch.float64, device="cuda")
                for c in range(nch):
                    n = min(32, L - 32 * c)
                    dctx = torch.zeros(B, L, H, 32, dtype=dt, device="cuda")
                    dctx[:, 32 * c: 32 * c + n, :, :n] = torch.eye(n, dtype=dt, device="cuda")[None, :, None, :]
                    dctx = (dctx.reshape(B, L, P) * rm.view(B, L, 1).to(dt)).contiguous()
                    dqkv = hip.attn_bwd(qkv, dctx, ctx, lse, ids, pad, causal, H, **kw)
                    Ab[:, :, 32 * c: 32 * c + n, :] = dqkv[:, :, 2 * P:].double().view(B, L, H, 32)[..., :n].permute(0, 2, 3, 1)
            finally:
                os.environ.pop("RG_ATTN_BWD_TWO_PHASE", None)
            _same_zeros(Ab, kmask, "backward mask (%s-pass form)" % form, where=live)
        # ---- values against float64 autograd through the host mask
        x = qkv.double().requires_grad_(True)
        cr, lr, _, _ = _ref64(x, ids, pad, causal, H, km)
        dctx = (_rnd(B, L, P, seed=L + 3, dt=dt) * rm.view(B, L, 1).to(dt)).contiguous()
        (cr * dctx.double()).sum().backward(retain_graph=True)
        dqkv = hip.attn_bwd(qkv, dctx, ctx, lse, ids, pad, causal, H, **kw)
        lv = torch.from_numpy(rows).cuda()
        _close(ctx[lv], cr.detach()[lv], tk, "ctx")
        torch.testing.assert_close(lse.transpose(1, 2)[lv].double(), lr.detach().transpose(1, 2)[lv], rtol=1e-4,
                                   atol=1e-3 if dt == torch.float32 else 3e-2)
        g = x.grad
        if tk == torch.float32:
            torch.testing.assert_close(dqkv.double(), g, rtol=1e-3, atol=1e-4)
        elif tk == "x3":
            err = float((dqkv.double() - g).abs().max()) / float(g.abs().max())
            assert err <= 6e-5, "dqkv: max error %.3g of max |value|" % err
        else:
            torch.testing.assert_close(dqkv.double(), g, rtol=5e-2, atol=5e-2)
        # ---- single-query kernels: row L-1 of the same index space
        if not causal:
            q_last = qkv[:, -1, :P].contiguous()
            kv = qkv[:, :, P:].contiguous()
            for c in range(nch):
                n = min(32, L - 32 * c)
                v = torch.zeros(B, L, H, 32, dtype=dt, device="cuda")
                v[:, 32 * c: 32 * c + n, :, :n] = torch.eye(n, dtype=dt, device="cuda")[None, :, None, :]
                kvo = torch.cat([qk[:, :, P:], v.reshape(B, L, P)], 2).contiguous()
                cl = hip.attn_lastq_fwd(q_last, kvo, ids, pad, H, drop_p=p, seed=seed)
                got = cl.double().view(B, H, 32)[..., :n]
                want = A[:, :, L - 1, 32 * c: 32 * c + n]
                _same_zeros(got, kmask[:, :, L - 1, 32 * c: 32 * c + n], "attn_lastq_fwd mask",
                            where=live[:, :, L - 1, 32 * c: 32 * c + n])
                _close(got, want, tk, "attn_lastq_fwd row")
            cl = hip.attn_lastq_fwd(q_last, kv, ids, pad, H, drop_p=p, seed=seed)
            _close(cl, cr.detach()[:, -1], tk, "attn_lastq_fwd ctx")
            x.grad = None
            (cr[:, -1] * dctx[:, -1].double()).sum().backward()
            dq, dkv = hip.attn_lastq_bwd(q_last, kv, dctx[:, -1].contiguous(), ids, pad, H, drop_p=p, seed=seed)
            t = dict(rtol=1e-3, atol=1e-4) if dt == torch.float32 else dict(rtol=5e-2, atol=5e-2)
            torch.testing.assert_close(dq.double(), x.grad[:, -1, :P], **t)
            torch.testing.assert_close(dkv.double(), x.grad[:, :, P:], **t)


@pytest.mark.parametrize("tier,L", [("bf16", 260), ("bf16", 416),                          # the 26-tile eight-wave form
                                    ("x3", 130), ("x3", 224), ("x3", 230), ("x3", 416)])   # restaged <14>, <14>, <16>, <26>
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_attention_backward_long_forms(tier, L, causal, p):
    """The backward forms the launcher selects by length alone, at the lower and the upper edge of their ranges, B = 2, H = 4, causal and
    not, without dropout and at p = 0.5: ctx and dqkv against float64 autograd through softmax(...) * host mask -- reference and tolerances
    of test_attention_masks."""
    from recguru_amd import hip
    dt = _tier(tier)
    B, H, seed = 2, 4, SEEDS[0]
    P = H * 32
    pad = 0 if causal else 51
    ids, rm = _attn_case(B, L, H, L)
    qkv = _rnd(B, L, 3 * P, seed=L + 1, dt=dt)
    km = _dev(dm.attn_mask(seed, p, H, L, range(B))) if p > 0 else torch.ones(B, H, L, L, dtype=torch.float64, device="cuda")
    dctx = (_rnd(B, L, P, seed=L + 3, dt=dt) * rm.view(B, L, 1).to(dt)).contiguous()
    kw = dict(drop_p=p, seed=seed, rowmask=rm)
    with _Tier(tier):
        ctx, lse = hip.attn_fwd(qkv, ids, pad, causal, H, **kw)
        dqkv = hip.attn_bwd(qkv, dctx, ctx, lse, ids, pad, causal, H, **kw)
    x = qkv.double().requires_grad_(True)
    cr, _, _, _ = _ref64(x, ids, pad, causal, H, km)
    (cr * dctx.double()).sum().backward()
    lv = rm.view(B, L) != 0
    _close(ctx[lv], cr.detach()[lv], _tolkey(tier), "ctx")
    if tier == "x3":
        err = float((dqkv.double() - x.grad).abs().max()) / float(x.grad.abs().max())
        assert err <= 6e-5, "dqkv: max error %.3g of max |value|" % err
    else:
        torch.testing.assert_close(dqkv.double(), x.grad, rtol=5e-2, atol=5e-2)


# ================================================================================================================ past the wrap
def test_attention_mask_past_the_32bit_wrap():
    """H = 8, L = 400 (LPAD 416), B = 3240: the attention index passes 2^32 inside sequence 3226 (head 3, query 40, key 256).
    f32 tier, p = 0.5: the forward's mask, dqkv under float64 autograd and the single-query forward, for sequences on both
    sides of the wrap, against the host mask (whose index wraps as the contract says)."""
    from recguru_amd import hip
    B, L, H, p, seed = 3240, 400, 8, 0.5, SEEDS[1]
    P = H * 32
    bs = [0, 1700, 3226, 3227, 3239]
    assert dm.attn_true_index(B - 1, H - 1, L - 1, L - 1, H, L) >= 1 << 32 > dm.attn_true_index(3226, 3, 40, 255, H, L)
    torch.cuda.empty_cache()
    gen = torch.Generator(device="cuda").manual_seed(5)
    qkv = torch.randn(B, L, 3 * P, device="cuda", generator=gen)
    ids = torch.ones(B, L, dtype=torch.int64, device="cuda")
    bi = torch.tensor(bs, device="cuda")
    kmask = dm.attn_mask(seed, p, H, L, bs)
    km = _dev(kmask)
    ctx, lse = hip.attn_fwd(qkv, ids, 0, False, H, drop_p=p, seed=seed)
    x = qkv[bi].double().requires_grad_(True)
    cr, lr, a_ref, _ = _ref64(x, ids[bi], 0, False, H, km)
    for i, b in enumerate(bs):
        err = float((ctx[b].double() - cr[i].detach()).abs().max())
        assert err <= F32_TOL * (1 + float(cr[i].detach().abs().max())), "ctx of sequence %d differs (max err %.3g)" % (b, err)
    torch.testing.assert_close(lse[bi].double(), lr.detach(), rtol=1e-4, atol=1e-3)
    # backward of those sequences under the forward's (host) mask
    dctx = torch.randn(B, L, P, device="cuda", generator=gen)
    dqkv = hip.attn_bwd(qkv, dctx, ctx, lse, ids, 0, False, H, drop_p=p, seed=seed)
    (cr * dctx[bi].double()).sum().backward()
    for i, b in enumerate(bs):
        g = x.grad[i]
        err = float((dqkv[b].double() - g).abs().max())
        assert err <= 1e-4 + 1e-3 * float(g.abs().max()), "dqkv of sequence %d differs (max err %.3g)" % (b, err)
    del dqkv, dctx
    # single-query forward == row L-1 of the full kernel and of the host-masked reference
    q_last = qkv[:, -1, :P].contiguous()
    kv = qkv[:, :, P:].contiguous()
    cl = hip.attn_lastq_fwd(q_last, kv, ids, 0, H, drop_p=p, seed=seed)
    del kv
    for i, b in enumerate(bs):
        torch.testing.assert_close(cl[b].double(), cr[i, -1].detach(), rtol=F32_TOL, atol=F32_TOL,
                                   msg=lambda m: "attn_lastq_fwd of sequence %d: %s" % (b, m))
    torch.testing.assert_close(cl, ctx[:, -1], rtol=F32_TOL, atol=F32_TOL)
    # the mask itself on key chunk 0 and the last chunk: V = one-hot over the chunk's keys
    live = a_ref.detach().cpu().numpy() > 1e-6
    for c in (0, (L - 1) // 32):
        n = min(32, L - 32 * c)
        qkv[:, :, 2 * P:] = 0
        qkv.view(B, L, 3, H, 32)[:, 32 * c: 32 * c + n, 2, :, :n] = torch.eye(n, device="cuda")[None, :, None, :]
        ctx1, _ = hip.attn_fwd(qkv, ids, 0, False, H, drop_p=p, seed=seed)
        got = ctx1[bi].view(len(bs), L, H, 32)[..., :n].permute(0, 2, 1, 3)
        for i, b in enumerate(bs):
            _same_zeros(got[i], kmask[i, :, :, 32 * c: 32 * c + n], "forward mask of sequence %d, keys %d.." % (b, 32 * c),
                        where=live[i, :, :, 32 * c: 32 * c + n])


# ================================================================================================================ seeds per site
_FWD_SEEDS = {"dropout_": ["seed"], "dropout_gelu": ["seed"], "add_drop_ln": ["seed"], "gemm_nt": ["drop_seed"],
              "embed_pe_fwd": ["seed"], "embed_pe_fwd_split": ["seed"], "attn_fwd": ["seed"], "attn_fwd_x": ["seed"],
              "attn_lastq_fwd": ["seed"], "attn_lastq_x_fwd": ["seed"], "post_attn_fwd": ["seed_h1", "seed_out"],
              "cross_drop_scale": ["seed"], "disc_rows": ["seeds_w", "seeds_g"]}
_DROP_P = {"dropout_": "drop_p", "dropout_gelu": "drop_p", "add_drop_ln": "drop_p", "gemm_nt": "drop_p", "embed_pe_fwd": "drop_p",
           "embed_pe_fwd_split": "drop_p", "attn_fwd": "drop_p", "attn_fwd_x": "drop_p", "attn_lastq_fwd": "drop_p",
           "attn_lastq_x_fwd": "drop_p", "post_attn_fwd": "drop_p", "cross_drop_scale": "drop_p", "disc_rows": "drop_p"}


def _record_forward_seeds(run):
    """Wrap the forward dropout launchers of `hip` (as hip.start_profile wraps them) while run() executes; returns the
    (launcher, argument, seed) of every launch that applied dropout."""
    import inspect
    from recguru_amd import hip
    seen, orig = [], {}

    def wrap(name, fn):
        sig = inspect.signature(fn)

        def rec(*a, **k):
            ba = sig.bind(*a, **k)
            ba.apply_defaults()
            if float(ba.arguments[_DROP_P[name]]) > 0:
                for arg in _FWD_SEEDS[name]:
                    v = ba.arguments[arg]
                    for s in (v if isinstance(v, (tuple, list)) else (v,)):
                        if not (name == "disc_rows" and arg == "seeds_g" and ba.arguments["alpha"] is None):
                            seen.append((name, arg, int(s)))
            return fn(*a, **k)
        return rec
    for name in _FWD_SEEDS:
        if hasattr(hip, name):
            orig[name] = getattr(hip, name)
            setattr(hip, name, wrap(name, orig[name]))
    try:
        run()
    finally:
        for name, fn in orig.items():
            setattr(hip, name, fn)
    return seen


def test_every_forward_dropout_launch_of_a_step_has_its_own_seed():
    """One training step of the autoencoder, one fused critic update and one generator W-loss with dropout on: no two forward dropout
    launches share a seed, and two ranks' streams (ops.manual_seed(s, rank)) share none."""
    from recguru_amd import ops, synthetic, training as T
    from recguru_amd.blocks import ScheduledOptim
    from recguru_amd.config import get_param
    from recguru_amd.models import Discriminator, MyAuto4Rec_c
    from recguru_amd.optim import Adam
    from parity_util import make_args
    with torch.random.fork_rng(devices=[torch.cuda.current_device()]):      # torch's generators too are left as they were
        _seeds_of_a_step(ops, synthetic, T, ScheduledOptim, get_param, Discriminator, MyAuto4Rec_c, Adam, make_args)


def _seeds_of_a_step(ops, synthetic, T, ScheduledOptim, get_param, Discriminator, MyAuto4Rec_c, Adam, make_args):
    torch.manual_seed(0)
    d, H, L, V, k, B = 128, 4, 24, 300, 5, 32
    param = get_param(make_args(d, H, k, L, V, V, 1, B, dropout=0.5), make_dirs=False)
    G = MyAuto4Rec_c("cuda", param).cuda()
    loaders = [synthetic.TensorLoader(synthetic.make_domain(2 * B, V, L, k, seed=s), B, "cuda") for s in (1, 2)]
    opt = ScheduledOptim(Adam(G.parameters(), betas=(0.9, 0.98), eps=1e-9), 1.0, d, 30)
    D = Discriminator(d, 1, 5 * d).cuda().train()
    assert D.drop_p() > 0
    real, fake = torch.randn(B, d, device="cuda"), torch.randn(B, d, device="cuda")
    alpha = torch.rand(B, 1, device="cuda")

    def step():
        T.train_recon_x(G, opt, 1, loaders, param, "cuda", loss_type="s_soft", opt_type="schedule", log_every=0)
        ops.critic_fused(D, real, fake, alpha)                      # fused discriminator: W rows and GP rows
        ops.disc_means(D, real, fake)                               # the generator's W-loss
        D.zero_grad(set_to_none=True)
    per_rank = []
    saved = dict(ops._SEED)                                       # the process's dropout stream is left as it was found
    try:
        for rank in (0, 1):
            ops.manual_seed(3, rank)
            seen = _record_forward_seeds(step)
            torch.cuda.synchronize()
            assert len(seen) >= 4, seen
            seeds = [s for _, _, s in seen]
            dup = {s for s in seeds if seeds.count(s) > 1}
            assert not dup, "forward dropout launches sharing a seed: %s" % [x for x in seen if x[2] in dup]
            per_rank.append(set(seeds))
    finally:
        ops._SEED.update(saved)
    assert not (per_rank[0] & per_rank[1]), "ranks 0 and 1 share seeds"
