"""The streaming attention core (416 < L <= 2048, csrc/attention_long.hip) and the looped single-query kernels
(512 < L <= 2048, csrc/attention_lastq.hip) against float64 attention with the host dropout mask of tests/dropmask.py and
autograd through it.

Lengths: 417 (the first past the resident kernels' limit: one key in a ragged 64-key block), 448 and 449 (the smallest
multiple of the 64-position block above 416, and one more), 2048 (the upper edge).  B = 2, H = 2: sequence 0 is full
length, sequence 1 is left-padded and comes with a row mask.  Non-causal cases use pad_value = 51 (no key masked: the
padding rows are live keys), causal ones pad_value = 0 (the left padding is masked: the query rows of the padded prefix
are fully masked rows).  Tolerances are those of tests/test_dropout_masks_gpu.py for the same quantities."""
import functools
import math

import numpy as np
import pytest
import torch

import dropmask as dm

pytestmark = pytest.mark.gpu

SEEDS = [(3 << 32) | 77, (11 << 32) | 77]
F32_TOL = 2e-5
BLOCK = 64                                             # positions per streamed block (attention_long.hip LK)
L_EDGE = 417
L_BLOCK = (416 // BLOCK + 1) * BLOCK                   # 448
L_MAX = 2048
DROPS = [(0.0, 0), (0.5, SEEDS[0]), (0.3, SEEDS[1])]


def _dev(m):
    return torch.from_numpy(np.ascontiguousarray(m)).cuda()


def _rnd(*shape, seed=0, scale=1.0, dt=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dt).cuda()


def _close(got, ref, dt, what):
    """The tier's tolerance: f32 2e-5; bf16 2e-2; relative to max |ref| for the bf16x3 tier."""
    got, ref = got.double(), ref.double()
    if dt == "x3":
        err = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
        assert err <= 4e-5, "%s: max error %.3g of max |value|" % (what, err)
    elif dt == torch.float32:
        torch.testing.assert_close(got, ref, rtol=F32_TOL, atol=F32_TOL, msg=lambda m: what + ": " + m)
    else:
        torch.testing.assert_close(got, ref, rtol=2e-2, atol=2e-2, msg=lambda m: what + ": " + m)


def _close_grad(got, ref, tk, what):
    got, ref = got.double(), ref.double()
    if tk == torch.float32:
        torch.testing.assert_close(got, ref, rtol=1e-3, atol=1e-4, msg=lambda m: what + ": " + m)
    elif tk == "x3":
        err = float((got - ref).abs().max()) / float(ref.abs().max())
        assert err <= 6e-5, "%s: max error %.3g of max |value|" % (what, err)
    else:
        torch.testing.assert_close(got, ref, rtol=5e-2, atol=5e-2, msg=lambda m: what + ": " + m)


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


def _attn_case(B, L, H, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 50, (B, L), generator=g)
    lens = torch.randint(max(1, L // 3), L + 1, (B,), generator=g)
    lens[0] = L
    rm = (torch.arange(L)[None, :] >= (L - lens)[:, None])
    ids = ids * rm.long()                                    # left padding carries id 0
    return ids.cuda(), rm.float().reshape(-1).cuda()


def _ref64(qkv, ids, pad, causal, H, kmask):
    """float64 attention with an explicit dropout multiplier kmask [B,H,L,L]: ctx, lse (of the undropped scores), A, A_drop."""
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


@functools.lru_cache(maxsize=2)
def _kmask(seed, p, H, L, B):
    """Host dropout multipliers [B, H, L, L] (numpy) -- computed once per (seed, p, L)."""
    if p <= 0:
        return np.ones((B, H, L, L))
    return dm.attn_mask(seed, p, H, L, range(B))


@functools.lru_cache(maxsize=2)
def _case(dt, L, causal, p, seed, B=2, H=2):
    """Inputs and the float64 reference (ctx, lse, A, A_drop, d qkv under a fixed dctx) of one case; the f32 and the bf16x3
    tier share it (same f32 inputs).  Nothing in it is modified by the tests."""
    P = H * 32
    pad = 0 if causal else 51
    ids, rm = _attn_case(B, L, H, L)
    qkv = torch.cat([_rnd(B, L, 2 * P, seed=L + 1, dt=dt), _rnd(B, L, P, seed=L + 2, dt=dt)], 2).contiguous()
    kmask = _kmask(seed, p, H, L, B)
    km = _dev(kmask)
    dctx = (_rnd(B, L, P, seed=L + 3, dt=dt) * rm.view(B, L, 1).to(dt)).contiguous()
    x = qkv.double().requires_grad_(True)
    cr, lr, a_ref, ad_ref = _ref64(x, ids, pad, causal, H, km)
    (cr * dctx.double()).sum().backward()
    return dict(ids=ids, rm=rm, qkv=qkv, kmask=kmask, dctx=dctx, pad=pad, ctx=cr.detach(), lse=lr.detach(), a=a_ref.detach(),
                ad=ad_ref.detach(), grad=x.grad)


def _check_values(tier, L, causal, p, seed):
    from recguru_amd import hip
    dt, tk = _tier(tier), _tolkey(tier)
    B, H = 2, 2
    c = _case(dt, L, causal, p, seed)
    kw = dict(drop_p=p, seed=seed, rowmask=c["rm"])
    with _Tier(tier):
        ctx, lse = hip.attn_fwd(c["qkv"], c["ids"], c["pad"], causal, H, **kw)
        dqkv = hip.attn_bwd(c["qkv"], c["dctx"], ctx, lse, c["ids"], c["pad"], causal, H, **kw)
    lv = c["rm"].view(B, L) != 0
    _close(ctx[lv], c["ctx"][lv], tk, "ctx")
    torch.testing.assert_close(lse.transpose(1, 2)[lv].double(), c["lse"].transpose(1, 2)[lv], rtol=1e-4,
                               atol=1e-3 if dt == torch.float32 else 3e-2)
    _close_grad(dqkv, c["grad"], tk, "dqkv")


@pytest.mark.parametrize("p,seed", DROPS)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", [L_EDGE, L_BLOCK, L_BLOCK + 1])
@pytest.mark.parametrize("tier", ["f32", "x3", "bf16"])
def test_long_attention_values(tier, L, causal, p, seed):
    """ctx on live rows, lse and dqkv against float64 attention / autograd through softmax(...) * host mask."""
    _check_values(tier, L, causal, p, seed)


@pytest.mark.parametrize("tier,causal", [("bf16", False), ("x3", True), ("f32", True)])
def test_long_attention_values_upper_edge(tier, causal):
    """L = 2048, p = 0.5: once per tier."""
    _check_values(tier, L_MAX, causal, 0.5, SEEDS[0])
    _case.cache_clear()
    _kmask.cache_clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("p,seed", DROPS[1:])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", [L_EDGE, L_BLOCK + 1])
@pytest.mark.parametrize("tier", ["f32", "x3", "bf16"])
def test_long_attention_masks(tier, L, causal, p, seed):
    """The dropout mask element by element: forward through one-hot V chunks (ctx[:, q, c] = A_drop[q, 32 chunk + c]), backward
    through one-hot dctx chunks (dV[key, c] = A_drop[32 chunk + c, key]) -- exact zeros where the host mask drops, nowhere else
    on live entries."""
    from recguru_amd import hip
    dt, tk = _tier(tier), _tolkey(tier)
    B, H = 2, 2
    P = H * 32
    c = _case(dt, L, causal, p, seed)
    ids, rm, qkv, pad, kmask = c["ids"], c["rm"], c["qkv"], c["pad"], c["kmask"]
    qk = qkv[:, :, :2 * P]
    rows = rm.view(B, L).cpu().numpy() != 0                      # live query rows
    live = (c["a"].cpu().numpy() > 1e-6) & rows[:, None, :, None]
    kw = dict(drop_p=p, seed=seed, rowmask=rm)
    nch = (L + 31) // 32
    eye = torch.eye(32, dtype=dt, device="cuda")
    with _Tier(tier):
        A = torch.zeros(B, H, L, L, dtype=torch.float64, device="cuda")
        for ch in range(nch):
            v = torch.zeros(B, L, H, 32, dtype=dt, device="cuda")
            n = min(32, L - 32 * ch)
            v[:, 32 * ch: 32 * ch + n, :, :n] = eye[:n, :n][None, :, None, :]
            ctx, _ = hip.attn_fwd(torch.cat([qk, v.reshape(B, L, P)], 2).contiguous(), ids, pad, causal, H, **kw)
            A[:, :, :, 32 * ch: 32 * ch + n] = ctx.double().view(B, L, H, 32)[..., :n].permute(0, 2, 1, 3)
        _same_zeros(A, kmask, "forward mask", where=live)
        lt = torch.from_numpy(live).cuda()
        _close(A[lt], c["ad"][lt], tk, "forward A_drop")
        ctx, lse = hip.attn_fwd(qkv, ids, pad, causal, H, **kw)
        Ab = torch.zeros(B, H, L, L, dtype=torch.float64, device="cuda")
        for ch in range(nch):
            n = min(32, L - 32 * ch)
            dctx = torch.zeros(B, L, H, 32, dtype=dt, device="cuda")
            dctx[:, 32 * ch: 32 * ch + n, :, :n] = eye[:n, :n][None, :, None, :]
            dctx = (dctx.reshape(B, L, P) * rm.view(B, L, 1).to(dt)).contiguous()
            dqkv = hip.attn_bwd(qkv, dctx, ctx, lse, ids, pad, causal, H, **kw)
            Ab[:, :, 32 * ch: 32 * ch + n, :] = dqkv[:, :, 2 * P:].double().view(B, L, H, 32)[..., :n].permute(0, 2, 3, 1)
        _same_zeros(Ab, kmask, "backward mask", where=live)


# ================================================================================================================ degenerate inputs
@pytest.mark.parametrize("tier", ["f32", "x3", "bf16"])
def test_long_attention_wholly_padded_sequence(tier):
    """A sequence with rowmask all 0 and ids all 0 next to a live one: its ctx, lse and every element of dqkv are exactly 0 (dqkv is
    written over NaN-free garbage: the output buffers come from torch.empty), and the live one does not notice its neighbour."""
    from recguru_amd import hip
    dt = _tier(tier)
    B, H, L, p, seed = 2, 2, L_EDGE, 0.5, SEEDS[0]
    P = H * 32
    qkv = _rnd(B, L, 3 * P, seed=5, dt=dt)
    ids = torch.randint(1, 50, (B, L), generator=torch.Generator().manual_seed(1)).cuda()
    ids[1] = 0
    rm = torch.ones(B, L, device="cuda")
    rm[1] = 0
    rm = rm.reshape(-1).contiguous()
    dctx = (_rnd(B, L, P, seed=6, dt=dt) * rm.view(B, L, 1).to(dt)).contiguous()
    for causal in (False, True):
        kw = dict(drop_p=p, seed=seed)
        with _Tier(tier):
            # poison the allocator's free blocks so that an unwritten element cannot be a lucky zero
            junk = torch.full((B, L, 3 * P), 7.0, dtype=dt, device="cuda")
            del junk
            ctx, lse = hip.attn_fwd(qkv, ids, 0, causal, H, rowmask=rm, **kw)
            junk = torch.full((B, L, 3 * P), 7.0, dtype=dt, device="cuda")
            del junk
            dqkv = hip.attn_bwd(qkv, dctx, ctx, lse, ids, 0, causal, H, rowmask=rm, **kw)
            ctx1, lse1 = hip.attn_fwd(qkv[:1].contiguous(), ids[:1].contiguous(), 0, causal, H, rowmask=rm[:L].contiguous(), **kw)
            dqkv1 = hip.attn_bwd(qkv[:1].contiguous(), dctx[:1].contiguous(), ctx1, lse1, ids[:1].contiguous(), 0, causal, H,
                                 rowmask=rm[:L].contiguous(), **kw)
        assert float(ctx[1].float().abs().max()) == 0.0 and float(lse[1].abs().max()) == 0.0
        assert float(dqkv[1].float().abs().max()) == 0.0
        assert torch.equal(ctx[0], ctx1[0]) and torch.equal(lse[0], lse1[0]) and torch.equal(dqkv[0], dqkv1[0])
        assert float(dqkv[0].float().abs().max()) > 0


@pytest.mark.parametrize("tier", ["f32", "x3", "bf16"])
def test_long_attention_without_rowmask(tier):
    """rowmask = None: every row is evaluated (also the rows of sequence 1's padded prefix)."""
    from recguru_amd import hip
    dt, tk = _tier(tier), _tolkey(tier)
    B, H, L = 2, 2, L_EDGE
    c = _case(dt, L, False, 0.0, 0)
    with _Tier(tier):
        ctx, lse = hip.attn_fwd(c["qkv"], c["ids"], c["pad"], False, H)
        dctx = _rnd(B, L, H * 32, seed=L + 4, dt=dt)
        dqkv = hip.attn_bwd(c["qkv"], dctx, ctx, lse, c["ids"], c["pad"], False, H)
    _close(ctx, c["ctx"], tk, "ctx")
    x = c["qkv"].double().requires_grad_(True)
    cr, _, _, _ = _ref64(x, c["ids"], c["pad"], False, H, 1.0)
    (cr * dctx.double()).sum().backward()
    _close_grad(dqkv, x.grad, tk, "dqkv")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("tier", ["f32", "x3", "bf16"])
def test_long_attention_every_key_masked(tier, causal):
    """Every key of sequence 1 equals pad_value, its rows are live: uniform attention over the L REAL keys -- the mean of V -- also
    where the causal form would not have visited the key blocks above the diagonal; no gradient reaches Q or K."""
    from recguru_amd import hip
    dt, tk = _tier(tier), _tolkey(tier)
    B, H, L = 2, 2, L_EDGE
    P = H * 32
    qkv = _rnd(B, L, 3 * P, seed=9, dt=dt)
    ids = torch.randint(1, 50, (B, L), generator=torch.Generator().manual_seed(2)).cuda()
    ids[1] = 7
    rm = torch.ones(B * L, device="cuda")
    dctx = _rnd(B, L, P, seed=10, dt=dt)
    with _Tier(tier):
        ctx, lse = hip.attn_fwd(qkv, ids, 7, causal, H, rowmask=rm)
        dqkv = hip.attn_bwd(qkv, dctx, ctx, lse, ids, 7, causal, H, rowmask=rm)
    x = qkv.double().requires_grad_(True)
    cr, lr, _, _ = _ref64(x, ids, 7, causal, H, 1.0)
    (cr * dctx.double()).sum().backward()
    mean_v = qkv[1, :, 2 * P:].double().mean(0)
    torch.testing.assert_close(cr.detach()[1], mean_v.expand(L, P), rtol=1e-12, atol=1e-12)
    _close(ctx, cr.detach(), tk, "ctx")
    torch.testing.assert_close(lse.double(), lr.detach(), rtol=1e-4, atol=1e-3 if dt == torch.float32 else 3e-2)
    _close_grad(dqkv, x.grad, tk, "dqkv")
    assert float(dqkv[1, :, :2 * P].float().abs().max()) == 0.0


# ================================================================================================================ reproducibility
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("tier", ["f32", "x3", "bf16"])
def test_long_attention_bit_reproducible(tier, causal):
    """L = 480, p = 0.5: two runs give identical bits, and the first two sequences of a batch of 3 equal the batch of 2 bit for bit
    (no float atomics, no dependence on the grid: DESIGN.md 2a)."""
    from recguru_amd import hip
    dt = _tier(tier)
    H, L, p, seed = 2, 480, 0.5, SEEDS[1]
    P = H * 32
    pad = 0 if causal else 51
    ids3, rm3 = _attn_case(3, L, H, 480)
    qkv3 = _rnd(3, L, 3 * P, seed=11, dt=dt)
    dctx3 = (_rnd(3, L, P, seed=12, dt=dt) * rm3.view(3, L, 1).to(dt)).contiguous()

    def run(B):
        rm = rm3[:B * L].contiguous()
        kw = dict(drop_p=p, seed=seed, rowmask=rm)
        q, i, d = qkv3[:B].contiguous(), ids3[:B].contiguous(), dctx3[:B].contiguous()
        with _Tier(tier):
            ctx, lse = hip.attn_fwd(q, i, pad, causal, H, **kw)
            return ctx, lse, hip.attn_bwd(q, d, ctx, lse, i, pad, causal, H, **kw)
    a, b, c3 = run(2), run(2), run(3)
    for x, y, z in zip(a, b, c3):
        assert torch.equal(x, y)
        assert torch.equal(x, z[:2])
    assert float(a[2].float().abs().max()) > 0


# ================================================================================================================ single-query kernels
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("p,seed", DROPS[:2])
@pytest.mark.parametrize("L", [513, 1025, 2048])
@pytest.mark.parametrize("tier", ["f32", "x3", "bf16"])
def test_lastq_looped(tier, L, p, seed, fold):
    """attn_lastq_fwd = row L - 1 of the float64 reference, attn_lastq_bwd = autograd's dq and dkv.  fold: the K / V rows of each
    sequence's padded prefix are the bias rows and are NOT fetched (handed over as NaN)."""
    from recguru_amd import hip
    dt, tk = _tier(tier), _tolkey(tier)
    B, H = 2, 2
    P = H * 32
    pad = 51
    ids, rm = _attn_case(B, L, H, L)
    qkv = _rnd(B, L, 3 * P, seed=L + 1, dt=dt)
    bkv = _rnd(2 * P, seed=L + 5, scale=0.5)
    kv_in = None
    if fold:
        pre = rm.view(B, L) == 0
        qkv[:, :, P:][pre] = bkv.to(dt)
        kv_in = qkv[:, :, P:].clone()
        kv_in[pre] = float("nan")
    q_last = qkv[:, -1, :P].contiguous()
    kv = qkv[:, :, P:].contiguous()
    kv_in = kv if kv_in is None else kv_in.contiguous()
    km = torch.ones(B, H, 1, L, dtype=torch.float64, device="cuda")
    if p > 0:
        b_, h_, k_ = np.arange(B)[:, None, None], np.arange(H)[None, :, None], np.arange(L)[None, None, :]
        km = _dev(dm.keep(seed, p, dm.attn_index(b_, h_, L - 1, k_, H, L)))[:, :, None, :]
    x = qkv.double().requires_grad_(True)
    # row L - 1 alone: non-causal, so the other query rows do not matter
    q, k, v = [t.reshape(B, L, H, 32).transpose(1, 2) for t in x.split(P, dim=2)]
    s = (q[:, :, -1:, :] @ k.transpose(-1, -2) / math.sqrt(32)).masked_fill(ids.eq(pad)[:, None, None, :], -1e9)
    cr = ((torch.softmax(s, -1) * km) @ v).transpose(1, 2).reshape(B, P)
    g = _rnd(B, P, seed=L + 3, dt=dt)
    (cr * g.double()).sum().backward()
    kw = dict(drop_p=p, seed=seed)
    if fold:
        kw.update(rowmask=rm, bkv=bkv)
    with _Tier(tier):
        cl = hip.attn_lastq_fwd(q_last, kv_in, ids, pad, H, **kw)
        dq, dkv = hip.attn_lastq_bwd(q_last, kv_in, g, ids, pad, H, **kw)
    _close(cl, cr.detach(), tk, "attn_lastq_fwd ctx")
    t = dict(rtol=1e-3, atol=1e-4) if dt == torch.float32 else dict(rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(dq.double(), x.grad[:, -1, :P], **t)
    torch.testing.assert_close(dkv.double(), x.grad[:, :, P:], **t)


# ================================================================================================================ limits
def test_long_attention_limits():
    """L = 2049 is refused by the attention core and the single-query kernels with the limit in the message; at L = 417 the head-major
    and the x-input forms are refused -- argument checks that return before any launch."""
    from recguru_amd import hip
    B, H = 1, 4
    P = H * 32
    L = L_MAX + 1
    qkv = torch.zeros(B, L, 3 * P, device="cuda")
    ids = torch.ones(B, L, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match=r"\(-2\).*attn_fwd.*2048"):
        hip.attn_fwd(qkv, ids, 0, False, H)
    ctx = torch.zeros(B, L, P, device="cuda")
    lse = torch.zeros(B, H, L, device="cuda")
    with pytest.raises(RuntimeError, match=r"\(-2\).*attn_bwd.*2048"):
        hip.attn_bwd(qkv, ctx, ctx, lse, ids, 0, False, H)
    with pytest.raises(RuntimeError, match=r"\(-2\).*attn_lastq_fwd.*2048"):
        hip.attn_lastq_fwd(qkv[:, -1, :P].contiguous(), qkv[:, :, P:].contiguous(), ids, 0, H)
    with pytest.raises(RuntimeError, match=r"\(-2\).*attn_lastq_bwd.*2048"):
        hip.attn_lastq_bwd(qkv[:, -1, :P].contiguous(), qkv[:, :, P:].contiguous(), ctx[:, -1].contiguous(), ids, 0, H)
    L = L_EDGE
    ids = torch.ones(B, L, dtype=torch.int64, device="cuda")
    hm = torch.zeros(3, B, H, L, 32, dtype=torch.bfloat16, device="cuda")
    pad_rows = torch.zeros(3 * H + 1, 32, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match=r"\(-2\).*attn_fwd.*head-major.*416"):
        hip.attn_fwd(hm, ids, 0, False, H, pad_rows=pad_rows)
    x = torch.zeros(B, L, 128, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(3 * P, 128, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match=r"\(-2\).*attn_fwd.*x-input.*416"):
        hip.attn_fwd_x(x, w, torch.zeros(3 * P, device="cuda"), ids, 0, False, H)
    dctx = torch.zeros(B, L, P, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match=r"\(-2\).*attn_bwd.*head-major.*416"):
        hip.attn_bwd(hm, dctx, dctx, torch.zeros(B, H, L, device="cuda"), ids, 0, False, H)
