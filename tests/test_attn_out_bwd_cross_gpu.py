"""rg_attn_out_bwd_cross (the decoder layer's attention tail backward with the cross-attention LayerNorm backward in front), the row
masks of rg_seq_wsum / rg_seq_sum that go with it, and the decoder layer with the fused call against the two launches it replaces.

The fused kernel repeats rg_ln_bwd's and rg_attn_out_bwd's arithmetic on the same rows, so dy1, dz and dctx are held to EQUALITY
on every row it is asked to produce; only the five column sums (f32 sums over the rows in another order) get a bound: rtol 2e-4,
atol 2e-4 of the largest reference sum -- the bound test_attn_out_bwd_equals_ln_bwd_plus_projection uses for the same kind of
reordered sum."""
import contextlib
import os
import subprocess
import sys

import pytest
import torch

import attn_out_bwd_cross_worker as worker

pytestmark = pytest.mark.gpu

D = 128
TIERS = ["bf16", "f32", "bf16x3"]
LENS = worker.LENS                 # live lengths of the B = 5 left-padded sequences of L = 40 (a full one, 16 +- 1, one row, none)
HERE = os.path.dirname(os.path.abspath(__file__))


@contextlib.contextmanager
def _tier(tier):
    from recguru_amd import hip
    prev, hip.SPLIT_OPERANDS = hip.SPLIT_OPERANDS, tier == "bf16x3"
    try:
        yield torch.bfloat16 if tier == "bf16" else torch.float32
    finally:
        hip.SPLIT_OPERANDS = prev


def rnd(*shape, dt=torch.float32, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dt).cuda()


def _left_pad_mask(B, L, seed):
    g0 = torch.Generator().manual_seed(seed)
    lens = torch.randint(0, L + 1, (B,), generator=g0)
    lens[0], lens[1] = 0, L
    return (torch.arange(L)[None, :] >= (L - lens)[:, None]).float().reshape(-1).cuda().contiguous()


def _sums_close(got, ref, base, what):
    """got / ref: accumulators that started at `base`; the bound is on the column sum itself."""
    scale = float((ref - base).abs().max())
    err = float((got - ref).abs().max())
    print("%s: max |fused - two launches| = %.3g, largest sum %.3g" % (what, err, scale))
    torch.testing.assert_close(got, ref, rtol=2e-4, atol=2e-4 * scale, msg=lambda m: "%s: %s" % (what, m))


@pytest.mark.parametrize("colsum", [False, True])
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("M,listed", [(64, False), (203, False), (9000, False), (9000, True)])
def test_kernel_equals_ln_bwd_then_attn_out_bwd(M, listed, tier, colsum):
    from recguru_amd import hip
    with _tier(tier) as dt:
        cg, cbe = 1 + 0.1 * rnd(D, seed=1), 0.1 * rnd(D, seed=2)
        g1, be1 = 1 + 0.1 * rnd(D, seed=3), 0.1 * rnd(D, seed=4)
        mask = _left_pad_mask(M // 120, 120, M) if listed else (torch.arange(M) % 5 != 1).float().cuda()
        live = hip.live_tiles(mask, M) if listed else None
        zc, z1 = rnd(M, D, seed=5), rnd(M, D, seed=6)
        rs = lambda z: 1 / torch.sqrt(z.var(1, unbiased=False) + 1e-8)
        rstd_c, rstd1 = rs(zc), rs(z1)
        y2 = torch.nn.functional.layer_norm(zc, (D,), cg, cbe, 1e-8).to(dt)
        y1 = torch.nn.functional.layer_norm(z1, (D,), g1, be1, 1e-8).to(dt)
        dy2 = rnd(M, D, dt=dt, seed=7) * mask[:, None].to(dt)
        Wo = rnd(D, D, scale=D ** -0.5, seed=8)
        split = hip.CAST_SPLIT if tier == "bf16x3" else 0
        Wot = hip.cast(Wo, dt, transpose=hip.CAST_TRANSPOSE)
        Wotp = hip.cast(Wo, dt, transpose=hip.CAST_TRANSPOSE | hip.CAST_PACK | split)
        base = [0.5 * rnd(D, seed=20 + i) for i in range(5)]         # the accumulators start non-zero: the sums are ADDED
        ref = [b.clone() for b in base]
        got = [b.clone() for b in base]
        # the two launches (rg_ln_bwd walks every row, as the decoder layer's call does; rg_attn_out_bwd takes the list)
        dy1_0 = hip.ln_bwd(dy2, y2, rstd_c, cg, cbe, mask, ref[0], ref[1], dz_colsum=ref[2] if colsum else None)
        dz_0, dctx_0 = hip.attn_out_bwd(dy1_0, y1, rstd1, g1, be1, mask, ref[3], ref[4], Wotp, live=live, w_packed=True)
        hip.POISON_UNWRITTEN = listed
        try:
            dy1, dz, dctx = hip.attn_out_bwd_cross(dy2, y2, rstd_c, cg, cbe, y1, rstd1, g1, be1, mask, got[0], got[1], got[3], got[4], Wotp,
                                                   dz_colsum=got[2] if colsum else None, live=live, w_packed=True)
        finally:
            hip.POISON_UNWRITTEN = False
        rows = torch.ones(M, dtype=torch.bool, device="cuda")
        if listed:
            r16 = torch.zeros((M + 15) // 16 * 16, device="cuda")
            r16[:M] = mask
            rows = r16.view(-1, 16).amax(1).repeat_interleave(16)[:M] != 0
            assert int((~rows).sum()) >= 16
            for name, t in (("dy1", dy1), ("dz", dz), ("dctx", dctx)):
                assert bool(torch.isnan(t[~rows].float()).all()), "%s: a row of an unlisted tile was written" % name
        dead = rows & (mask == 0)
        assert int(dead.sum()) > 0
        for name, a, b in (("dy1", dy1, dy1_0), ("dz", dz, dz_0), ("dctx", dctx, dctx_0)):
            assert torch.equal(a[rows], b[rows]), "%s differs from the two launches on %d live-tile rows" % (name, int((a[rows] != b[rows]).any(1).sum()))
            assert float(a[dead].float().abs().max()) == 0.0, "%s: a masked row inside a live tile is not zero" % name
        for i, name in enumerate(("dcgamma", "dcbeta", "dz_colsum", "dgamma1", "dbeta1")):
            if i == 2 and not colsum:
                assert torch.equal(got[2], base[2])
                continue
            _sums_close(got[i], ref[i], base[i], name)
        # row-major Wo^T (fragments gathered -- and in the bf16x3 tier split -- by the kernel): the same product, no column sums asked for
        _, dz_r, dctx_r = hip.attn_out_bwd_cross(dy2, y2, rstd_c, cg, cbe, y1, rstd1, g1, be1, mask, None, None, None, None, Wot,
                                                 live=live, w_packed=False)
        assert torch.equal(dctx_r[rows], dctx[rows]) and torch.equal(dz_r[rows], dz[rows])


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _seq_case(dt):
    B, L, H = 5, 40, 4
    lens = torch.tensor(LENS)
    mask = (torch.arange(L)[None, :] >= (L - lens)[:, None]).reshape(-1).cuda()
    x = rnd(B * L, D, dt=dt, seed=11)
    zero = torch.where(mask[:, None], x, torch.zeros_like(x))
    nan = torch.where(mask[:, None], x, torch.full_like(x, float("nan")))
    s = torch.rand(B * L, H, generator=torch.Generator().manual_seed(12)).cuda()
    return B, L, H, mask.float().contiguous(), zero, nan, s


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_seq_wsum_and_seq_sum_skip_masked_rows(dt):
    """With a row mask: the same bits as the unmasked call on an input whose dead rows are zero, and dead rows are never read (NaN
    there changes nothing)."""
    from recguru_amd import hip
    B, L, H, mask, zero, nan, s = _seq_case(dt)
    ref = hip.seq_wsum(zero, s, B, L, H)
    assert torch.equal(_bits(hip.seq_wsum(zero, s, B, L, H, rowmask=mask)), _bits(ref))
    assert torch.equal(_bits(hip.seq_wsum(nan, s, B, L, H, rowmask=mask)), _bits(ref))
    assert float(ref[4].float().abs().max()) == 0.0 and float(ref[0].float().abs().max()) > 0
    ref = hip.seq_sum(zero, B, L)
    assert torch.equal(_bits(hip.seq_sum(zero, B, L, rowmask=mask)), _bits(ref))
    assert torch.equal(_bits(hip.seq_sum(nan, B, L, rowmask=mask)), _bits(ref))
    assert float(ref[4].float().abs().max()) == 0.0 and float(ref[0].float().abs().max()) > 0


# positions in DecoderLayerFn's parameter list of the five column sums the fused kernel forms in another order
COLSUMS = {8: "g1", 9: "be1", 13: "cross bo", 14: "cross gamma", 15: "cross beta"}
LAYER_CASES = [(tier, p) for tier in ("bf16", "bf16x3") for p in (0.0, 0.5)]


def _names(res):
    return ["out", "dx", "du"] + ["parameter gradient %d" % i for i in range(len(res[0]) - 3)]


@pytest.mark.parametrize("tier,drop_p", LAYER_CASES)
def test_decoder_layer_fused_equals_two_launches(tier, drop_p):
    """DecoderLayerFn forward + backward (B = 5, L = 40, H = 4, d = 128, a wholly padded sequence among them) with
    ops.FUSE_ATTN_OUT_BWD_CROSS off, on and on again, same weights, inputs and dropout seeds, in the shipped library: out, dx and du
    have the same bits in all three.  The parameter gradients are float-atomic sums over workgroups there (rg_gemm_tn splits the
    rows), not the same bits in any two runs of EITHER path: they are held to the column sums' bound here and to equality under the
    order-independent accumulators below."""
    off, on, on2 = worker.run_case(tier, drop_p)
    for i, (name, a, b, c) in enumerate(zip(_names([off]), off, on, on2)):
        assert (a is None) == (b is None) == (c is None), name
        if a is None:
            continue
        assert not bool(torch.isnan(b.float()).any()), name
        if i < 3:
            assert torch.equal(a, b), "%s: fused and two-launch paths differ (max %.3g)" % (name, float((a.float() - b.float()).abs().max()))
            assert torch.equal(b, c), "%s: two runs with the fused call differ" % name
        elif i - 3 != 3:        # (WK.bias: structurally gradient-free -- a constant added to a softmax row --, atomic-order noise around 0)
            _sums_close(b.float(), a.float(), torch.zeros_like(a.float()), name)


@pytest.fixture(scope="module")
def det_runs(tmp_path_factory):
    """All four layer cases, off / on / on, in ONE fresh process on the deterministic library (RG_DETERMINISTIC=1 is read when
    recguru_amd is imported): every accumulation into global memory is an integer add there, so a weight gradient is a function of
    its operands alone and `the same bits` is a claim about the kernels under test."""
    out = str(tmp_path_factory.mktemp("cross") / "det.pt")
    env = dict(os.environ, RG_DETERMINISTIC="1")
    p = subprocess.run([sys.executable, os.path.join(HERE, "attn_out_bwd_cross_worker.py"), out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()[-4000:]
    return torch.load(out)


@pytest.mark.parametrize("tier,drop_p", LAYER_CASES)
def test_decoder_layer_fused_same_bits_as_two_launches_deterministic_accumulators(det_runs, tier, drop_p):
    """The issue's layer check in full: dx, du and every parameter gradient except the five LayerNorm / bias column sums are
    bit-equal between the fused call and the two launches; those five agree to the bound; two runs with the fused call are
    bit-equal everywhere; no accumulator escaped the fixed-point arenas."""
    assert det_runs["det_enabled"] >= 7 and det_runs["det_fault"] == 0
    off, on, on2 = det_runs["%s/%g" % (tier, drop_p)]
    for i, (name, a, b, c) in enumerate(zip(_names([off]), off, on, on2)):
        assert (a is None) == (b is None) == (c is None), name
        if a is None:
            continue
        assert not bool(torch.isnan(b.float()).any()), name
        assert torch.equal(b, c), "%s: two runs with the fused call differ" % name
        if i - 3 in COLSUMS:
            _sums_close(b, a, torch.zeros_like(a), "%s (%s)" % (name, COLSUMS[i - 3]))
        else:
            assert torch.equal(a, b), "%s: fused and two-launch paths differ (max %.3g)" % (name, float((a.float() - b.float()).abs().max()))
