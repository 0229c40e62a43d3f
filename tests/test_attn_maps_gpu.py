"""Attention maps on request on the GPU: hip.attn_probs / attn_cross_probs / attn_rollout (csrc/attention_map.hip) against the float64
restatement tests/attn_map_ref.py, and return_attn=True of the model layers against the reference's maps (tests/golden/attn_maps_case*.npz)
and the CPU oracle.  The `[attn_maps]` lines printed here are kept in profiles/attn_maps/test_printout.txt."""
import ctypes

import numpy as np
import pytest
import torch

import attn_map_ref as R
from attn_maps_util import CASES, SCALE, check_exact, dyadic_maps, load_case, oracle_params, stack_maps
from oracle import recguru_oracle as O
from parity_util import make_args

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-3, 1e-5                  # the project's bound for the f32 / bf16x3 tiers; a ceiling for the kernel in every tier
TIERS = ["f32", "bf16", "bf16x3"]
LENGTHS = [1, 15, 16, 17, 63, 64, 65, 129, 200, 417]
GUARD = 1024                             # floats behind an output: 4 KB


@pytest.fixture(autouse=True)
def _restore_tier():
    from recguru_amd import ops
    yield
    ops.set_compute_dtype(torch.bfloat16)


def set_tier(tier):
    from recguru_amd import ops
    ops.set_compute_dtype({"f32": torch.float32, "bf16": torch.bfloat16, "bf16x3": "bf16x3"}[tier])
    return torch.bfloat16 if tier == "bf16" else torch.float32


def np_(t):
    return t.detach().float().cpu().numpy()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def say(capsys, msg):
    with capsys.disabled():
        print("\n[attn_maps] " + msg, end="")


def err_of(got, ref):
    """(max |err|, max |err| / (ATOL + RTOL |ref|): <= 1 passes)"""
    e = np.abs(got.astype(np.float64) - ref)
    return float(e.max()), float((e / (ATOL + RTOL * np.abs(ref))).max())


# ---- inputs shared by the kernel tests ----------------------------------------------------------------------------------------
def five_users(rng, L, pad):
    """no padding; left-padded by 1; left-padded to one live key; all padding; a pad id in the middle of the live range"""
    ids = rng.integers(1, 30, size=(5, L)).astype(np.int64)
    ids[ids == pad] = 31
    ids[1, :1] = pad
    ids[2, :L - 1] = pad
    ids[3, :] = pad
    if L >= 3:
        ids[4, L // 2] = pad
    return ids


_INPUTS = {}


def inputs(L, H, pad=0):
    """(ids [B, L], qkv f32 [B, L, 3*H*32], its bf16 rounding as f32) -- N(0, 1) entries, scores O(1); B = 5 (B = 1 at L = 2048)"""
    key = (L, H, pad)
    if key not in _INPUTS:
        rng = np.random.default_rng(1000 * L + 10 * H + pad)
        ids = five_users(rng, L, pad)
        if L == 2048:
            ids = ids[4:5].copy()
            ids[0, :5] = pad
        qkv = rng.standard_normal((ids.shape[0], L, 3 * H * 32)).astype(np.float32)
        q16 = torch.as_tensor(qkv).to(torch.bfloat16).float().numpy()
        _INPUTS[key] = (ids, qkv, q16)
    return _INPUTS[key]


_REFS = {}


def reference(L, H, pad, causal, bf16):
    key = (L, H, pad, causal, bf16)
    if key not in _REFS:
        ids, qkv, q16 = inputs(L, H, pad)
        q, k = R.split_heads(q16 if bf16 else qkv, H)
        _REFS[key] = R.probs(q, k, ids, pad, causal, SCALE)
    return _REFS[key]


def run_shape(tier, L, H, pad, causal, worst):
    from recguru_amd import hip
    dt = set_tier(tier)
    ids_np, qkv_np, q16_np = inputs(L, H, pad)
    B = ids_np.shape[0]
    ids = torch.as_tensor(ids_np).cuda()
    qkv = torch.as_tensor(q16_np if tier == "bf16" else qkv_np).cuda().to(dt)
    n = B * H * L * L
    buf = torch.full((n + GUARD,), float("nan"), device="cuda", dtype=torch.float32)
    out = buf[:n].view(B, H, L, L)
    res = hip.attn_probs(qkv, ids, pad, H, causal, out=out)
    assert res is out
    got = np_(out)
    assert not np.isnan(got).any(), "an element was left unwritten"
    assert bool(torch.isnan(buf[n:]).all()), "the guard band behind the output was written"
    ref = reference(L, H, pad, causal, tier == "bf16")
    e_abs, e_rel = err_of(got, ref)
    worst[0], worst[1] = max(worst[0], e_abs), max(worst[1], e_rel)
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL, err_msg=str((tier, L, H, pad, causal)))
    check_exact(got, ids_np, pad, causal, str((tier, L, H, pad, causal)))
    assert np.abs(got.astype(np.float64).sum(-1) - 1).max() <= 1e-5
    # a second call: the same bits
    assert torch.equal(bits(hip.attn_probs(qkv, ids, pad, H, causal)), bits(out))
    # the b_stride form: layer 1 of a [B, 3, H, L, L] tensor in place, the other layers' poison intact
    out5 = torch.full((B, 3, H, L, L), float("nan"), device="cuda", dtype=torch.float32)
    assert hip.attn_probs(qkv, ids, pad, H, causal, out=out5, layer=1) is out5
    assert torch.equal(bits(out5[:, 1]), bits(out))
    assert bool(torch.isnan(out5[:, 0]).all()) and bool(torch.isnan(out5[:, 2]).all())
    # user b alone: the bits it had inside the batch
    for b in range(B if B > 1 else 0):
        assert torch.equal(bits(hip.attn_probs(qkv[b:b + 1].contiguous(), ids[b:b + 1].contiguous(), pad, H, causal)), bits(out[b:b + 1])), b


# ---- a. the kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("tier", TIERS)
def test_attn_probs_against_float64(tier, L, capsys):
    worst = [0.0, 0.0]
    for H in (1, 3, 4):
        for causal in (False, True):
            run_shape(tier, L, H, 0, causal, worst)
    say(capsys, "attn_probs %-6s L=%-4d B=5 H=1,3,4 both masks: max|err| %.3g, largest err / (1e-5 + 1e-3 |ref|) %.3g" % (tier, L, worst[0], worst[1]))


@pytest.mark.parametrize("tier", TIERS)
def test_attn_probs_longest_and_other_pad_value(tier, capsys):
    worst = [0.0, 0.0]
    for causal in (False, True):
        run_shape(tier, 2048, 1, 0, causal, worst)
    say(capsys, "attn_probs %-6s L=2048 B=1 H=1 both masks: max|err| %.3g, largest err / (1e-5 + 1e-3 |ref|) %.3g" % (tier, worst[0], worst[1]))
    worst = [0.0, 0.0]
    for causal in (False, True):
        run_shape(tier, 65, 3, 37, causal, worst)            # the cross model's encoder masks on the EOS id, not on 0
    say(capsys, "attn_probs %-6s L=65 B=5 H=3 pad_value=37: max|err| %.3g, largest err / (1e-5 + 1e-3 |ref|) %.3g" % (tier, worst[0], worst[1]))


def test_attn_probs_refusals_launch_nothing():
    from recguru_amd import hip
    set_tier("f32")
    B, L, H = 2, 16, 2
    qkv = torch.randn(B, L, 3 * H * 32, device="cuda")
    ids = torch.ones(B, L, dtype=torch.int64, device="cuda")
    out = torch.full((B, H, L, L), float("nan"), device="cuda")
    fn = hip.lib().rg_attn_probs

    def call(dtype=hip.F32, **kw):
        f = dict(qkv=qkv.data_ptr(), key_ids=ids.data_ptr(), pad_value=0, causal=0, probs=out.data_ptr(), b_stride=H * L * L, B=B, L=L, H=H,
                 dk=32, scale=SCALE)
        f.update(kw)
        a = hip.AttnProbsArgs(*[f[n] for n, _ in hip.AttnProbsArgs._fields_])
        rc = fn(ctypes.byref(a), dtype, hip._stream())
        return rc, hip.lib().rg_last_error().decode()
    assert call(dk=64)[0] == -2 and "d_k" in call(dk=64)[1]
    assert call(L=2049, b_stride=H * 2049 * 2049)[0] == -2
    assert call(dtype=7)[0] == -2
    assert call(L=0)[0] == -1
    assert call(probs=None)[0] == -1 and call(qkv=None)[0] == -1 and call(key_ids=None)[0] == -1
    assert call(b_stride=H * L * L - 1)[0] == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call()[0] == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())


# ---- b. the cross maps ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 17, 64, 200])
def test_attn_cross_probs_bit_for_bit(L):
    from recguru_amd import hip
    for H, pad in ((1, 0), (3, 0), (4, 37)):
        ids_np = five_users(np.random.default_rng(L + H), L, pad)
        ids = torch.as_tensor(ids_np).cuda()
        want = R.cross_probs(ids_np, pad, L, H)
        n = 5 * H * L * L
        buf = torch.full((n + GUARD,), float("nan"), device="cuda", dtype=torch.float32)
        out = hip.attn_cross_probs(ids, pad, H, out=buf[:n].view(5, H, L, L))
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), (L, H, pad)
        assert bool(torch.isnan(buf[n:]).all())
        out5 = torch.full((5, 2, H, L, L), float("nan"), device="cuda", dtype=torch.float32)
        hip.attn_cross_probs(ids, pad, H, out=out5, layer=0)
        assert torch.equal(bits(out5[:, 0]), bits(out)) and bool(torch.isnan(out5[:, 1]).all())
        assert torch.equal(bits(hip.attn_cross_probs(ids[3:4].contiguous(), pad, H)), bits(out[3:4]))


# ---- c. the rollout -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 16, 65, 200])
def test_rollout_dyadic_fixtures_bit_for_bit(L):
    from recguru_amd import hip
    rng = np.random.default_rng(L)
    for H in (1, 2, 4):
        for N in (1, 3):
            B = 3
            maps = dyadic_maps(rng, B, N, H, L)
            query = rng.integers(0, L, size=B)
            dev = torch.as_tensor(maps).cuda()
            for q_np, q_dev in ((None, None), (query, torch.as_tensor(query).cuda())):
                want = R.rollout(maps, q_np, 0.5)
                assert np.array_equal(want.astype(np.float32).astype(np.float64), want)          # every intermediate is exact in f32
                got = hip.attn_rollout(dev, q_dev, 0.5)
                assert np.array_equal(got.cpu().numpy().view(np.uint32), want.astype(np.float32).view(np.uint32)), (L, H, N, q_np)
                assert torch.equal(bits(hip.attn_rollout(dev, q_dev, 0.5)), bits(got))


def test_rollout_random_maps_and_refusals(capsys):
    from recguru_amd import hip
    rng = np.random.default_rng(11)
    worst = 0.0
    for B, N, H, L in ((3, 2, 4, 200), (2, 3, 3, 65), (4, 1, 1, 17), (1, 2, 2, 417)):
        maps = rng.random((B, N, H, L, L)).astype(np.float32)
        maps[:, :, :, :, 1::3] = 0
        maps = (maps / maps.sum(-1, keepdims=True)).astype(np.float32)
        if N > 1:
            maps[:, -1] = np.tril(maps[:, -1])          # a causal top layer: most rows of r stay zero there
            maps[:, -1] = (maps[:, -1] / maps[:, -1].sum(-1, keepdims=True)).astype(np.float32)
        query = rng.integers(0, L, size=B)
        dev = torch.as_tensor(maps).cuda()
        bound = (N * (L + H) + 4) * 2.0 ** -24
        for alpha in (0.5, 0.2):
            want = R.rollout(maps, query, alpha)
            got = hip.attn_rollout(dev, torch.as_tensor(query).cuda(), alpha).cpu().numpy().astype(np.float64)
            err = float(np.abs(got - want).max())
            worst = max(worst, err / bound)
            assert err <= bound, (B, N, H, L, alpha, err, bound)
            assert float(np.abs(got.sum(-1) - 1).max()) <= bound
        last = torch.full((B,), L - 1, dtype=torch.int64, device="cuda")
        assert torch.equal(bits(hip.attn_rollout(dev)), bits(hip.attn_rollout(dev, last)))
        for bad in (-1, L):
            out = torch.full((B, L), float("nan"), device="cuda")
            q = last.clone()
            q[B - 1] = bad
            with pytest.raises(RuntimeError, match=r"rg_attn_rollout failed \(-1\): attn_rollout: query\[%d\] = %d is outside" % (B - 1, bad)):
                hip.attn_rollout(dev, q, 0.5, out=out)
            torch.cuda.synchronize()
            assert bool(torch.isnan(out).all())
    say(capsys, "attn_rollout random row-stochastic maps: largest |err| / ((N (L + H) + 4) 2^-24) = %.3g" % worst)


# ---- d. the models --------------------------------------------------------------------------------------------------------------
def build_single(name):
    from recguru_amd.config import get_param
    from recguru_amd.models import MyRec
    z, cfg, st, bt = load_case(name)
    B, L, d, H, N, Va, Vb, k, nb = [int(x) for x in z["meta"]]
    param = get_param(make_args(d, H, k, L, Va, Vb, N, B), make_dirs=False)
    M = MyRec("cuda", param, None, dec_rec=False, fix_enc=False, sas=False).to(torch.float32)
    res = M.load_state_dict(st, strict=False)
    assert all(kk.endswith(".pe") for kk in res.missing_keys) and not res.unexpected_keys
    return z, param, M.cuda().eval(), bt[0].cuda(), bt[1].cuda()


def single_maps(M, enc_in, dec_in):
    with torch.no_grad():
        h_enc, enc_self = M.AutoEnc.get_seq_embed(enc_in, return_attn=True)
        h_dec, dec_self, dec_enc = M.AutoEnc.get_dec_out(enc_in, dec_in, return_attn=True)
        h_rec, rec_self, rec_enc = M.get_embedding(enc_in, dec_in, return_attn=True)
        plain = (M.AutoEnc.get_seq_embed(enc_in), M.AutoEnc.get_dec_out(enc_in, dec_in), M.get_embedding(enc_in, dec_in))
        u_last, last_maps = M.AutoEnc.get_seq_embed(enc_in, last_only=True, return_attn=True)
        u_plain = M.AutoEnc.get_seq_embed(enc_in, last_only=True)
    # without the keyword: today's tuples, None in the map slots; with it: the same hidden states, bit for bit
    assert isinstance(plain[0], tuple) and len(plain[0]) == 2 and plain[0][1] is None
    assert isinstance(plain[1], tuple) and len(plain[1]) == 3 and plain[1][1] is None and plain[1][2] is None
    assert torch.is_tensor(plain[2])
    assert torch.equal(plain[0][0], h_enc) and torch.equal(plain[1][0], h_dec) and torch.equal(plain[2], h_rec)
    assert len(u_plain) == 2 and u_plain[1] is None and torch.equal(u_plain[0], u_last) and u_last.dim() == 2
    assert torch.equal(bits(last_maps), bits(enc_self))          # last_only: the last layer's map is still the full one
    maps = {"enc_self": enc_self, "dec_self": dec_self, "dec_enc": dec_enc, "rec_self": rec_self, "rec_enc": rec_enc}
    for t in maps.values():
        assert t.dtype == torch.float32 and t.is_contiguous()
    return {k: v.cpu().numpy() for k, v in maps.items()}


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", CASES)
def test_model_maps_against_the_reference(name, tier, capsys):
    set_tier(tier)
    z, param, M, enc_in, dec_in = build_single(name)
    got = single_maps(M, enc_in, dec_in)
    enc_np, dec_np = enc_in.cpu().numpy(), dec_in.cpu().numpy()
    B, N, H, L, _ = z["enc_self"].shape
    cross = R.cross_probs(enc_np, 0, L, H)
    for tag, ids, causal in (("enc_self", enc_np, False), ("dec_self", dec_np, True), ("rec_self", dec_np, True)):
        assert got[tag].shape == z[tag].shape
        e_abs, e_rel = err_of(got[tag], z[tag].astype(np.float64))
        say(capsys, "%s %-6s %-8s vs the reference's map: max|err| %.3g, largest err / (1e-5 + 1e-3 |ref|) %.3g%s"
            % (name, tier, tag, e_abs, e_rel, "  (not asserted in this tier)" if tier == "bf16" else ""))
        if tier != "bf16":
            np.testing.assert_allclose(got[tag], z[tag], rtol=RTOL, atol=ATOL, err_msg=tag)
        check_exact(got[tag], ids, 0, causal, "%s %s %s" % (name, tier, tag))
        assert np.abs(got[tag].astype(np.float64).sum(-1) - 1).max() <= 1e-5
    for tag in ("dec_enc", "rec_enc"):
        for l in range(N):
            assert np.array_equal(got[tag][:, l].view(np.uint32), cross.view(np.uint32)), (tag, l)
            assert np.array_equal(got[tag][:, l].view(np.uint32), z[tag][:, l].view(np.uint32)), (tag, l)


def test_single_model_explain():
    from recguru_amd import auto_training as at
    set_tier("f32")
    z, param, M, enc_in, dec_in = build_single(CASES[1])
    for training in (False, True):                          # dropout rate 0: train mode is allowed, and left as found
        M.train(training)
        ex = at.explain(M, enc_in, dec_in, param)
        assert M.training is training and M.AutoEnc.encoder.training is training
    assert sorted(ex) == ["dec_enc", "dec_rollout", "dec_self", "enc_rollout", "enc_self"]
    np.testing.assert_allclose(np_(ex["enc_self"]), z["enc_self"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(np_(ex["dec_self"]), z["rec_self"], rtol=RTOL, atol=ATOL)
    assert np.array_equal(np_(ex["dec_enc"]), z["rec_enc"])
    B, N, H, L, _ = z["enc_self"].shape
    for tag in ("enc", "dec"):
        want = R.rollout(np_(ex[tag + "_self"]), None, 0.5)
        assert float(np.abs(np_(ex[tag + "_rollout"]) - want).max()) <= (N * (L + H) + 4) * 2.0 ** -24
        assert tuple(ex[tag + "_rollout"].shape) == (B, L)


def test_cross_model_maps_and_explain(capsys):
    """MyAuto4Rec_c, d 128 / H 4 / N 2, synthetic users: get_seq_embed (key-pad = the EOS id) and recommend_forward against the restatement
    on the oracle's layer inputs; training.explain's rollouts against the restatement's rollout of the returned maps."""
    from recguru_amd import synthetic, training as T
    from recguru_amd.config import get_param
    from recguru_amd.models import MyAuto4Rec_c
    set_tier("f32")
    B, L, d, H, N, V = 6, 24, 128, 4, 2, 60
    param = get_param(make_args(d, H, 5, L, V, V, N, B), make_dirs=False)
    torch.manual_seed(5)
    G = MyAuto4Rec_c("cuda", param, wf=None, enc_share=True, dec_rec=False).to(torch.float32)
    st = {k: v.detach().clone() for k, v in G.state_dict().items() if not k.endswith(".pe")}
    for k in st:                                               # default initialisation has zero biases: give every parameter a value
        if k.endswith(".bias"):
            st[k] = 0.1 * torch.randn_like(st[k])
    G.load_state_dict(st, strict=False)
    G = G.cuda()
    dm = synthetic.make_domain(B, V, L, 5, seed=9, min_len=2)
    enc_in, dec_in = torch.as_tensor(dm["enc_in"]), torch.as_tensor(dm["dec_in"])
    dec_in[2] = 0                                              # one user whose decoder input is all padding
    enc_in[1, :L // 2] = 0                                     # ... and one left-padded to half the length
    dec_in[1, :L // 2] = 0
    assert enc_in.shape == (B, L)
    eos = param.vocab_size_a
    cfg = O.Cfg(d, H, N, L, 5, param.vocab_size_a, param.vocab_size_b)
    p = oracle_params(st, d, pe_keys=("pos_emb_a.pe", "pos_emb_b.pe"))
    mask = O.nonpad(dec_in, 0).double()                        # the recommender path: the encoder row mask comes from dec_in
    with torch.no_grad():
        taps = []
        enc_out = O.cross_get_seq_embed(p, cfg, enc_in, "a", mask, collect=taps)
        ref_enc = stack_maps(p, "encoder.", "enc_self_attn", taps[:N], enc_in, eos, False, H)
        x0 = O.embed_pe(p["src_emb_a.weight"], p["pos_emb_a.pe"][0], dec_in, mask)
        taps = []
        O.decoder_m(p, "recommend_a.", x0, enc_out[:, -1, :].unsqueeze(1).repeat(1, L, 1), O.pad_key_mask(dec_in, 0, L) | O.causal_mask(B, L),
                    O.pad_key_mask(enc_in, 0, L), mask, N, H, cfg.d_k, False, collect=taps)
        ref_dec = stack_maps(p, "recommend_a.", "dec_self_attn", [x0] + taps[:N - 1], dec_in, 0, True, H)
    e, di = enc_in.cuda(), dec_in.cuda()
    G.train()                                                  # rate 0: allowed; explain must leave the flag alone
    ex = T.explain(G, e, di, param, domain="a", device="cuda")
    assert G.training and G.encoder.training
    G.eval()
    m_dev = T.get_pad_mask(di, 0, "cuda")
    with torch.no_grad():
        x, enc_self = G.get_seq_embed(e, "a", m_dev, return_attn=True)
        h, dec_self, dec_enc = G.recommend_forward(e, di, "a", m_dev, return_attn=True)
        assert torch.equal(G.get_seq_embed(e, "a", m_dev), x) and torch.equal(G.recommend_forward(e, di, "a", m_dev), h)
        out3 = G.get_dec_out(e, di, "a", m_dev)
        assert len(out3) == 3 and out3[1] is None and out3[2] is None
        h3, s3, c3 = G.get_dec_out(e, di, "a", m_dev, return_attn=True)
        assert torch.equal(h3, out3[0]) and s3.shape == c3.shape == (B, N, H, L, L)
    for tag, got, ref in (("enc_self", enc_self, ref_enc), ("dec_self", dec_self, ref_dec)):
        e_abs, e_rel = err_of(np_(got), ref)
        say(capsys, "cross model f32 %-8s vs the restatement on the oracle's layer inputs: max|err| %.3g, largest err / (1e-5 + 1e-3 |ref|) %.3g"
            % (tag, e_abs, e_rel))
        np.testing.assert_allclose(np_(got), ref, rtol=RTOL, atol=ATOL, err_msg=tag)
    check_exact(np_(enc_self), enc_in.numpy(), eos, False, "cross enc_self")
    check_exact(np_(dec_self), dec_in.numpy(), 0, True, "cross dec_self")
    assert np.array_equal(np_(dec_enc), np.broadcast_to(R.cross_probs(enc_in.numpy(), 0, L, H)[:, None], (B, N, H, L, L)))
    assert torch.equal(bits(ex["enc_self"]), bits(enc_self)) and torch.equal(bits(ex["dec_self"]), bits(dec_self)) and torch.equal(bits(ex["dec_enc"]), bits(dec_enc))
    bound = (N * (L + H) + 4) * 2.0 ** -24
    for tag in ("enc", "dec"):
        want = R.rollout(np_(ex[tag + "_self"]), None, 0.5)
        assert float(np.abs(np_(ex[tag + "_rollout"]) - want).max()) <= bound
        assert float(np.abs(np_(ex[tag + "_rollout"]).astype(np.float64).sum(-1) - 1).max()) <= bound + 1e-5
