"""Pin the CPU oracle against vectors captured from the reference itself (oracle/gen_golden.py)."""
import math

import numpy as np
import pytest
import torch

from golden_util import arrays_to_manifest, load_case, make_state, sample
from oracle import recguru_oracle as O

CASES = ["case1", "case2"]


def load(name, dtype=torch.float32):
    z = load_case(name)
    B, L, d, H, N, Va, Vb, k, nb = [int(x) for x in z["meta"]]
    cfg = O.Cfg(d, H, N, L, k, Va + 1, Vb + 1, n_bpr_neg=nb)
    st = {}
    for tag in ("G", "D", "R"):
        man = arrays_to_manifest(z[tag + ".keys"], z[tag + ".shapes"], z[tag + ".ndim"])
        w = make_state(man, int(z[tag + ".seed"]))
        st[tag] = {kk: torch.as_tensor(v).to(dtype) for kk, v in w.items()}
        for kk, shp in man:
            if kk.endswith(".pe"):
                st[tag][kk] = O.positional_table(shp[1], shp[2], dtype).unsqueeze(0)
    bt = {}
    for dom in "ab":
        bt[dom] = tuple(torch.as_tensor(z["%s.%s" % (nm, dom)]) for nm in ("enc_in", "dec_in", "dec_out", "n_items"))
    return z, cfg, st, bt


def close(a, b, rtol=2e-4, atol=2e-6):
    a = a.detach().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    np.testing.assert_allclose(a, np.asarray(b, dtype=np.float64), rtol=rtol, atol=atol)


def _pe_recipe(L, d):
    """transformer.py:95-101's fp32 steps with exp / sin / cos evaluated in float64 and rounded to fp32 (the same on every host);
    returns the table and the fp32 angle under every element."""
    arg = np.arange(0, d, 2, dtype=np.float32) * np.float32(-(math.log(10000.0) / d))
    div = np.exp(arg.astype(np.float64)).astype(np.float32)
    ang = np.arange(L, dtype=np.float32)[:, None] * div[None, :]
    pe, angle = np.zeros((L, d), np.float32), np.zeros((L, d), np.float32)
    pe[:, 0::2], pe[:, 1::2] = np.sin(ang.astype(np.float64)), np.cos(ang.astype(np.float64))
    angle[:, 0::2], angle[:, 1::2] = ang, ang
    return pe, angle


@pytest.mark.parametrize("name", CASES)
def test_pe_table(name):
    """The positional table against the reference's own (tests/golden, captured on one host).  torch's fp32 exp / sin / cos go through
    MKL, which picks its kernels by CPU, so their last bits differ between hosts -- and one ulp of div_term moves an angle pos * div_term
    by up to two ulps (4.8e-7 in these rows).  The recipe is pinned host-independently (float64 transcendentals rounded to fp32) at the
    capture's tolerance; the table this host computes -- the oracle's, and the product's (the same torch steps) -- is held to that
    recipe within those last-bit effects: 3 ulps of the angle (one of div_term times pos, one of the product) and 2 of the value."""
    z, cfg, st, bt = load(name)
    host = st["G"]["pos_emb_a.pe"][0, :cfg.L].double().numpy()
    exact, angle = _pe_recipe(cfg.L, host.shape[1])
    close(exact, z["pe_head"], rtol=1e-6, atol=1e-7)
    bound = 3 * np.spacing(np.abs(angle)).astype(np.float64) + 2 * np.spacing(np.abs(exact)).astype(np.float64)
    assert (np.abs(host - exact) <= bound).all(), float((np.abs(host - exact) / bound).max())


@pytest.mark.parametrize("name", CASES)
def test_user_embed_and_layers(name):
    z, cfg, st, bt = load(name)
    col = []
    seq = bt["a"][0]
    mask = O.nonpad(seq)
    out = O.cross_get_seq_embed(st["G"], cfg, seq, "a", mask, collect=col)
    close(col[0], z["tap.embed_pe.a"])
    for i in range(cfg.n_layers):
        close(col[i + 1], z["tap.user_enc_layer%d.a" % i] * mask.unsqueeze(2).numpy())
    close(out[:, -1, :], z["user_embed.a"])
    close(O.get_user_embed(st["G"], cfg, bt["b"][0], "b"), z["user_embed.b"])


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("collapsed", [False, True])
def test_recon_logits_loss(name, collapsed):
    z, cfg, st, bt = load(name)
    enc_in, dec_in, dec_out, n_items = bt["a"]
    mask = O.nonpad(dec_out).view(-1)
    col = []
    h = O.cross_get_dec_out(st["G"], cfg, enc_in, dec_in, "a", mask, collapsed=collapsed, collect=col)
    d_mask = O.nonpad(enc_in).unsqueeze(2).numpy()
    for i in range(cfg.n_layers):
        close(col[i], z["tap.ae_dec_layer%d.a" % i] * d_mask, rtol=5e-4, atol=5e-6)
    lg = O.cross_forward(st["G"], cfg, enc_in, dec_in, dec_out, n_items, "a", mask, collapsed)
    close(lg, z["logits.a"], rtol=5e-4, atol=2e-5)
    close(O.loss_ae_cross(st["G"], cfg, *bt["a"], domain="a", collapsed=collapsed), z["loss_ae.a"], rtol=1e-5)
    close(O.loss_ae_cross(st["G"], cfg, *bt["b"], domain="b", collapsed=collapsed), z["loss_ae.b"], rtol=1e-5)


def close_frac(a, b, rtol, atol, bad_frac=0.005, msg=""):
    """allclose, tolerating a tiny fraction of elements: one Adam step moves an element whose
    gradient is at rounding-noise level by up to lr in either direction."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    bad = np.abs(a - b) > atol + rtol * np.abs(b)
    assert bad.mean() <= bad_frac, "%s: %d/%d elements differ (max %g)" % (msg, bad.sum(), bad.size, np.abs(a - b).max())


def _grad_check(params, z, prefix, rtol=2e-3, atol=2e-6, skip=()):
    n = 0
    for k, t in params.items():
        key = prefix + k
        if key not in z:
            continue
        if any(s in k for s in skip):
            continue
        assert t.grad is not None, k
        g = sample(t.grad.numpy())
        ref = z[key]
        scale = max(float(np.abs(ref).max()), 1e-12)
        np.testing.assert_allclose(g, ref, rtol=rtol, atol=atol + 1e-4 * scale, err_msg=k)
        n += 1
    assert n >= 8


# WQ/WK of the degenerate cross-attention get exactly-zero gradients in the collapsed form and
# rounding-noise gradients (|g| ~ 1e-9) in the reference; see DESIGN.md "dead parameters".
DEAD = ("dec_enc_attn.WQ", "dec_enc_attn.WK")
# every key bias is structurally gradient-free too (softmax is invariant to a per-query constant),
# so after Adam its value is sign(noise) * lr in the reference: excluded from post-step checks.
NOISE = DEAD + ("WK.bias",)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("collapsed", [False, True])
def test_recon_grads_and_noam_adam_step(name, collapsed):
    z, cfg, st, bt = load(name)
    p = O.leafify(st["G"])
    la = O.loss_ae_cross(p, cfg, *bt["a"], domain="a", collapsed=collapsed)
    lb = O.loss_ae_cross(p, cfg, *bt["b"], domain="b", collapsed=collapsed)
    la.backward()
    lb.backward()
    _grad_check(p, z, "gradG_recon.", skip=DEAD)
    if collapsed:
        for k, t in p.items():
            if any(s in k for s in DEAD) and (k.startswith("decoder_a") or k.startswith("decoder_b")):
                assert t.grad is None or float(t.grad.abs().max()) == 0.0
                assert float(np.abs(z["gradG_recon." + k]).max()) < 1e-6
        return
    lrs = [O.noam_lr(s, cfg.d_model, 7) for s in range(1, 11)]
    np.testing.assert_allclose(lrs, z["noam_lr"], rtol=1e-12)
    trainable = {k: t for k, t in p.items() if t.requires_grad}
    opt = O.Adam(trainable, lrs[0], (0.9, 0.98), 1e-9)
    opt.step()
    for k, t in trainable.items():
        if any(s in k for s in NOISE):
            continue                         # Adam amplifies rounding-noise gradients of dead params
        close_frac(sample(t.detach().numpy()), z["G_after_recon_step." + k],
                   rtol=1e-4, atol=2e-4 * lrs[0] + 1e-6, msg=k)


@pytest.mark.parametrize("name", CASES)
def test_bpr_recommend(name):
    z, cfg, st, bt = load(name)
    p = O.leafify(st["G"])
    enc_in, dec_in, dec_out, _ = bt["a"]
    nb = torch.as_tensor(z["n_items_bpr.a"])
    mask = O.nonpad(dec_out).view(-1)
    loss = O.loss_bpr_cross(p, cfg, enc_in, dec_in, dec_out, nb, mask, "a", fixed_enc=True)
    close(loss, z["loss_bpr.a"], rtol=1e-5)
    loss.backward()
    _grad_check(p, z, "gradG_bpr.", skip=DEAD)


@pytest.mark.parametrize("name", CASES)
def test_discriminator_gp(name):
    z, cfg, st, bt = load(name)
    pD = O.leafify(st["D"])
    ae = torch.as_tensor(z["user_embed.a"])
    be = torch.as_tensor(z["user_embed.b"])
    alpha = torch.as_tensor(z["alpha"])
    close(O.discriminator(pD, ae), z["D_real"], rtol=1e-4, atol=1e-6)
    close(O.discriminator(pD, be), z["D_fake"], rtol=1e-4, atol=1e-6)
    dis_loss, gp, d_cost, w_d = O.critic_losses(pD, ae, be, alpha)
    close(dis_loss, z["dis_loss"], rtol=1e-4, atol=1e-7)
    close(gp, z["gp"], rtol=1e-4)
    dis_loss.backward()
    gp.backward()
    _grad_check(pD, z, "gradD_critic.", rtol=1e-3)
    # closed form GP == autograd GP (value and weight grads), no bias gradient
    gp2, gw = O.gradient_penalty_closed(st["D"], ae, be, alpha)
    close(gp2, z["gp"], rtol=1e-4)
    pD2 = O.leafify(st["D"])
    O.gradient_penalty_autograd(pD2, ae, be, alpha).backward()
    for k, g in gw.items():
        np.testing.assert_allclose(g.numpy(), pD2[k].grad.numpy(), rtol=2e-3, atol=1e-7, err_msg=k)
    for k, t in pD2.items():
        if k.endswith(".bias"):
            assert t.grad is None or float(t.grad.abs().max()) == 0.0
    opt = O.Adam(pD, 1e-4, (0.5, 0.9), 1e-8)
    opt.step()
    for k, t in pD.items():
        close_frac(sample(t.detach().numpy()), z["D_after_critic_step." + k], rtol=1e-4, atol=2e-6, msg=k)


@pytest.mark.parametrize("name", CASES)
def test_generator_step(name):
    z, cfg, st, bt = load(name)
    pG = O.leafify(st["G"])
    pD = st["D"]
    ae = O.get_user_embed(pG, cfg, bt["a"][0], "a")
    be = O.get_user_embed(pG, cfg, bt["b"][0], "b")
    g_dis = O.discriminator(pD, ae).mean() - O.discriminator(pD, be).mean()
    close(g_dis, z["g_dis_loss"], rtol=1e-4, atol=1e-7)
    g_dis.backward()
    _grad_check(pG, z, "gradG_gdis.")
    for t in pG.values():
        t.grad = None
    opt = O.Adam({k: t for k, t in pG.items() if t.requires_grad}, 1e-4, (0.5, 0.9), 1e-8)
    O.generator_step(pG, pD, cfg, bt["a"], bt["b"], opt)
    for k, t in pG.items():
        if not t.requires_grad or any(s in k for s in NOISE):
            continue
        close_frac(sample(t.detach().numpy()), z["G_after_gen_step." + k], rtol=1e-4, atol=1e-5, msg=k)


@pytest.mark.parametrize("name", CASES)
def test_single_domain(name):
    z, cfg, st, bt = load(name)
    p = O.leafify(st["R"])
    enc_in, dec_in, dec_out, n_items = bt["a"]
    lg = O.single_forward(p, cfg, enc_in, dec_in, dec_out, n_items, pre="AutoEnc.")
    close(lg, z["single.logits"], rtol=5e-4, atol=2e-5)
    loss = O.loss_ae_single(p, cfg, enc_in, dec_in, dec_out, n_items)
    close(loss, z["single.loss_ae"], rtol=1e-5)
    loss.backward()
    _grad_check(p, z, "gradR_recon.", skip=DEAD)
    assert float(p["AutoEnc.src_emb.weight"].grad[0].abs().max()) >= 0.0
    nb = torch.as_tensor(z["n_items_bpr.a"])
    pl, nl = O.myrec_bpr_logits(st["R"], cfg, enc_in, dec_in, dec_out, nb)
    close(pl, z["single.p_logits"], rtol=5e-4, atol=2e-5)
    close(nl, z["single.n_logits"], rtol=5e-4, atol=2e-5)
    m = O.nonpad(dec_in).view(-1)
    close(O.bpr_loss_sas(pl, nl, m), z["single.loss_bpr_sas"], rtol=1e-5)
    close(O.bpr_loss(pl, nl, m), z["single.loss_bpr"], rtol=1e-5)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("collapsed", [False, True])
def test_ranking_eval(name, collapsed):
    """get_scores / double-argsort rank / hit-NDCG-MRR@k against the reference (oracle/gen_golden_eval.py)."""
    z, cfg, st, bt = load(name)
    ze = load_case("eval_" + name)
    cand = int(ze["candidate_size"])
    for dom in "ab":
        enc_in, dec_in = bt[dom][0], bt[dom][1]
        sc = O.get_scores(st["G"], cfg, enc_in, dec_in, torch.as_tensor(ze["target.%s" % dom]),
                          torch.as_tensor(ze["n_items.%s" % dom]), dom, cand, collapsed=collapsed)
        close(sc, ze["scores.%s" % dom], rtol=2e-4, atol=2e-5)
        ranks = O.ranks_from_scores(sc).numpy()
        assert (ranks == ze["ranks.%s" % dom]).all()
        for i, k in enumerate((1, 5, 10, 20, 30)):
            np.testing.assert_allclose(O.metrics_at_k(ranks, k), ze["metrics.%s" % dom][i], rtol=1e-12, atol=0)


def test_loss_curves_through_reference_drivers():
    """20 phase-1 steps + 5 phase-2 + 5 phase-3 iterations of the reference's own train_recon_x / train_gan_all
    (oracle/gen_golden_curves.py) replayed by the oracle's restatement of those drivers, point by point.

    Tolerance: phase 1 rtol 1e-3.  From the second phase-2 iteration on the REFERENCE's trajectory is discontinuous
    in rounding noise (ReLU masks inside the gradient penalty, Adam's +-lr steps on rounding-level gradients): the
    fixture stores, per series, the band the same arithmetic spans under different rounding (gen_golden_curves.py
    add_bands); parity_util.curve_bands turns it into the bound 2 x band + 2e-5 used here and by the GPU replay."""
    from parity_util import curve_bands, curve_replay_oracle
    z = load_case("curves1")
    p1, p2, p3, lr_last = curve_replay_oracle(z, torch.float32)
    np.testing.assert_allclose(p1, z["phase1.loss"], rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(lr_last, float(z["phase1.lr_last"]), rtol=1e-12)
    bands = curve_bands(z)
    for i, nm in enumerate(("D_cost", "Wasserstein_D", "recon_a", "recon_b", "g_dis")):
        np.testing.assert_allclose(p2[:, i], z["phase2." + nm], rtol=1e-3, atol=bands["phase2." + nm], err_msg=nm)
    np.testing.assert_allclose(p3[:, 0], z["phase3.loss_recommend"], rtol=1e-3, atol=bands["phase3.loss_recommend"])
    np.testing.assert_allclose(p3[:, 1], z["phase3.loss_recon_rec"], rtol=1e-3, atol=bands["phase3.loss_recon_rec"])


def test_overlap_term_and_recommendation_tune_through_reference_drivers():
    """tests/golden/curves2.npz: the reference's train_gan_all(overlap=True) -- phase 2 with the MSE between the two user
    embeddings of overlapped users (gan_training.py:28-35,:494-507) -- and recommendation_tune (:895-969), recorded through
    the reference's own drivers (oracle/gen_golden_curves2.py), replayed by the oracle's restatement within the stored
    rounding bands (2 x band + 2e-5, as for curves1)."""
    from parity_util import curve2_replay_oracle, curve_bands
    z = load_case("curves2")
    p2, p3, tune = curve2_replay_oracle(z, torch.float32)
    bands = curve_bands(z)
    for i, nm in enumerate(("D_cost", "Wasserstein_D", "recon_a", "recon_b", "g_dis")):
        np.testing.assert_allclose(p2[:, i], z["phase2." + nm], rtol=1e-4, atol=bands["phase2." + nm], err_msg=nm)
    np.testing.assert_allclose(p3[:, 0], z["phase3.loss_recommend"], rtol=1e-4, atol=bands["phase3.loss_recommend"])
    np.testing.assert_allclose(p3[:, 1], z["phase3.loss_recon_rec"], rtol=1e-4, atol=bands["phase3.loss_recon_rec"])
    np.testing.assert_allclose(tune, z["tune.loss"], rtol=1e-4, atol=bands["tune.loss"])
    assert p2.shape == (3, 5) and p3.shape == (3, 2) and tune.shape == (6,)
