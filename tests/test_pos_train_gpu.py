"""Learned positions (pos_train=True) on the HIP path: fixture parity with the reference (tools/gen_golden_pos_train.py), the autograd
op against the kernel restatement, the cross model's extension against the CPU oracle, training steps, scoring and the entry point."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import pos_grad_ref
from golden_util import load_case, sample
from oracle import recguru_oracle as O
from parity_util import batches, case_param, max_err, state_of
from pos_train_util import CASES, PE_KEY, POS_KEY, case_args, load, oracle_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEAD = ("dec_enc_attn.WQ", "dec_enc_attn.WK")
SEED = 0x5EED00000000BEEF


@pytest.fixture(autouse=True)
def _f32_tier():
    from recguru_amd import ops
    ops.set_compute_dtype(torch.float32)
    yield
    ops.set_compute_dtype(torch.bfloat16)


def np_(t):
    return t.detach().float().cpu().numpy()


def grad_close(got, ref, msg, rtol=2e-3):
    """tests/test_parity_gpu.py::check_grads' rule: rtol 2e-3, atol 2e-6 + 2e-4 * the tensor's scale."""
    scale = max(float(np.abs(ref).max()), 1e-12)
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=2e-6 + 2e-4 * scale, err_msg=msg)


def build_single(z, st, pos_train=True, **kw):
    from recguru_amd.config import get_param
    from recguru_amd.models import MyRec
    param = get_param(case_args(z, pos_train=pos_train, **kw), make_dirs=False)
    R = MyRec("cuda", param, None, dec_rec=False, fix_enc=False, sas=False, pos_train=pos_train).to(torch.float32)
    if pos_train:
        R.load_state_dict(st, strict=True)
    else:
        R.load_state_dict({k: v for k, v in st.items() if k != POS_KEY}, strict=False)
    return param, R.cuda()


# ---- 1. fixture parity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["f32", "bf16x3"])
@pytest.mark.parametrize("name", CASES)
def test_fixture_parity(name, tier):
    from recguru_amd import ops
    ops.set_compute_dtype(torch.float32 if tier == "f32" else tier)
    z, cfg, man, st, bt = load(name)
    param, R = build_single(z, st)
    R.eval()
    enc_in, dec_in, dec_out, n_items = (t.cuda() for t in bt)
    m_in = (dec_in != 0).float().view(-1)
    with torch.no_grad():
        ue = R.AutoEnc.get_seq_embed(enc_in, last_only=True)[0]
        bpr = R(enc_in, dec_in, dec_out, torch.as_tensor(z["n_items_bpr"]).cuda(), recon=False).bpr(m_in)
    np.testing.assert_allclose(np_(ue), z["user_embed"], rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(float(bpr), float(z["loss_bpr"]), rtol=1e-3, atol=1e-5)
    loss = R(enc_in, dec_in, dec_out, n_items, recon=True).loss(m_in)
    np.testing.assert_allclose(float(loss.detach()), float(z["loss_ae"]), rtol=1e-3, atol=1e-5)
    loss.backward()
    n = 0
    for k, p in R.named_parameters():
        key = "gradR_recon." + k
        if key not in z or any(s in k for s in DEAD):
            continue
        assert p.grad is not None, k
        grad_close(np_(p.grad) if k == POS_KEY else sample(np_(p.grad)), z[key], k)
        n += 1
    assert n >= 8 and z["gradR_recon." + POS_KEY].shape == tuple(R.AutoEnc.pos_emb.table().shape)


@pytest.mark.parametrize("name", CASES)
def test_bf16_tier_is_finite_and_its_drift_is_printed(name, capsys):
    from recguru_amd import ops
    ops.set_compute_dtype(torch.bfloat16)
    z, cfg, man, st, bt = load(name)
    param, R = build_single(z, st)
    R.eval()
    enc_in, dec_in, dec_out, n_items = (t.cuda() for t in bt)
    m_in = (dec_in != 0).float().view(-1)
    with torch.no_grad():
        ue = R.AutoEnc.get_seq_embed(enc_in, last_only=True)[0]
    loss = R(enc_in, dec_in, dec_out, n_items, recon=True).loss(m_in)
    loss.backward()
    g = np_(R.AutoEnc.pos_emb.table().grad)
    e_abs, e_rel = max_err(np_(ue), z["user_embed"])
    l_rel = abs(float(loss.detach()) - float(z["loss_ae"])) / abs(float(z["loss_ae"]))
    g_rel = max_err(g, z["gradR_recon." + POS_KEY])[1]
    with capsys.disabled():
        print("\n[bf16 tier %s] user_embed max|err|=%.3g (rel-to-max %.3g)  loss_ae rel err=%.3g  position-table grad rel-to-max %.3g"
              % (name, e_abs, e_rel, l_rel, g_rel))
    assert np.isfinite(np_(ue)).all() and np.isfinite(float(loss.detach())) and np.isfinite(g).all()
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in R.parameters())


# ---- 2. the op ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["f32", "bf16", "bf16_split_resid"])
def test_embed_pe_position_gradient(tier, monkeypatch):
    from recguru_amd import ops
    ops.set_compute_dtype(torch.float32 if tier == "f32" else torch.bfloat16)
    monkeypatch.setattr(ops, "_RESID", torch.float32 if tier == "bf16_split_resid" else torch.bfloat16)      # (set_residual_dtype, undone after the test)
    assert ops._split_resid() == (tier == "bf16_split_resid")
    monkeypatch.setattr(ops, "_draw", lambda: SEED)
    B, L, d, V, p = 5, 7, 128, 23, 0.5
    rng = np.random.default_rng(17)
    table = torch.nn.Parameter(torch.as_tensor(rng.standard_normal((V, d)), dtype=torch.float32).cuda())
    pe_np = rng.standard_normal((L + 2, d)).astype(np.float32)
    pe = torch.nn.Parameter(torch.as_tensor(pe_np).cuda())
    ids = torch.as_tensor(rng.integers(1, V, size=(B, L))).cuda()
    lens = np.array([7, 4, 1, 6, 2])
    mask_np = (np.arange(L)[None, :] >= (L - lens)[:, None]).astype(np.float32)
    mask = torch.as_tensor(mask_np).cuda()
    out = ops.embed_pe(table, pe, ids, mask, drop_p=p)
    with torch.no_grad():
        out_buf = ops.embed_pe(table, pe.detach().clone(), ids, mask, drop_p=p)          # the same values as a plain buffer
    assert out.dtype == out_buf.dtype and torch.equal(out.view(torch.int32 if tier == "f32" else torch.int16),
                                                      out_buf.view(torch.int32 if tier == "f32" else torch.int16))
    dx = torch.as_tensor(rng.standard_normal((B, L, d)), dtype=torch.float32).cuda().to(out.dtype)
    out.backward(dx)
    assert pe.grad is not None and tuple(pe.grad.shape) == (L + 2, d) and table.grad is not None
    prior = np.zeros((L + 2, d), np.float32)
    ref, abs_sum = pos_grad_ref.pos_grad(dx.float().cpu().numpy().astype(np.float64), mask_np, prior, p, SEED)
    got = np_(pe.grad).astype(np.float64)
    assert (np.abs(got[:L] - ref[:L]) <= pos_grad_ref.bound(B, prior[:L], abs_sum)).all()
    assert float(np.abs(got[L:]).max()) == 0.0 and float(np.abs(ref).max()) > 0
    # the forward is the restatement's mask too: dropped elements are exactly zero where keep is
    keep = pos_grad_ref.keep_array(SEED, p, B, L, d)
    assert np.array_equal(np_(out) == 0, (keep * mask_np[:, :, None]) == 0)


# ---- 3. the cross model's extension -----------------------------------------------------------------------------------------
def test_cross_model_against_oracle():
    from recguru_amd import training as T
    from recguru_amd.models import MyAuto4Rec_c
    z = load_case("case1")
    param = case_param(z)
    B, L = z["enc_in.a"].shape
    G = MyAuto4Rec_c("cuda", param, wf=None, enc_share=True, dec_rec=False, pos_train=True).to(torch.float32)
    st = state_of(z, "G")
    rng = np.random.default_rng(91)
    pos = {"pos_emb_%s.pos_emb.weight" % dom: torch.as_tensor(rng.standard_normal((param.enc_maxlen, param.d_model)), dtype=torch.float32)
           for dom in "ab"}
    st.update(pos)
    G.load_state_dict(st, strict=True)
    G = G.cuda().eval()
    cfg = O.Cfg(param.d_model, param.num_heads, param.num_blocks, L, param.n_negs, param.vocab_size_a, param.vocab_size_b)
    pairs = tuple(("pos_emb_%s.pos_emb.weight" % dom, "pos_emb_%s.pe" % dom) for dom in "ab")
    bt, cb = batches(z, "cuda"), batches(z, "cpu")
    p = oracle_params(st, pairs)
    for dom in "ab":
        ref = O.loss_ae_cross(p, cfg, *cb[dom], domain=dom)
        (g_ref,) = torch.autograd.grad(ref, p["pos_emb_%s.pe" % dom])
        mask = T.get_pad_mask(bt[dom][2], 0, "cuda")
        loss = T.loss_ae(G, *bt[dom], True, B, L, param, mask, "cuda", domain=dom)
        np.testing.assert_allclose(float(loss.detach()), float(ref.detach()), rtol=1e-3, atol=1e-5)
        loss.backward()
        grad_close(np_(G._emb(dom)[1].table().grad), g_ref[0].numpy(), "pos_emb_" + dom)
    # fixed_enc + recommend_forward: the position gradient comes from the decoder-side stage only
    assert param.fixed_enc
    G.zero_grad(set_to_none=True)
    enc_in, dec_in, dec_out, _ = cb["a"]
    nb = torch.as_tensor(z["n_items_bpr.a"])
    m_ref = O.nonpad(dec_out).view(-1)
    ref = O.loss_bpr_cross(p, cfg, enc_in, dec_in, dec_out, nb, m_ref, "a", fixed_enc=True)
    (g_ref,) = torch.autograd.grad(ref, p["pos_emb_a.pe"])
    mask = T.get_pad_mask(bt["a"][2], 0, "cuda")
    loss = T.loss_bpr_func(G, bt["a"][0], bt["a"][1], bt["a"][2], nb.cuda(), mask, "a", param)
    np.testing.assert_allclose(float(loss.detach()), float(ref.detach()), rtol=1e-3, atol=1e-5)
    loss.backward()
    grad_close(np_(G.pos_emb_a.table().grad), g_ref[0].numpy(), "pos_emb_a (fixed_enc)")
    assert G.pos_emb_b.table().grad is None and G.encoder.layers[0].pos_ffn.l1.weight.grad is None


# ---- 4. training, and the fixed path --------------------------------------------------------------------------------------
def _one_batch_loader(bt):
    enc_in, dec_in, dec_out, n_items = (t.cuda() for t in bt)
    zero = torch.zeros(enc_in.shape[0], dtype=torch.long, device="cuda")
    return [((enc_in, dec_in, dec_out), n_items, zero, zero)]


def _train3(R, param, bt):
    from recguru_amd import auto_training as at, blocks
    from recguru_amd.optim import Adam
    opt = blocks.ScheduledOptim(Adam(R.parameters(), betas=(0.9, 0.99), eps=1e-09), 1.0, param.d_model, 4)
    ld = _one_batch_loader(bt)
    losses, _ = at.train(R, opt, 3, [ld, ld], param, "cuda", neg_sample=True, loss_type="s_soft", opt_type="schedule", epochs=3,
                         max_steps=3, verbose=False)
    torch.cuda.synchronize()
    return opt, losses


def test_three_training_steps_move_the_table(tmp_path):
    from recguru_amd.models import MyRec
    z, cfg, man, st, bt = load(CASES[1])
    param, R = build_single(z, st, dropout=0.5, result_path=str(tmp_path))
    assert param.pos_train is True and param.dropout_rate == 0.5
    before = R.AutoEnc.pos_emb.table().detach().clone()
    opt, losses = _train3(R, param, bt)
    table = R.AutoEnc.pos_emb.table()
    assert len(losses) == 3 and all(np.isfinite(losses))
    assert not torch.equal(table.detach(), before) and float((table.detach() - before).abs().max()) > 0
    assert all(bool(torch.isfinite(v).all()) for v in R.state_dict().values())
    assert table in opt._optimizer.state and opt._optimizer.state[table]["step"] == 3
    assert bool(torch.isfinite(opt._optimizer.state[table]["exp_avg"]).all()) and float(opt._optimizer.state[table]["exp_avg"].abs().max()) > 0
    R2 = MyRec("cuda", param, None, pos_train=True).to(torch.float32)
    R2.load_state_dict({k: v.cpu() for k, v in R.state_dict().items()}, strict=True)
    for k, v in R.state_dict().items():
        assert torch.equal(R2.state_dict()[k].cpu(), v.cpu()), k


def test_fixed_positions_launch_nothing_new(tmp_path, monkeypatch):
    from recguru_amd import hip
    z, cfg, man, st, bt = load(CASES[1])
    param, R = build_single(z, st, pos_train=False, dropout=0.5, result_path=str(tmp_path))

    def boom(*a, **kw):
        raise AssertionError("pos_grad launched on the fixed-position path")
    monkeypatch.setattr(hip, "pos_grad", boom)
    pe0 = R.AutoEnc.pos_emb.pe.detach().clone()
    opt, losses = _train3(R, param, bt)
    assert len(losses) == 3 and all(np.isfinite(losses))
    assert torch.equal(R.AutoEnc.pos_emb.pe.view(torch.int32), pe0.view(torch.int32))
    keys = list(R.state_dict().keys())
    assert PE_KEY in keys and POS_KEY not in keys and [k for k in keys if k != PE_KEY] == [k for k, _ in man if k != POS_KEY]


# ---- 5. scoring -----------------------------------------------------------------------------------------------------------
def _oracle_rec_state(p, cfg, enc_in, dec_in):
    """The last state of MyRec's recommender decoder (AutoEnc4Rec.py:55-85), as O.myrec_bpr_logits builds it."""
    B, L = enc_in.shape
    u = O.single_get_seq_embed(p, cfg, enc_in, "AutoEnc.")[:, -1, :]
    mask = O.nonpad(dec_in, cfg.pad_index)
    x = O.embed_pe(p["AutoEnc.src_emb.weight"], p[PE_KEY][0], dec_in, mask)
    self_masked = O.pad_key_mask(dec_in, cfg.pad_index, L) | O.causal_mask(B, L)
    cross_masked = O.pad_key_mask(enc_in, cfg.pad_index, L)
    h = O.decoder_m(p, "recommend.", x, u.unsqueeze(1).repeat(1, L, 1), self_masked, cross_masked, mask, cfg.n_layers, cfg.n_heads, cfg.d_k, False)
    return h[:, -1, :]


def test_scoring_and_length_check():
    from recguru_amd import auto_training as at
    z, cfg, man, st, bt = load(CASES[0])
    param, R = build_single(z, st)
    R.eval()
    enc_in, dec_in = bt[0], bt[1]
    with torch.no_grad():
        h = _oracle_rec_state(oracle_params(st), cfg, enc_in, dec_in)
        full = (h @ st["AutoEnc.src_emb.weight"].t()).numpy()                     # [B, V + 2] oracle scores of every table row
    B, V, C, K = enc_in.shape[0], param.vocab_size - 1, 9, 5
    rng = np.random.default_rng(5)
    target = torch.as_tensor(rng.integers(1, V + 1, size=B))
    cand = torch.as_tensor(rng.integers(1, V + 1, size=(B, C)))
    param.candidate_size = C
    sc = at.get_scores(R, enc_in.cuda(), dec_in.cuda(), target.cuda(), cand.cuda(), param)
    cols = torch.cat([target.view(B, 1), cand], 1).numpy()
    np.testing.assert_allclose(np_(sc), np.take_along_axis(full, cols, 1), rtol=1e-3, atol=2e-5)
    ids, scores = at.recommend(R, enc_in.cuda(), dec_in.cuda(), K, param, exclude_seen=False)
    ids, scores = ids.cpu().numpy(), np_(scores)
    assert ids.shape == (B, K) and ids.min() >= 1 and ids.max() <= V
    np.testing.assert_allclose(scores, np.take_along_axis(full, ids, 1), rtol=1e-3, atol=2e-5)
    np.testing.assert_allclose(scores, -np.sort(-full[:, 1:V + 1], axis=1)[:, :K], rtol=1e-3, atol=2e-5)
    L1 = param.enc_maxlen + 1
    long_ids = torch.ones(2, L1, dtype=torch.long, device="cuda")
    with pytest.raises(ValueError):
        at.recommend(R, long_ids, long_ids, K, param, exclude_seen=False)
    with pytest.raises(ValueError):
        R(long_ids, long_ids, long_ids, torch.ones(2, L1 * param.n_negs, dtype=torch.long, device="cuda"), recon=True)


# ---- 6. the entry point -----------------------------------------------------------------------------------------------------
def test_train_auto_entry_point_with_learned_positions(tmp_path):
    res = str(tmp_path)
    r = subprocess.run([sys.executable, "train_auto.py", "--synthetic", "8192", "--seq_len", "50", "--d_model", "64", "--n_head", "2",
                        "--batch_size", "1024", "--batch_size_val", "128", "--vocab_size_a", "10000", "--n_negs", "30", "--steps", "3",
                        "--tune_steps", "3", "--epochs", "1", "--pos_train", "True", "--result_path", res],
                       cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-4000:]
    assert "saved" in out
    vals = [float(v) for v in re.findall(r"(?:Reconstruction|BPR) loss after \d+ epochs: (\S+)", out)]
    assert len(vals) >= 2 and all(np.isfinite(vals))
    sub = [d for d in os.listdir(res) if os.path.isdir(os.path.join(res, d))]
    sd = torch.load(os.path.join(res, sub[0], "model", "model"), map_location="cpu", weights_only=True)
    assert tuple(sd[POS_KEY].shape) == (50, 64) and PE_KEY not in sd and bool(torch.isfinite(sd[POS_KEY]).all())
    assert os.path.exists(os.path.join(res, sub[0], "result_sas_org.pickle"))
