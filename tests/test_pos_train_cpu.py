"""Learned positions (pos_train=True) without a GPU: the CPU oracle against fixtures written by the reference itself
(tools/gen_golden_pos_train.py), the module surface and state_dict keys, and the float64 restatement of the position-gradient
kernel (tests/pos_grad_ref.py) against torch autograd."""
import argparse

import numpy as np
import pytest
import torch

import pos_grad_ref
from golden_util import sample
from oracle import recguru_oracle as O
from pos_train_util import CASES, PE_KEY, POS_KEY, case_args, load, oracle_params


def close(a, b, rtol=1e-5, atol=2e-6):
    a = a.detach().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    np.testing.assert_allclose(a, np.asarray(b, dtype=np.float64), rtol=rtol, atol=atol)


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_the_reference_with_learned_positions(name):
    """The unchanged oracle, fed the learned table as '<prefix>pos_emb.pe' = weight[None], reproduces the reference's losses, user
    embedding and -- by autograd with respect to that leaf -- its position-table gradient (rtol 1e-5 on the losses, as
    test_oracle_golden.py holds the other cases; gradients by its rule).  This licenses the oracle as the reference at other shapes."""
    z, cfg, man, st, bt = load(name)
    assert (POS_KEY, (cfg.L, cfg.d_model)) in man and not any(k.endswith(".pe") for k, _ in man)
    p = oracle_params(st)
    enc_in, dec_in, dec_out, n_items = bt
    assert int((dec_in[4] != 0).sum()) == 0                        # the length-1 user's decoder is all padding
    close(O.single_get_seq_embed(p, cfg, enc_in, "AutoEnc.")[:, -1, :], z["user_embed"], rtol=2e-4)
    loss = O.loss_ae_single(p, cfg, enc_in, dec_in, dec_out, n_items)
    close(loss, z["loss_ae"], rtol=1e-5, atol=0)
    pl, nl = O.myrec_bpr_logits(p, cfg, enc_in, dec_in, dec_out, torch.as_tensor(z["n_items_bpr"]))
    close(O.bpr_loss(pl, nl, O.nonpad(dec_in).view(-1)), z["loss_bpr"], rtol=1e-5, atol=0)
    (g_pe,) = torch.autograd.grad(loss, p[PE_KEY], retain_graph=True)
    ref = z["gradR_recon." + POS_KEY]
    assert ref.shape == (cfg.L, cfg.d_model) and float(np.abs(ref).max()) > 0
    # rtol 1e-5, element-wise and of the table's scale: both sides sum the same f32 terms in different orders, so an element near zero
    # carries the absolute rounding error of the large ones
    scale = float(np.abs(ref).max())
    np.testing.assert_allclose(g_pe[0].numpy(), ref, rtol=1e-5, atol=1e-5 * scale)
    loss.backward()
    n = 0
    for k, t in p.items():
        key = "gradR_recon." + k
        if key not in z or "dec_enc_attn.WQ" in k or "dec_enc_attn.WK" in k:
            continue
        s = max(float(np.abs(z[key]).max()), 1e-12)
        np.testing.assert_allclose(sample(t.grad.numpy()), z[key], rtol=2e-3, atol=2e-6 + 1e-4 * s, err_msg=k)
        n += 1
    assert n >= 8


def test_state_keys_and_module_surface():
    from recguru_amd import blocks
    from recguru_amd.config import get_param
    from recguru_amd.models import MyAuto4Rec_c, MyRec
    z, cfg, man, st, bt = load(CASES[0])
    param = get_param(case_args(z), make_dirs=False)
    assert param.pos_train is False
    a = case_args(z)
    a.pos_train = True
    assert get_param(a, make_dirs=False).pos_train is True
    R = MyRec("cpu", param, None, pos_train=True)
    assert isinstance(R.AutoEnc.pos_emb, blocks.PositionalEncodingM)
    assert list(R.state_dict().keys()) == [k for k, _ in man]
    assert tuple(R.state_dict()[POS_KEY].shape) == (param.enc_maxlen, param.d_model)
    assert R.AutoEnc.pos_emb.table() is R.AutoEnc.pos_emb.pos_emb.weight and R.AutoEnc.pos_emb.table().requires_grad
    R.load_state_dict(st, strict=True)
    R.train()
    R.AutoEnc.pos_emb.dropout_rate = 0.25
    assert R.AutoEnc.pos_emb.drop_p() == 0.25
    R.eval()
    assert R.AutoEnc.pos_emb.drop_p() == 0.0
    # default initialisation in the reference's construction position: the same draws as nn.Embedding + nn.Embedding under one seed
    torch.manual_seed(5)
    R2 = MyRec("cpu", param, None, pos_train=True)
    torch.manual_seed(5)
    e = torch.nn.Embedding(param.vocab_size + 1, param.d_model, padding_idx=0)
    pe = torch.nn.Embedding(param.enc_maxlen, param.d_model)
    assert torch.equal(R2.AutoEnc.src_emb.weight, e.weight) and torch.equal(R2.AutoEnc.pos_emb.pos_emb.weight, pe.weight)
    # the fixed path is unchanged
    F = MyRec("cpu", param, None, pos_train=False)
    keys = list(F.state_dict().keys())
    assert PE_KEY in keys and POS_KEY not in keys and isinstance(F.AutoEnc.pos_emb, blocks.PositionalEncoding)
    assert [k for k in keys if k != PE_KEY] == [k for k, _ in man if k != POS_KEY]
    assert not F.AutoEnc.pos_emb.table().requires_grad
    # the cross model's extension, off by default
    Gd = MyAuto4Rec_c("cpu", param)
    assert "pos_emb_a.pe" in Gd.state_dict() and "pos_emb_a.pos_emb.weight" not in Gd.state_dict()
    G = MyAuto4Rec_c("cpu", param, pos_train=True)
    sd = G.state_dict()
    for dom in "ab":
        assert tuple(sd["pos_emb_%s.pos_emb.weight" % dom].shape) == (param.enc_maxlen, param.d_model)
        assert "pos_emb_%s.pe" % dom not in sd
    # sas=True stays refused
    with pytest.raises(NotImplementedError):
        MyRec("cpu", param, None, sas=True, pos_train=True)
    # a batch longer than the table is refused before anything is launched
    ids = torch.ones(2, param.enc_maxlen + 1, dtype=torch.long)
    with pytest.raises(ValueError):
        R.AutoEnc._embed(ids, torch.ones(2, param.enc_maxlen + 1))
    with pytest.raises(ValueError):
        G._embed(ids, "a", torch.ones(2, param.enc_maxlen + 1))


def test_drivers_take_pos_train(monkeypatch):
    import sys
    import train_auto
    import train_gan
    for mod in (train_auto, train_gan):
        monkeypatch.setattr(sys, "argv", [mod.__name__ + ".py"])
        assert mod.parse().pos_train is False
        monkeypatch.setattr(sys, "argv", [mod.__name__ + ".py", "--pos_train", "True"])
        assert mod.parse().pos_train is True
        monkeypatch.setattr(sys, "argv", [mod.__name__ + ".py", "--pos_train", "False"])
        assert mod.parse().pos_train is False


@pytest.mark.parametrize("p,seed", [(0.0, 0), (0.5, 0xF00DFACE12345678), (0.1, 0x8000000000000001)])
def test_restatement_agrees_with_autograd(p, seed):
    """pos_grad_ref against torch autograd through keep * (E[ids] + P[:L]) * mask, in float64, built from the same keep array."""
    rng = np.random.default_rng(3)
    B, L, d, V, rows = 5, 7, 16, 11, 9
    ids = torch.as_tensor(rng.integers(0, V, size=(B, L)))
    mask = (rng.random((B, L)) < 0.6).astype(np.float64)
    mask[1] = 0.0                                                 # an all-padding sequence
    mask[:, 3] = 0.0                                              # a position that is padding everywhere
    keep = pos_grad_ref.keep_array(seed, p, B, L, d)
    if p:
        assert 0 < (keep == 0).mean() < 1 and set(np.unique(keep)) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}
    E = torch.as_tensor(rng.standard_normal((V, d)))
    P = torch.as_tensor(rng.standard_normal((rows, d))).requires_grad_(True)
    x = torch.as_tensor(keep) * (E[ids] + P[:L].unsqueeze(0)) * torch.as_tensor(mask).unsqueeze(2)
    dx = rng.standard_normal((B, L, d))
    (g,) = torch.autograd.grad(x, P, torch.as_tensor(dx))
    prior = rng.standard_normal((rows, d))
    dxn = dx.copy()
    dxn[mask == 0] = np.nan                                       # a masked position's dx row is never used
    got, abs_sum = pos_grad_ref.pos_grad(dxn, mask, prior, p, seed)
    np.testing.assert_allclose(got - prior, g.numpy(), rtol=1e-12, atol=1e-12)
    assert np.array_equal(got[L:], prior[L:]) and np.array_equal(got[3], prior[3])
    assert (abs_sum >= np.abs(got[:L] - prior[:L]) - 1e-12).all()
