"""The model stacks at sequence lengths past the resident attention kernels' limit (L > 416): the streaming attention core
(csrc/attention_long.hip) at L = 448 and, at L = 600, the looped single-query kernels of the last encoder layer, against the
CPU oracle -- user embeddings, the reconstruction loss and four gradient tensors (first and last encoder layer, one decoder
layer, the item table), after tests/test_config5_gpu.py::test_config5_vs_oracle and at its tolerances.  Then the full-catalogue
recommendation against a dense product of the oracle's state, exact zeros on padded rows, and the whole model at L = 2048.
"""
import numpy as np
import pytest
import torch

from parity_util import make_args, max_err

pytestmark = pytest.mark.gpu
SHAPE = dict(d=128, H=4, N=2, k=30, V=2000, B=4)
GRAD_KEYS = ("encoder.layers.0.enc_self_attn.WQ.weight", "encoder.layers.1.pos_ffn.layer_norm.weight",
             "decoder_a.layers.1.dec_self_attn.WV.weight", "src_emb_a.weight")


@pytest.fixture(autouse=True)
def _restore_tier():
    from recguru_amd import ops
    yield
    ops.set_compute_dtype(torch.bfloat16)


def _setup(L, device, seed=7, dropout=0.0, N=None, B=None, d=None, H=None):
    from recguru_amd import config, models, synthetic
    c = SHAPE
    B = B or c["B"]
    param = config.get_param(make_args(d or c["d"], H or c["H"], c["k"], L, c["V"], c["V"], N or c["N"], B, dropout=dropout), make_dirs=False)
    torch.manual_seed(seed)
    G = models.MyAuto4Rec_c(device, param, wf=None, enc_share=True, dec_rec=False).to(torch.float32)
    with torch.no_grad():                                   # N(0, 1) tables make |logit| ~ 11: scale them like a trained model's
        G.src_emb_a.weight.mul_(0.25)
        G.src_emb_b.weight.mul_(0.25)
    dom = synthetic.make_domain(B, c["V"], L, c["k"], seed=seed)
    bt = tuple(torch.as_tensor(dom[n]) for n in ("enc_in", "dec_in", "dec_out", "n_items"))
    return param, G, bt


_ORACLE = {}


def _oracle(L):
    """User embeddings, reconstruction loss, its gradients and the recommender state from the CPU oracle (cached: the tiers share it)."""
    if L in _ORACLE:
        return _ORACLE[L]
    from oracle import recguru_oracle as O
    c = SHAPE
    param, G, bt = _setup(L, "cpu")
    sd = {k: v.detach().clone() for k, v in G.state_dict().items()}
    cfg = O.Cfg(c["d"], c["H"], c["N"], L, c["k"], c["V"] + 1, c["V"] + 1)
    p = {k: v.clone().requires_grad_(k in GRAD_KEYS) for k, v in sd.items()}
    with torch.no_grad():
        ue_ref = O.get_user_embed(sd, cfg, bt[0], "a").numpy()
        h_rec = O.cross_get_dec_out(sd, cfg, bt[0], bt[1], "a", O.nonpad(bt[1], 0), True, dec_prefix="recommend_a.",
                                    d_mask_from="dec", detach_enc=True)[:, -1, :]
    la = O.loss_ae_cross(p, cfg, *bt, domain="a", collapsed=True)
    la.backward()
    _ORACLE[L] = dict(ue=ue_ref, la=float(la.detach()), grads={k: p[k].grad.numpy().copy() for k in GRAD_KEYS}, sd=sd, bt=bt, param=param,
                      h_rec=h_rec)
    return _ORACLE[L]


def _gpu_model(ref):
    from recguru_amd import models
    G = models.MyAuto4Rec_c("cuda", ref["param"], wf=None, enc_share=True, dec_rec=False).to(torch.float32)
    G.load_state_dict(ref["sd"])
    return G.cuda()


def _errors(tier, L):
    from recguru_amd import ops, training as T
    ref = _oracle(L)
    ops.set_compute_dtype(tier)
    G = _gpu_model(ref)
    cb = tuple(t.cuda() for t in ref["bt"])
    with torch.no_grad():
        ue = T.get_user_embed(G, cb[0], "a", ref["param"], "cuda", 0).float().cpu().numpy()
    mask = T.get_pad_mask(cb[2], 0, "cuda")
    la = T.loss_ae(G, *cb, True, SHAPE["B"], L, ref["param"], mask, "cuda", domain="a")
    la.backward()
    ue_err, l_rel = max_err(ue, ref["ue"])[1], abs(float(la.detach()) - ref["la"]) / ref["la"]
    params = dict(G.named_parameters())
    gerr = {}
    for k in GRAD_KEYS:
        g, r = params[k].grad.float().cpu().numpy(), ref["grads"][k]
        assert np.isfinite(g).all(), k
        gerr[k] = float(np.abs(g - r).max() / max(np.abs(r).max(), 1e-30))
    return ue, ue_err, l_rel, gerr


def _assert_vs_oracle(tier, L, capsys):
    ue, ue_err, l_rel, gerr = _errors(tier, L)
    ref = _oracle(L)
    with capsys.disabled():
        print("\n[L = %d, %s tier] user_embed err rel-to-max %.3g | loss_ae rel %.3g | gradient err / max: %s"
              % (L, tier, ue_err, l_rel, ", ".join("%s %.2g" % (".".join(k.split(".")[-3:-1]) or k, v) for k, v in gerr.items())))
    if tier in ("f32", "bf16x3"):                          # the north-star tolerance, as test_config5_vs_oracle asserts it
        np.testing.assert_allclose(ue, ref["ue"], rtol=1e-3, atol=1e-5)
        assert l_rel <= 1e-5
        assert max(gerr.values()) <= 1e-3
    else:                                                  # the bf16 bounds of test_config5_vs_oracle
        assert ue_err <= 0.02 and l_rel <= 3e-4
        assert max(gerr.values()) <= 0.025


@pytest.mark.parametrize("tier", ["f32", "bf16x3", "bf16"])
def test_long_sequence_vs_oracle(tier, capsys):
    """L = 448 (d = 128, H = 4, N = 2, k = 30, V = 2000, B = 4): every attention call of the encoder and the decoder runs the streaming
    form; the last encoder layer's single query still takes the straight-line kernels (L <= 512)."""
    _assert_vs_oracle(tier, 448, capsys)


def test_long_sequence_looped_single_query_vs_oracle(capsys):
    """L = 600, f32 tier: get_user_embed and loss_ae's backward go through the looped single-query kernels (L > 512)."""
    _assert_vs_oracle("f32", 600, capsys)


def test_recommend_matches_dense_scores_of_the_oracle_state():
    """training.recommend at L = 448 (f32 tier, K = 10, nothing excluded): for each user the ids of the ten highest entries of
    h @ table.T over the catalogue rows, h the oracle's last recommender-decoder state; get_seq_embed is exactly zero on padded rows."""
    from recguru_amd import ops, training as T
    L, K = 448, 10
    ref = _oracle(L)
    ops.set_compute_dtype("f32")
    G = _gpu_model(ref).eval()
    cb = tuple(t.cuda() for t in ref["bt"])
    ids, _ = T.recommend(G, cb[0], cb[1], K, ref["param"], domain="a", device="cuda", exclude_seen=False)
    V = SHAPE["V"]
    dense = ref["h_rec"].double() @ ref["sd"]["src_emb_a.weight"][1:V + 1].double().T          # catalogue ids 1 .. V
    want = torch.topk(dense, K, dim=1).indices + 1
    assert ids.shape == (SHAPE["B"], K)
    assert torch.equal(ids.cpu(), want), (ids.cpu(), want)
    with torch.no_grad():
        full = G.get_seq_embed(cb[0], "a", (cb[0] != 0).float())
    pad = cb[0] == 0
    assert pad.any() and float(full[pad].abs().max()) == 0.0
    assert float(full[~pad].abs().max()) > 0


def test_long_sequence_list_driven_batch():
    """B = 40 at L = 448 (17 920 rows: the padded-tile lists, the list-driven projections and the fused block are in use, the rows of
    dctx in padded tiles are unwritten): the bf16 tier's loss and gradients against the f32 tier's on the same weights and batch.  The
    f32 tier is within 1e-3 of the oracle and the bf16 tier within 0.025 / 3e-4 (test_long_sequence_vs_oracle), so the two are within
    their sum of each other."""
    from recguru_amd import ops, training as T
    L, B = 448, 40
    param, G0, bt = _setup(L, "cpu", seed=5, B=B)
    sd = {k: v.detach().clone() for k, v in G0.state_dict().items()}
    cb = tuple(t.cuda() for t in bt)
    out = {}
    for tier in ("f32", "bf16"):
        ops.set_compute_dtype(tier)
        G = _gpu_model(dict(param=param, sd=sd))
        mask = T.get_pad_mask(cb[2], 0, "cuda")
        la = T.loss_ae(G, *cb, True, B, L, param, mask, "cuda", domain="a")
        la.backward()
        params = dict(G.named_parameters())
        out[tier] = (float(la.detach()), {k: params[k].grad.float().clone() for k in GRAD_KEYS})
    assert abs(out["bf16"][0] - out["f32"][0]) / out["f32"][0] <= 3e-4 + 1e-5
    for k in GRAD_KEYS:
        g, r = out["bf16"][1][k], out["f32"][1][k]
        assert torch.isfinite(g).all() and float(r.abs().max()) > 0
        assert float((g - r).abs().max() / r.abs().max()) <= 0.025 + 1e-3, k


@pytest.mark.parametrize("d,H,L", [(128, 4, 2048), (256, 8, 1024)])
@pytest.mark.parametrize("tier", ["bf16", "f32"])
def test_whole_model_at_the_upper_edge(tier, d, H, L):
    """d = 128 / H = 4 at L = 2048 and d = 256 / H = 8 at L = 1024 (the bound rg_seq_wsum's LDS sets for the decoder's dropout
    path at that width), with dropout: a training step's loss and gradients are finite, the user embedding of the last-position
    path equals row L - 1 of the full encoder, recommend and evaluation_full run."""
    from recguru_amd import ops, synthetic, training as T
    B = 2
    ops.set_compute_dtype(tier)
    param, G, bt = _setup(L, "cuda", seed=3, dropout=0.2, N=1, B=B, d=d, H=H)
    G = G.cuda()
    cb = tuple(t.cuda() for t in bt)
    G.train()
    mask = T.get_pad_mask(cb[2], 0, "cuda")
    la = T.loss_ae(G, *cb, True, B, L, param, mask, "cuda", domain="a")
    la.backward()
    assert np.isfinite(float(la.detach()))
    for k_, p in G.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all(), k_
    assert float(G.encoder.layers[0].enc_self_attn.WQ.weight.grad.abs().max()) > 0
    G.eval()
    with torch.no_grad():
        full = G.get_seq_embed(cb[0], "a", (cb[0] != 0).float())
        ue = T.get_user_embed(G, cb[0], "a", param, "cuda", 0)
    s_ = float(full[:, -1, :].float().abs().max())
    assert float((ue.float() - full[:, -1, :].float()).abs().max()) <= (0.03 if tier == "bf16" else 1e-4) * s_
    ids, sc = T.recommend(G, cb[0], cb[1], 10, param, domain="a", device="cuda")
    assert ids.shape == (B, 10) and int(ids.min()) >= 1 and torch.isfinite(sc).all()
    dom = synthetic.make_domain(B, SHAPE["V"], L, SHAPE["k"], seed=3)
    t = {k: torch.as_tensor(v).cuda() for k, v in dom.items()}
    data = (t["enc_in"], t["dec_in"], t["val"])
    param.eval_steps = 1
    res = T.evaluation_full(G, [(data, (t["enc_in"], t["dec_in"], t["test"]), None, None)], "cuda", param, k_val=[10], domain="a")
    assert 0.0 <= res["10"]["ht_eval"][0] <= 1.0
