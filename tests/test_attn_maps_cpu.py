"""Host-side checks of the attention-map feature (return_attn, rg_attn_probs / rg_attn_cross_probs / rg_attn_rollout): the float64
restatement tests/attn_map_ref.py against the reference's own maps (tests/golden/attn_maps_case*.npz, tools/gen_golden_attn_maps.py),
the rollout restatement on fixtures with known answers, and the Python surface -- defaults and refusals that need no device."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import attn_map_ref as R
from attn_maps_util import CASES, check_exact, dyadic_maps, load_case, single_ref_maps
from parity_util import make_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the restatement is the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference_maps(name):
    z, cfg, st, bt = load_case(name)
    enc_in, dec_in = bt[0].numpy(), bt[1].numpy()
    ref = single_ref_maps(name)
    n_exact = np.zeros(3, np.int64)
    for tag, ids, causal in (("enc_self", enc_in, False), ("dec_self", dec_in, True), ("rec_self", dec_in, True)):
        gold = z[tag]
        assert gold.dtype == np.float32 and gold.shape == ref[tag].shape
        # both sides are the same f32 arithmetic restated; the reference's own row sums are off by up to 2.4e-7
        np.testing.assert_allclose(ref[tag], gold, rtol=1e-5, atol=1e-7, err_msg=tag)
        n_exact += check_exact(gold, ids, 0, causal, tag)
        # ... and the restatement has the same exact entries
        r32 = ref[tag].astype(np.float32)
        n_exact += check_exact(r32, ids, 0, causal, tag + " (restatement)")
    assert (n_exact > 0).all()          # the fixtures carry zero, one-hot and uniform rows


@pytest.mark.parametrize("name", CASES)
def test_cross_maps_closed_form_is_the_reference(name):
    z, cfg, st, bt = load_case(name)
    B, N, H, L, _ = z["dec_enc"].shape
    want = R.cross_probs(bt[0].numpy(), 0, L, H)
    for tag in ("dec_enc", "rec_enc"):
        for l in range(N):
            assert np.array_equal(z[tag][:, l].view(np.uint32), want.view(np.uint32)), (tag, l)
    assert np.array_equal(R.cross_probs(np.zeros((2, 5), np.int64), 0, 5, 3), np.full((2, 3, 5, 5), np.float32(1) / np.float32(5)))


# ---- 2. the rollout restatement ---------------------------------------------------------------------------------------------
def test_rollout_restatement():
    rng = np.random.default_rng(3)
    B, N, H, L = 3, 3, 2, 9
    maps = rng.random((B, N, H, L, L))
    maps /= maps.sum(-1, keepdims=True)
    out = R.rollout(maps, None, 0.5)
    assert np.abs(out.sum(-1) - 1).max() <= N * L * 2.0 ** -52
    eye = np.broadcast_to(np.eye(L), (B, N, H, L, L))
    q = np.array([0, 4, 8])
    assert np.array_equal(R.rollout(eye, q, 0.3), np.eye(L)[q])
    assert np.array_equal(R.rollout(maps, np.full(B, L - 1), 0.5), out)
    # one layer, by hand: r = alpha e_q + (1 - alpha) mean_h maps[b, 0, h, q]
    one = R.rollout(maps[:, :1], q, 0.25)
    for b in range(B):
        want = 0.25 * np.eye(L)[q[b]] + 0.75 * maps[b, 0, :, q[b]].mean(0)
        np.testing.assert_allclose(one[b], want, rtol=0, atol=1e-15)
    # dyadic fixtures: float32 arithmetic in ANY order gives the float64 answer
    for Hd in (1, 2, 4):
        dm = dyadic_maps(rng, 2, 3, Hd, 16)
        o64 = R.rollout(dm, None, 0.5)
        assert np.array_equal(o64.astype(np.float32).astype(np.float64), o64) and np.abs(o64.sum(-1) - 1).max() == 0


# ---- 3. the host surface ----------------------------------------------------------------------------------------------------
def test_return_attn_defaults_to_false_everywhere():
    from recguru_amd import auto_training, blocks, hip, models, training
    for fn in (models.MyAuto4Rec.get_seq_embed, models.MyAuto4Rec.get_dec_out, models.MyAuto4Rec.decode_with, models.MyRec.get_embedding,
               models.MyAuto4Rec_c.get_seq_embed, models.MyAuto4Rec_c.get_dec_out, models.MyAuto4Rec_c.recommend_forward,
               blocks.EncoderM.forward, blocks.DecoderM.forward):
        assert inspect.signature(fn).parameters["return_attn"].default is False, fn
    assert inspect.signature(blocks.EncoderM.forward).parameters["last_only"].default is False
    assert [k for k in inspect.signature(hip.attn_probs).parameters][:7] == ["qkv", "key_ids", "pad_value", "H", "causal", "out", "layer"]
    assert [k for k in inspect.signature(hip.attn_cross_probs).parameters][:5] == ["enc_ids", "pad_value", "H", "out", "layer"]
    sig = inspect.signature(hip.attn_rollout).parameters
    assert [k for k in sig][:3] == ["maps", "query", "alpha"] and sig["query"].default is None and sig["alpha"].default == 0.5
    assert inspect.signature(training.explain).parameters["alpha"].default == 0.5
    assert inspect.signature(training.explain).parameters["domain"].default == "a"
    assert inspect.signature(auto_training.explain).parameters["alpha"].default == 0.5


def test_abi_surface():
    from recguru_amd import hip
    hdr = open(os.path.join(ROOT, "include", "recguru_hip.h")).read()
    for name in ("rg_attn_probs", "rg_attn_cross_probs", "rg_attn_rollout"):
        assert name in hip.SYMBOLS and re.search(r"\bint %s\(" % name, hdr), name
    body = re.search(r"typedef struct \{([^}]*)\} rg_attn_probs_args;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)\s*[;,]", body)
    assert names == [n for n, _ in hip.AttnProbsArgs._fields_], names
    src = open(os.path.join(ROOT, "recguru_amd", "csrc", "attention_map.hip")).read()
    assert "rg_det.hip.h" not in src and "atomic" not in src.replace("no atomics", "")
    for name in ("attn_probs", "attn_cross_probs", "attn_rollout"):
        assert name in hip._PLAIN


def _models(dropout):
    from recguru_amd.config import get_param
    from recguru_amd.models import MyAuto4Rec_c, MyRec
    param = get_param(make_args(64, 2, 5, 20, 51, 51, 2, 4, dropout=dropout), make_dirs=False)
    return param, MyRec("cpu", param, None), MyAuto4Rec_c("cpu", param, wf=None, enc_share=True, dec_rec=False)


def test_training_mode_with_dropout_refuses_maps_before_any_device_work():
    param, R_, G = _models(0.5)
    assert param.dropout_rate == 0.5 and R_.training and G.training
    ids = torch.ones(2, 20, dtype=torch.long)                  # CPU tensors: any launch would raise RuntimeError, not ValueError
    mask = torch.ones(2, 20)
    calls = [lambda: R_.AutoEnc.get_seq_embed(ids, return_attn=True), lambda: R_.AutoEnc.get_dec_out(ids, ids, return_attn=True),
             lambda: R_.AutoEnc.decode_with(R_.recommend, ids, ids, return_attn=True), lambda: R_.get_embedding(ids, ids, return_attn=True),
             lambda: G.get_seq_embed(ids, "a", mask, return_attn=True), lambda: G.get_dec_out(ids, ids, "a", mask, return_attn=True),
             lambda: G.recommend_forward(ids, ids, "a", mask, return_attn=True)]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError, match="return_attn"):
            call()
    # the stacks refuse on their own too
    x = torch.zeros(2, 20, 64)
    with pytest.raises(ValueError, match="return_attn"):
        G.encoder(x, ids, 51, mask, return_attn=True)
    with pytest.raises(ValueError, match="return_attn"):
        R_.recommend(x, x[:, -1], ids, ids, mask, return_attn=True)
    # eval(), or a rate of 0, passes the check and dies at the first launch instead: there is no CPU path
    R_.eval()
    with pytest.raises(RuntimeError):
        R_.get_embedding(ids, ids, return_attn=True)
    param0, R0, G0 = _models(0.0)
    with pytest.raises(RuntimeError):
        G0.get_seq_embed(ids, "a", mask, return_attn=True)
    # a batch longer than the positional table keeps its ValueError
    from recguru_amd.models import MyRec
    from recguru_amd.config import get_param
    p2 = get_param(make_args(64, 2, 5, 20, 51, 51, 1, 4, pos_train=True), make_dirs=False)
    R2 = MyRec("cpu", p2, None, pos_train=True).eval()
    long_ids = torch.ones(2, 21, dtype=torch.long)
    with pytest.raises(ValueError, match="positional table"):
        R2.get_embedding(long_ids, long_ids, return_attn=True)
