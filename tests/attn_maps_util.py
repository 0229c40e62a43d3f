"""Helpers shared by the attention-map tests: the fixtures of tools/gen_golden_attn_maps.py as model state and as the parameter dict
of the CPU oracle, and the float64 maps that tests/attn_map_ref.py gives on the oracle's layer inputs (its collect= taps)."""
import math

import numpy as np
import torch

import attn_map_ref as R
from oracle import recguru_oracle as O
from pos_train_util import load

CASES = ["attn_maps_case1", "attn_maps_case2"]
PE_KEY = "AutoEnc.pos_emb.pe"
SCALE = 1.0 / math.sqrt(32.0)
_CACHE = {}


def load_case(name):
    """(fixture, oracle Cfg, model state, batch (enc_in, dec_in, dec_out, n_items)), loaded once."""
    if name not in _CACHE:
        z, cfg, man, st, bt = load(name)
        _CACHE[name] = (z, cfg, st, bt)
    return _CACHE[name]


def oracle_params(st, d, pe_keys=(PE_KEY,), dtype=torch.float64):
    st = dict(st)
    for k in pe_keys:
        st[k] = O.positional_table(5000, d).unsqueeze(0)
    return {k: v.detach().to(dtype) for k, v in st.items()}


def layer_map(p, pre, x, key_ids, pad_value, causal, H):
    """attn_map_ref.probs on the float64 projection of the layer input x [B, L, d] with the weights p[pre + 'WQ' / 'WK']"""
    x = x.detach().double().numpy()
    B, L, _ = x.shape

    def proj(nm):
        w, b = p[pre + nm + ".weight"].double().numpy(), p[pre + nm + ".bias"].double().numpy()
        return (x @ w.T + b).reshape(B, L, H, 32).transpose(0, 2, 1, 3)
    return R.probs(proj("WQ"), proj("WK"), key_ids.numpy(), pad_value, causal, SCALE)


def stack_maps(p, pre, attn, inputs, key_ids, pad_value, causal, H):
    """[B, N, H, L, L] float64: layer l's map from inputs[l]"""
    return np.stack([layer_map(p, "%slayers.%d.%s." % (pre, l, attn), x, key_ids, pad_value, causal, H) for l, x in enumerate(inputs)], 1)


def single_ref_maps(name):
    """The float64 restatement of the fixture's three self maps: {'enc_self', 'dec_self', 'rec_self'}"""
    key = ("ref", name)
    if key not in _CACHE:
        z, cfg, st, bt = load_case(name)
        enc_in, dec_in = bt[0], bt[1]
        B, L = enc_in.shape
        p = oracle_params(st, cfg.d_model)
        H, N = cfg.n_heads, cfg.n_layers
        with torch.no_grad():
            taps = []
            enc_out = O.single_get_seq_embed(p, cfg, enc_in, "AutoEnc.", collect=taps)
            out = {"enc_self": stack_maps(p, "AutoEnc.encoder.", "enc_self_attn", taps[:N], enc_in, 0, False, H)}
            mask = O.nonpad(dec_in, cfg.pad_index).double()
            x0 = O.embed_pe(p["AutoEnc.src_emb.weight"], p[PE_KEY][0], dec_in, mask)
            self_masked = O.pad_key_mask(dec_in, cfg.pad_index, L) | O.causal_mask(B, L)
            cross_masked = O.pad_key_mask(enc_in, cfg.pad_index, L)
            rep = enc_out[:, -1, :].unsqueeze(1).repeat(1, L, 1)
            for tag, pre in (("dec_self", "AutoEnc.decoder."), ("rec_self", "recommend.")):
                taps = []
                O.decoder_m(p, pre, x0, rep, self_masked, cross_masked, mask, N, H, cfg.d_k, False, collect=taps)
                out[tag] = stack_maps(p, pre, "dec_self_attn", [x0] + taps[:N - 1], dec_in, 0, True, H)
        _CACHE[key] = out
    return _CACHE[key]


def exact_sets(key_ids, pad_value, causal):
    """(zero [B, L, L]: masked keys of rows with a visible key; onehot [B, L, L]: the visible key of rows with exactly one;
    uniform [B, L]: rows without a visible key)"""
    vis = R.visible(key_ids, pad_value, causal)
    n = vis.sum(-1)
    return (~vis) & (n > 0)[:, :, None], vis & (n == 1)[:, :, None], n == 0


def check_exact(maps, key_ids, pad_value, causal, what=""):
    """the three exact properties on maps [B, H, L, L] or [B, N, H, L, L] float32"""
    maps = np.asarray(maps)
    assert maps.dtype == np.float32
    if maps.ndim == 4:
        maps = maps[:, None]
    L = maps.shape[-1]
    zero, onehot, uniform = exact_sets(np.asarray(key_ids), pad_value, causal)
    z = np.broadcast_to(zero[:, None, None], maps.shape)
    o = np.broadcast_to(onehot[:, None, None], maps.shape)
    u = np.broadcast_to(uniform[:, None, None, :, None], maps.shape)
    bits = maps.view(np.uint32)
    assert (bits[z] == 0).all(), "%s: a masked key of a row with a visible key is not +0.0" % what
    assert (maps[o] == np.float32(1.0)).all(), "%s: a one-key row is not exactly 1" % what
    assert (bits[u] == (np.float32(1) / np.float32(L)).view(np.uint32)).all(), "%s: a row without a visible key is not float32(1/L)" % what
    return int(z.sum()), int(o.sum()), int(u.sum())


def dyadic_maps(rng, B, N, H, L):
    """Row-stochastic maps whose rows are uniform over 1, 2, 4 or 8 keys (fewer where L is smaller): every rollout intermediate is a
    dyadic rational with few bits, exact in f32."""
    m = np.zeros((B, N, H, L, L), np.float32)
    sizes = [s for s in (1, 2, 4, 8) if s <= L]
    for idx in np.ndindex(B, N, H, L):
        s = sizes[rng.integers(len(sizes))]
        m[idx][rng.choice(L, size=s, replace=False)] = np.float32(1.0 / s)
    return m
