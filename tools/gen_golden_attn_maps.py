"""Golden attention maps of the single-domain model, by importing the reference (build container only; the reference never
travels, only these vectors do).

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_attn_maps.py
Writes tests/golden/attn_maps_case{1,2}.npz.  Weights come from a seed (tests/golden_util.make_state); only the manifest, the
seed, the integer inputs and the outputs are stored.

Per case: MyRec("cpu", p, None, dec_rec=False, fix_enc=False, sas=False, pos_train=False) in eval() with dropout 0 --
  enc_self             AutoEnc.get_seq_embed(enc_in)[1]
  dec_self, dec_enc    AutoEnc.get_dec_out(enc_in, dec_in)[1:]
  rec_self, rec_enc    the `recommend` stack called the way get_embedding calls it (which drops its maps)
  h_enc, h_dec, h_rec  the three hidden outputs
each map [B, n_layers, H, L, L] float32.  Users of lengths (20, 13, 7, 2, 1, 20): the length-1 user's decoder input is all
padding (every row uniform 1 / L), the length-13 / 7 / 2 users are left-padded (uniform padded-prefix rows under the causal mask, a
one-hot first live row, exact zeros at masked keys).
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference/GURU"
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

import AutoEnc4Rec as single_m             # noqa: E402
import Transformer.transformer as tr      # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
from gen_golden_pos_train import make_batch, make_param   # noqa: E402
from golden_util import make_state, manifest_to_arrays     # noqa: E402


def recommend_maps(R, enc_in, dec_in):
    """R.recommend over the encoder's last state with get_embedding's masks, keeping the maps get_embedding discards."""
    p = R.param
    enc_out, _ = R.AutoEnc.get_seq_embed(enc_in)
    enc_rep = enc_out[:, -1:, :].repeat(1, p.enc_maxlen, 1)
    mask = (dec_in != p.pad_index).to(torch.float32)
    x = R.AutoEnc.pos_emb(R.AutoEnc.src_emb(dec_in), mask)
    self_mask = torch.gt(tr.get_attn_pad_mask(dec_in, dec_in, p.pad_index) + tr.get_attn_subsequent_mask(dec_in), 0)
    cross_mask = tr.get_attn_pad_mask(dec_in, enc_in, p.pad_index)
    return R.recommend(x, enc_in, enc_rep, self_mask, cross_mask, mask)


def run_case(name, d, H, N, seed, B=6, L=20, V=50, k=5, lengths=(20, 13, 7, 2, 1, 20)):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    param = make_param(d, H, k, L, V, N, B)
    out = {"meta": np.array([B, L, d, H, N, V, V, k, param.n_bpr_neg], dtype=np.int64)}
    R = single_m.MyRec("cpu", param, None, dec_rec=False, fix_enc=False, sas=False, pos_train=False).to(torch.float32)
    R.eval()
    manifest = [(kk, tuple(v.shape)) for kk, v in R.state_dict().items()]
    st = make_state(manifest, seed * 1000 + 7)
    res = R.load_state_dict({kk: torch.as_tensor(v) for kk, v in st.items()}, strict=False)
    assert all(kk.endswith(".pe") for kk in res.missing_keys) and not res.unexpected_keys       # (the fixed 'pe' buffer keeps its values)
    out["R.keys"], out["R.shapes"], out["R.ndim"] = manifest_to_arrays(manifest)
    out["R.seed"] = np.array(seed * 1000 + 7, dtype=np.int64)
    enc, di, do, negs = make_batch(rng, L, V, k, lengths)
    for nm, t in zip(("enc_in", "dec_in", "dec_out", "n_items"), (enc, di, do, negs)):
        out[nm] = t.numpy()
    assert int((di[4] != 0).sum()) == 0                     # the length-1 user's decoder is all padding
    with torch.no_grad():
        h_enc, enc_self = R.AutoEnc.get_seq_embed(enc)
        h_dec, dec_self, dec_enc = R.AutoEnc.get_dec_out(enc, di)
        h_rec, rec_self, rec_enc = recommend_maps(R, enc, di)
        assert torch.equal(h_rec, R.get_embedding(enc, di))
    for nm, t in (("enc_self", enc_self), ("dec_self", dec_self), ("dec_enc", dec_enc), ("rec_self", rec_self), ("rec_enc", rec_enc),
                  ("h_enc", h_enc), ("h_dec", h_dec), ("h_rec", h_rec)):
        out[nm] = t.numpy().astype(np.float32)
    for nm in ("enc_self", "dec_self", "dec_enc", "rec_self", "rec_enc"):
        assert out[nm].shape == (B, N, H, L, L), (nm, out[nm].shape)
    path = os.path.join(HERE, "..", "tests", "golden", "attn_maps_%s.npz" % name)
    np.savez_compressed(path, **out)
    print(name, "row-sum error %.3g" % float(np.abs(out["enc_self"].sum(-1) - 1).max()), "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    run_case("case1", d=128, H=4, N=1, seed=41)          # d = 128, one block: the fused layer path
    run_case("case2", d=64, H=2, N=2, seed=43)           # d = 64, two blocks: the unfused path
