"""Golden vectors of the single-domain model with LEARNED positions (pos_train=True), by importing the reference (build container
only; the reference never travels, only these vectors do).

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_pos_train.py
Writes tests/golden/pos_train_case{1,2}.npz.  Weights come from a seed (tests/golden_util.make_state: the key
AutoEnc.pos_emb.pos_emb.weight takes its generic branch); only the manifest, the seed, the integer inputs and the outputs are stored.

Per case: MyRec("cpu", p, None, dec_rec=False, fix_enc=False, sas=False, pos_train=True) in eval() (dropout is the identity) --
the reconstruction loss (recon=True logits through the reference's SampledCrossEntropyLoss, mask dec_in != 0, train_auto.py:109-110),
the recon=False BPR loss, the user embedding enc_out[:, -1] and the gradient of the reconstruction loss for every parameter
(sampled; the position table's is stored whole).
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

REF = "/root/reference/GURU"
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

import config_auto4rec as param_c          # noqa: E402
import AutoEnc4Rec as single_m             # noqa: E402
import tools.lossfunctions as lf           # noqa: E402
from data.data_loader import seq_padding   # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
from golden_util import make_state, manifest_to_arrays, sample  # noqa: E402

POS_KEY = "AutoEnc.pos_emb.pos_emb.weight"


def make_param(d_model, n_head, n_negs, L, V, n_blocks, batch):
    args = argparse.Namespace(date="golden", d_model=d_model, n_head=n_head, d_ff=512, n_negs=n_negs,
                              decoder_neg=True, fix_enc=True, lr=0.01, batch_size=batch, batch_size_val=4,
                              dataset_pick=1, run=1, target_domain="a", cross="True", sas="False",
                              result_path=tempfile.mkdtemp(prefix="rg_golden_"))
    p = param_c.get_param(args)
    p.enc_maxlen = p.rec_maxlen = L
    p.vocab_size_a = p.vocab_size_b = p.vocab_size = V + 1
    p.dropout_rate = 0.0
    p.num_blocks = n_blocks
    return p


def make_batch(rng, L, V, k, lengths):
    enc, dec_i, dec_o, negs = [], [], [], []
    for n in lengths:
        e, di, do = seq_padding(rng.integers(1, V + 1, size=n).tolist(), L, L, V + 1)
        enc.append(e)
        dec_i.append(di)
        dec_o.append(do)
        negs.append(rng.integers(1, V + 1, size=L * k))
    t = lambda a: torch.as_tensor(np.stack(a), dtype=torch.long)
    return t(enc), t(dec_i), t(dec_o), t(negs)


def run_case(name, d, H, N, seed, B=6, L=20, V=50, k=5, lengths=(20, 13, 7, 2, 1, 20)):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    param = make_param(d, H, k, L, V, N, B)
    out = {"meta": np.array([B, L, d, H, N, V, V, k, param.n_bpr_neg], dtype=np.int64)}
    R = single_m.MyRec("cpu", param, None, dec_rec=False, fix_enc=False, sas=False, pos_train=True).to(torch.float32)
    R.eval()
    manifest = [(kk, tuple(v.shape)) for kk, v in R.state_dict().items()]
    assert (POS_KEY, (L, d)) in manifest and not any(kk.endswith(".pe") for kk, _ in manifest)
    st = make_state(manifest, seed * 1000 + 3)
    R.load_state_dict({kk: torch.as_tensor(v) for kk, v in st.items()}, strict=True)
    out["R.keys"], out["R.shapes"], out["R.ndim"] = manifest_to_arrays(manifest)
    out["R.seed"] = np.array(seed * 1000 + 3, dtype=np.int64)

    enc, di, do, negs = make_batch(rng, L, V, k, lengths)
    for nm, t in zip(("enc_in", "dec_in", "dec_out", "n_items"), (enc, di, do, negs)):
        out[nm] = t.numpy()
    assert int((di[4] != 0).sum()) == 0                     # the length-1 user's decoder is all padding
    m_in = (di != 0).view(-1).to(torch.float32)             # train_auto.py:109-110 (dec_in mask)
    logits = R(enc, di, do, negs, recon=True)
    loss = lf.SampledCrossEntropyLoss(reduction="none")(logits, torch.zeros(B * L).long(), k + 1, mask=m_in)
    out["loss_ae"] = loss.detach().numpy()
    R.zero_grad()
    loss.backward()
    for kk, v in R.named_parameters():
        if v.grad is not None:
            g = v.grad.detach().numpy().copy()
            out["gradR_recon." + kk] = g if kk == POS_KEY else sample(g)
    R.zero_grad()
    nb = torch.as_tensor(rng.integers(1, V + 1, size=(B, L * param.n_bpr_neg)), dtype=torch.long)
    out["n_items_bpr"] = nb.numpy()
    with torch.no_grad():
        p_l, n_l = R(enc, di, do, nb, recon=False)
        out["loss_bpr"] = lf.BPRLoss()(p_l, n_l, mask=m_in).numpy()
        out["user_embed"] = R.AutoEnc.get_seq_embed(enc)[0][:, -1, :].numpy()
    path = os.path.join(HERE, "..", "tests", "golden", "pos_train_%s.npz" % name)
    np.savez_compressed(path, **out)
    print(name, float(out["loss_ae"]), float(out["loss_bpr"]), "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    run_case("case1", d=128, H=4, N=1, seed=31)          # d = 128, one block: the fused layer path
    run_case("case2", d=64, H=2, N=2, seed=37)           # d = 64, two blocks: the unfused path
