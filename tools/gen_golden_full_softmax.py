"""Golden vectors of the full-catalogue softmax reconstruction loss (decoder_neg=False), by importing the reference (build
container only; the reference never travels, only these vectors do).

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_full_softmax.py
Writes tests/golden/full_case{1,2}.npz.  Weights come from a seed (tests/golden_util.make_state); big arrays are sampled.

Per case: the cross-domain generator MyAuto4Rec_c(decoder_neg=False) on a batch of domain a and of domain b, and the
single-domain MyRec(recon=True) on the batch of domain a -- the reference's own full logits, its SampledCrossEntropyLoss with
the 1-D label dec_out and the domain's class count (quirk Q15: the reference passes a [n, 1] label, which nn.CrossEntropyLoss
refuses), the gradient of every parameter (src_emb row 0 and projection_{a|b}.weight included) and the state_dict manifests.
Modules in eval() mode: dropout is the identity.
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
import AutoEnc4Rec_cross as cross_m        # noqa: E402
import gan_training as gt                  # noqa: E402
import tools.lossfunctions as lf           # noqa: E402
from data.data_loader import seq_padding   # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
from golden_util import make_state, manifest_to_arrays, sample  # noqa: E402


def make_param(d_model, n_head, n_negs, L, V_a, V_b, n_blocks, batch):
    args = argparse.Namespace(date="golden", d_model=d_model, n_head=n_head, d_ff=512, n_negs=n_negs,
                              decoder_neg=False, fix_enc=True, lr=0.01, batch_size=batch, batch_size_val=4,
                              dataset_pick=1, run=1, target_domain="a", cross="True", sas="False",
                              result_path=tempfile.mkdtemp(prefix="rg_golden_"))
    p = param_c.get_param(args)
    p.decoder_neg = False
    p.enc_maxlen = p.rec_maxlen = L
    p.vocab_size_a, p.vocab_size_b, p.vocab_size = V_a + 1, V_b + 1, V_a + 1
    p.dropout_rate = 0.0
    p.num_blocks = n_blocks
    return p


def make_batch(rng, L, V, lengths):
    enc, dec_i, dec_o = [], [], []
    for n in lengths:
        e, di, do = seq_padding(rng.integers(1, V + 1, size=n).tolist(), L, L, V + 1)
        enc.append(e)
        dec_i.append(di)
        dec_o.append(do)
    t = lambda a: torch.as_tensor(np.stack(a), dtype=torch.long)
    return t(enc), t(dec_i), t(dec_o)


def seed_weights(module, tag, seed, out):
    manifest = [(k, tuple(v.shape)) for k, v in module.state_dict().items()]
    st = make_state(manifest, seed)
    sd = module.state_dict()
    for k, v in st.items():
        sd[k] = torch.as_tensor(v)
    module.load_state_dict(sd)
    out[tag + ".keys"], out[tag + ".shapes"], out[tag + ".ndim"] = manifest_to_arrays(manifest)
    out[tag + ".seed"] = np.array(seed, dtype=np.int64)


def grads(prefix, module, out):
    for k, v in module.named_parameters():
        if v.grad is not None:
            out[prefix + k] = sample(v.grad.detach().numpy().copy())


def run_case(name, B, L, d, H, N, V_a, V_b, lengths_a, lengths_b, seed):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    k = 4                                             # n_negs: unused by the full path
    param = make_param(d, H, k, L, V_a, V_b, N, B)
    out = {"meta": np.array([B, L, d, H, N, V_a, V_b, k], dtype=np.int64)}
    ce = lf.SampledCrossEntropyLoss()

    # cross domain: logits = projection_{a|b}(dec_out), V_{a|b} + 1 classes
    G = cross_m.MyAuto4Rec_c("cpu", param, wf=None, enc_share=True, dec_rec=False).to(torch.float32)
    G.eval()
    seed_weights(G, "G", seed * 1000 + 1, out)
    for dom, V, lengths in (("a", V_a, lengths_a), ("b", V_b, lengths_b)):
        enc, di, do = make_batch(rng, L, V, lengths)
        for nm, t in zip(("enc_in", "dec_in", "dec_out"), (enc, di, do)):
            out["%s.%s" % (nm, dom)] = t.numpy()
        mask = gt.get_pad_mask(do, param.pad_index, "cpu")
        G.zero_grad()
        logits = G(enc, di, do, None, dom, mask)
        C = V + 1
        assert logits.shape == (B, L, C)
        loss = ce(logits, do.view(-1), C, mask=mask)
        loss.backward()
        out["logits.%s" % dom] = logits.detach().numpy()
        out["mask.%s" % dom] = mask.numpy()
        out["loss.%s" % dom] = loss.detach().numpy()
        grads("gradG.%s." % dom, G, out)

    # single domain: MyRec(recon=True) logits = h @ src_emb.weight.T over all V + 2 rows; mask (dec_in != pad), train_auto.py:109-110
    R = single_m.MyRec("cpu", param, None, dec_rec=False, fix_enc=False, sas=False, pos_train=False).to(torch.float32)
    R.eval()
    seed_weights(R, "R", seed * 1000 + 3, out)
    enc, di, do = (torch.as_tensor(out["%s.a" % nm]) for nm in ("enc_in", "dec_in", "dec_out"))
    mask = (di != param.pad_index).view(-1).to(torch.float32)
    R.zero_grad()
    logits = R(enc, di, do, None, recon=True)
    C = param.vocab_size + 1
    assert logits.shape == (B, L, C)
    loss = ce(logits, do.view(-1), C, mask=mask)
    loss.backward()
    out["logits.s"] = logits.detach().numpy()
    out["mask.s"] = mask.numpy()
    out["loss.s"] = loss.detach().numpy()
    grads("gradR.", R, out)
    out["gradR_src_emb_row0"] = R.AutoEnc.src_emb.weight.grad[0].detach().numpy().copy()
    np.savez_compressed(os.path.join(HERE, "..", "tests", "golden", "full_%s.npz" % name), **out)
    print(name, float(out["loss.a"]), float(out["loss.b"]), float(out["loss.s"]))


if __name__ == "__main__":
    # case1 like golden case1: d = 64, ragged lengths, one sequence truncated (longer than L)
    run_case("case1", B=4, L=12, d=64, H=2, N=1, V_a=50, V_b=40, lengths_a=[3, 7, 12, 19], lengths_b=[5, 2, 14, 9], seed=7)
    # case2: d = 128, V_a != V_b, class counts 98 / 61 / 99 (no multiple of 16 or 32)
    run_case("case2", B=4, L=16, d=128, H=4, N=2, V_a=97, V_b=60, lengths_a=[16, 4, 25, 9], lengths_b=[11, 3, 16, 30], seed=11)
