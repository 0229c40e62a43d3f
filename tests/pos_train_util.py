"""Helpers of the learned-position tests: the pos_train fixtures (tools/gen_golden_pos_train.py) as model state and as the
parameter dict of the unchanged CPU oracle, which reads the positional table from '<prefix>pos_emb.pe' -- fed the learned weight
under that key, as a leaf, it restates the learned-position model and autograd gives the table's gradient."""
import torch

from golden_util import arrays_to_manifest, load_case, make_state
from oracle import recguru_oracle as O

CASES = ["pos_train_case1", "pos_train_case2"]
POS_KEY = "AutoEnc.pos_emb.pos_emb.weight"
PE_KEY = "AutoEnc.pos_emb.pe"


def load(name):
    """(fixture, oracle Cfg, manifest, model state {key: f32 tensor}, batch (enc_in, dec_in, dec_out, n_items))."""
    z = load_case(name)
    B, L, d, H, N, Va, Vb, k, nb = [int(x) for x in z["meta"]]
    cfg = O.Cfg(d, H, N, L, k, Va + 1, Vb + 1, n_bpr_neg=nb)
    man = arrays_to_manifest(z["R.keys"], z["R.shapes"], z["R.ndim"])
    st = {kk: torch.as_tensor(v) for kk, v in make_state(man, int(z["R.seed"])).items()}
    bt = tuple(torch.as_tensor(z[nm]) for nm in ("enc_in", "dec_in", "dec_out", "n_items"))
    return z, cfg, man, st, bt


def oracle_params(st, pos_keys=((POS_KEY, PE_KEY),)):
    """Autograd leaves for the oracle: every weight, and each learned table as '<...>.pe' = weight[None], a leaf too."""
    p = O.leafify({k: v for k, v in st.items() if k not in dict(pos_keys)})
    for wk, pk in pos_keys:
        p[pk] = st[wk].detach().clone()[None].requires_grad_(True)
    return p


def case_args(z, **kw):
    from parity_util import make_args
    B, L, d, H, N, Va, Vb, k, nb = [int(x) for x in z["meta"]]
    return make_args(d, H, k, L, Va, Vb, N, B, **kw)
