"""One process of tests/test_hard_negs_gpu.py, run with RG_DETERMINISTIC=1 (librecguru_hip_det.so); writes every number the test
compares to argv[2].

  python tests/hard_negs_worker.py kernel <out.npz>   the invariance case of the test file (ids / scores) in every tier
  python tests/hard_negs_worker.py models <out.npz>   per tier, five losses (cross recon, cross bpr, single recon, MyRec bpr, cross
                                                      recon with k_hard < k): loss and every parameter gradient once with
                                                      n_items = HardNegatives(...) and once with hip.hard_negs called by hand on the
                                                      same decoder states and the plain tensor passed
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

TIERS = ["bf16", "bf16x3", "f32"]


def _inputs(z, dom, V, k, rng, device):
    """a golden batch's sequences, a pool of a third of the ids, a private draw that avoids the pool, per-sequence exclusion rows"""
    enc_in, dec_in, dec_out = (torch.as_tensor(z["%s.%s" % (nm, dom)]).to(device) for nm in ("enc_in", "dec_in", "dec_out"))
    B, L = dec_out.shape
    ids = rng.permutation(np.arange(1, V))
    pool, rest = np.sort(ids[:len(ids) // 3]), ids[len(ids) // 3:]
    private = rest[rng.integers(0, len(rest), size=(B, L * k))]
    rows = [np.unique(pool[rng.integers(0, len(pool), size=int(rng.integers(0, 6)))]) for _ in range(B)]
    import hard_negs_ref as HR
    ex, lo, hi = HR.flat_excl(rows, rng)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(device)
    return enc_in, dec_in, dec_out, t(pool), t(private), t(ex), t(lo), t(hi)


def _grads(model):
    return {k: p.grad.detach().float().cpu().numpy().copy() for k, p in model.named_parameters() if p.grad is not None}


def run_models(out):
    from golden_util import load_case
    from parity_util import build_cross, case_param
    from recguru_amd import auto_training as AT, hip, ops, training as T
    from recguru_amd.models import HardNegatives, MyRec
    dev = "cuda"
    z = load_case("case1")
    for tier in TIERS:
        ops.set_compute_dtype({"bf16": torch.bfloat16, "bf16x3": "bf16x3", "f32": torch.float32}[tier])
        param, G, _ = build_cross(z, dev)
        assert param.dropout_rate == 0
        G.train()
        z2 = load_case("case2")
        p2 = case_param(z2)
        p2.vocab_size = p2.vocab_size_a
        torch.manual_seed(11)
        Rm = MyRec(dev, p2, None).to(torch.float32).to(dev)
        Rm.train()
        rng = np.random.default_rng(7500)

        def cross_recon(n_items, enc_in, dec_in, dec_out, mask):
            B, L = dec_out.shape
            return T.loss_ae(G, enc_in, dec_in, dec_out, n_items, True, B, L, param, mask, dev, domain="a")

        def cross_bpr(n_items, enc_in, dec_in, dec_out, mask):
            return T.loss_bpr_func(G, enc_in, dec_in, dec_out, n_items, mask, "a", param)

        def single_recon(n_items, enc_in, dec_in, dec_out, mask):
            B, L = dec_out.shape
            return AT.loss_ae(Rm, enc_in, dec_in, dec_out, n_items, True, B, L, p2, mask)

        def single_bpr(n_items, enc_in, dec_in, dec_out, mask):
            return AT.loss_bpr_func(Rm, enc_in, dec_in, dec_out, n_items, mask)

        cases = [("cross_recon", G, z, "a", param.vocab_size_a, param.n_negs, param.n_negs, 0, cross_recon,
                  lambda e, di, m: G.get_dec_out(e, di, "a", m)[0], lambda: G.item_table("a")),
                 ("cross_bpr", G, z, "a", param.vocab_size_a, param.n_bpr_neg, param.n_bpr_neg, 0, cross_bpr,
                  lambda e, di, m: G.recommend_forward(e, di, "a", m.view(-1, param.rec_maxlen)), lambda: G.item_table("a")),
                 ("single_recon", Rm, z2, "a", p2.vocab_size, p2.n_negs, p2.n_negs, 0, single_recon,
                  lambda e, di, m: Rm.AutoEnc.get_dec_out(e, di)[0], lambda: Rm.AutoEnc.src_emb.weight),
                 ("single_bpr", Rm, z2, "a", p2.vocab_size, p2.num_train_neg, p2.num_train_neg, 0, single_bpr,
                  lambda e, di, m: Rm.get_embedding(e, di), lambda: Rm.AutoEnc.src_emb.weight),
                 ("cross_recon_partial", G, z, "b", param.vocab_size_b, param.n_negs, 2, 1, None,
                  lambda e, di, m: G.get_dec_out(e, di, "b", m)[0], lambda: G.item_table("b"))]
        for name, model, zz, dom, V, k, k_hard, skip, loss_fn, h_fn, table_fn in cases:
            if loss_fn is None:
                loss_fn = lambda n_items, e, di, do, m: T.loss_ae(G, e, di, do, n_items, True, do.shape[0], do.shape[1], param, m, dev, domain="b")
            enc_in, dec_in, dec_out, pool, private, ex, lo, hi = _inputs(zz, dom, V, k, rng, dev)
            B, L = dec_out.shape
            mask = T.get_pad_mask(dec_out, 0, dev)
            run = "%s.%s" % (tier, name)
            # by hand: the same decoder states, the kernel called here, the plain tensor passed
            with torch.no_grad():
                h = h_fn(enc_in, dec_in, mask)
            neg = private.reshape(B * L, k).clone()
            hip.hard_negs(h.detach().contiguous().view(B * L, -1), ops.shadow(table_fn()), pool, dec_out.reshape(-1), mask, L, k_hard,
                          skip=skip, excl=ex, excl_lo=lo, excl_hi=hi, out=neg, checked=True)
            model.zero_grad(set_to_none=True)
            loss = loss_fn(neg.view(B, L * k), enc_in, dec_in, dec_out, mask)
            loss.backward()
            out[run + "|loss.plain"] = np.array([float(loss.detach())], dtype=np.float32)
            for kk, g in _grads(model).items():
                out[run + "|g.plain." + kk] = g
            model.zero_grad(set_to_none=True)
            loss = loss_fn(HardNegatives(private, pool, k_hard, skip, ex, lo, hi), enc_in, dec_in, dec_out, mask)
            loss.backward()
            out[run + "|loss.hard"] = np.array([float(loss.detach())], dtype=np.float32)
            for kk, g in _grads(model).items():
                out[run + "|g.hard." + kk] = g
            for nm, t in (("neg", neg), ("private", private.reshape(B * L, k)), ("labels", dec_out.reshape(-1)), ("mask", mask), ("pool", pool),
                          ("excl", ex), ("excl_lo", lo), ("excl_hi", hi)):
                out[run + "|" + nm] = t.cpu().numpy()
            out[run + "|k_hard"] = np.array(k_hard)
            out[run + "|L"] = np.array(L)
    ops.set_compute_dtype(torch.bfloat16)


def run_kernel(out):
    from recguru_amd import hip, ops
    from test_hard_negs_gpu import invariance_results
    for tier in TIERS:
        ops.set_compute_dtype({"bf16": torch.bfloat16, "bf16x3": "bf16x3", "f32": torch.float32}[tier])
        ids, sc = invariance_results(hip, tier, torch.bfloat16 if tier == "bf16" else torch.float32)
        out[tier + ".ids"], out[tier + ".scores"] = ids, sc


def main():
    mode, out_path = sys.argv[1:3]
    from recguru_amd import hip
    torch.cuda.set_device(0)
    out = {}
    {"kernel": run_kernel, "models": run_models}[mode](out)
    torch.cuda.synchronize()
    out["det_enabled"] = np.array(int(hip.lib().rg_det_enabled()))
    np.savez(out_path, **out)


if __name__ == "__main__":
    main()
