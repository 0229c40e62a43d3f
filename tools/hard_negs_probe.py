"""Timing probe of the hard-negative selection (csrc/hard_negs.hip) against the route the project had before it --
hip.topk_list over ALL positions with (sequence's history + label) as a CSR exclusion -- in the same run, and of what the feature
adds to a training step:

  python tools/hard_negs_probe.py [--shape configs1|config5|both] [--tiers bf16,bf16x3] [--no_steps] [--out profiles/hard_negs/probe.txt]

  configs1   100 k items, d = 128, B = 4096, L = 200, k = 30, C in {1024, 8192}
  config5    2 M items,   d = 256, B = 4096, L = 400, k = 30, C in {1024, 8192}

Synthetic Zipf users (recguru_amd.synthetic, lengths U{5..L+20}) with their real dec_out mask and labels; the pool is what
DeviceLoader(hard_negs=C) draws (so fewer than C distinct ids), the exclusion rows the domain's.  Every figure is the median of --reps
HIP-event timings after --warmup untimed calls.  The old route's time is the hip.topk_list call alone (its one host wait included,
as every call has it); building its per-position CSR is timed once and shown beside it.  TFLOP/s count live positions x C x d x 2.
Steps (configs1's model, 3 blocks, dropout 0.5, device loaders included in the step): training.recon_step with the sampled softmax
(k = 30) and with the BPR loss of the recommender phase (k = n_bpr_neg), with --hard_negs 8192 and without."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"configs1": dict(V=100000, d=128, B=4096, L=200, k=30, Cs=(1024, 8192)),
          "config5": dict(V=2000000, d=256, B=4096, L=400, k=30, Cs=(1024, 8192))}


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


class _Lines(list):
    def append(self, s):                       # shown as it is measured: a shape takes minutes
        list.append(self, s)
        print(s, flush=True)


def position_csr(dom, users, labels, L):
    """per POSITION the sorted unique ids of (its sequence's exclusion row + its label): what hip.topk_list needs to leave out what
    rg_hard_negs leaves out.  (values, offsets [n + 1])"""
    n = labels.numel()
    lo, hi = dom.excl_off[users], dom.excl_off[users + 1]
    seq_len = (hi - lo).repeat_interleave(L)                                   # [n] ids of the row of each position
    pos = torch.arange(n, device=labels.device).repeat_interleave(seq_len)
    start = lo.repeat_interleave(L).repeat_interleave(seq_len)
    first = torch.cumsum(seq_len, 0) - seq_len
    ids = dom.excl[start + (torch.arange(pos.numel(), device=labels.device) - first.repeat_interleave(seq_len))]
    big = int(dom.V) + 2
    keys = torch.cat([pos * big + ids, torch.arange(n, device=labels.device) * big + labels])
    keys = torch.unique(keys)                                                   # sorted: by position, then id
    counts = torch.bincount(keys // big, minlength=n)
    off = torch.zeros(n + 1, dtype=torch.int64, device=labels.device)
    off[1:] = torch.cumsum(counts, 0)
    return (keys % big).contiguous(), off


def probe_kernel(name, cfg, tiers, reps, warmup, lines):
    from recguru_amd import hip, ops, sampler, synthetic
    V, d, B, L, k = cfg["V"], cfg["d"], cfg["B"], cfg["L"], cfg["k"]
    seqs, val, test, _ = synthetic.make_users(B, V, L, seed=1, min_len=5)
    dom = sampler.DeviceDomain(seqs, val, test, V, "cuda")
    users = torch.arange(B, device="cuda")
    (enc_in, dec_in, dec_out), _, _, _ = dom.batch(users, L, L, V + 1, L, sampler.batch_seed(1, 0, 0))
    labels = dec_out.reshape(-1).contiguous()
    mask = (dec_out != 0).reshape(-1).to(torch.float32).contiguous()
    n, rows = labels.numel(), V + 2
    nl = float(mask.sum())
    live = hip.live_tiles(mask, n)
    lo, hi = dom.excl_off[users].contiguous(), dom.excl_off[users + 1].contiguous()
    g = torch.Generator(device="cuda").manual_seed(0)
    h32 = torch.randn(n, d, device="cuda", generator=g) * 0.5
    w32 = torch.randn(rows, d, device="cuda", generator=g) * 0.1
    lines.append("%s: B=%d L=%d d=%d table rows=%d positions=%d live=%d (%.1f %%), live 16-row tiles %d of %d, k=%d"
                 % (name, B, L, d, rows, n, nl, 100 * nl / n, int(live[0]), (n + 15) // 16, k))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    cv, coff = position_csr(dom, users, labels, L)
    e1.record()
    torch.cuda.synchronize()
    lines.append("%s: per-position CSR of the old route: %d ids, %.1f MB, built in %.1f ms (torch, once; not in the figures below)"
                 % (name, cv.numel(), cv.numel() * 8 / 1e6, e0.elapsed_time(e1)))
    livemask = mask != 0
    for tier in tiers:
        ops.set_compute_dtype(torch.bfloat16 if tier == "bf16" else "bf16x3")
        h = h32.to(ops.compute_dtype()).contiguous()
        w = w32.to(ops.compute_dtype()).contiguous()
        for C in cfg["Cs"]:
            pool = dom.shared_candidates(C, sampler.batch_seed(1, 0, 1) ^ sampler.HARD_POOL_SEED)
            Cd = pool.numel()
            out = torch.full((n, k), -1, dtype=torch.int64, device="cuda")
            st = {}

            def new():
                hip.hard_negs(h, w, pool, labels, mask, L, k, excl=dom.excl, excl_lo=lo, excl_hi=hi, out=out, checked=True)

            def old():
                st["ids"] = hip.topk_list(h, w, k, pool, excl=cv, excl_off=coff)[0]

            mn = timed(new, reps, warmup)
            mo = timed(old, reps, warmup)
            same = bool(torch.equal(out[livemask], st["ids"][livemask]))
            fl = 2.0 * nl * Cd * d
            lines.append("%-7s %-9s C=%-5d (%5d distinct) hard_negs %8.2f ms %6.1f TFLOP/s | topk_list over all positions %8.2f ms | "
                         "old / new = %5.2fx | same ids on live positions: %s" % (tier, name, C, Cd, mn, fl / mn / 1e9, mo, mo / mn, same))
            del out, st
        del h, w
        torch.cuda.empty_cache()


def probe_steps(tiers, reps, warmup, lines, C=8192):
    from recguru_amd import blocks, config, models, ops, optim, sampler, synthetic, training as T
    cfg = SHAPES["configs1"]
    V, d, B, L = cfg["V"], cfg["d"], cfg["B"], cfg["L"]
    a = argparse.Namespace(date="probe", d_model=d, n_head=4, d_ff=512, n_negs=cfg["k"], decoder_neg=True, fix_enc=True, lr=0.01,
                           batch_size=B, batch_size_val=256, dataset_pick=1, run=1, target_domain="a", cross="True", sas="False",
                           result_path="/tmp/rg_probe", seq_len=L, vocab_size_a=V, vocab_size_b=V, n_blocks=3, dropout=0.5)
    param = config.get_param(a, make_dirs=False)
    doms = []
    for seed in (1, 2):
        seqs, val, test, _ = synthetic.make_users(2 * B, V, L, seed=seed, min_len=5)
        doms.append(sampler.DeviceDomain(seqs, val, test, V, "cuda"))
    for tier in tiers:
        ops.set_compute_dtype(torch.bfloat16 if tier == "bf16" else "bf16x3")
        torch.manual_seed(0)
        G = models.MyAuto4Rec_c("cuda", param, wf=None, enc_share=True, dec_rec=False).to(torch.float32).to("cuda")
        G.train()
        opt = blocks.ScheduledOptim(optim.Adam(G.parameters(), betas=(0.9, 0.98), eps=1e-09), 1.0, param.d_model, param.n_warmup_steps)
        g_params = list(G.parameters())
        for what, loss_type, kk in (("AE step (sampled softmax, k=%d)" % cfg["k"], "s_soft", cfg["k"]),
                                    ("recommender step (BPR, k=%d)" % param.n_bpr_neg, "bpr", param.n_bpr_neg)):
            ms = {}
            for hard in (0, C):
                its = [T._Cycler(sampler.DeviceLoader(dm, B, L, L, V + 1, L * kk, seed=s, shuffle=False, hard_negs=hard))
                       for s, dm in enumerate(doms)]

                def step():
                    ba, bb = its[0].next("cuda"), its[1].next("cuda")
                    return T.recon_step(G, opt, ba[:4], bb[:4], param, "cuda", T._NoDP(), g_params, True, loss_type, "schedule")

                ms[hard] = timed(step, reps, warmup)
            lines.append("%-7s %-40s without %8.2f ms | --hard_negs %d %8.2f ms | ratio %5.3f"
                         % (tier, what, ms[0], C, ms[C], ms[C] / ms[0]))
        del G, opt, g_params
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["configs1", "config5", "both"])
    ap.add_argument("--tiers", default="bf16,bf16x3")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no_steps", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lines = _Lines()
    for name in (("configs1", "config5") if a.shape == "both" else (a.shape,)):
        probe_kernel(name, SHAPES[name], a.tiers.split(","), a.reps, a.warmup, lines)
    if not a.no_steps:
        probe_steps(a.tiers.split(","), a.reps, a.warmup, lines)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
