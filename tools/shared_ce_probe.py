"""Timing probe of the sampled softmax over batch-shared candidates (csrc/shared_ce.hip) against the per-position
sampled softmax (csrc/loss.hip) on the same rows, in the same run:

  python tools/shared_ce_probe.py [--shape configs1|config5|both] [--tiers bf16,bf16x3] [--out profiles/shared_ce/probe.txt]

  configs1   100 k items, d = 128, B = 4096, L = 200, C in {1024, 8192};         per-position k = 30
  config5    2 M items,   d = 256, B = 4096, L = 400, C in {1024, 8192, 65536};  per-position k = 1024

Synthetic Zipf users (recguru_amd.synthetic, lengths U{5..L+20}) with their real dec_in mask; the candidates are what
DeviceLoader(shared_negs=C) draws (so fewer than C distinct ids), the per-position negatives what the device sampler draws.  Every
figure is the median of --reps HIP-event timings after --warmup untimed calls: forward + backward of the loss (ops level, table
gradient accumulated into a persistent .grad), and for the shared form also its pieces (training forward; candidate route of the
backward; the whole backward = candidate route + scaled copy + target scatter).  TFLOP/s count live rows x C x d x 2 per product, two
products in the forward, two in the candidate route."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"configs1": dict(V=100000, d=128, B=4096, L=200, k=30, Cs=(1024, 8192)),
          "config5": dict(V=2000000, d=256, B=4096, L=400, k=1024, Cs=(1024, 8192, 65536))}


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


def probe(name, cfg, tiers, reps, warmup, lines):
    from recguru_amd import hip, ops, sampler, synthetic
    V, d, B, L, k = cfg["V"], cfg["d"], cfg["B"], cfg["L"], cfg["k"]
    seqs, val, test, _ = synthetic.make_users(B, V, L, seed=1, min_len=5)
    dom = sampler.DeviceDomain(seqs, val, test, V, "cuda")
    users = torch.arange(B, device="cuda")
    (enc_in, dec_in, dec_out), neg, _, _ = dom.batch(users, L, L, V + 1, L * k, sampler.batch_seed(1, 0, 0))
    dec_out = dec_out.reshape(-1).contiguous()
    neg = neg.reshape(-1).contiguous()
    mask = (dec_in != 0).reshape(-1).to(torch.float32).contiguous()
    n, rows = dec_in.numel(), V + 2
    nl = float(mask.sum())
    g = torch.Generator(device="cuda").manual_seed(0)
    h32 = torch.randn(n, d, device="cuda", generator=g) * 0.5
    w32 = torch.randn(rows, d, device="cuda", generator=g) * 0.1
    live = hip.live_tiles(mask, n)
    lines.append("%s: B=%d L=%d d=%d table rows=%d positions=%d live=%d (%.1f %%), live 16-row tiles %d of %d"
                 % (name, B, L, d, rows, n, nl, 100 * nl / n, int(live[0]), (n + 15) // 16))
    for tier in tiers:
        ops.set_compute_dtype(torch.bfloat16 if tier == "bf16" else "bf16x3")
        h = h32.to(ops.compute_dtype()).contiguous()
        wp = torch.nn.Parameter(w32.clone())
        hh = h.detach().clone().requires_grad_(True)

        def per_position():
            hh.grad = None
            ops.sampled_softmax_loss(hh, wp, dec_out, neg, mask, k).backward()

        ms0 = timed(per_position, reps, warmup)
        lines.append("%-7s %-9s per-position k=%-5d fwd+bwd %9.2f ms" % (tier, name, k, ms0))
        for C in cfg["Cs"]:
            cand = dom.shared_candidates(C, sampler.batch_seed(1, 0, 1))
            Cd = cand.numel()
            w = ops.shadow(wp)
            sums = torch.zeros(2, device="cuda")
            sums[1] = nl
            one = torch.ones(1, device="cuda")
            st = {}

            def shared():
                hh.grad = None
                ops.shared_softmax_loss(hh, wp, dec_out, cand, mask).backward()

            def fwd_train():
                st["f"] = hip.shared_ce_fwd(h, w, dec_out, cand, mask, live, sums, train=True)

            def bwd(target_route):
                lse, wc, _, coef = st["f"]
                hip.shared_ce_bwd(h, rows, dec_out, cand, mask, live, wc, lse, coef, sums, one, wp.grad, target_route=target_route)

            ms = timed(shared, reps, warmup)
            mf = timed(fwd_train, reps, warmup)
            mc = timed(lambda: bwd(False), reps, warmup)
            mb = timed(lambda: bwd(True), reps, warmup)
            fl = 4.0 * nl * Cd * d
            lines.append("%-7s %-9s shared C=%-6d (%6d distinct) fwd+bwd %9.2f ms = %5.2fx the per-position time | fwd %8.2f ms %6.1f TFLOP/s | "
                         "candidate route %8.2f ms %6.1f TFLOP/s | whole bwd %8.2f ms"
                         % (tier, name, C, Cd, ms, ms / ms0, mf, fl / mf / 1e9, mc, fl / mc / 1e9, mb))
            with torch.no_grad():
                lines.append("%-7s %-9s shared C=%-6d loss %.6f (per-position k=%d: %.6f)"
                             % (tier, name, C, float(ops.shared_softmax_loss(hh.detach(), wp, dec_out, cand, mask)), k,
                                float(ops.sampled_softmax_loss(hh.detach(), wp, dec_out, neg, mask, k))))
        del wp, hh, h
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["configs1", "config5", "both"])
    ap.add_argument("--tiers", default="bf16,bf16x3")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lines = _Lines()
    for name in (("configs1", "config5") if a.shape == "both" else (a.shape,)):
        probe(name, SHAPES[name], a.tiers.split(","), a.reps, a.warmup, lines)
    txt = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
