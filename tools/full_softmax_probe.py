"""Timing probe of the full-catalogue softmax loss (csrc/full_ce.hip) at BASELINE configs[1]'s shape: single domain, 100 k items,
B = 4096, L = 200, d = 128, synthetic Zipf users (recguru_amd.synthetic, lengths U{5..220}) and their real dec_in mask.

  python tools/full_softmax_probe.py [--B 4096] [--reps 5] [--tiers bf16,bf16x3] [--out profiles/r07/full_softmax_probe.txt]

Per tier (bf16, bf16x3): the training-form forward (rg_full_ce_fwd, train=1), the inference form, the dW kernel (rg_full_ce_dw) and
FullSoftmaxLoss forward + backward, each as the median of --reps HIP-event timings after one warm-up; executed TFLOP/s count the live
rows only (live x C x d x 2 per product: 2 products in the training forward, 1 in the inference form, 2 in dW); the fraction of the
2.5 PF bf16 peak and of the best on-box MFMA issue loop (profiles/r06/peaks.txt); and, for comparison, the sampled-softmax loss
(ops.sampled_softmax_loss, k = 30) forward + backward on the same rows.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 2500.0              # TFLOP/s, dense bf16 MFMA
LOOP = 1705.3              # TFLOP/s, profiles/r06/peaks.txt mfma_16x16x32_bf16_4wave_per_simd


def timed(fn, reps):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--L", type=int, default=200)
    ap.add_argument("--V", type=int, default=100000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tiers", default="bf16,bf16x3", help="comma-separated subset of bf16, bf16x3 (counter passes: one tier)")
    a = ap.parse_args()
    from recguru_amd import hip, ops, synthetic
    torch.cuda.set_device(0)
    dm = synthetic.make_domain(a.B, a.V, a.L, 30, seed=1, min_len=5)
    dec_in = torch.as_tensor(dm["dec_in"]).cuda()
    dec_out = torch.as_tensor(dm["dec_out"]).cuda().reshape(-1).contiguous()
    neg = torch.as_tensor(dm["n_items"]).cuda().reshape(-1).contiguous()
    mask = (dec_in != 0).reshape(-1).to(torch.float32).contiguous()
    n, C, d = dec_in.numel(), a.V + 2, a.d
    nl = float(mask.sum())
    g = torch.Generator(device="cuda").manual_seed(0)
    h32 = torch.randn(n, d, device="cuda", generator=g) * 0.5
    w32 = torch.randn(C, d, device="cuda", generator=g) * 0.1
    lines = ["configs[1] shape: B=%d L=%d d=%d C=%d rows=%d live=%d (%.1f %%)" % (a.B, a.L, d, C, n, nl, 100 * nl / n)]
    live = hip.live_tiles(mask, n)
    lines.append("live 16-row tiles: %d of %d" % (int(live[0]), (n + 15) // 16))
    for tier in a.tiers.split(","):
        ops.set_compute_dtype(torch.bfloat16 if tier == "bf16" else "bf16x3")
        dt = ops.compute_dtype()
        h = h32.to(dt).contiguous()
        wp = torch.nn.Parameter(w32.clone())
        w = ops.shadow(wp)
        sums = torch.zeros(2, device="cuda")
        sums[1] = nl
        one = torch.ones(1, device="cuda")
        dw = torch.zeros(C, d, device="cuda")
        st = {}

        def fwd_train():
            st["lse"], _ = hip.full_ce_fwd(h, w, dec_out, mask, live, sums, train=True)

        def fwd_infer():
            hip.full_ce_fwd(h, w, dec_out, mask, live, sums, train=False)

        def dwk():
            hip.full_ce_dw(h, w, dec_out, mask, live, st["lse"], sums, one, dw)

        hh = h.detach().clone().requires_grad_(True)

        def loss_bwd():
            wp.grad = None
            ops.full_softmax_loss(hh, wp, dec_out, mask).backward()

        def sampled():
            ops.sampled_softmax_loss(hh, wp, dec_out, neg, mask, 30).backward()

        fl = 2.0 * nl * C * d
        for name, fn, passes in (("fwd train", fwd_train, 2), ("fwd infer", fwd_infer, 1), ("dW", dwk, 2),
                                 ("loss fwd+bwd", loss_bwd, 4), ("sampled k=30 fwd+bwd", sampled, 0)):
            ms = timed(fn, a.reps)
            if passes:
                tf = fl * passes / ms / 1e9
                lines.append("%-7s %-22s %9.2f ms  %7.1f TFLOP/s  %5.1f %% of 2.5 PF  %5.1f %% of the MFMA loop"
                             % (tier, name, ms, tf, 100 * tf / PEAK, 100 * tf / LOOP))
            else:
                lines.append("%-7s %-22s %9.2f ms" % (tier, name, ms))
        lines.append("%-7s loss %.6f" % (tier, float(ops.full_softmax_loss(hh.detach(), wp, dec_out, mask))))
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
