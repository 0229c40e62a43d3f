"""Timing probe of the logQ correction of the per-position sampled softmax (csrc/loss.hip BIAS instantiations): what
the two bias inputs cost, against the same loss without them, in the same run:

  python tools/logq_probe.py [--shape configs1|config5|both] [--tiers bf16,bf16x3] [--out profiles/logq/probe.txt]

  configs1   100 k items, d = 128, B = 4096, L = 200, k = 30      (training form with the rows in registers)
  config5    2 M items,   d = 256, B = 4096, L = 400, k = 1024    (online form)

Synthetic Zipf users (recguru_amd.synthetic, lengths U{5..L+20}) with their real dec_in mask and a Zipf item-frequency vector, so
that the negatives are the alias table's frequency-weighted draws (popular rows, and their biases, come from cache) and the biases
are the tables DeviceLoader(logq=True) hands out.  Forward + backward of ops.sampled_softmax_loss (table gradient accumulated into
a persistent .grad), with and without biases ALTERNATING call by call; each figure is the median of --reps HIP-event timings after
--warmup untimed pairs.  The byte model: 4 more bytes per gathered row of 2 d (bf16) or 4 d (f32) bytes."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"configs1": dict(V=100000, d=128, B=4096, L=200, k=30),
          "config5": dict(V=2000000, d=256, B=4096, L=400, k=1024)}


def timed_pair(fa, fb, reps, warmup):
    """Median ms of fa and of fb, the two called in turn."""
    ts = ([], [])
    for i in range(warmup + reps):
        for fn, acc in ((fa, ts[0]), (fb, ts[1])):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                acc.append(e0.elapsed_time(e1))
    return float(np.median(ts[0])), float(np.median(ts[1])), float(np.min(ts[0])), float(np.min(ts[1]))


class _Lines(list):
    def append(self, s):                       # shown as it is measured: a shape takes minutes
        list.append(self, s)
        print(s, flush=True)


def probe(name, cfg, tiers, reps, warmup, lines):
    from recguru_amd import ops, sampler, synthetic
    V, d, B, L, k = cfg["V"], cfg["d"], cfg["B"], cfg["L"], cfg["k"]
    seqs, val, test, _ = synthetic.make_users(B, V, L, seed=1, min_len=5)
    wf = np.zeros(V + 1)
    wf[1:] = 1.0 / np.arange(1, V + 1, dtype=np.float64)
    dom = sampler.DeviceDomain(seqs, val, test, V, "cuda", wf=wf)
    users = torch.arange(B, device="cuda")
    (enc_in, dec_in, dec_out), n_items, _, _ = dom.batch(users, L, L, V + 1, L * k, sampler.batch_seed(1, 0, 0), logq=True)
    dec_out = dec_out.reshape(-1).contiguous()
    neg = n_items.ids.reshape(-1).contiguous()
    neg_bias = n_items.neg_bias
    pos_bias = n_items.pos_bias.repeat_interleave(L).contiguous()
    mask = (dec_in != 0).reshape(-1).to(torch.float32).contiguous()
    n, rows = dec_in.numel(), V + 2
    nl = float(mask.sum())
    g = torch.Generator(device="cuda").manual_seed(0)
    h32 = torch.randn(n, d, device="cuda", generator=g) * 0.5
    w32 = torch.randn(rows, d, device="cuda", generator=g) * 0.1
    lines.append("%s: B=%d L=%d d=%d k=%d table rows=%d positions=%d live=%d (%.1f %%), distinct negative ids %d"
                 % (name, B, L, d, k, rows, n, nl, 100 * nl / n, int(torch.unique(neg[:50000000]).numel())))
    for tier in tiers:
        ops.set_compute_dtype(torch.bfloat16 if tier == "bf16" else "bf16x3")
        h = h32.to(ops.compute_dtype()).contiguous()
        wp = torch.nn.Parameter(w32.clone())
        hh = h.detach().clone().requires_grad_(True)

        def plain():
            hh.grad = None
            ops.sampled_softmax_loss(hh, wp, dec_out, neg, mask, k).backward()

        def biased():
            hh.grad = None
            ops.sampled_softmax_loss(hh, wp, dec_out, neg, mask, k, neg_bias=neg_bias, pos_bias=pos_bias).backward()

        m0, m1, lo0, lo1 = timed_pair(plain, biased, reps, warmup)
        row_bytes = d * h.element_size()
        lines.append("%-7s %-9s fwd+bwd without biases %9.3f ms (min %9.3f) | with biases %9.3f ms (min %9.3f) | ratio %.4f (of minima "
                     "%.4f) | byte model %.4f" % (tier, name, m0, lo0, m1, lo1, m1 / m0, lo1 / lo0, 1.0 + 4.0 / row_bytes))
        with torch.no_grad():
            lines.append("%-7s %-9s loss without %.6f with %.6f"
                         % (tier, name, float(ops.sampled_softmax_loss(hh.detach(), wp, dec_out, neg, mask, k)),
                            float(ops.sampled_softmax_loss(hh.detach(), wp, dec_out, neg, mask, k, neg_bias=neg_bias, pos_bias=pos_bias))))
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
