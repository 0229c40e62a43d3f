"""Timing probe of the wide top-K (rg_topk_wide, csrc/topk_wide.hip) against the shipped pass (rg_topk_scores, K <= 128)
and the dense form (hip.gemm_nt to an f32 [B, items] matrix, then torch.topk), in one run, alternating:

  python tools/topk_wide_probe.py [--shape 100k|2m|both] [--tiers bf16,f32] [--B 256,4096] [--out profiles/topk_wide/probe.txt]

  100k   100 000 items, d = 128        2m   2 000 000 items, d = 256        B in {256, 4096}

Per (shape, tier, B): topk_scores at K = 100 and 128, topk_wide at K = 100, 128, 256 and 1024, dense at the same four K.  Every figure
is the median of --reps HIP-event timings after --warmup untimed calls; the forms take turns inside every repetition, so a drift of
the device hits all of them alike.  min .. max of the repetitions is the run's own spread.  Per form the peak of the bytes the call
holds beyond its operands (workspace and outputs; the dense form's score matrix), and for topk_wide the levels of the radix select
that did work, read from the workspace state (largest over the users / mean).  --dense_gib caps the dense form's score matrix;
--dense_reps shortens its repetitions where a call takes seconds."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"100k": dict(V=100000, d=128), "2m": dict(V=2000000, d=256)}
NARROW_K = (100, 128)
WIDE_K = (100, 128, 256, 1024)


def timed_in_turns(fns, reps, warmup):
    """{name: [ms per repetition]}: every repetition times each form once, in the order given"""
    for _ in range(warmup):
        for fn, _ in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for rep in range(reps):
        for name, (fn, nrep) in fns.items():
            if rep >= nrep:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1))
    return ts


def peak_bytes(fn):
    """bytes the call allocates beyond what is live before it (the caching allocator's peak; a cached workspace is dropped first)"""
    from recguru_amd import hip
    hip._TN_WS.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


class _Lines(list):
    def append(self, s):                       # shown as it is measured
        list.append(self, s)
        print(s, flush=True)


def probe(name, cfg, tiers, Bs, reps, warmup, dense_gib, dense_reps, lines):
    from recguru_amd import hip, ops
    V, d = cfg["V"], cfg["d"]
    g = torch.Generator(device="cuda").manual_seed(0)
    w32 = torch.randn(V + 2, d, device="cuda", generator=g) * 0.1
    lines.append("%s: %d items, d=%d, table rows=%d" % (name, V, d, V + 2))
    for tier in tiers:
        ops.set_compute_dtype(torch.bfloat16 if tier == "bf16" else torch.float32)
        table = w32.to(ops.compute_dtype()).contiguous()
        for B in Bs:
            h = (torch.randn(B, d, device="cuda", generator=g) * 0.5).to(table.dtype).contiguous()
            dense_ok = float(B) * V * 4 <= dense_gib * (1 << 30)

            def dense(K):
                s = hip.gemm_nt(h, table[1:V + 1], out_f32=True)
                return torch.topk(s, K, dim=1)
            fns = {}
            for K in NARROW_K:
                fns["topk_scores K=%d" % K] = ((lambda K=K: hip.topk_scores(h, table, K, 1, V)), reps)
            for K in WIDE_K:
                fns["topk_wide   K=%d" % K] = ((lambda K=K: hip.topk_wide(h, table, K, 1, V)), reps)
            if dense_ok:
                for K in WIDE_K:
                    fns["dense       K=%d" % K] = ((lambda K=K: dense(K)), min(reps, dense_reps))
            if dense_ok:
                try:
                    dense(WIDE_K[0])
                except (RuntimeError, AssertionError) as e:          # the GEMM refuses the shape: said, not hidden
                    lines.append("%-4s %-4s B=%-4d dense: not run (%s)" % (tier, name, B, str(e).splitlines()[0][:120]))
                    fns = {k: v for k, v in fns.items() if not k.startswith("dense")}
            ts = timed_in_turns(fns, reps, warmup)
            for key, (fn, _) in fns.items():
                t = ts[key]
                extra = ""
                if key.startswith("topk_wide"):
                    fn()
                    fault, levels, kept = hip.topk_wide_state(h.device, B)
                    extra = "  levels %d (mean %.2f), keys kept <= %d, fault word %d" % (int(levels.max()), float(levels.float().mean()), int(kept.max()), fault)
                lines.append("%-4s %-4s B=%-4d %-18s %10.3f ms  (min %10.3f .. max %10.3f, %2d reps)  peak %8.1f MB%s"
                             % (tier, name, B, key, float(np.median(t)), min(t), max(t), len(t), peak_bytes(fn) / 1e6, extra))
            if not dense_ok:
                lines.append("%-4s %-4s B=%-4d dense: [B, items] f32 = %.1f GB is above --dense_gib, not run" % (tier, name, B, float(B) * V * 4 / 1e9))
        del table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["100k", "2m", "both"])
    ap.add_argument("--tiers", default="bf16,f32")
    ap.add_argument("--B", default="256,4096")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dense_gib", type=float, default=40.0)
    ap.add_argument("--dense_reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lines = _Lines()
    lines.append("one MI355X; median of %d device-event timings after %d untimed calls, the forms in turns (dense: %d)" % (a.reps, a.warmup, min(a.reps, a.dense_reps)))
    for name in (("100k", "2m") if a.shape == "both" else (a.shape,)):
        probe(name, SHAPES[name], a.tiers.split(","), [int(x) for x in a.B.split(",")], a.reps, a.warmup, a.dense_gib, a.dense_reps, lines)
    txt = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
