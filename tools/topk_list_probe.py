"""Timing probe of top-K / exact rank over a candidate list shared by the batch (rg_topk_list, csrc/topk.hip) against
the full-catalogue pass (rg_topk_scores) over the same table, in the same run:

  python tools/topk_list_probe.py [--shape 100k|2m|both] [--tiers bf16,f32] [--out profiles/topk_list/probe.txt]

  100k   100 000 items, d = 128        2m   2 000 000 items, d = 256        B in {256, 4096}, K in {10, 100}, ranks asked for

Lists: every item (the price of the indirection against the contiguous walk, row for row) and a random ascending 1/2, 1/8 and 1/64
of the items.  Every figure is the median of --reps HIP-event timings after --warmup untimed calls; a list call's time includes the
wait for its one-word check.  Per list the probe also prices the alternative it did not build -- gather the listed rows into a
contiguous buffer once, then the range walk -- as n_list * d * 2 element sizes of traffic at the gather-copy rate of
profiles/r06/peaks.txt plus the range walk over n_list contiguous rows of the same table, measured.  Last, the [B, C]-expanded form (hip.rank_scores with the
list repeated for every user; ranks only) at the largest C whose ids stay under --expand_gib."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"100k": dict(V=100000, d=128), "2m": dict(V=2000000, d=256)}
FRACTIONS = (1, 2, 8, 64)
COPY_GBPS = 5500.0          # profiles/r06/peaks.txt: gather_copy_{256,512,1024}B_rows, 5.4 - 5.7 TB/s of row read + row write


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
    def append(self, s):                       # shown as it is measured
        list.append(self, s)
        print(s, flush=True)


def probe(name, cfg, tiers, Bs, Ks, reps, warmup, expand_gib, lines):
    from recguru_amd import hip, ops
    V, d = cfg["V"], cfg["d"]
    g = torch.Generator(device="cuda").manual_seed(0)
    w32 = torch.randn(V + 2, d, device="cuda", generator=g) * 0.1
    lists = {}
    for f in FRACTIONS:
        if f == 1:
            lists[f] = torch.arange(1, V + 1, device="cuda")
        else:
            lists[f] = torch.sort(torch.randperm(V, device="cuda", generator=g)[: V // f] + 1).values.contiguous()
    lines.append("%s: %d items, d=%d, table rows=%d; lists of %s ids" % (name, V, d, V + 2, ", ".join(str(lists[f].numel()) for f in FRACTIONS)))
    for tier in tiers:
        ops.set_compute_dtype(torch.bfloat16 if tier == "bf16" else torch.float32)
        table = w32.to(ops.compute_dtype()).contiguous()
        esz = table.element_size()
        for B in Bs:
            h = (torch.randn(B, d, device="cuda", generator=g) * 0.5).to(table.dtype).contiguous()
            target = torch.randint(1, V + 1, (B,), device="cuda", generator=g)
            for K in Ks:
                full = timed(lambda: hip.topk_scores(h, table, K, 1, V, target=target), reps, warmup)
                lines.append("%-4s %-4s B=%-4d K=%-3d range walk, all %d items            %9.3f ms  (%.1f GB/s of table)"
                             % (tier, name, B, K, V, full, V * d * esz / full / 1e6))
                for f in FRACTIONS:
                    rows = lists[f]
                    n = rows.numel()
                    ms = timed(lambda: hip.topk_list(h, table, K, rows, target=target), reps, warmup)
                    # what the copy form's walk would cost: the range walk over n contiguous rows, measured (targets folded into them)
                    tgt_n = (target - 1) % n + 1
                    walk = full if f == 1 else timed(lambda: hip.topk_scores(h, table, K, 1, n, target=tgt_n), reps, warmup)
                    copy_ms = n * d * esz * 2 / COPY_GBPS / 1e6
                    lines.append("%-4s %-4s B=%-4d K=%-3d list of 1/%-2d = %7d ids              %9.3f ms  = %5.2fx the range walk | %6.2f ns per id (range walk: "
                                 "%6.2f ns per item) | copy form: %8.3f ms copy (priced) + %8.3f ms range walk over %d contiguous rows (measured) = %8.3f ms"
                                 % (tier, name, B, K, f, n, ms, ms / full, ms * 1e6 / n, full * 1e6 / V, copy_ms, walk, n, copy_ms + walk))
            # the [B, C]-expanded form: the list's ids once per user, every user gathers every row again; ranks only
            C = int(min(V, expand_gib * (1 << 30) // (8 * B)))
            rows = lists[max(f for f in FRACTIONS if lists[f].numel() >= C)][:C]          # the sparsest of the lists that holds C ids
            cand = rows.unsqueeze(0).expand(B, rows.numel()).contiguous()
            ms = timed(lambda: hip.rank_scores(h, table, target, cand, want_scores=False), reps, warmup)
            ml = timed(lambda: hip.topk_list(h, table, 0, rows, target=target), reps, warmup)
            lines.append("%-4s %-4s B=%-4d rank only, C=%d: [B, C]-expanded rank_scores %9.3f ms (%.2f GB of ids, %.1f GB of row reads) | topk_list %9.3f ms"
                         % (tier, name, B, rows.numel(), ms, cand.numel() * 8 / 1e9, float(B) * rows.numel() * d * esz / 1e9, ml))
            del cand
            torch.cuda.empty_cache()
        del table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["100k", "2m", "both"])
    ap.add_argument("--tiers", default="bf16,f32")
    ap.add_argument("--B", default="256,4096")
    ap.add_argument("--K", default="10,100")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--expand_gib", type=float, default=4.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lines = _Lines()
    lines.append("one MI355X; median of %d device-event timings after %d untimed calls" % (a.reps, a.warmup))
    for name in (("100k", "2m") if a.shape == "both" else (a.shape,)):
        probe(name, SHAPES[name], a.tiers.split(","), [int(x) for x in a.B.split(",")], [int(x) for x in a.K.split(",")], a.reps, a.warmup,
              a.expand_gib, lines)
    txt = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
