"""Time rg_topk_scores alone (full-catalogue top-K + rank, csrc/topk.hip) against the only alternative the tree had before it: hip.gemm_nt
to a dense [B, C] f32 score matrix followed by torch.topk -- where that matrix fits in memory.

  python tools/bench_topk.py [--iters 20] [--warmup 3] [--out profiles/topk/bench_topk.json]

Shapes: the bench catalogue (100 k items, d = 128, B = 256 and 4096, K = 100) and config-5's (2 M items, d = 256, B = 256, K = 100), each
in the bf16 and the split-operand (x3) tier.  HIP events around the timed loop, warm-up first, a device sync on both sides.  Per case the
JSON holds both times, the bytes of table the fused pass has to read once, the resulting GB/s next to the read-only stream rate of
profiles/r06/peaks.txt, and the peak device memory of both paths."""
import argparse
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("bench_catalogue", 100000, 128, 256, 100), ("bench_catalogue", 100000, 128, 4096, 100), ("config5", 2000000, 256, 256, 100)]


def peak_read_rate():
    try:
        for ln in open(os.path.join(ROOT, "profiles", "r06", "peaks.txt")):
            m = re.match(r"hbm_read_only\s+([0-9.]+) GB/s", ln)
            if m:
                return float(m.group(1))
    except OSError:
        pass
    return None


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk", "bench_topk.json"))
    args = ap.parse_args()
    from recguru_amd import hip
    torch.cuda.set_device(0)
    free_total = torch.cuda.mem_get_info()[1]
    peak = peak_read_rate()
    cases = []
    for name, C, d, B, K in SHAPES:
        for tier, dtype in (("bf16", torch.bfloat16), ("x3", torch.float32)):
            g = torch.Generator(device="cuda").manual_seed(1)
            h = torch.randn(B, d, device="cuda", generator=g).to(dtype)
            table = (0.1 * torch.randn(C + 1, d, device="cuda", generator=g)).to(dtype)
            target = torch.randint(1, C + 1, (B,), device="cuda", generator=g)
            hip.SPLIT_OPERANDS = tier == "x3"
            # the rank part waits for the stream once per call (its targets are checked on the host): timed as its own row
            fused_ms, fused_mem = timed(lambda: hip.topk_scores(h, table, K, 1, C), args.warmup, args.iters)
            rank_ms, _ = timed(lambda: hip.topk_scores(h, table, K, 1, C, target=target), args.warmup, args.iters)
            fused_mem += hip._tn_workspace(h.device, 0, "topk").numel() * 4          # the cached workspace is allocated before the timed loop
            table_bytes = C * d * table.element_size()
            row = {"shape": name, "items": C, "d": d, "B": B, "K": K, "tier": tier, "fused_topk_ms": fused_ms, "fused_topk_and_rank_ms": rank_ms,
                   "table_bytes": table_bytes, "fused_table_GBps": table_bytes / fused_ms / 1e6, "hbm_read_only_GBps_r06": peak,
                   "fused_peak_bytes": int(fused_mem), "dense_scores_bytes": B * C * 4}
            dense_need = B * C * 4 * 3                                               # scores + torch.topk's scratch
            if dense_need < 0.6 * free_total:
                cat = table[1:C + 1]

                def dense():
                    s = hip.gemm_nt(h, cat, out_f32=True)
                    return torch.topk(s, K, dim=1)
                dense_ms, dense_mem = timed(dense, args.warmup, args.iters)
                row.update(dense_gemm_topk_ms=dense_ms, dense_peak_bytes=int(dense_mem), fused_not_slower=bool(fused_ms <= dense_ms))
            else:
                row.update(dense_gemm_topk_ms=None, dense_peak_bytes=None, fused_not_slower=None,
                           note="the dense [B, C] f32 matrix and torch.topk's scratch do not fit: only the fused path runs")
            hip.SPLIT_OPERANDS = False
            cases.append(row)
            print(json.dumps(row), flush=True)
            del h, table
            torch.cuda.empty_cache()
    fits = [c for c in cases if c["dense_gemm_topk_ms"] is not None]
    slower = [c for c in fits if not c["fused_not_slower"]]
    finding = ("the fused pass is SLOWER than gemm_nt + torch.topk in %d of the %d cases where the dense matrix fits (%s x the dense time); "
               "it runs in %s x less memory" % (len(slower), len(fits),
                                                " / ".join("%.1f" % (c["fused_topk_ms"] / c["dense_gemm_topk_ms"]) for c in fits),
                                                " / ".join("%.0f" % (c["dense_peak_bytes"] / max(c["fused_peak_bytes"], 1)) for c in fits)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "finding": finding, "cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
