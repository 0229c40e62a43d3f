"""Timing probe of the attention-map kernel (rg_attn_probs, csrc/attention_map.hip) beside a plain device fill of the
same number of output bytes, in the same run:

  python tools/attn_map_probe.py [--out profiles/attn_maps/probe.txt]

Per shape -- (B 256, L 200, H 4), the bench model's slice, and (B 8, L 2048, H 4) -- and tier (bf16, f32, bf16x3), both masks: HIP
events, median of 21 calls after 3, kernel and fill alternated call by call.  Reported: time, output bytes over time, that rate as
a share of the write ceiling measured on this kind of device (profiles/r06/peaks.txt: hbm_write_best), and the ratio to the fill.
Also the cross-map fill and the rollout at the same shapes (one number each).  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from recguru_amd import hip, ops  # noqa: E402

REPS, WARMUP = 21, 3


def write_ceiling():
    with open(os.path.join(ROOT, "profiles", "r06", "peaks.txt")) as f:
        last = [ln for ln in f.read().splitlines() if ln.startswith("{")][-1]
    return float(json.loads(last)["hbm_write_best"]["value"])


def timed_pair(fa, fb):
    """medians (ms) of fa and fb, alternated call by call"""
    ta, tb = [], []
    for i in range(WARMUP + REPS):
        for fn, acc in ((fa, ta), (fb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= WARMUP:
                acc.append(e0.elapsed_time(e1))
    return statistics.median(ta), statistics.median(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_map_probe: needs a GPU")
    peak = write_ceiling()
    lines = ["# tools/attn_map_probe.py: HIP events, median of %d calls after %d, kernel and fill alternated; one %s"
             % (REPS, WARMUP, torch.cuda.get_device_name(0) or "device"),
             "# share = output GB/s over hbm_write_best = %.1f GB/s (profiles/r06/peaks.txt); fill = torch fill_ of the same [B,H,L,L] f32 tensor" % peak]
    for B, L, H in ((256, 200, 4), (8, 2048, 4)):
        nbytes = 4.0 * B * H * L * L
        ids = torch.randint(1, 1000, (B, L), device="cuda", dtype=torch.int64)
        lens = torch.randint(L // 4, L + 1, (B,), device="cuda")
        ids[torch.arange(L, device="cuda")[None, :] < (L - lens)[:, None]] = 0           # left padding
        out = torch.empty(B, H, L, L, device="cuda", dtype=torch.float32)
        for tier, dt in (("bf16", torch.bfloat16), ("f32", torch.float32), ("bf16x3", "bf16x3")):
            ops.set_compute_dtype(dt)
            qkv = torch.randn(B, L, 3 * H * 32, device="cuda").to(ops.compute_dtype())
            for causal in (False, True):
                ms, fill = timed_pair(lambda: hip.attn_probs(qkv, ids, 0, H, causal, out=out), lambda: out.fill_(0.25))
                gbs = nbytes / ms / 1e6
                lines.append("attn_probs  %-6s B=%-3d L=%-4d H=%d %-10s %8.3f ms  %7.1f GB/s out  %5.1f %% of the write ceiling | fill %7.3f ms  ratio %.2f"
                             % (tier, B, L, H, "causal" if causal else "non-causal", ms, gbs, 100.0 * gbs / peak, fill, ms / fill))
        ops.set_compute_dtype(torch.bfloat16)
        ms, fill = timed_pair(lambda: hip.attn_cross_probs(ids, 0, H, out=out), lambda: out.fill_(0.25))
        lines.append("attn_cross_probs   B=%-3d L=%-4d H=%d            %8.3f ms  %7.1f GB/s out  %5.1f %% of the write ceiling | fill %7.3f ms  ratio %.2f"
                     % (B, L, H, ms, nbytes / ms / 1e6, 100.0 * nbytes / ms / 1e6 / peak, fill, ms / fill))
        qkv = torch.randn(B, L, 3 * H * 32, device="cuda").to(torch.bfloat16)
        maps = torch.empty(B, 2, H, L, L, device="cuda", dtype=torch.float32)
        for causal in (False, True):
            for layer in range(2):
                hip.attn_probs(qkv, ids, 0, H, causal, out=maps, layer=layer)
            ms, fill = timed_pair(lambda: hip.attn_rollout(maps), lambda: out.fill_(0.25))
            lines.append("attn_rollout       B=%-3d L=%-4d H=%d N=2 %-10s %8.3f ms  (%.1f MB of maps; reads only the rows with r[q] != 0)"
                         % (B, L, H, "causal" if causal else "non-causal", ms, 2 * nbytes / 1e6))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
