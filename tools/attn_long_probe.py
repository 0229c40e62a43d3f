"""Probe (not a test): what a (query, key) pair costs in the streaming attention core (csrc/attention_long.hip, L > 416)
against the resident kernels at L = 416 in the same run.

bf16 tier, H = 4, token-major qkv, full-length sequences (no padding, no row mask), non-causal, B * L ~ 819 200 tokens
(the bench shape's token count).  hip.attn_fwd and hip.attn_bwd are timed with device events: 3 warm-up calls, then the
median of 21 calls.  Prints, per length and dropout rate, the milliseconds per call and the picoseconds per executed
(query, key) pair = time / (B * H * L * L), and the ratio of the latter to the L = 416 row.

  python tools/attn_long_probe.py [out.txt]
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recguru_amd import hip          # noqa: E402

H, TOKENS, WARM, RUNS = 4, 819200, 3, 21
P = H * 32


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("attn_long_probe: no GPU (a timing needs one)")
    lines = ["# %s | H = %d, B * L ~ %d tokens, bf16, non-causal, median of %d runs after %d warm-up calls (min .. max in brackets)"
             % (torch.cuda.get_device_name(0), H, TOKENS, RUNS, WARM),
             "# %5s %5s %4s | %22s %9s %6s | %22s %9s %6s" % ("L", "B", "p", "fwd ms", "ps/pair", "x416", "bwd ms", "ps/pair", "x416")]
    base = {}
    for L in (416, 448, 1024, 2048):
        B = max(1, round(TOKENS / L))
        g = torch.Generator(device="cuda").manual_seed(L)
        qkv = (torch.randn(B, L, 3 * P, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
        dctx = (torch.randn(B, L, P, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
        ids = torch.ones(B, L, dtype=torch.int64, device="cuda")
        pairs = float(B) * H * L * L
        for p in (0.0, 0.5):
            kw = dict(drop_p=p, seed=7)
            ctx, lse = hip.attn_fwd(qkv, ids, 0, False, H, **kw)
            f = timed(lambda: hip.attn_fwd(qkv, ids, 0, False, H, **kw))
            b = timed(lambda: hip.attn_bwd(qkv, dctx, ctx, lse, ids, 0, False, H, **kw))
            fp, bp = f[0] * 1e9 / pairs, b[0] * 1e9 / pairs
            if L == 416:
                base[p] = (fp, bp)
            lines.append("  %5d %5d %4.1f | %7.3f [%6.3f..%6.3f] %9.3f %6.2f | %7.3f [%6.3f..%6.3f] %9.3f %6.2f"
                         % (L, B, p, f[0], f[1], f[2], fp, fp / base[p][0], b[0], b[1], b[2], bp, bp / base[p][1]))
        del qkv, dctx, ctx, lse
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
