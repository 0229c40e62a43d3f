"""Timing probe of the weight average the Adam update keeps (rg_adam_multi_dev3 / rg_ema_swap_multi in csrc/optim.hip)
against the update without it, in the same run:

  python tools/ema_probe.py [--sets gen,table] [--out profiles/ema/probe.txt]

  gen     the parameters of the bench-shape generator (MyAuto4Rec_c: L = 200, d = 128, H = 4, N = 3, 100 000 items per domain)
  table   one 2 000 000 x 256 table

The two parameter sets and the timing method are tools/adam_clip_probe.py's (its "plain" line in profiles/adamw/probe.txt is the
yardstick the option-off launch of this run is held against).  Every parameter has a randn gradient.  Two groups of figures, each the
median of --reps HIP-event timings after --warmup untimed calls: the launches alone, every variant over ONE optimizer's device table
(the same p, g, m, v and average buffers), and Adam.step() / swap_ema() as the drivers call them (host work included).  The byte model
beside them: the update reads p, g, m, v and writes p, m, v (7 f32 accesses per element); the fused average reads and writes e on top
(9 / 7 = 1.286); a SEPARATE pass would read p and e and write e (10 / 7 = 1.429, and a launch); a swap reads and writes both buffers
(4 accesses)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from adam_clip_probe import _Lines, gen_params, timed  # noqa: E402


def probe(name, params, reps, warmup, lines):
    from recguru_amd import hip
    from recguru_amd.optim import Adam
    g = torch.Generator(device="cuda").manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, device="cuda", generator=g) * 1e-2
    n = sum(p.numel() for p in params)
    lines.append("%s: %d parameters, %d elements (%.1f MB of f32 each for p, g, m, v and the average)" % (name, len(params), n, n * 4 / 1e6))
    lr, b1, b2, eps = 1e-4, 0.9, 0.98, 1e-9
    # the launches, all over ONE table and ONE set of averages (differences are the kernels', not the allocator's)
    opt = Adam(params, lr=lr, betas=(b1, b2), eps=eps, max_norm=1.0, weight_decay=0.01, skip_nonfinite=True, ema_decay=0.999, ema_warmup=True)
    opt.step()                                              # builds the device tables, the moments, the averages and the control record
    c, ctl = opt._tables["all"], opt._ctl
    opt.swap_ema()
    opt.swap_ema()                                          # builds the pair table
    pr = opt._pairs
    norm = lambda: hip.grad_sqnorm_multi(c["dev"], c["n"], c["partial"], ctl, 1.0, True)
    off = lambda wd=0.0, k=None: hip.adam_multi_dev2(c["dev"], c["n"], lr, b1, b2, eps, wd, False, k)
    on = lambda wd=0.0, k=None, d=0.999, w=False: hip.adam_multi_dev3(c["dev"], c["ema"], c["n"], lr, b1, b2, eps, wd, False, k, d, w)
    launches = [("plain", lambda: hip.adam_multi_dev(c["dev"], c["n"], lr, b1, b2, eps), 7),
                ("off (dev2)", lambda: off(), 7),
                ("ema (dev3)", lambda: on(), 9),
                ("ema, warm-up", lambda: on(w=True), 9),
                ("ema, decay 0", lambda: on(d=0.0), 9),
                ("off, clip+decay", lambda: (norm(), off(0.01, ctl)), 8),
                ("ema, clip+decay", lambda: (norm(), on(0.01, ctl)), 10),
                ("swap", lambda: hip.ema_swap_multi(pr["dev"], pr["n"]), 4),
                ("swap (back)", lambda: hip.ema_swap_multi(pr["dev"], pr["n"]), 4),
                ("off (again)", lambda: off(), 7),
                ("plain (again)", lambda: hip.adam_multi_dev(c["dev"], c["n"], lr, b1, b2, eps), 7)]
    t_off = None
    for vname, fn, acc in launches:
        t = timed(fn, reps, warmup)
        if vname == "off (dev2)":
            t_off = t
        rel = "" if t_off is None else "  x%.3f of off (byte model x%.3f; a separate averaging pass: x%.3f)" % (t / t_off, acc / 7.0, 10.0 / 7.0)
        lines.append("  launches  %-16s %8.3f ms%s  %6.0f GB/s of its %d f32 accesses per element; %d segments"
                     % (vname, t, rel, n * 4 * acc / t / 1e6, acc, c["n"]))
    del opt, c, ctl, pr
    torch.cuda.empty_cache()
    # Adam.step() and swap_ema() as the drivers call them, one optimizer (with its own moments) per variant
    t_off = None
    for vname, kw in (("off", {}), ("ema", dict(ema_decay=0.999)), ("ema, warm-up", dict(ema_decay=0.999, ema_warmup=True)),
                      ("off, clip+decay", dict(max_norm=1.0, weight_decay=0.01)),
                      ("ema, clip+decay", dict(max_norm=1.0, weight_decay=0.01, ema_decay=0.999)), ("off (again)", {})):
        opt = Adam(params, lr=lr, betas=(b1, b2), eps=eps, **kw)
        opt.step()
        t = timed(opt.step, reps, warmup)
        t_off = t_off or t
        lines.append("  step()    %-16s %8.3f ms  x%.3f of off" % (vname, t, t / t_off))
        if vname == "ema":
            opt.swap_ema()
            opt.swap_ema()
            ts = timed(opt.swap_ema, 2 * (reps // 2), 2 * (warmup // 2 + 1))          # an even number of swaps: the weights are back
            lines.append("  swap_ema()                 %8.3f ms  x%.3f of off (bump and refresh_shadows included; no cached copies here)" % (ts, ts / t_off))
        del opt
        torch.cuda.empty_cache()
    for p in params:
        p.grad = None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="gen,table")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = _Lines()
    lines.append("# tools/ema_probe.py --sets %s | %s; median of %d device-event timings after %d untimed calls"
                 % (a.sets, torch.cuda.get_device_name(0), a.reps, a.warmup))
    for s in a.sets.split(","):
        if s == "gen":
            probe("gen (bench-shape generator)", gen_params(), a.reps, a.warmup, lines)
        elif s == "table":
            probe("table (2 000 000 x 256)", [torch.nn.Parameter(torch.randn(2000000, 256, device="cuda") * 0.1)], a.reps, a.warmup, lines)
        else:
            sys.exit("unknown set %r" % s)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
