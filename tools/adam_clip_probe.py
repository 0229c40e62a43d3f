"""Timing probe of the optimizer options (csrc/optim.hip) against the plain step of the same run:

  python tools/adam_clip_probe.py [--sets gen,table] [--out profiles/adamw/probe.txt]

  gen     the parameters of the bench-shape generator (MyAuto4Rec_c: L = 200, d = 128, H = 4, N = 3, 100 000 items per domain)
  table   one 2 000 000 x 256 table

Variants, every parameter with a randn gradient: plain (rg_adam_multi_dev), decay (rg_adam_multi_dev2, coupled weight decay),
decoupled (the AdamW form), clip (rg_grad_sqnorm_multi + rg_adam_multi_dev2 reading the control record), and the norm's two
launches alone.  Two groups of figures, each the median of --reps HIP-event timings after --warmup untimed calls: the launches alone,
every variant over ONE optimizer's device table (the same buffers), and Adam.step() as the drivers call it (host work included; one
optimizer, with its own moment buffers, per variant).  The byte model beside them: the update
reads p, g, m, v and writes p, m, v (7 f32 accesses per element), the norm pass reads g once more (8 / 7 = 1.143 of the plain step)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def gen_params():
    from recguru_amd import config, models
    a = argparse.Namespace(date="probe", d_model=128, n_head=4, d_ff=512, n_negs=30, decoder_neg=True, fix_enc=True, lr=0.01,
                           batch_size=4096, batch_size_val=256, dataset_pick=1, run=1, target_domain="a", cross="True", sas="False",
                           result_path="/tmp/rg_probe", seq_len=200, vocab_size_a=100000, vocab_size_b=100000, n_blocks=3, dropout=0.5)
    torch.manual_seed(0)
    G = models.MyAuto4Rec_c("cuda", config.get_param(a, make_dirs=False), wf=None, enc_share=True, dec_rec=False).to(torch.float32).cuda()
    return list(G.parameters())


def probe(name, params, reps, warmup, lines):
    from recguru_amd import hip
    from recguru_amd.optim import Adam
    g = torch.Generator(device="cuda").manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, device="cuda", generator=g) * 1e-2
    n = sum(p.numel() for p in params)
    lines.append("%s: %d parameters, %d elements (%.1f MB of f32 each for p, g, m, v)" % (name, len(params), n, n * 4 / 1e6))
    lr, b1, b2, eps = 1e-4, 0.9, 0.98, 1e-9
    variants = [("plain", {}), ("decay", dict(weight_decay=0.01)), ("decoupled", dict(weight_decay=0.01, decoupled=True)),
                ("clip", dict(max_norm=1.0)), ("clip+decay+skip", dict(max_norm=1.0, weight_decay=0.01, skip_nonfinite=True))]
    # the launches, all over ONE table (the same p, g, m, v buffers: differences are the kernels', not the allocator's)
    opt = Adam(params, lr=lr, betas=(b1, b2), eps=eps, max_norm=1.0, weight_decay=0.01, skip_nonfinite=True)
    opt.step()                                              # builds the device table, the moments and the control record
    c, ctl = opt._tables["all"], opt._ctl
    norm = lambda skip=False: hip.grad_sqnorm_multi(c["dev"], c["n"], c["partial"], ctl, 1.0, skip)
    upd = lambda wd=0.0, dec=False, k=None: hip.adam_multi_dev2(c["dev"], c["n"], lr, b1, b2, eps, wd, dec, k)
    launches = [("plain", lambda: hip.adam_multi_dev(c["dev"], c["n"], lr, b1, b2, eps), 7),
                ("dev2, neutral", lambda: upd(), 7),
                ("decay", lambda: upd(0.01), 7),
                ("decoupled", lambda: upd(0.01, True), 7),
                ("norm alone", lambda: norm(), 1),
                ("clip", lambda: (norm(), upd(0.0, False, ctl)), 8),
                ("clip+decay+skip", lambda: (norm(True), upd(0.01, False, ctl)), 8),
                ("plain (again)", lambda: hip.adam_multi_dev(c["dev"], c["n"], lr, b1, b2, eps), 7)]
    t_plain = None
    for vname, fn, acc in launches:
        t = timed(fn, reps, warmup)
        t_plain = t_plain or t
        lines.append("  launches  %-16s %8.3f ms  x%.3f of plain (byte model x%.3f; %6.0f GB/s of its %d f32 accesses per element; %d segments)"
                     % (vname, t, t / t_plain, acc / 7.0, n * 4 * acc / t / 1e6, acc, c["n"]))
    del opt, c, ctl
    torch.cuda.empty_cache()
    # Adam.step() as the drivers call it, one optimizer (with its own moments) per variant
    t_plain = None
    for vname, kw in variants:
        opt = Adam(params, lr=lr, betas=(b1, b2), eps=eps, **kw)
        opt.step()
        t = timed(opt.step, reps, warmup)
        t_plain = t_plain or t
        lines.append("  step()    %-16s %8.3f ms  x%.3f of plain" % (vname, t, t / t_plain))
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
    lines.append("# tools/adam_clip_probe.py --sets %s | %s; median of %d device-event timings after %d untimed calls"
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
