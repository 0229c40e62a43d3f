"""Timing probe of the position-table gradient (rg_pos_grad, csrc/elementwise.hip):

  python tools/pos_grad_probe.py [--out profiles/pos_train/probe.txt] [--no_step]

  kernels   the two launches of rg_pos_grad together, beside rg_embed_scatter_bwd and its binned form over the same dx, mask and
            dropout seed, at the bench shape (B 4096, L 200, d 128) and at config 5's (B 1024, L 400, d 256): bf16, p = 0.5, the
            bench's padding pattern (recguru_amd.synthetic lengths, left padding).  The variants alternate inside every round; each
            figure is the median (and the minimum) over --rounds rounds of a HIP-event timing of --calls back-to-back calls.
  bytes     what the pair must move -- the live dx rows, the mask, the partial rows written and read back, dP read and written --
            and the rate that makes, beside the box's read-stream ceiling (profiles/r06: 7.19 TB/s).
  step      one auto_training reconstruction step (MyRec, bench shape, bf16, dropout 0.5) with pos_train off and on, alternated
            in one process; the spread of the off variant over its repeats stands beside the difference.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CEILING = 7.19e12            # bytes / s, read stream (profiles/r06)


class _Lines(list):
    def append(self, s):
        list.append(self, s)
        print(s, flush=True)


def event_us(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3


def alternate(variants, rounds, calls, warmup=2):
    for _, fn in variants:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            ts[name].append(event_us(fn, calls))
    return ts


def kernels(B, L, d, V, rounds, calls, lines):
    from recguru_amd import hip, synthetic
    dom = synthetic.make_domain(B, V, L, 1, seed=1)
    ids = torch.as_tensor(dom["enc_in"]).cuda().reshape(-1).contiguous()
    mask = (ids != 0).float()
    ntok, nlive = B * L, float(mask.sum())
    dx = (torch.randn(ntok, d, device="cuda") * 0.3).to(torch.bfloat16)
    dE = torch.zeros(V + 2, d, device="cuda")
    dP = torch.zeros(L, d, device="cuda")
    p, seed = 0.5, 5
    slices = hip.pos_grad_workspace(B, L, d) // (L * d * 4)
    variants = [("pos_grad (2 launches)", lambda: hip.pos_grad(dx, mask, dP, B, L, p, seed)),
                ("embed_scatter_bwd", lambda: hip.embed_scatter_bwd(dx, ids, mask, dE, 0, p, seed))]
    if hip.embed_scatter_binned_supported(ntok, d, dE.shape[0]):
        variants.append(("embed_scatter_bwd_binned", lambda: hip.embed_scatter_bwd_binned(dx, ids, mask, dE, 0, p, seed)))
    ts = alternate(variants, rounds, calls)
    lines.append("B %d  L %d  d %d  bf16  p %.1f  live positions %.1f %%  batch slices %d (partials %.1f MB)"
                 % (B, L, d, p, 100 * nlive / ntok, slices, slices * L * d * 4 / 1e6))
    for name, _ in variants:
        lines.append("  %-28s median %8.1f us   min %8.1f us" % (name, np.median(ts[name]), np.min(ts[name])))
    by_dx, by_mask, by_part, by_dp = nlive * d * 2, ntok * 4, 2.0 * slices * L * d * 4, 2.0 * L * d * 4
    by = by_dx + by_mask + by_part + by_dp
    t = float(np.median(ts["pos_grad (2 launches)"])) * 1e-6
    lines.append("  bytes the pair must move: live dx rows %.1f MB + mask %.1f MB + partials written and read %.1f MB + dP %.2f MB = %.1f MB"
                 % (by_dx / 1e6, by_mask / 1e6, by_part / 1e6, by_dp / 1e6, by / 1e6))
    lines.append("  -> %.2f TB/s = %.2f of the %.2f TB/s read-stream ceiling; at the ceiling the pair would take %.1f us"
                 % (by / t / 1e12, by / t / CEILING, CEILING / 1e12, by / CEILING * 1e6))
    r = float(np.median(ts["pos_grad (2 launches)"])) / float(np.median(ts["embed_scatter_bwd"]))
    lines.append("  pos_grad / embed_scatter_bwd = %.2f" % r)


def step_cost(rounds, steps, lines):
    from recguru_amd import auto_training as at, blocks, config, models, ops, synthetic
    from recguru_amd.optim import Adam
    B, L, d, H, N, V, k = 4096, 200, 128, 4, 3, 100000, 30
    ops.set_compute_dtype(torch.bfloat16)
    dom = synthetic.make_domain(B, V, L, k, seed=1)
    enc_in, dec_in, dec_out, n_items = (torch.as_tensor(dom[n]).cuda() for n in ("enc_in", "dec_in", "dec_out", "n_items"))
    mask = (dec_in != 0).view(-1).float()
    fns = {}
    for pos_train in (False, True):
        a = argparse.Namespace(date="probe", d_model=d, n_head=H, d_ff=512, n_negs=k, decoder_neg=True, fix_enc=False, lr=0.01, batch_size=B,
                               batch_size_val=256, dataset_pick=1, run=1, target_domain="a", cross="False", sas="False",
                               result_path="/tmp/rg_probe", seq_len=L, vocab_size_a=V, vocab_size_b=V, n_blocks=N, dropout=0.5,
                               pos_train=pos_train)
        param = config.get_param(a, make_dirs=False)
        torch.manual_seed(0)
        R = models.MyRec("cuda", param, None, dec_rec=False, fix_enc=False, sas=False, pos_train=param.pos_train).to(torch.float32).cuda()
        R.train()
        opt = blocks.ScheduledOptim(Adam(R.parameters(), betas=(0.9, 0.99), eps=1e-09), 1.0, d, 1000)

        def step(R=R, opt=opt, param=param):
            opt.zero_grad()
            loss = at.loss_ae(R, enc_in, dec_in, dec_out, n_items, True, B, L, param, mask)
            loss.backward()
            opt.step_and_update_lr()
        fns["pos_train on" if pos_train else "pos_train off"] = step
    ts = alternate(list(fns.items()), rounds, steps, warmup=3)
    off, on = np.array(ts["pos_train off"]) / 1e3, np.array(ts["pos_train on"]) / 1e3
    lines.append("auto_training reconstruction step, B %d  L %d  d %d  N %d  bf16  dropout 0.5, %d rounds of %d steps, variants alternated:"
                 % (B, L, d, N, rounds, steps))
    lines.append("  pos_train off  median %8.3f ms   min %8.3f   max %8.3f   (spread of its repeats %.3f ms)"
                 % (np.median(off), off.min(), off.max(), off.max() - off.min()))
    lines.append("  pos_train on   median %8.3f ms   min %8.3f   max %8.3f" % (np.median(on), on.min(), on.max()))
    lines.append("  on - off (medians) %+.3f ms = %+.2f %%" % (np.median(on) - np.median(off), 100 * (np.median(on) / np.median(off) - 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--step_rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no_step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = _Lines()
    lines.append("# tools/pos_grad_probe.py | %s; HIP-event timings, %d rounds of %d calls, variants alternated inside a round"
                 % (torch.cuda.get_device_name(0), a.rounds, a.calls))
    kernels(4096, 200, 128, 100000, a.rounds, a.calls, lines)
    kernels(1024, 400, 256, 2000000, a.rounds, a.calls, lines)
    if not a.no_step:
        step_cost(a.step_rounds, a.steps, lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
