"""Subprocess side of tests/test_shared_ce_gpu.py (a fresh process per library / process group).

  python tests/shared_ce_worker.py det <out.npz>       two forward + backward runs of the shared-candidate softmax loss (bf16x3, then
                                                       bf16): loss, dh and the whole table gradient of both runs (RG_DETERMINISTIC
                                                       from the environment)
  python tests/shared_ce_worker.py dp <out.npz>        one data-parallel rank (RANK / WORLD_SIZE / MASTER_* from the env, gloo, every
                                                       rank on GPU 0): the sequences rank::world of the problem with the SAME candidate
                                                       list, global mask count, table gradient SUM-all-reduced; rank 0 writes the
                                                       rank-summed loss, its dh rows and the table gradient
  python tests/shared_ce_worker.py one <out.npz>       the same problem in one process
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def problem(B=64, L=50, d=128, rows=3001, C=257, seed=5, device="cuda"):
    """Decoder states [B, L, d], a table [rows, d], targets, a sorted candidate list that holds some of the targets and a ragged
    left-padded mask (lengths U{3..L})."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(B, L, d, generator=g) * 0.5
    w = torch.randn(rows, d, generator=g) * 0.2
    lab = torch.randint(1, rows, (B, L), generator=g)
    lens = torch.randint(3, L + 1, (B,), generator=g)
    mask = (torch.arange(L)[None, :] >= (L - lens)[:, None]).to(torch.float32)
    lab = lab * mask.long()
    cand = torch.sort(torch.randperm(rows, generator=g)[:C])[0]
    return h.to(device), w.to(device), lab.to(device), cand.to(device), mask.reshape(-1).to(device)


def run(h, w, lab, cand, mask):
    from recguru_amd import ops
    hh = h.to(ops.compute_dtype()).detach().requires_grad_(True)
    wp = torch.nn.Parameter(w.clone())
    loss = ops.shared_softmax_loss(hh, wp, lab, cand, mask, skip_row=0)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss), hh.grad.float().cpu().numpy(), wp.grad.cpu().numpy()


def main():
    from recguru_amd import ops
    mode, out = sys.argv[1], sys.argv[2]
    torch.cuda.set_device(0)
    res = {}
    if mode == "det":
        for tier in ("bf16x3", "bf16"):
            ops.set_compute_dtype(tier)
            prob = problem()
            for r in range(2):
                res["loss.%s.%d" % (tier, r)], res["dh.%s.%d" % (tier, r)], res["dE.%s.%d" % (tier, r)] = run(*prob)
        from recguru_amd import hip
        res["det_fault"] = np.array(hip.det_fault() if hip.DETERMINISTIC else 0)
    else:
        ops.set_compute_dtype("bf16x3")
        h, w, lab, cand, mask = problem()
        if mode == "dp":
            import torch.distributed as dist
            from recguru_amd import dist as rdist
            dp = rdist.init_from_env("gloo")
            ops.set_data_parallel(dp)
            sl = slice(dp.rank, None, dp.world)
            h, lab, mask = h[sl].contiguous(), lab[sl].contiguous(), mask.view(h.shape[0], -1)[sl].reshape(-1).contiguous()
            loss, dh, dE = run(h, w, lab, cand, mask)
            t = torch.tensor([loss], dtype=torch.float64)
            dist.all_reduce(t)
            g = torch.as_tensor(dE)
            dist.all_reduce(g)
            loss, dE = float(t[0]), g.numpy()
            ops.set_data_parallel(None)
            if dp.rank != 0:
                dist.barrier()
                return
            dist.barrier()
        else:
            loss, dh, dE = run(h, w, lab, cand, mask)
        res.update(loss=np.array(loss), dh=dh, dE=dE)
    np.savez(out, **res)


if __name__ == "__main__":
    main()
