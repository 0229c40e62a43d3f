"""Subprocess side of tests/test_full_softmax_gpu.py (a fresh process per library / process group).

  python tests/full_softmax_worker.py det <out.npz>       two forward + backward runs of the full softmax loss (bf16x3, then bf16):
                                                          loss, dh and dW of both runs (RG_DETERMINISTIC from the environment)
  python tests/full_softmax_worker.py dp <out.npz>        one data-parallel rank (RANK / WORLD_SIZE / MASTER_* from the env, gloo,
                                                          every rank on GPU 0): the rows rank::world of the problem, global mask
                                                          count, dW SUM-all-reduced; rank 0 writes loss, its dh rows and dW
  python tests/full_softmax_worker.py one <out.npz>       the same problem in one process
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def problem(B=64, L=50, d=128, C=3001, seed=5, device="cuda"):
    """Decoder states [B, L, d], a weight [C, d], labels and a ragged left-padded mask (lengths U{3..L})."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(B, L, d, generator=g) * 0.5
    w = torch.randn(C, d, generator=g) * 0.2
    lab = torch.randint(1, C, (B, L), generator=g)
    lens = torch.randint(3, L + 1, (B,), generator=g)
    mask = (torch.arange(L)[None, :] >= (L - lens)[:, None]).to(torch.float32)
    lab = lab * mask.long()
    return h.to(device), w.to(device), lab.to(device), mask.reshape(-1).to(device)


def run(h, w, lab, mask):
    from recguru_amd import ops
    hh = h.to(ops.compute_dtype()).detach().requires_grad_(True)
    wp = torch.nn.Parameter(w.clone())
    loss = ops.full_softmax_loss(hh, wp, lab, mask)
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
                res["loss.%s.%d" % (tier, r)], res["dh.%s.%d" % (tier, r)], res["dw.%s.%d" % (tier, r)] = run(*prob)
        from recguru_amd import hip
        res["det_fault"] = np.array(hip.det_fault() if hip.DETERMINISTIC else 0)
    else:
        ops.set_compute_dtype("bf16x3")
        h, w, lab, mask = problem()
        if mode == "dp":
            import torch.distributed as dist
            from recguru_amd import dist as rdist
            dp = rdist.init_from_env("gloo")
            ops.set_data_parallel(dp)
            sl = slice(dp.rank, None, dp.world)
            h, lab, mask = h[sl].contiguous(), lab[sl].contiguous(), mask.view(h.shape[0], -1)[sl].reshape(-1).contiguous()
            loss, dh, dw = run(h, w, lab, mask)
            t = torch.tensor([loss], dtype=torch.float64)
            dist.all_reduce(t)
            g = torch.as_tensor(dw)
            dist.all_reduce(g)
            loss, dw = float(t[0]), g.numpy()
            ops.set_data_parallel(None)
            if dp.rank != 0:
                dist.barrier()
                return
            dist.barrier()
        else:
            loss, dh, dw = run(h, w, lab, mask)
        res.update(loss=np.array(loss), dh=dh, dw=dw)
    np.savez(out, **res)


if __name__ == "__main__":
    main()
