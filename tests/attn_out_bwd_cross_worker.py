"""The decoder-layer runs of tests/test_attn_out_bwd_cross_gpu.py: DecoderLayerFn forward + backward with the fused attention-tail
backward (ops.FUSE_ATTN_OUT_BWD_CROSS) off, on and on again, on the same weights, inputs and dropout seeds.

  python tests/attn_out_bwd_cross_worker.py <out.pt>    all four cases (bf16 / bf16x3 x p = 0 / 0.5) in this process -- started with
                                                        RG_DETERMINISTIC=1 by the test -- saved as CPU tensors
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))

LENS = (40, 17, 16, 1, 0)          # live lengths of the B = 5 left-padded sequences of L = 40


def _layer_params(d, H, dff, seed):
    g = torch.Generator().manual_seed(seed)
    P = H * 32
    r = lambda *s, sc=1.0: torch.nn.Parameter((torch.randn(*s, generator=g) * sc).cuda())
    ln = lambda: [torch.nn.Parameter((1 + 0.1 * torch.randn(d, generator=g)).cuda()), torch.nn.Parameter((0.1 * torch.randn(d, generator=g)).cuda())]
    att = [r(P, d, sc=d ** -0.5), r(P, sc=0.1), r(P, d, sc=d ** -0.5), r(P, sc=0.1), r(P, d, sc=d ** -0.5), r(P, sc=0.1), r(d, P, sc=P ** -0.5), r(d, sc=0.1)] + ln()
    cross = [r(P, d, sc=d ** -0.5), r(P, sc=0.1), r(d, P, sc=P ** -0.5), r(d, sc=0.1)] + ln()
    ffn = [r(dff, d, sc=d ** -0.5), r(dff, sc=0.1), r(d, dff, sc=dff ** -0.5), r(d, sc=0.1)] + ln()
    return att + cross + ffn


def run_case(tier, drop_p):
    """[out, dx, du, parameter gradients ...] of the three runs (flag off, on, on)."""
    from recguru_amd import ops
    d, H, dff, B, L = 128, 4, 512, 5, 40
    prev = ops.FUSE_ATTN_OUT_BWD_CROSS
    try:
        ops.set_compute_dtype(torch.bfloat16 if tier == "bf16" else tier)
        dt = ops.compute_dtype()
        g0 = torch.Generator().manual_seed(5)
        ids = torch.zeros(B, L, dtype=torch.long)
        for b, n in enumerate(LENS):
            ids[b, L - n:] = torch.randint(1, 5000, (n,), generator=g0)            # left-padded
        ids = ids.cuda()
        rowmask = (ids != 0).float()
        x0 = (torch.randn(B, L, d, generator=g0) * 0.7).cuda() * rowmask[..., None]
        u0 = (torch.randn(B, d, generator=g0) * 0.7).cuda()
        gout = (torch.randn(B, L, d, generator=g0) * 0.1).cuda() * rowmask[..., None]
        res = []
        for fused in (False, True, True):
            ops.FUSE_ATTN_OUT_BWD_CROSS = fused
            prm = _layer_params(d, H, dff, 77)
            x = x0.to(dt).requires_grad_(True)
            u = u0.to(dt).requires_grad_(True)
            ops.manual_seed(123)
            with ops.masked_input(True):
                out = ops.DecoderLayerFn.run(x, u, ids, ids, rowmask, H, drop_p, *prm)
            out.backward(gout.to(out.dtype))
            torch.cuda.synchronize()
            res.append([out.detach(), x.grad, u.grad] + [None if p.grad is None else p.grad.clone() for p in prm])
    finally:
        ops.FUSE_ATTN_OUT_BWD_CROSS = prev
        ops.set_compute_dtype(torch.bfloat16)
    return res


def main():
    from recguru_amd import hip
    torch.cuda.set_device(0)
    out = {}
    for tier in ("bf16", "bf16x3"):
        for p in (0.0, 0.5):
            out["%s/%g" % (tier, p)] = [[None if t is None else t.cpu() for t in run] for run in run_case(tier, p)]
    out["det_enabled"] = int(hip.lib().rg_det_enabled())
    out["det_fault"] = int(hip.det_fault()) if hip.DETERMINISTIC else -1
    torch.save(out, sys.argv[1])


if __name__ == "__main__":
    main()
