"""One process of tests/test_topk_gpu.py::test_repeat_and_batch_split_invariance.  Run with RG_DETERMINISTIC=1 (librecguru_hip_det.so)
or without (librecguru_hip.so): the random fixture's 37 users at C = 4099, d = 128, K = 100 in every tier as one call, the same call
again, and as calls of 5 + 16 + 16 users; writes ids / scores / rank of each to argv[1].

  python tests/topk_worker.py <out.npz>
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    out_path = sys.argv[1]
    from recguru_amd import hip, ops
    import topk_ref as R
    from test_topk_gpu import TIERS, random_case
    torch.cuda.set_device(0)
    B, C, d, K = 37, 4099, 128, 100
    out = {}
    for tier in TIERS:
        ops.set_compute_dtype({"bf16": torch.bfloat16, "bf16x3": "bf16x3", "f32": torch.float32}[tier])
        dtype = torch.bfloat16 if tier == "bf16" else torch.float32
        hn, wn, target, rows, _, _ = random_case(B, C, d, tier)
        h, table, tg = torch.as_tensor(hn).cuda().to(dtype), torch.as_tensor(wn).cuda().to(dtype), torch.as_tensor(target).cuda()

        def run(b0, b1):
            v, o = R.csr(rows[b0:b1])
            res = hip.topk_scores(h[b0:b1].contiguous(), table, K, 1, C, target=tg[b0:b1], excl=torch.as_tensor(v).cuda(),
                                  excl_off=torch.as_tensor(o).cuda())
            return [t.cpu().numpy() for t in res]
        one, again = run(0, B), run(0, B)
        parts = [run(0, 5), run(5, 21), run(21, 37)]
        for i, name in enumerate(("ids", "scores", "rank")):
            out["%s.one.%s" % (tier, name)] = one[i]
            out["%s.again.%s" % (tier, name)] = again[i]
            out["%s.split.%s" % (tier, name)] = np.concatenate([p[i] for p in parts])
    out["det_enabled"] = np.array(int(hip.lib().rg_det_enabled()))
    np.savez(out_path, **out)


if __name__ == "__main__":
    main()
