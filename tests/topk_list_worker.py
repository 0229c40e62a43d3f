"""One process of tests/test_topk_list_gpu.py::test_deterministic_library_gives_the_same_bits.  Run with RG_DETERMINISTIC=1
(librecguru_hip_det.so): the additivity case's 70 users over a list of 1 040 ids at d = 128, K = 100, in every tier; writes ids /
scores / rank of each to argv[1].

  python tests/topk_list_worker.py <out.npz>
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
    from test_topk_list_gpu import TIERS, additivity_case
    torch.cuda.set_device(0)
    out = {}
    for tier in TIERS:
        ops.set_compute_dtype({"bf16": torch.bfloat16, "bf16x3": "bf16x3", "f32": torch.float32}[tier])
        dtype = torch.bfloat16 if tier == "bf16" else torch.float32
        hn, wn, rows, target, excl = additivity_case()
        v, o = R.csr(excl)
        res = hip.topk_list(torch.as_tensor(hn).cuda().to(dtype), torch.as_tensor(wn).cuda().to(dtype), 100, torch.as_tensor(rows).cuda(),
                            target=torch.as_tensor(target).cuda(), excl=torch.as_tensor(v).cuda(), excl_off=torch.as_tensor(o).cuda())
        for name, t in zip(("ids", "scores", "rank"), res):
            out["%s.%s" % (tier, name)] = t.cpu().numpy()
    out["det_enabled"] = np.array(int(hip.lib().rg_det_enabled()))
    np.savez(out_path, **out)


if __name__ == "__main__":
    main()
