"""One process of tests/test_topk_wide_gpu.py::test_repeat_and_batch_split_invariance.  Run with RG_DETERMINISTIC=1
(librecguru_hip_det.so) or without (librecguru_hip.so): the random fixture's 37 users at C = 4099, d = 128, K = 300 in every tier
through hip.topk_wide as one call, the same call again, and as calls of 5 + 16 + 16 users, in the range form and over a list;
writes ids / scores of each to argv[1].

  python tests/topk_wide_worker.py <out.npz>
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
    from test_topk_list_gpu import make_list
    torch.cuda.set_device(0)
    B, C, d, K = 37, 4099, 128, 300
    lst = torch.as_tensor(make_list(2500, C + 1, np.random.default_rng(3))).cuda()
    out = {}
    for tier in TIERS:
        ops.set_compute_dtype({"bf16": torch.bfloat16, "bf16x3": "bf16x3", "f32": torch.float32}[tier])
        dtype = torch.bfloat16 if tier == "bf16" else torch.float32
        hn, wn, _, rows, _, _ = random_case(B, C, d, tier)
        h, table = torch.as_tensor(hn).cuda().to(dtype), torch.as_tensor(wn).cuda().to(dtype)

        def run(b0, b1, form):
            v, o = R.csr(rows[b0:b1])
            kw = dict(first_row=1, n_rows=C) if form == "range" else dict(rows=lst)
            res = hip.topk_wide(h[b0:b1].contiguous(), table, K, excl=torch.as_tensor(v).cuda(), excl_off=torch.as_tensor(o).cuda(), **kw)
            fault = hip.topk_wide_state(h.device, b1 - b0)[0]
            assert fault == 0, fault
            return [t.cpu().numpy() for t in res]
        for form in ("range", "list"):
            one, again = run(0, B, form), run(0, B, form)
            parts = [run(0, 5, form), run(5, 21, form), run(21, 37, form)]
            for i, name in enumerate(("ids", "scores")):
                out["%s.%s.one.%s" % (tier, form, name)] = one[i]
                out["%s.%s.again.%s" % (tier, form, name)] = again[i]
                out["%s.%s.split.%s" % (tier, form, name)] = np.concatenate([p[i] for p in parts])
    out["det_enabled"] = np.array(int(hip.lib().rg_det_enabled()))
    np.savez(out_path, **out)


if __name__ == "__main__":
    main()
