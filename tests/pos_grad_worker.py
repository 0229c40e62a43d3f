"""One process of test_pos_grad_gpu.py::test_same_bits_in_both_libraries.  Run with RG_DETERMINISTIC=1 (librecguru_hip_det.so) or
without (librecguru_hip.so): hip.pos_grad on fixed inputs (a multi-slice shape, the generic body; both dtypes; p = 0.5 and 0.1), every
result written to argv[1] with the library's rg_det_enabled()."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    from recguru_amd import hip
    torch.cuda.set_device(0)
    out = {"det_enabled": np.array(int(hip.lib().rg_det_enabled()))}
    rng = np.random.default_rng(2024)
    for d, B, L in ((128, 37, 3), (40, 3, 9), (256, 2, 5)):
        dx32 = torch.as_tensor(rng.standard_normal((B, L, d)), dtype=torch.float32).cuda()
        mask = torch.as_tensor((rng.random(B * L) < 0.7).astype(np.float32)).cuda()
        prior = torch.as_tensor(rng.standard_normal((L + 1, d)), dtype=torch.float32).cuda()
        for dtype in (torch.float32, torch.bfloat16):
            for p, seed in ((0.5, 0xF00DFACE12345678), (0.1, 0x8000000000000001)):
                dP = prior.clone()
                hip.pos_grad(dx32.to(dtype).contiguous(), mask, dP, B, L, p, seed)
                out["dP.%d.%d.%d.%s.%g" % (d, B, L, "bf16" if dtype == torch.bfloat16 else "f32", p)] = dP.cpu().numpy()
    torch.cuda.synchronize()
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
