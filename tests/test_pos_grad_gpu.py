"""rg_pos_grad (the gradient of a learned positional table, csrc/elementwise.hip) through hip.pos_grad against the float64 restatement
of its contract (tests/pos_grad_ref.py), in both dtypes.

Shapes: the smallest at which each mechanism can go wrong (see SHAPES).  Two kinds of assertion:
  exact    dx holds small integers and p is 0 or 0.5 (kept elements scaled by exactly 2), the prior dP holds integers: every partial sum is
           an integer far below 2^24, so the result must equal the restatement bit for bit in ANY summation order;
  bounded  random dx (exactly representable in the dtype): |got - ref| <= (B + 3) * 2^-24 * (|prior| + sum_b |term_b|) element-wise -- a
           chain of at most B + 1 f32 additions plus the scaling by inv_keep and the final add onto dP (pos_grad_ref.bound).
Masked positions hold NaN in dx: their rows must not reach the result.  Index wrap past 2^32 needs 4 G elements and is not tested.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pos_grad_ref

pytestmark = pytest.mark.gpu

# (d, B, L): what it reaches
SHAPES = [
    (128, 5, 7),      # position tail inside a wave's 4-position block; batch not a multiple of the unroll
    (64, 3, 33),      # 8 positions per wave, one over
    (256, 2, 5),      # widest specialised row
    (40, 3, 9),       # the generic body
    (128, 37, 3),     # two or more batch slices, the last one ragged (37 is prime: ragged for any slice length)
    (128, 1, 1),      # smallest shape
]
SEEDS = {0.0: 0, 0.5: 0xF00DFACE12345678, 0.1: 0x8000000000000001}
DTYPES = [torch.float32, torch.bfloat16]


def make_mask(rng, B, L):
    """Left padding with random lengths, one all-padding sequence (B >= 2), one position that is padding in every sequence (L >= 2)."""
    lens = rng.integers(1, L + 1, size=B)
    lens[0] = L
    m = (np.arange(L)[None, :] >= (L - lens)[:, None]).astype(np.float32)
    dead_pos = None
    if B >= 2:
        m[B - 1] = 0.0
    if L >= 2:
        dead_pos = L // 2
        m[:, dead_pos] = 0.0
    return m, dead_pos


def run(dx, mask, dP, p, seed):
    from recguru_amd import hip
    B, L, d = dx.shape
    hip.pos_grad(dx, mask, dP, B, L, p, seed)
    torch.cuda.synchronize()
    return dP.cpu().numpy()


def device_inputs(dx_np, mask_np, dtype):
    dx = torch.as_tensor(dx_np, dtype=torch.float32).to(dtype).cuda().contiguous()
    poisoned = dx.clone()
    poisoned[torch.as_tensor(mask_np == 0).cuda()] = float("nan")        # a masked position's dx row is not read / never used
    return poisoned, torch.as_tensor(mask_np).cuda().reshape(-1).contiguous(), dx.float().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("d,B,L", SHAPES)
def test_exact_on_integers(d, B, L, dtype):
    from recguru_amd import hip
    rng = np.random.default_rng(d * 1000 + B * 10 + L)
    mask, dead_pos = make_mask(rng, B, L)
    dx, m, dx64 = device_inputs(rng.integers(-4, 5, size=(B, L, d)), mask, dtype)
    rows = L + 3
    prior = rng.integers(-8, 9, size=(rows, d)).astype(np.float32)
    prior[prior == 0] = 3.0
    if (d, B, L) == (128, 37, 3):
        # the slice count from the workspace size: a launcher change cannot turn this into a one-slice case unnoticed
        assert hip.pos_grad_workspace(B, L, d) // (L * d * 4) >= 2
    assert hip.pos_grad_workspace(B, L, d) % (L * d * 4) == 0 and hip.pos_grad_workspace(B, L, d) > 0
    for p in (0.0, 0.5):
        ref, _ = pos_grad_ref.pos_grad(dx64, mask, prior, p, SEEDS[p])
        dP = torch.as_tensor(prior).cuda()
        got = run(dx, m, dP, p, SEEDS[p])
        assert np.array_equal(got.astype(np.float64), ref), (p, np.abs(got - ref).max())
        assert np.array_equal(got[L:].view(np.uint32), prior[L:].view(np.uint32))                  # rows >= L: untouched bits
        if dead_pos is not None:
            assert np.array_equal(got[dead_pos].view(np.uint32), prior[dead_pos].view(np.uint32))  # all-padding position
        got2 = run(dx, m, dP, p, SEEDS[p])                                                          # two calls add twice
        assert np.array_equal(got2.astype(np.float64), 2 * ref - prior.astype(np.float64))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("d,B,L", SHAPES)
def test_bounded_on_random_data_and_same_bits_twice(d, B, L, dtype, capsys):
    rng = np.random.default_rng(7 + d * 1000 + B * 10 + L)
    mask, dead_pos = make_mask(rng, B, L)
    dx, m, dx64 = device_inputs(rng.standard_normal((B, L, d)), mask, dtype)
    rows = L + 2
    prior = rng.standard_normal((rows, d)).astype(np.float32)
    for p in (0.0, 0.5, 0.1):
        ref, abs_sum = pos_grad_ref.pos_grad(dx64, mask, prior, p, SEEDS[p])
        got = run(dx, m, torch.as_tensor(prior).cuda(), p, SEEDS[p])
        again = run(dx, m, torch.as_tensor(prior).cuda(), p, SEEDS[p])
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32))                           # identical inputs, identical bits
        bound = pos_grad_ref.bound(B, prior[:L], abs_sum)
        err = np.abs(got[:L].astype(np.float64) - ref[:L])
        share = float((err / np.maximum(bound, 1e-300)).max())
        with capsys.disabled():
            print("\n[pos_grad d=%d B=%d L=%d %s p=%.1f] max |err| %.3g, largest share of the bound %.3f"
                  % (d, B, L, "bf16" if dtype == torch.bfloat16 else "f32", p, float(err.max()), share))
        assert np.isfinite(got).all()
        assert (err <= bound).all(), share
        assert np.array_equal(got[L:].view(np.uint32), prior[L:].view(np.uint32))
        if dead_pos is not None:
            assert np.array_equal(got[dead_pos].view(np.uint32), prior[dead_pos].view(np.uint32))
        if p > 0 and mask.sum() * d >= 256:          # the dropout mask is the restatement's: without it the bound is missed by far
            nodrop, _ = pos_grad_ref.pos_grad(dx64, mask, prior, 0.0, 0)
            assert (np.abs(got[:L] - nodrop[:L]) > bound).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_all_zero_mask_leaves_dP_untouched(dtype):
    B, L, d = 5, 7, 128
    dx = torch.full((B, L, d), float("nan"), dtype=dtype, device="cuda")
    prior = np.random.default_rng(1).standard_normal((L + 1, d)).astype(np.float32)
    got = run(dx, torch.zeros(B * L, device="cuda"), torch.as_tensor(prior).cuda(), 0.5, SEEDS[0.5])
    assert np.array_equal(got.view(np.uint32), prior.view(np.uint32))


def test_refusals_come_before_any_launch():
    from recguru_amd import hip
    B, L, d = 3, 5, 64
    lib = hip.lib()
    need = hip.pos_grad_workspace(B, L, d)
    assert need > 0 and need % (L * d * 4) == 0
    assert hip.pos_grad_workspace(B, L, 12) == 0 and hip.pos_grad_workspace(0, L, d) == 0 and hip.pos_grad_workspace(B, 0, d) == 0
    dx = torch.ones(B, L, d, device="cuda")
    mask = torch.ones(B * L, device="cuda")
    prior = torch.full((L, d), 2.0, device="cuda")
    dP = prior.clone()
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)

    def call(dx_, mask_, dP_, ws_, nbytes, dtype, d_=d):
        return lib.rg_pos_grad(vp(dx_), vp(mask_), vp(dP_), B, L, d_, ctypes.c_float(0.0), ctypes.c_uint64(0), vp(ws_),
                               ctypes.c_size_t(nbytes), dtype, None)
    INVALID, UNSUPPORTED = -1, -2
    assert call(None, mask, dP, ws, need, hip.F32) == INVALID
    assert call(dx, None, dP, ws, need, hip.F32) == INVALID
    assert call(dx, mask, None, ws, need, hip.F32) == INVALID
    assert call(dx, mask, dP, None, need, hip.F32) == INVALID
    assert call(dx, mask, dP, ws, need, 7) == INVALID
    assert call(dx, mask, dP, ws, need, hip.X3) == INVALID
    assert call(dx, mask, dP, ws, need - 1, hip.F32) == INVALID
    assert b"workspace" in lib.rg_last_error()
    assert call(dx, mask, dP, ws, need, hip.F32, 12) == UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(dP, prior)                                   # nothing was launched
    assert call(dx, mask, dP, ws, need, hip.F32) == 0
    torch.cuda.synchronize()
    assert torch.equal(dP, prior + B)
    with pytest.raises(RuntimeError):
        hip.pos_grad(torch.ones(B, L, 12, device="cuda"), mask, torch.zeros(L, 12, device="cuda"), B, L)


def test_same_bits_in_both_libraries(tmp_path):
    """The summation order is fixed by (B, L, d), so librecguru_hip.so and librecguru_hip_det.so (RG_DETERMINISTIC=1) return the same
    bits without any deterministic-arena wrapping: one worker process per library on the same inputs."""
    here = os.path.dirname(os.path.abspath(__file__))
    got = {}
    for det in (False, True):
        env = dict(os.environ)
        env.pop("RG_DETERMINISTIC", None)
        if det:
            env["RG_DETERMINISTIC"] = "1"
        out = str(tmp_path / ("det%d.npz" % det))
        r = subprocess.run([sys.executable, os.path.join(here, "pos_grad_worker.py"), out], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=300)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        got[det] = dict(np.load(out))
    assert int(got[False]["det_enabled"]) == 0 and int(got[True]["det_enabled"]) >= 7     # (the translation units that accumulate, as tests/test_det_gpu.py reads it)
    keys = [k for k in got[False] if k.startswith("dP.")]
    assert len(keys) == 12 and sorted(keys) == sorted(k for k in got[True] if k.startswith("dP."))
    for k in keys:
        assert np.array_equal(got[False][k].view(np.uint32), got[True][k].view(np.uint32)), k
