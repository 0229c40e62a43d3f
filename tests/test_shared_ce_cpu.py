"""The float64 restatement the GPU tests of the shared-candidate softmax rely on (tests/shared_ce_ref.py), pinned on the CPU against
the two losses it must reduce to, and the config default of --shared_negs."""
import argparse

import torch

from shared_ce_ref import shared_ce_ref


def _problem(n=70, d=16, rows=41, seed=0):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(n, d, generator=g, dtype=torch.float64)
    E = torch.randn(rows, d, generator=g, dtype=torch.float64) * 0.7
    mask = (torch.rand(n, generator=g) > 0.3).to(torch.float64)
    assert 0 < int(mask.sum()) < n
    return g, h, E, mask


def _autograd(loss_fn, h, E):
    hh, EE = h.clone().requires_grad_(True), E.clone().requires_grad_(True)
    loss = loss_fn(hh, EE)
    loss.backward()
    return float(loss.detach()), hh.grad, EE.grad


def test_all_rows_is_plain_cross_entropy():
    g, h, E, mask = _problem()
    rows = E.shape[0]
    y = torch.randint(0, rows, (h.shape[0],), generator=g)

    def ce(hh, EE):
        l = torch.nn.functional.cross_entropy(hh @ EE.T, y, reduction="none")
        return (l * mask).sum() / mask.sum()
    loss, dh, dE = _autograd(ce, h, E)
    got = shared_ce_ref(h, E, y, torch.arange(rows), mask, chunk=16)
    assert abs(got[0] - loss) <= 1e-12
    assert float((got[1] - dh).abs().max()) <= 1e-12 and float((got[2] - dE).abs().max()) <= 1e-12
    assert float(got[1][mask == 0].abs().max()) == 0.0


def test_disjoint_candidates_is_the_sampled_loss():
    g, h, E, mask = _problem(seed=1)
    rows = E.shape[0]
    S = torch.arange(3, rows, 4)                         # 3, 7, 11, ...
    pool = torch.tensor([r for r in range(rows) if r not in set(S.tolist())])
    y = pool[torch.randint(0, pool.numel(), (h.shape[0],), generator=g)]
    cb = torch.randn(S.numel(), generator=g, dtype=torch.float64)
    pb = torch.randn(h.shape[0], generator=g, dtype=torch.float64)

    def sampled(hh, EE):
        z = torch.cat([(hh * EE[y]).sum(1, keepdim=True) + pb[:, None], hh @ EE[S].T + cb[None, :]], 1)     # [z_pos, z_S], label 0
        l = torch.nn.functional.cross_entropy(z, torch.zeros(hh.shape[0], dtype=torch.long), reduction="none")
        return (l * mask).sum() / mask.sum()
    loss, dh, dE = _autograd(sampled, h, E)
    got = shared_ce_ref(h, E, y, S, mask, cand_bias=cb, pos_bias=pb, chunk=16)
    assert abs(got[0] - loss) <= 1e-12
    assert float((got[1] - dh).abs().max()) <= 1e-12 and float((got[2] - dE).abs().max()) <= 1e-12


def test_accidental_hits_leave_the_sum_and_skip_row_the_target_route():
    g, h, E, mask = _problem(seed=2)
    rows = E.shape[0]
    S = torch.tensor([0, 5, 9, rows - 1])
    y = S[torch.randint(0, S.numel(), (h.shape[0],), generator=g)]            # every target is a candidate

    def hit(hh, EE):
        z = hh @ EE[S].T                                                      # the target's own column stands for z_pos
        l = torch.nn.functional.cross_entropy(z, torch.searchsorted(S, y), reduction="none")
        return (l * mask).sum() / mask.sum()
    loss, dh, dE = _autograd(hit, h, E)
    got = shared_ce_ref(h, E, y, S, mask)
    assert abs(got[0] - loss) <= 1e-12 and float((got[1] - dh).abs().max()) <= 1e-12 and float((got[2] - dE).abs().max()) <= 1e-12
    skipped = shared_ce_ref(h, E, y, S, mask, skip_row=5)
    p = torch.exp((h * E[5]).sum(1) - skipped[3]) - 1.0
    sel = (y == 5) & (mask != 0)
    route = ((p * mask / mask.sum())[sel, None] * h[sel]).sum(0)
    assert float((got[2][5] - skipped[2][5] - route).abs().max()) <= 1e-12
    assert torch.equal(torch.cat([got[2][:5], got[2][6:]]), torch.cat([skipped[2][:5], skipped[2][6:]]))


def test_get_param_defaults_shared_negs_to_zero():
    from parity_util import make_args
    from recguru_amd.config import get_param
    a = make_args(64, 2, 8, 20, 300, 300, 1, 32)
    assert not hasattr(a, "shared_negs")
    assert get_param(a, make_dirs=False).shared_negs == 0
    b = argparse.Namespace(**vars(a))
    b.shared_negs = 256
    assert get_param(b, make_dirs=False).shared_negs == 256
