"""Hard negatives without a GPU: the float64 restatement of tests/hard_negs_ref.py on cases enumerated by hand, the configuration
options and the argument checks of models.HardNegatives / the loaders' and drivers' refusals."""
import numpy as np
import pytest
import torch

import hard_negs_ref as HR
from parity_util import make_args

NEG = -np.inf


def _run(S, pool, labels, L, k, skip, excl=None, mask=None, ld=None, fill=-9):
    S = np.asarray(S, dtype=np.float64)
    n = S.shape[0]
    mask = np.ones(n) if mask is None else np.asarray(mask)
    el = HR.eligible(pool, labels, L, excl)
    return HR.select(S, pool, el, mask, k, skip, np.full((n, ld or k), fill, dtype=np.int64))


def test_restatement_on_hand_made_cases():
    pool = np.array([2, 5, 7, 11])
    #             id   2    5    7    11
    S = np.array([[1.0, 3.0, 3.0, 0.5],      # a tie between 5 and 7: the lower id first
                  [4.0, 9.0, 1.0, 2.0],      # the label 5 is in the pool: never returned
                  [1.0, 2.0, 3.0, 4.0],      # the exclusion row holds 6 (not in the pool) and 11
                  [1.0, 2.0, 3.0, 4.0]])     # the row covers the whole pool: nothing eligible
    labels = np.array([99, 5, 99, 99])
    excl = [[], [], [6, 11], [2, 5, 7, 11]]
    out, sc = _run(S, pool, labels, 1, 3, 0, excl)
    assert out.tolist() == [[5, 7, 2], [2, 11, 7], [7, 5, 2], [-9, -9, -9]]
    assert sc.tolist() == [[3.0, 3.0, 1.0], [4.0, 2.0, 1.0], [3.0, 2.0, 1.0], [NEG, NEG, NEG]]
    # skip drops the head of the order; |E_t| < skip + k leaves the trailing slots as they were (scores -inf); columns >= k untouched
    out, sc = _run(S, pool, labels, 1, 3, 2, excl, ld=5)
    assert out.tolist() == [[2, 11, -9, -9, -9], [7, -9, -9, -9, -9], [2, -9, -9, -9, -9], [-9] * 5]
    assert sc.tolist() == [[1.0, 0.5, NEG], [1.0, NEG, NEG], [1.0, NEG, NEG], [NEG, NEG, NEG]]
    # the exclusion row belongs to the SEQUENCE (L = 2: positions 0, 1 share row 0), the label to the position; mask == 0: not written
    out, sc = _run(S, pool, labels, 2, 1, 0, [[7], [2]], mask=[1, 1, 0, 1])
    assert out.tolist() == [[5], [2], [-9], [11]]
    assert sc.tolist() == [[3.0], [4.0], [NEG], [4.0]]
    # a pool id outside the table is ineligible
    el = HR.eligible(np.array([2, 5, 70]), np.array([0]), 1, None, table_rows=12)
    assert el.tolist() == [[True, True, False]]


def test_flat_exclusion_layout():
    rows = [[5, 3, 3], [], [9]]
    v, lo, hi = HR.flat_excl(rows, np.random.default_rng(0))
    for b, r in enumerate(rows):
        assert v[lo[b]:hi[b]].tolist() == sorted(set(r))
    assert len(v) == 3 + 4 * 3                     # gaps of foreign ids around every row


def test_config_reads_the_three_options():
    from recguru_amd.config import get_param, hard_negs_options
    p = get_param(make_args(64, 2, 5, 20, 51, 51, 1, 4), make_dirs=False)
    assert (p.hard_negs, p.hard_k, p.hard_skip) == (0, 0, 0)
    assert hard_negs_options(p) == {}
    p = get_param(make_args(64, 2, 5, 20, 51, 51, 1, 4, hard_negs=257, hard_k=3, hard_skip=2), make_dirs=False)
    assert (p.hard_negs, p.hard_k, p.hard_skip) == (257, 3, 2)
    assert hard_negs_options(p) == {"hard_negs": 257, "hard_k": 3, "hard_skip": 2}
    assert hard_negs_options(p, 5)["hard_k"] == 3 and hard_negs_options(p, 2)["hard_k"] is None      # above a phase's k: all of that phase's
    p = get_param(make_args(64, 2, 5, 20, 51, 51, 1, 4, hard_negs=257), make_dirs=False)
    assert hard_negs_options(p) == {"hard_negs": 257, "hard_k": None, "hard_skip": 0}


def test_drivers_refuse_runs_without_private_negatives():
    from recguru_amd.config import get_param, hard_negs_options
    with pytest.raises(ValueError, match="shared_negs"):
        hard_negs_options(get_param(make_args(64, 2, 5, 20, 51, 51, 1, 4, hard_negs=64, shared_negs=32), make_dirs=False))
    with pytest.raises(ValueError, match="decoder_neg"):
        hard_negs_options(get_param(make_args(64, 2, 5, 20, 51, 51, 1, 4, hard_negs=64, decoder_neg=False), make_dirs=False))
    # off: neither combination is looked at
    assert hard_negs_options(get_param(make_args(64, 2, 5, 20, 51, 51, 1, 4, shared_negs=32, decoder_neg=False), make_dirs=False)) == {}
    for driver in ("train_gan.py", "train_auto.py"):
        import os
        src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), driver)).read()
        for flag in ("--hard_negs", "--hard_k", "--hard_skip", "hard_negs_options(param)"):
            assert flag in src, (driver, flag)


def test_hard_negatives_argument_checks():
    from recguru_amd.models import HardNegatives, resolve_negatives
    priv = torch.zeros(3, 10, dtype=torch.int64)
    pool = torch.arange(1, 8)
    hn = HardNegatives(priv, pool, 2, skip=1)
    assert (hn.k_hard, hn.skip) == (2, 1) and hn.private is priv and hn.pool is pool and hn.excl is None
    moved = hn.to("cpu")
    assert isinstance(moved, HardNegatives) and (moved.k_hard, moved.skip) == (2, 1)
    for bad in (lambda: HardNegatives(priv, pool, 0), lambda: HardNegatives(priv, pool, 2, skip=-1),
                lambda: HardNegatives(priv.view(-1), pool, 2), lambda: HardNegatives(priv, pool.view(1, -1), 2),
                lambda: HardNegatives(priv.float(), pool, 2), lambda: HardNegatives(priv, pool[:0], 2),
                lambda: HardNegatives(priv, pool, 2, excl=pool), lambda: HardNegatives(priv, pool, 2, excl_lo=pool[:3], excl_hi=pool[:3]),
                lambda: HardNegatives(priv, pool, 2, excl=pool, excl_lo=pool[:2], excl_hi=pool[:2])):
        with pytest.raises(ValueError):
            bad()
    # a plain tensor passes through resolve_negatives untouched; k_hard > k and a private draw of another size are refused before
    # any device work (CPU tensors: a launch would raise RuntimeError, not ValueError)
    assert resolve_negatives(None, None, None, priv, 5, None) is priv
    h = torch.zeros(3, 2, 64)
    with pytest.raises(ValueError, match="k_hard"):
        resolve_negatives(h, torch.zeros(9, 64), torch.zeros(3, 2, dtype=torch.int64), HardNegatives(priv, pool, 6), 5, torch.ones(6))
    with pytest.raises(ValueError, match="private"):
        resolve_negatives(h, torch.zeros(9, 64), torch.zeros(3, 2, dtype=torch.int64), HardNegatives(priv, pool, 2), 4, torch.ones(6))


def test_loader_refuses_hard_with_shared():
    from recguru_amd import sampler
    dom = sampler.DeviceDomain([[1, 2, 3], [2, 3, 4]], [5, 6], [7, 8], 20, "cpu")
    with pytest.raises(ValueError, match="shared_negs"):
        sampler.DeviceLoader(dom, 2, 4, 4, 21, 8, shared_negs=16, hard_negs=16)
    with pytest.raises(ValueError, match="shared_negs"):
        dom.batch(torch.arange(2), 4, 4, 21, 8, 0, shared_negs=16, hard_negs=16)


def test_symbol_is_declared_and_bound():
    import os
    from recguru_amd import hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "recguru_hip.h")).read()
    assert "int rg_hard_negs(const rg_hard_negs_args* args /* host */, int dtype, void* stream);" in hdr
    assert "rg_hard_negs" in hip.SYMBOLS
    src = open(os.path.join(root, "recguru_amd", "csrc", "hard_negs.hip")).read()
    assert '#include "rg_det.hip.h"' not in src and "atomicAdd" not in src          # the same code in both libraries
    names = [n for n, _ in hip.HardNegsArgs._fields_]
    assert names == ["h", "table", "table_rows", "pool", "C", "labels", "mask", "live16", "excl", "excl_lo", "excl_hi", "out",
                     "out_scores", "n", "L", "d", "k", "skip", "ld_out", "checked"]
