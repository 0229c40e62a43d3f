"""Host-side checks of the full-catalogue scoring feature: the float64 restatement (tests/topk_ref.py) on hand-written cases, the
metrics of a known rank vector, and the ABI surface (header and hip.SYMBOLS)."""
import os
import re

import numpy as np

import topk_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ties_put_the_lower_id_first():
    S = np.array([[1.0, 3.0, 3.0, 2.0, 3.0]])
    ids, sc = R.topk(S, 4, 10, R.eligible(1, 10, 5))
    assert ids.tolist() == [[11, 12, 14, 13]]
    assert sc.tolist() == [[3.0, 3.0, 3.0, 2.0]]


def test_rank_counts_strictly_greater_scores_only():
    S = np.array([[5.0, 2.0, 2.0, 7.0, 2.0, 1.0]])
    el = R.eligible(1, 0, 6)
    assert R.rank(S, [1], 0, el).tolist() == [2]            # 5 and 7; the two ties at 2 do not count
    assert R.rank(S, [3], 0, el).tolist() == [0]
    assert R.rank(S, [5], 0, el).tolist() == [5]


def test_excluded_ids_leave_the_rank_and_the_list_but_the_target_stays():
    S = np.array([[5.0, 2.0, 4.0, 7.0], [5.0, 2.0, 4.0, 7.0]])
    rows = [[3, 1], []]                                      # user 0: ids 3 (the best) and 1 (its own target) excluded
    el = R.eligible(2, 0, 4, rows)
    assert R.rank(S, [1, 1], 0, el).tolist() == [2, 3]       # the target in its own exclusion row is still ranked
    ids, _ = R.topk(S, 2, 0, el)
    assert ids.tolist() == [[0, 2], [3, 0]]
    vals, off = R.csr(rows)
    assert vals.tolist() == [1, 3] and off.tolist() == [0, 2, 2]


def test_exclusion_ids_outside_the_catalogue_are_ignored():
    el = R.eligible(1, 1, 3, [[0, 2, 4, 99]])
    assert el.tolist() == [[True, False, True]]


def test_fewer_than_k_eligible_fill_with_minus_one_and_minus_inf():
    S = np.array([[1.0, 2.0, 3.0]])
    ids, sc = R.topk(S, 5, 1, R.eligible(1, 1, 3, [[2]]))
    assert ids.tolist() == [[3, 1, -1, -1, -1]]
    assert sc[0, :2].tolist() == [3.0, 1.0] and np.all(np.isneginf(sc[0, 2:]))


def test_rounding_follows_the_tier():
    x = np.array([1.0 + 2.0 ** -10, 1.0 + 2.0 ** -30], dtype=np.float64)
    assert R.round_tier(x, "bf16").tolist() == [1.0, 1.0]
    assert R.round_tier(x, "f32").tolist() == [1.0 + 2.0 ** -10, 1.0]
    assert R.round_tier(x, "bf16x3").tolist() == [1.0 + 2.0 ** -10, 1.0]


def test_rank_interval_brackets_the_exact_rank():
    rng = np.random.default_rng(0)
    S = rng.normal(size=(3, 50))
    el = R.eligible(3, 0, 50, [[1, 2], [], [7]])
    tgt = [4, 9, 7]
    lo, hi = R.rank_interval(S, np.full(3, 0.05), tgt, 0, el)
    rk = R.rank(S, tgt, 0, el)
    assert np.all(lo <= rk) and np.all(rk <= hi) and np.any(lo < hi)
    lo0, hi0 = R.rank_interval(S, np.zeros(3), tgt, 0, el)
    assert lo0.tolist() == rk.tolist() == hi0.tolist()


def test_metrics_of_a_known_rank_vector():
    r = np.array([0, 3, 9, 10, 250], dtype=np.int32)
    m = R.metrics_of(r, [1, 10])
    assert m["1"] == (0.2, 0.2, 0.2)
    np.testing.assert_allclose(m["10"][0], 3 / 5)
    np.testing.assert_allclose(m["10"][1], (1.0 + 1.0 / np.log2(5.0) + 1.0 / np.log2(11.0)) / 5, rtol=1e-15)
    np.testing.assert_allclose(m["10"][2], (1.0 + 1.0 / 4 + 1.0 / 10) / 5, rtol=1e-15)


def test_header_and_binding_declare_the_entry_points():
    from recguru_amd import hip
    hdr = open(os.path.join(ROOT, "include", "recguru_hip.h")).read()
    declared = set(re.findall(r"\b(rg_[a-z0-9_]+)\s*\(", hdr))
    for name in ("rg_topk_workspace", "rg_topk_scores"):
        assert name in declared, name
        assert name in hip.SYMBOLS, name
    assert "rg_topk_args" in hdr
    fields = [f[0] for f in hip.TopkArgs._fields_]
    assert fields == ["h", "table", "first_row", "n_rows", "target", "excl", "excl_off", "topk_ids", "topk_scores", "rank", "workspace",
                      "workspace_bytes", "B", "d", "K"]
    # every helper of the unit is internal: the two entry points are its only extern "C" definitions
    src = open(os.path.join(ROOT, "recguru_amd", "csrc", "topk.hip")).read()
    assert sorted(re.findall(r'extern "C" [a-z_]+ (rg_[a-z0-9_]+)\(', src)) == ["rg_topk_scores", "rg_topk_workspace"]
    assert "rg_det.hip.h\"" not in src.split("namespace {")[0].replace("does not include rg_det.hip.h", "")


def test_seen_rows_builds_sorted_unique_csr():
    import torch
    from recguru_amd.training import seen_rows
    enc = torch.tensor([[0, 0, 5, 3, 5, 9], [0, 0, 0, 0, 0, 0], [9, 2, 2, 1, 7, 8]])          # pad 0, EOS 9
    vals, off = seen_rows(enc, 0, 9)
    assert vals.tolist() == [3, 5, 1, 2, 7, 8] and off.tolist() == [0, 2, 2, 6]
