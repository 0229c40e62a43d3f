"""Host-side checks of the candidate-list scoring feature (rg_topk_list): item_list's normalisation and refusals, the ABI surface
(header and hip.SYMBOLS), the numpy helpers tests/test_topk_list_gpu.py relies on -- against tests/topk_ref.py on a case enumerated by
hand -- and the input condition of its random fixtures, which the float64 reference alone must satisfy."""
import os
import re
import types

import numpy as np
import pytest
import torch

import topk_ref as R
import test_topk_list_gpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------
# item_list
# ---------------------------------------------------------------------------------------------------------------------
def _param():
    # EOS ids as config.py derives them: vocab_size_a = items of a + 1 -> items 1 .. 9 in a, 1 .. 5 in b
    return types.SimpleNamespace(vocab_size_a=10, vocab_size_b=6, vocab_size=10)


@pytest.mark.parametrize("make", [lambda x: x, np.array, torch.tensor, lambda x: torch.tensor(x, dtype=torch.int32)])
def test_item_list_sorts_and_removes_duplicates(make):
    from recguru_amd import auto_training, training
    for fn in (lambda a: training.item_list(a, _param()), lambda a: auto_training.item_list(a, _param())):
        t = fn(make([7, 2, 9, 2, 1, 7]))
        assert t.dtype == torch.int64 and t.dim() == 1 and t.is_contiguous() and t.device.type == "cpu"
        assert t.tolist() == [1, 2, 7, 9]
    assert training.item_list(make([5, 1]), _param(), domain="b").tolist() == [1, 5]
    assert training.item_list(make([[3, 1], [1, 2]]), _param(), device="cpu").tolist() == [1, 2, 3]


def test_item_list_refuses_empty_non_integer_and_foreign_ids():
    from recguru_amd import auto_training, training
    p = _param()
    for fn in (lambda a, **kw: training.item_list(a, p, **kw), lambda a, **kw: auto_training.item_list(a, p)):
        for empty in ([], np.zeros(0, dtype=np.int64), torch.zeros(0, dtype=torch.int64)):
            with pytest.raises(ValueError, match="empty"):
                fn(empty)
        for bad in ([1.0, 2.0], np.array([1.5]), torch.tensor([1.0]), torch.tensor([True]), ["3"]):
            with pytest.raises(ValueError, match="integers"):
                fn(bad)
        with pytest.raises(ValueError, match=r"id 0 is outside the item ids 1 \.\. 9"):          # pad
            fn([3, 0])
        with pytest.raises(ValueError, match=r"id 10 is outside the item ids 1 \.\. 9"):         # EOS
            fn([3, 10])
        with pytest.raises(ValueError, match=r"id -4 is outside"):
            fn(torch.tensor([-4, 2]))
    with pytest.raises(ValueError, match=r"id 6 is outside the item ids 1 \.\. 5"):
        training.item_list([6], p, domain="b")
    assert training.item_list([9], p).tolist() == [9] and training.item_list([5], p, domain="b").tolist() == [5]


def test_among_is_a_keyword_of_the_four_functions_and_defaults_to_none():
    import inspect
    from recguru_amd import auto_training, training
    for fn in (training.recommend, training.evaluation_full, auto_training.recommend, auto_training.evaluation_full):
        assert inspect.signature(fn).parameters["among"].default is None, fn


# ---------------------------------------------------------------------------------------------------------------------
# ABI surface
# ---------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_list_entry_points():
    from recguru_amd import hip
    hdr = open(os.path.join(ROOT, "include", "recguru_hip.h")).read()
    declared = set(re.findall(r"\b(rg_[a-z0-9_]+)\s*\(", hdr))
    for name in ("rg_topk_list_workspace", "rg_topk_list"):
        assert name in declared, name
        assert name in hip.SYMBOLS, name
    assert "rg_topk_list_args" in hdr
    body = re.search(r"typedef struct \{([^}]*)\} rg_topk_list_args;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    in_header = [re.findall(r"[A-Za-z_]\w*", n)[-1] for decl in body.split(";") if decl.strip() for n in decl.split(",")]   # declarators' names
    fields = [f[0] for f in hip.TopkListArgs._fields_]
    assert fields == in_header == ["h", "table", "table_rows", "rows", "n_list", "target", "excl", "excl_off", "topk_ids", "topk_scores",
                                   "rank", "workspace", "workspace_bytes", "B", "d", "K"]
    # rg_topk_args is as it was
    assert [f[0] for f in hip.TopkArgs._fields_] == ["h", "table", "first_row", "n_rows", "target", "excl", "excl_off", "topk_ids",
                                                    "topk_scores", "rank", "workspace", "workspace_bytes", "B", "d", "K"]
    src = open(os.path.join(ROOT, "recguru_amd", "csrc", "topk.hip")).read()
    assert '#include "rg_det.hip.h"' not in src and "atomicAdd(a.rank" in src
    assert not re.search(r"atomic(Add|Max|Min)\s*\(\s*\(?\s*float", src)


# ---------------------------------------------------------------------------------------------------------------------
# the GPU tests' numpy helpers on a case small enough to enumerate by hand
# ---------------------------------------------------------------------------------------------------------------------
#            table row   0    1    2    3    4    5    6    7
S_TABLE = np.array([[9.0, 5.0, 2.0, 7.0, 5.0, 1.0, 7.0, 3.0],
                    [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]])
ROWS = np.array([1, 3, 4, 6, 7], dtype=np.int64)          # the list; rows 0, 2 and 5 are outside it


def test_helpers_on_a_hand_case():
    excl = [[6, 2, 0], []]                                   # user 0: 6 is in the list, 2 and 0 are not (they count for nothing)
    el = G.list_eligible(ROWS, excl, 2)
    assert el.tolist() == [[True, True, True, False, True], [True] * 5]
    # user 0, target 4 (in the list, score 5): higher are 3 (7) and 6 (7, excluded) -> 1; row 1 ties at 5 and does not count
    # user 1, target 5 (outside the list, score 6): higher among the list are 6 and 7 -> 2
    assert G.list_rank(S_TABLE, ROWS, np.array([4, 5]), el).tolist() == [1, 2]
    # a target in its own exclusion run is still ranked: user 0, target 6 (score 7): nothing in the list is strictly higher;
    # user 1, target 0 (score 1, outside the list): all five ids of the list are
    assert G.list_rank(S_TABLE, ROWS, np.array([6, 0]), el).tolist() == [0, 5]
    ids, sc = G.list_topk(S_TABLE, ROWS, 4, el)
    assert ids.tolist() == [[3, 1, 4, 7], [7, 6, 4, 3]]       # ties (5.0 at rows 1 and 4): the lower id first
    assert sc.tolist() == [[7.0, 5.0, 5.0, 3.0], [8.0, 7.0, 5.0, 4.0]]
    ids6, sc6 = G.list_topk(S_TABLE, ROWS, 6, el)
    assert ids6[0].tolist() == [3, 1, 4, 7, -1, -1] and np.all(np.isneginf(sc6[0, 4:])) and ids6[1].tolist() == [7, 6, 4, 3, 1, -1]
    assert G.positions(ids6, ROWS).tolist() == [[1, 0, 2, 4, -1, -1], [4, 3, 2, 1, 0, -1]]
    with pytest.raises(AssertionError):
        G.positions(np.array([[2]]), ROWS)
    # the same answers from topk_ref over the whole table with the complement of the list added to the exclusion runs
    comp = G.complement_excl(excl, ROWS, 0, 8, 2)
    assert [c.tolist() for c in comp] == [[0, 2, 5, 6], [0, 2, 5]]
    el_full = R.eligible(2, 0, 8, comp)
    ids_r, sc_r = R.topk(S_TABLE, 6, 0, el_full)
    assert ids_r.tolist() == ids6.tolist() and sc_r.tolist() == sc6.tolist()
    assert R.rank(S_TABLE, [4, 5], 0, el_full).tolist() == [1, 2]
    # zero tolerance: the interval is the rank
    lo, hi = G.list_rank_interval(S_TABLE, np.zeros(2), ROWS, np.array([4, 5]), el)
    assert lo.tolist() == [1, 2] and hi.tolist() == [2, 2]   # hi counts the tie at row 1 (>=)
    lo, hi = G.list_rank_interval(S_TABLE, np.full(2, 0.6), ROWS, np.array([4, 5]), el)
    assert lo.tolist() == [1, 1] and hi.tolist() == [2, 3]
    assert G.near_ties_at_cut(S_TABLE[:, ROWS], np.zeros(2), 2, el).tolist() == [2, 1]


def test_merge_topk_is_the_top_k_of_the_union():
    ids1, sc1 = np.array([[3, 1, -1]]), np.array([[7.0, 5.0, -np.inf]], dtype=np.float32)
    ids2, sc2 = np.array([[6, 4, 7]]), np.array([[7.0, 5.0, 3.0]], dtype=np.float32)
    ids, sc = G.merge_topk(ids1, sc1, ids2, sc2, 3)
    assert ids.tolist() == [[3, 6, 1]] and sc.tolist() == [[7.0, 7.0, 5.0]] and sc.dtype == np.float32
    ids, sc = G.merge_topk(ids1, sc1, ids2, sc2, 6)
    assert ids.tolist() == [[3, 6, 1, 4, 7, -1]] and np.isneginf(sc[0, 5])


def test_list_makers():
    rng = np.random.default_rng(0)
    for n in G.LIST_SIZES:
        rows = G.make_list(n, G.T_ROWS, rng)
        assert len(rows) == n and rows.dtype == np.int64 and np.all(np.diff(rows) > 0) and rows[-1] == G.T_ROWS - 1 and rows[0] >= 0
        tg = G.make_targets(rows, G.T_ROWS, 9, rng)
        assert np.isin(tg[0::2], rows).all() and not np.isin(tg[1::2], rows).any() and tg.min() >= 0 and tg.max() < G.T_ROWS
        ex = G.make_excl(rows, tg, G.T_ROWS, rng)
        assert ex[0] == [] and int(tg[1]) in ex[1] and G.T_ROWS in ex[8]
        assert G.list_eligible(rows, ex, 9)[8].sum() <= 3
    assert G.make_list(G.T_ROWS - 1, G.T_ROWS, rng).tolist() == list(range(1, G.T_ROWS))
    assert np.diff(G.make_list(15, G.T_ROWS, rng)).max() > 100          # large gaps


# ---------------------------------------------------------------------------------------------------------------------
# the random fixtures' input condition holds for the float64 reference alone (checked here, before any GPU run)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", G.TIERS)
@pytest.mark.parametrize("B,n_list,d,K", G.RANDOM_CASES)
def test_random_fixtures_meet_check_topk_input_condition(B, n_list, d, K, tier):
    _, _, rows, target, excl, S, Tb = G.random_list_case(B, n_list, d, tier)
    for use in (excl, None):
        el = G.list_eligible(rows, use, B)
        assert G.near_ties_at_cut(S[:, rows], Tb, K, el).max() <= 5          # topk_ref.check_topk's max_near
        lo, hi = G.list_rank_interval(S, Tb, rows, target, el)
        assert np.all(lo <= hi) and (hi - lo).max() <= max(2, 0.005 * n_list)   # the rank is pinned to a narrow interval
