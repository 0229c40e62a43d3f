"""Host-side checks of the wide top-K feature (rg_topk_wide): the ABI surface (header, hip.SYMBOLS, the struct mirror), the workspace
query against the formula the header states, the source rules of csrc/topk_wide.hip, the chain oracle of tests/test_topk_wide_gpu.py
against tests/topk_ref.py on a hand-sized case, the input condition of its derived-bound test on the float64 reference alone, and the
signatures of recommend."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import topk_ref as R
import test_topk_wide_gpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_declare_the_wide_entry_points():
    from recguru_amd import hip
    hdr = open(os.path.join(ROOT, "include", "recguru_hip.h")).read()
    declared = set(re.findall(r"\b(rg_[a-z0-9_]+)\s*\(", hdr))
    for name in ("rg_topk_wide_workspace", "rg_topk_wide"):
        assert name in declared, name
        assert name in hip.SYMBOLS, name
    body = re.search(r"typedef struct \{([^}]*)\} rg_topk_wide_args;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    in_header = [re.findall(r"[A-Za-z_]\w*", n)[-1] for decl in body.split(";") if decl.strip() for n in decl.split(",")]   # declarators' names
    fields = [f[0] for f in hip.TopkWideArgs._fields_]
    assert fields == in_header == ["h", "table", "first_row", "n_rows", "rows", "n_list", "table_rows", "excl", "excl_off", "topk_ids",
                                   "topk_scores", "workspace", "workspace_bytes", "B", "d", "K"]
    assert "target" not in fields and "rank" not in fields          # ranks stay with the K = 0 calls
    # the mirror's types: pointers and size_t 8 bytes, long long 8, int 4 -- the C struct's layout on this ABI
    assert ctypes.sizeof(hip.TopkWideArgs) == 13 * 8 + 3 * 4 + 4


def _workspace(B, d, n_rows, K):
    from recguru_amd import hip
    fn = hip.lib().rg_topk_wide_workspace
    fn.restype = ctypes.c_size_t
    return int(fn(B, d, ctypes.c_longlong(n_rows), K))


def _formula(B):
    """include/recguru_hip.h: 256 + align256(32 B) + B (1024 + 16384)"""
    return 256 + (32 * B + 255) // 256 * 256 + B * (1024 + 16384)


def test_workspace_query():
    assert _workspace(37, 128, 10 ** 3, 300) == _workspace(37, 128, 2 ** 31 - 1, 300) == _formula(37)
    assert _workspace(4096, 256, 2 * 10 ** 6, 1024) == _formula(4096) == 256 + 131072 + 4096 * 17408
    assert _workspace(1, 64, 1, 1) == _formula(1) == 256 + 256 + 17408
    assert _workspace(37, 128, 1000, 1) == _workspace(37, 64, 1000, 1024)          # among the supported shapes a function of B alone
    for K in (0, 1025, -1):
        assert _workspace(37, 128, 1000, K) == 0
    assert _workspace(37, 96, 1000, 300) == 0
    assert _workspace(0, 128, 1000, 300) == 0
    assert _workspace(37, 128, 0, 300) == 0 and _workspace(37, 128, 2 ** 31, 300) == 0


def test_source_rules_of_the_unit():
    src = open(os.path.join(ROOT, "recguru_amd", "csrc", "topk_wide.hip")).read()
    common = open(os.path.join(ROOT, "recguru_amd", "csrc", "topk_common.hip.h")).read()
    for text in (src, common):
        assert not re.search(r"#\s*include\s*\"rg_det\.hip\.h\"", text)          # (recguru_amd/build.py compiles a unit twice on that line)
        assert not re.search(r"atomic(Add|Sub|Max|Min|Exch|CAS)\s*\(\s*\(?\s*(float|double)", text)
        assert not re.search(r"atomic\w*_f(32|64)|unsafeAtomic|__hip_atomic\w*\(\s*\(\s*(float|double)", text)
    # every atomic of the unit has an integer destination: the LDS bins, hist, the cursor, the fault word
    dests = re.findall(r"atomic(?:Add|Sub|Or|Min)\(([^,]+),", src)
    assert dests and all(re.match(r"&bins\[|a\.hist\b|&a\.st\[b\]\.cursor|a\.fault|fault", d.strip()) for d in dests), dests
    assert '#include "topk_common.hip.h"' in src
    assert sorted(re.findall(r'extern "C" [a-z_]+ (rg_[a-z0-9_]+)\(', src)) == ["rg_topk_wide", "rg_topk_wide_workspace"]
    # ONE score function and ONE key for every top-K entry point: defined in the shared header only
    topk = open(os.path.join(ROOT, "recguru_amd", "csrc", "topk.hip")).read()
    for name in ("tk_scores", "tk_make_key", "tk_load_row", "tk_load_users", "tk_excluded", "tk_list_id"):
        pat = r"__device__ __forceinline__ [\w:<> ]+ %s\(" % name
        assert len(re.findall(pat, common)) == 1, name
        assert not re.findall(pat, src) and not re.findall(pat, topk), name
    # no waiting between workgroups: no loop that polls memory
    assert not re.search(r"while\s*\([^)]*(volatile|atomic|__hip_atomic_load)", src)


#            row     0    1    2    3    4    5    6    7    8
S_HAND = np.array([[9.0, 5.0, 2.0, 7.0, 5.0, 1.0, 7.0, 3.0, 5.0],
                   [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]])


def test_chain_oracle_on_a_hand_case():
    first_row, n = 10, 9
    for excl in (None, [[13, 99], [10, 11, 18]]):
        calls = []

        def call(rows):
            calls.append([list(r) for r in rows])
            return R.topk(S_HAND, 2, first_row, R.eligible(2, first_row, n, rows))
        for k in (2, 5, 7, 9, 12):
            ids, sc = G.chain_topk(call, 2, k, 2, excl)
            ids_ref, sc_ref = R.topk(S_HAND, k, first_row, R.eligible(2, first_row, n, excl))
            assert ids.tolist() == ids_ref.tolist() and sc.tolist() == sc_ref.tolist(), (k, excl)
        if excl is None:
            ids, _ = G.chain_topk(call, 2, 5, 2, None)
            assert ids.tolist() == [[10, 13, 16, 11, 14], [10, 11, 12, 13, 14]]          # ties: the lower id first, across chunk borders
            assert calls[-3] == [[], []] and calls[-2] == [[10, 13], [10, 11]] and calls[-1] == [[10, 13, 16, 11], [10, 11, 12, 13]]


@pytest.mark.parametrize("tier", G.TIERS)
@pytest.mark.parametrize("B,C,d,K,most", [(37, 4099, 128, 1024, 10), (16, 100003, 128, 1024, 10), (37, 4099, 256, 300, 5), (5, 1001, 64, 300, 12),
                                          (37, 4099, 128, 300, 12), (37, 4099, 256, 1024, 12), (5, 1001, 64, 1024, 12)])
def test_derived_bound_input_condition(B, C, d, K, most, tier):
    """topk_ref.check_topk's max_near = 12 is a condition on the inputs: the float64 reference alone has at most that many eligible
    ids within 2 T_b of the cut (the counts of the first two cases are the ones the feature's issue states)"""
    from test_topk_list_gpu import near_ties_at_cut
    _, _, _, rows, S, Tb = G._case(B, C, d, tier)
    for use in (rows, None):
        assert near_ties_at_cut(S, Tb, K, R.eligible(B, 1, C, use)).max() <= most


def test_recommend_signatures_are_unchanged():
    from recguru_amd import auto_training, training
    assert str(inspect.signature(training.recommend)) == \
        "(model, enc_in, dec_in, k, param, domain='a', device=None, exclude_seen=True, sas=False, among=None)"
    assert str(inspect.signature(auto_training.recommend)) == "(model, enc_in, dec_in, k, param, exclude_seen=True, sas=False, among=None)"
    from recguru_amd import hip
    assert str(inspect.signature(hip.topk_wide)) == "(h, table, k, first_row=None, n_rows=None, rows=None, excl=None, excl_off=None)"
    assert hip.TOPK_WIDE_MAX_K == 1024 and training.TOPK_NARROW_MAX_K == 128
