"""The logQ correction of the sampled softmax without a GPU: what the correction buys on the float64 restatement
(tests/logq_ref.py), the host tables of sampler.DeviceDomain against the restatement's, the ctypes mirror of rg_item_loss_args, the
value class models.LogQNegatives, the loaders' and drivers' refusals and the flag."""
import os
import re

import numpy as np
import pytest
import torch

import logq_ref as R
from parity_util import make_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", [7, 8, 9])
def test_the_correction_recovers_the_full_softmax(seed):
    """k = 512 draws per position over 200 items: the uncorrected loss sits 1.7 - 1.8 above the softmax over the catalogue, the
    corrected one within 0.01 of it (bound: a tenth of the uncorrected distance)."""
    fx = R.fixture(seed)
    full, _ = R.full_loss_ref(fx["h"], fx["E"], fx["y"], fx["mask"], rows=fx["items"])
    unc = R.logq_loss_ref(fx["h"], fx["E"], fx["y"], fx["neg"], fx["mask"])[0]
    cor = R.logq_loss_ref(fx["h"], fx["E"], fx["y"], fx["neg"], fx["mask"], fx["neg_bias"], fx["pos_bias"])[0]
    print("seed %d: full %.4f uncorrected %.4f corrected %.4f" % (seed, full, unc, cor))
    assert abs(cor - full) <= 0.1 * abs(unc - full)


def test_the_shared_correction_recovers_the_full_softmax():
    """One list of the distinct ids among 1 024 draws over 2 000 items: rms per-position error against the softmax over the
    catalogue, corrected at most a quarter of uncorrected."""
    fx = R.shared_fixture(7)
    _, pf = R.full_loss_ref(fx["h"], fx["E"], fx["y"], fx["mask"], rows=fx["items"])
    _, pu = R.shared_loss_ref(fx["h"], fx["E"], fx["y"], fx["cand"], fx["mask"])
    _, pc = R.shared_loss_ref(fx["h"], fx["E"], fx["y"], fx["cand"], fx["mask"], fx["cand_bias"])
    rms = lambda a: float(np.sqrt(np.mean(a * a)))
    print("shared: rms corrected %.4f uncorrected %.4f (%d candidates)" % (rms(pc - pf), rms(pu - pf), len(fx["cand"])))
    assert rms(pc - pf) <= 0.25 * rms(pu - pf)


def test_per_position_form_is_importance_weighting():
    """The shift-invariance the design rests on: adding -log Q_j to the negatives and log k - log(1 - m) to the positive is weighting
    every negative by 1 / (k Q'_j), Q' = Q / (1 - m)."""
    fx = R.fixture(3, n=4, k=9)
    per = R.logq_loss_ref(fx["h"], fx["E"], fx["y"], fx["neg"], fx["mask"], fx["neg_bias"], fx["pos_bias"])[4]
    for t in range(4):
        z0 = fx["E"][fx["y"][t]] @ fx["h"][t]
        qp = fx["Q"][fx["neg"][t]] / (1.0 - fx["Q"][fx["y"][t]])
        s = np.exp(z0) + (np.exp(fx["E"][fx["neg"][t]] @ fx["h"][t]) / (9 * qp)).sum()
        np.testing.assert_allclose(per[t], np.log(s) - z0, rtol=1e-12)


def _domain(V, wf, seqs, val, test):
    from recguru_amd import sampler
    return sampler.DeviceDomain(seqs, val, test, V, "cpu", wf=wf)


def test_host_tables_with_frequencies_and_a_zero_frequency_id():
    V = 30
    rng = np.random.RandomState(0)
    wf = rng.randint(1, 50, size=V + 1).astype(np.float64)
    wf[7] = 0.0                                                      # a zero-frequency id (a label, or a fall-back draw)
    seqs = [[1, 2, 3, 7], [5, 5, 9], [30, 29, 28, 27, 26]]
    val, test = [4, 6, 1], [8, 7, 2]
    dom = _domain(V, wf, seqs, val, test)
    nb, m_u, shift = dom.logq_tables()
    ref_nb = R.neg_bias_table(V, wf)
    assert nb.dtype == torch.float32 and nb.shape == (V + 2,) and bool(torch.isfinite(nb).all())
    np.testing.assert_array_equal(nb.numpy(), ref_nb.astype(np.float32))
    assert nb[0] == 0 and nb[V + 1] == 0 and nb[7] == nb[1:V + 1].max()       # the floor: the smallest positive Q
    excl = [set(s) | {t} for s, t in zip(seqs, test)]                # the sampler's exclusion rows (quirk Q14: not the validation item)
    ref_m = R.exclusion_mass(V, excl, wf)
    np.testing.assert_allclose(m_u, ref_m, rtol=1e-13, atol=0)
    np.testing.assert_allclose(shift.numpy(), (R.pos_bias_of(ref_m, 1, V, wf)).astype(np.float32), rtol=1e-6)
    assert dom.logq_tables()[0] is nb                                # built once
    for N in (1, 64, 100000):                                        # 100000 draws: every inclusion probability rounds to 1
        inc = dom.inclusion_bias(N)
        ref = R.inclusion_bias_table(V, N, wf)
        assert inc.dtype == torch.float32 and bool(torch.isfinite(inc).all())
        np.testing.assert_array_equal(inc.numpy(), ref.astype(np.float32))
        assert dom.inclusion_bias(N) is inc                          # cached per N
    assert float(dom.inclusion_bias(100000)[1:V + 1].abs().max()) == 0.0
    assert float(dom.inclusion_bias(1)[3]) == pytest.approx(float(nb[3]), rel=1e-6)      # one draw: the inclusion probability is Q


def test_host_tables_uniform():
    V = 20
    seqs, val, test = [[1, 2, 3], [2, 3, 4, 5, 6]], [5, 7], [7, 8]
    dom = _domain(V, None, seqs, val, test)
    nb, m_u, shift = dom.logq_tables()
    np.testing.assert_allclose(nb[1:V + 1].numpy(), np.full(V, np.log(V), dtype=np.float32), rtol=1e-7)
    assert nb[0] == 0 and nb[V + 1] == 0
    np.testing.assert_allclose(m_u, [4 / V, 6 / V], rtol=1e-13)
    np.testing.assert_array_equal(nb.numpy(), R.neg_bias_table(V).astype(np.float32))
    np.testing.assert_allclose(m_u, R.exclusion_mass(V, [set(s) | {t} for s, t in zip(seqs, test)]), rtol=1e-13)
    np.testing.assert_array_equal(dom.inclusion_bias(16).numpy(), R.inclusion_bias_table(V, 16).astype(np.float32))


def test_binding_mirrors_the_header():
    import ctypes
    from recguru_amd import hip
    hdr = open(os.path.join(ROOT, "include", "recguru_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} rg_item_loss_args;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+)?(void|float|int64_t|long long|int)\s*(\*?)\s*(\w+)$", decl)
        assert m, decl
        ptr = bool(m.group(3))
        fields.append((m.group(4), ctypes.c_void_p if ptr else {"long long": ctypes.c_longlong, "int": ctypes.c_int}[m.group(2)]))
    mirror = [(n, t) for n, t in hip.ItemLossArgs._fields_]
    assert [n for n, _ in mirror] == [n for n, _ in fields]
    assert all(ctypes.sizeof(a) == ctypes.sizeof(b) for (_, a), (_, b) in zip(mirror, fields))
    assert [n for n, _ in mirror][-2:] == ["neg_bias", "pos_bias"]          # appended: every earlier constructor call stays valid
    a = hip.ItemLossArgs(*([None] * 10), 3, 64, 5, 0, -1)
    assert a.neg_bias is None and a.pos_bias is None and ctypes.sizeof(a) == 10 * 8 + 8 + 3 * 4 + 4 + 8 + 16
    n = len(hip.SYMBOLS)
    assert n == 101                                                  # no new entry point
    for doc in ("README.md", "INTEGRATION.md"):
        assert "%d entry points" % n in open(os.path.join(ROOT, doc)).read(), doc
    assert "neg_bias" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_value_class():
    from recguru_amd.models import LogQNegatives, resolve_negatives
    ids = torch.zeros(3, 10, dtype=torch.int64)
    nb, pb = torch.zeros(9), torch.zeros(3)
    v = LogQNegatives(ids, neg_bias=nb, pos_bias=pb)
    assert v.ids is ids and v.neg_bias is nb and v.pos_bias is pb and v.cand_bias is None and v.dim() == 2
    moved = v.to("cpu")
    assert isinstance(moved, LogQNegatives) and moved.neg_bias.dtype == torch.float32 and moved.ids.shape == (3, 10)
    cand = torch.arange(1, 6)
    s = LogQNegatives(cand, cand_bias=torch.zeros(5)).to("cpu")
    assert s.dim() == 1 and s.neg_bias is None and s.cand_bias.numel() == 5
    for bad in (lambda: LogQNegatives(ids.float(), neg_bias=nb), lambda: LogQNegatives(ids, cand_bias=torch.zeros(30)),
                lambda: LogQNegatives(cand, neg_bias=nb), lambda: LogQNegatives(cand, cand_bias=torch.zeros(4)),
                lambda: LogQNegatives(ids, pos_bias=torch.zeros(4)), lambda: LogQNegatives(ids, neg_bias=nb.double()),
                lambda: LogQNegatives(ids.view(3, 5, 2), neg_bias=nb)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError, match="BPR"):                     # the BPR paths take no LogQNegatives
        resolve_negatives(None, None, None, v, 5, None)


def test_handles_carry_the_biases_and_bpr_refuses():
    from recguru_amd import models
    h, table = torch.zeros(3, 2, 64), torch.zeros(9, 64)
    lab = torch.ones(3, 2, dtype=torch.int64)
    v = models.LogQNegatives(torch.ones(3, 10, dtype=torch.int64), neg_bias=torch.zeros(9), pos_bias=torch.tensor([1.0, 2.0, 3.0]))
    sl = models.sampled_handle(h, table, lab, v, 5, 0)
    assert isinstance(sl, models.SampledLogits) and sl.neg is v.ids and sl.neg_bias is v.neg_bias and sl.skip_row == 0
    assert sl.pos_bias.tolist() == [1.0, 1.0, 2.0, 2.0, 3.0, 3.0]            # per user -> per position, by the labels' [B, L]
    with pytest.raises(ValueError, match="pos_bias holds 3 values for 6 positions"):
        models.SampledLogits(h, table, lab, v.ids, 5, 0, pos_bias=v.pos_bias)
    with pytest.raises(ValueError, match="BPR"):
        sl.bpr(torch.ones(6))
    sh = models.sampled_handle(h, table, lab, models.LogQNegatives(torch.arange(1, 4), cand_bias=torch.zeros(3)), 5)
    assert isinstance(sh, models.SharedLogits) and sh.cand_bias.numel() == 3
    plain = models.sampled_handle(h, table, lab, v.ids, 5)
    assert isinstance(plain, models.SampledLogits) and plain.neg_bias is None and plain.pos_bias is None
    assert isinstance(models.sampled_handle(h, table, lab, torch.arange(1, 4), 5), models.SharedLogits)


def test_ops_refuse_a_bias_with_bpr_and_a_wrong_size():
    from recguru_amd import hip, ops
    h, table = torch.zeros(4, 64, requires_grad=True), torch.zeros(9, 64)
    pos, neg, mask = torch.ones(4, dtype=torch.int64), torch.ones(4, 5, dtype=torch.int64), torch.ones(4)
    with pytest.raises(ValueError, match="BPR"):
        ops.bpr_loss(h, table, pos, neg, mask, 5, neg_bias=torch.zeros(9))
    with pytest.raises(ValueError, match="neg_bias has 8 elements, expected 9"):
        hip._item_bias(torch.zeros(8), None, table, 4)
    with pytest.raises(ValueError, match="pos_bias has 5 elements, expected 4"):
        hip._item_bias(None, torch.zeros(5), table, 4)
    with pytest.raises(ValueError, match="f32"):
        hip._item_bias(torch.zeros(9, dtype=torch.float64), None, table, 4)


def test_loaders_and_drivers_refuse_what_cannot_be_corrected():
    from recguru_amd import sampler
    from recguru_amd.config import get_param, logq_options
    dom = sampler.DeviceDomain([[1, 2, 3], [2, 3, 4]], [5, 6], [7, 8], 20, "cpu")
    with pytest.raises(ValueError, match="hard_negs"):
        sampler.DeviceLoader(dom, 2, 4, 4, 21, 8, hard_negs=16, logq=True)
    with pytest.raises(ValueError, match="hard_negs"):
        dom.batch(torch.arange(2), 4, 4, 21, 8, 0, hard_negs=16, logq=True)
    assert sampler.DeviceLoader(dom, 2, 4, 4, 21, 8, logq=True).logq and not sampler.DeviceLoader(dom, 2, 4, 4, 21, 8).logq
    mk = lambda **kw: get_param(make_args(64, 2, 5, 20, 51, 51, 1, 4, **kw), make_dirs=False)
    assert mk().logq is False and logq_options(mk()) == {}
    assert mk(logq=True).logq is True and logq_options(mk(logq=True)) == {"logq": True}
    assert logq_options(mk(logq=True, shared_negs=64)) == {"logq": True}
    with pytest.raises(ValueError, match="decoder_neg"):
        logq_options(mk(logq=True, decoder_neg=False))
    with pytest.raises(ValueError, match="hard_negs"):
        logq_options(mk(logq=True, hard_negs=64))
    assert logq_options(mk(decoder_neg=False, hard_negs=64)) == {}   # off: neither combination is looked at


@pytest.mark.parametrize("script", ["train_gan.py", "train_auto.py"])
def test_flag_parsing(script, monkeypatch):
    import importlib.util
    import sys
    spec = importlib.util.spec_from_file_location("drv_" + script[:-3], os.path.join(ROOT, script))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for argv, want in (([], False), (["--logq", "True"], True), (["--logq", "False"], False)):
        monkeypatch.setattr(sys, "argv", [script] + argv)
        assert mod.parse().logq is want
    src = open(os.path.join(ROOT, script)).read()
    assert "logq_options(param)" in src
