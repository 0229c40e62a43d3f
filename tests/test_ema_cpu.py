"""Host-side checks of the weight average (ema_decay / ema_warmup of recguru_amd.optim.Adam): the float64 restatement of
tests/ema_ref.py against values computed by hand, constructor validation, optim.options, the flags of both entry scripts and the
configuration defaults, the state_dict layout with the option off, and the ABI surface."""
import argparse
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

from ema_ref import RefEmaAdam, decay_at

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hand_case(**kw):
    """lr = 0.1, betas = (0, 0), eps = 0: m = g, v = g^2 and both bias corrections are 1, so every update is p -= 0.1 * sign(g).
    A = [1, 2] has gradients in steps 1 and 2, B = [0] in steps 2 and 3."""
    ref = RefEmaAdam([dict(params=[np.array([1.0, 2.0]), np.array([0.0])], lr=0.1, betas=(0.0, 0.0), eps=0.0)], **kw)
    grads = [[np.array([1.0, -1.0]), None], [np.array([2.0, 3.0]), np.array([-1.0])], [None, np.array([5.0])]]
    return ref, grads


def test_restatement_against_hand_computed_values():
    ref, grads = _hand_case(ema_decay=0.5)
    g = ref.groups[0]
    assert g["ema"] == [None, None]
    ref.step([grads[0]])
    # A: e0 = [1, 2] (before the update), p = [0.9, 2.1], e = 0.5 e0 + 0.5 p = [0.95, 2.05];  B: no gradient yet, no average
    np.testing.assert_allclose(g["params"][0], [0.9, 2.1], rtol=0, atol=1e-15)
    np.testing.assert_allclose(g["ema"][0], [0.95, 2.05], rtol=0, atol=1e-15)
    assert g["ema"][1] is None and g["t"] == [1, 0]
    ref.step([grads[1]])
    # A: p = [0.8, 2.0], e = [0.875, 2.025];  B: e0 = 0 (its value before ITS first update), p = 0.1, e = 0.05
    np.testing.assert_allclose(g["ema"][0], [0.875, 2.025], rtol=0, atol=1e-15)
    np.testing.assert_allclose(g["ema"][1], [0.05], rtol=0, atol=1e-15)
    ref.step([grads[2]])
    # A: no gradient -- average, weights and count stay;  B: p = 0.0, e = 0.025
    np.testing.assert_allclose(g["params"][0], [0.8, 2.0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(g["ema"][0], [0.875, 2.025], rtol=0, atol=1e-15)
    np.testing.assert_allclose(g["ema"][1], [0.025], rtol=0, atol=1e-15)
    assert g["t"] == [2, 2]


def test_restatement_warmup_and_skip_by_hand():
    assert decay_at(0.5, True, 1) == 2.0 / 11.0 and decay_at(0.5, True, 2) == 0.25 and decay_at(0.5, True, 18) == 0.5
    assert decay_at(0.2, True, 2) == 0.2 and decay_at(0.999, False, 1) == 0.999 and decay_at(0.0, True, 5) == 0.0
    ref, grads = _hand_case(ema_decay=0.5, ema_warmup=True)
    g = ref.groups[0]
    for gs in grads:
        ref.step([gs])
    # A: t = 1: d = 2/11, e = 2/11 [1, 2] + 9/11 [0.9, 2.1];  t = 2: d = 3/12, e = 0.25 e + 0.75 [0.8, 2.0]
    a1 = np.array([2.0 / 11 * 1.0 + 9.0 / 11 * 0.9, 2.0 / 11 * 2.0 + 9.0 / 11 * 2.1])
    np.testing.assert_allclose(g["ema"][0], 0.25 * a1 + 0.75 * np.array([0.8, 2.0]), rtol=0, atol=1e-15)
    # B: t = 1: e = 9/11 * 0.1;  t = 2: e = 0.25 e + 0.75 * 0.0
    np.testing.assert_allclose(g["ema"][1], [0.25 * 9.0 / 11 * 0.1], rtol=0, atol=1e-15)
    # skip: step 2 carries a NaN -- nothing moves, B's average is still created from its weights, both counts advance, and step 3 uses
    # the warm-up factor of the ADVANCED count (B: t = 2 -> 3/12, not 2/11)
    ref, grads = _hand_case(ema_decay=0.5, ema_warmup=True, skip_nonfinite=True)
    g = ref.groups[0]
    grads[1][0][1] = float("nan")
    ref.step([grads[0]])
    before = (g["params"][0].copy(), g["ema"][0].copy())
    ref.step([grads[1]])
    assert ref.skipped == 1 and g["t"] == [2, 1]
    np.testing.assert_array_equal(g["params"][0], before[0])
    np.testing.assert_array_equal(g["ema"][0], before[1])
    np.testing.assert_array_equal(g["ema"][1], [0.0])
    np.testing.assert_array_equal(g["params"][1], [0.0])
    ref.step([grads[2]])
    # B's first APPLIED update has t = 2 (both bias corrections are 1 here): p = -0.1, e = 0.25 * 0 + 0.75 * -0.1
    np.testing.assert_allclose(g["params"][1], [-0.1], rtol=0, atol=1e-15)
    np.testing.assert_allclose(g["ema"][1], [-0.075], rtol=0, atol=1e-15)


def test_constructor_validation_and_attributes():
    from recguru_amd.optim import Adam, AdamW, averaged, has_average
    a = torch.nn.Parameter(torch.zeros(3))
    o = Adam([a])
    assert o.ema_decay is None and o.ema_warmup is False and o.ema_swapped is False and o._neutral() and not has_average(o)
    for d in (0.0, 0.5, 0.999):
        o = Adam([a], ema_decay=d, ema_warmup=True)
        assert o.ema_decay == d and o.ema_warmup is True and not o._neutral() and has_average(o)
    assert AdamW([a], ema_decay=0.9).ema_decay == 0.9 and AdamW([a]).ema_decay is None
    for bad in (1.0, -0.1, 2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ema_decay"):
            Adam([a], ema_decay=bad)
        with pytest.raises(ValueError, match="ema_decay"):
            AdamW([a], ema_decay=bad)
    with pytest.raises(ValueError, match="unknown group option"):            # it belongs to the optimizer, not to a group
        Adam([{"params": [a], "ema_decay": 0.9}])
    # without an average: swap_ema() and averaged() do nothing (no GPU here: a launch would raise)
    o = Adam([a])
    o.swap_ema()
    assert o.ema_swapped is False
    with averaged(o, None):
        assert o.ema_swapped is False

    class Wrapped(object):                                                   # blocks.ScheduledOptim's shape
        _optimizer = o
    with averaged(Wrapped()):
        pass
    assert not has_average(Wrapped())


def test_swapped_optimizer_refuses_step_and_state_dicts():
    """No parameter has an average yet, so the swap launches nothing and the flag logic runs without a GPU."""
    from recguru_amd.optim import Adam
    a = torch.nn.Parameter(torch.zeros(3))
    o = Adam([a], ema_decay=0.9)
    sd = o.state_dict()
    o.swap_ema()
    assert o.ema_swapped is True
    for call in (o.step, o.state_dict, lambda: o.load_state_dict(sd)):
        with pytest.raises(RuntimeError, match="averaged weights"):
            call()
    o.swap_ema()
    assert o.ema_swapped is False
    with pytest.raises(KeyError):
        with o.averaged():
            assert o.ema_swapped is True
            raise KeyError("x")
    assert o.ema_swapped is False
    o.load_state_dict(sd)


def test_options_equal_todays_dict_when_off_and_carry_the_keys_when_on(tmp_path):
    from recguru_amd.config import get_param
    from recguru_amd.optim import options
    a = argparse.Namespace(date="sas_org", d_model=32, n_head=1, d_ff=512, n_negs=30, decoder_neg=True, fix_enc=True,
                           lr=0.01, batch_size=1024, batch_size_val=256, dataset_pick=1, run=1, target_domain="a",
                           cross="True", sas="False", result_path=str(tmp_path))
    p = get_param(a)                                                         # a Namespace without the two names
    assert p.ema_decay == 0.0 and p.ema_warmup is False
    assert options(p) == {"weight_decay": 0.0, "decoupled": False, "max_norm": None, "skip_nonfinite": False}
    assert options(p, critic=True) == {"skip_nonfinite": False}
    assert options(argparse.Namespace()) == {"weight_decay": 0.0, "decoupled": False, "max_norm": None, "skip_nonfinite": False}
    a.ema_decay, a.ema_warmup = 0.0, True                                    # warm-up alone does not switch it on
    assert options(get_param(a)) == {"weight_decay": 0.0, "decoupled": False, "max_norm": None, "skip_nonfinite": False}
    a.ema_decay = 0.995
    p = get_param(a)
    assert p.ema_decay == 0.995 and p.ema_warmup is True
    assert options(p) == {"weight_decay": 0.0, "decoupled": False, "max_norm": None, "skip_nonfinite": False,
                          "ema_decay": 0.995, "ema_warmup": True}
    assert options(p, critic=True) == {"skip_nonfinite": False}              # the critic is not averaged


@pytest.mark.parametrize("script", ["train_gan.py", "train_auto.py"])
def test_entry_scripts_parse_the_two_flags(script, monkeypatch):
    spec = importlib.util.spec_from_file_location("ema_cpu_" + script[:-3], os.path.join(ROOT, script))
    mod = importlib.util.module_from_spec(spec)
    monkeypatch.setattr(sys, "path", list(sys.path))                         # the scripts put their directory in front
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", [script])
    args = mod.parse()
    assert args.ema_decay == 0.0 and args.ema_warmup is False
    monkeypatch.setattr(sys, "argv", [script, "--ema_decay", "0.999", "--ema_warmup", "True"])
    args = mod.parse()
    assert args.ema_decay == 0.999 and args.ema_warmup is True


def test_state_dict_without_the_option_has_no_ema_key():
    from recguru_amd.optim import Adam
    a, b = (torch.nn.Parameter(torch.zeros(n)) for n in (3, 4))
    o = Adam([a, b], weight_decay=0.1)
    o.state[a] = {"step": 2, "exp_avg": torch.ones(3), "exp_avg_sq": torch.ones(3)}
    sd = o.state_dict()
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    assert [k for k in sd["param_groups"][0]] == ["lr", "betas", "eps", "weight_decay", "decoupled"]
    # an optimizer WITHOUT the option drops a checkpoint's average; one WITH it restores it, and accepts a checkpoint without the key
    sd["state"][0]["ema"] = torch.full((3,), 7.0)
    o.load_state_dict(sd)
    assert "ema" not in o.state[a] and "ema" not in o.state_dict()["state"][0]
    o = Adam([a, b], ema_decay=0.9)
    o.load_state_dict(sd)
    assert torch.equal(o.state[a]["ema"], torch.full((3,), 7.0)) and torch.equal(o.state_dict()["state"][0]["ema"], torch.full((3,), 7.0))
    del sd["state"][0]["ema"]
    o.load_state_dict(sd)
    assert "ema" not in o.state[a]


def test_binding_mirrors_the_header():
    from recguru_amd import hip
    hdr = open(os.path.join(ROOT, "include", "recguru_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} rg_ema_pair;", hdr).group(1)
    fields = re.findall(r"(float\*|long long)\s+(\w+);", body)
    code = {"float*": "<u8", "long long": "<i8"}
    assert [(n, code[t]) for t, n in fields] == hip.EMA_PAIR_DTYPE and np.dtype(hip.EMA_PAIR_DTYPE).itemsize == 24
    for name in ("rg_adam_multi_dev3", "rg_ema_swap_multi"):
        assert name in hip.SYMBOLS and re.search(r"\bint %s\(" % name, hdr), name
        assert name[3:] in hip._PLAIN and callable(getattr(hip, name[3:]))
    # the pinned mirrors did not move
    assert np.dtype(hip.ADAM_SEG_DEV_DTYPE).itemsize == 48 and np.dtype(hip.ADAM_CTL_DTYPE).itemsize == 32
    n = len(hip.SYMBOLS)
    for doc in ("README.md", "INTEGRATION.md"):
        assert "%d entry points" % n in open(os.path.join(ROOT, doc)).read(), doc
