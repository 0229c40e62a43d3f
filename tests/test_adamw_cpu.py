"""CPU tests of the optimizer options (recguru_amd/optim.py): the float64 restatement the GPU tests hold the kernels to
(tests/adamw_ref.py) is torch's own arithmetic, and the host-side surface -- configuration, constructor, load_state_dict -- behaves."""
import argparse

import numpy as np
import pytest
import torch

from adamw_ref import RefAdam, clip_coef, total_sq

SHAPES = [(1,), (129,), (37, 16), (5,)]


def _problem(seed):
    rs = np.random.RandomState(seed)
    params = [rs.randn(*s) for s in SHAPES]
    grads = [[rs.randn(*s) for s in SHAPES] for _ in range(5)]
    return params, grads


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("max_norm", [None, 1.5, 1e4])
def test_restatement_is_torch_adam_and_adamw_behind_clip_grad_norm(decoupled, max_norm):
    """5 steps on float64 CPU tensors to 1e-12; parameter 3 has no gradient on steps 1 and 3 (per-parameter step counts), and
    max_norm = 1.5 clips (the norm of ~760 randn values is ~27) while 1e4 does not."""
    params, grads = _problem(3)
    for st in (1, 3):
        grads[st][3] = None
    tp = [torch.nn.Parameter(torch.tensor(p, dtype=torch.float64)) for p in params]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    topt = cls(tp, lr=1e-2, betas=(0.5, 0.9), eps=1e-8, weight_decay=0.05)
    ref = RefAdam([{"params": params, "lr": 1e-2, "betas": (0.5, 0.9), "eps": 1e-8, "weight_decay": 0.05, "decoupled": decoupled}],
                  max_norm=max_norm)
    for gs in grads:
        for p, g in zip(tp, gs):
            p.grad = None if g is None else torch.tensor(g, dtype=torch.float64)
        if max_norm is not None:
            tn = torch.nn.utils.clip_grad_norm_(tp, max_norm)
        topt.step()
        rn = ref.step([gs])
        if max_norm is not None:
            assert abs(float(tn) - rn) <= 1e-12 * rn
        for p, r in zip(tp, ref.groups[0]["params"]):
            np.testing.assert_allclose(p.detach().numpy(), r, rtol=1e-12, atol=1e-12)
    assert ref.groups[0]["t"] == [5, 5, 5, 3]
    assert [int(topt.state[p]["step"]) for p in tp] == [5, 5, 5, 3]


def test_restatement_skip_rule():
    params, grads = _problem(4)
    ref = RefAdam([{"params": params, "lr": 1e-2, "betas": (0.5, 0.9)}], skip_nonfinite=True)
    ref.step([grads[0]])
    before = [p.copy() for p in ref.groups[0]["params"]]
    bad = [g.copy() for g in grads[1]]
    bad[2][3, 4] = np.inf
    ref.step([bad])
    assert ref.skipped == 1 and ref.groups[0]["t"] == [2, 2, 2, 2]
    for a, b in zip(before, ref.groups[0]["params"]):
        np.testing.assert_array_equal(a, b)
    assert clip_coef(total_sq([np.array([3.0, 4.0])]), 1.0) == 1.0 / (5.0 + 1e-6) and clip_coef(25.0, None) == 1.0


def test_get_param_exposes_the_optimizer_options_with_neutral_defaults(tmp_path):
    """The namespace is test_get_param_surface_matches_reference_defaults': it has none of the four names."""
    from recguru_amd.config import get_param
    from recguru_amd.optim import options
    a = argparse.Namespace(date="sas_org", d_model=32, n_head=1, d_ff=512, n_negs=30, decoder_neg=True, fix_enc=True,
                           lr=0.01, batch_size=1024, batch_size_val=256, dataset_pick=1, run=1, target_domain="a",
                           cross="True", sas="False", result_path=str(tmp_path))
    p = get_param(a)
    assert (p.weight_decay, p.decoupled_wd, p.clip_norm, p.skip_nonfinite) == (0.0, False, 0.0, False)
    assert options(p) == {"weight_decay": 0.0, "decoupled": False, "max_norm": None, "skip_nonfinite": False}
    a.weight_decay, a.decoupled_wd, a.clip_norm, a.skip_nonfinite = 0.01, True, 2.0, True
    p = get_param(a)
    assert (p.weight_decay, p.decoupled_wd, p.clip_norm, p.skip_nonfinite) == (0.01, True, 2.0, True)
    assert options(p) == {"weight_decay": 0.01, "decoupled": True, "max_norm": 2.0, "skip_nonfinite": True}
    assert options(p, critic=True) == {"skip_nonfinite": True}           # the W-GAN pair: no decay, no clip


def test_constructor_options_and_group_dicts():
    from recguru_amd.optim import Adam, AdamW
    a, b, c = (torch.nn.Parameter(torch.zeros(n)) for n in (3, 4, 5))
    o = Adam([a, b], lr=1e-2)
    assert o._neutral() and o.param_groups[0]["weight_decay"] == 0.0 and o.param_groups[0]["decoupled"] is False
    assert o.max_norm is None and o.skip_nonfinite is False and o.grad_norm() is None and o.skipped_steps() == 0
    o = Adam([{"params": [a], "weight_decay": 0.1}, {"params": [b, c], "lr": 3e-3, "betas": (0.5, 0.9), "decoupled": True}],
             lr=1e-2, eps=1e-9, weight_decay=0.02, max_norm=1.0, skip_nonfinite=True)
    g0, g1 = o.param_groups
    assert (g0["lr"], g0["betas"], g0["eps"], g0["weight_decay"], g0["decoupled"]) == (1e-2, (0.9, 0.999), 1e-9, 0.1, False)
    assert (g1["lr"], g1["betas"], g1["eps"], g1["weight_decay"], g1["decoupled"]) == (3e-3, (0.5, 0.9), 1e-9, 0.02, True)
    assert g0["params"] == [a] and len(g1["params"]) == 2 and o.max_norm == 1.0 and o.skip_nonfinite and not o._neutral()
    assert not Adam([a], skip_nonfinite=True)._neutral() and not Adam([a], max_norm=1.0)._neutral() and Adam([a], max_norm=0.0)._neutral()
    w = AdamW(iter([a, b]))
    assert w.param_groups[0]["weight_decay"] == 1e-2 and w.param_groups[0]["decoupled"] is True and isinstance(w, Adam)
    assert [k for k in o.state_dict()["param_groups"][1]] == ["lr", "betas", "eps", "weight_decay", "decoupled"]
    for bad in (dict(weight_decay=-0.1), dict(max_norm=-1.0)):
        with pytest.raises(ValueError, match="< 0"):
            Adam([a], **bad)
    with pytest.raises(ValueError, match="unknown group option"):
        Adam([{"params": [a], "amsgrad": True}])


def test_load_state_dict_takes_weight_decay_and_still_rejects_amsgrad():
    from recguru_amd.optim import Adam
    tp = [torch.nn.Parameter(torch.randn(6))]
    tp[0].grad = torch.randn(6)
    for cls, dec in ((torch.optim.Adam, False), (torch.optim.AdamW, True)):
        t = cls(tp, lr=2e-3, betas=(0.5, 0.9), weight_decay=0.05)
        t.step()
        o = Adam([torch.nn.Parameter(tp[0].detach().clone())])
        o.load_state_dict(t.state_dict())
        g = o.param_groups[0]
        assert (g["lr"], tuple(g["betas"]), g["weight_decay"], g["decoupled"]) == (2e-3, (0.5, 0.9), 0.05, dec)
        assert not o._neutral() and o.state[o.param_groups[0]["params"][0]]["step"] == 1
        o2 = Adam([torch.nn.Parameter(tp[0].detach().clone())])
        o2.load_state_dict(o.state_dict())                                  # its own layout round-trips the same options
        assert o2.param_groups[0]["weight_decay"] == 0.05 and o2.param_groups[0]["decoupled"] == dec
    for key in ("amsgrad", "maximize"):
        sd = torch.optim.Adam(tp, **{key: True}).state_dict()
        with pytest.raises(ValueError, match="amsgrad / maximize are not implemented"):
            Adam([torch.nn.Parameter(torch.zeros(6))]).load_state_dict(sd)


def test_binding_mirrors_the_header():
    """hip.sqnorm_chain is RG_SQNORM_CHAIN, hip.ADAM_CTL_DTYPE is rg_adam_ctl (both read from include/recguru_hip.h)."""
    import os
    import re
    from recguru_amd import hip
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "recguru_hip.h")).read()
    m = re.search(r"#define RG_SQNORM_CHAIN\(chunk, nsegs\) \\\n\s*(.*)\n", hdr)
    expr = m.group(1).replace("(int)", "").replace("(long long)", "").replace("/", "//")
    for chunk, nsegs in ((1, 1), (1024, 1), (1025, 3), (65536, 1), (65536, 257), (65536, 2 ** 31 - 1)):
        assert hip.sqnorm_chain(chunk, nsegs) == eval(expr, {"chunk": chunk, "nsegs": nsegs}), (chunk, nsegs)
    assert hip.sqnorm_chain(hip.ADAM_CHUNK, 1000) == 76
    body = re.search(r"typedef struct \{([^}]*)\} rg_adam_ctl;", hdr).group(1)
    fields = re.findall(r"^\s*(double|float|int|long long)\s+(\w+);", body, flags=re.M)
    code = {"double": "<f8", "float": "<f4", "int": "<i4", "long long": "<i8"}
    assert [(n, code[t]) for t, n in fields] == hip.ADAM_CTL_DTYPE
    assert np.dtype(hip.ADAM_CTL_DTYPE).itemsize == 32
    assert "rg_grad_sqnorm_multi" in hip.SYMBOLS and "rg_adam_multi_dev2" in hip.SYMBOLS
