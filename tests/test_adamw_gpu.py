"""GPU tests of the optimizer options (csrc/optim.hip, recguru_amd/optim.py): global-norm clipping, coupled / decoupled weight decay
and the non-finite skip, against the float64 restatement of tests/adamw_ref.py (which tests/test_adamw_cpu.py holds to torch).

Shapes: the smallest that reach every code path -- 1 element, 129 (scalar tail behind the 16-byte loads), 37 x 16, a misaligned view
(base[1:]: the scalar walk), 65536 + 3 (two segments), one parameter without a gradient, and 257 five-element parameters (the
finalize's second, ragged round).

Bounds.  total_sq: (RG_SQNORM_CHAIN + 1) * 2^-24 relative, derived beside the macro in include/recguru_hip.h (a chain of roundings
over non-negative terms).  Updates: rtol 1e-5 / atol 1e-6 against float64, the bound test_adam_state_dict_roundtrip_and_external_edits
holds the plain update to; every case prints its measured share of that bound (profiles/adamw/test_printout.txt: at most 0.12 of it)."""
import math

import numpy as np
import pytest
import torch

from adamw_ref import RefAdam, total_sq
from parity_util import make_args

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-6
LR, BETAS, EPS = 1e-2, (0.5, 0.9), 1e-8
U = 2.0 ** -24


@pytest.fixture(autouse=True)
def _restore_tier():
    from recguru_amd import ops
    yield
    ops.set_compute_dtype(torch.bfloat16)


def _params(seed, many=False):
    """The standard set (the last parameter never gets a gradient), or the 257 five-element parameters."""
    g = torch.Generator().manual_seed(seed)
    if many:
        return [torch.nn.Parameter(torch.randn(5, generator=g).cuda()) for _ in range(257)]
    base = torch.randn(132, generator=g).cuda()
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g).cuda()) for s in ((1,), (129,), (37, 16))]
    ps.append(torch.nn.Parameter(base[1:]))
    assert ps[-1].data_ptr() % 16 == 4
    ps.append(torch.nn.Parameter(torch.randn(65536 + 3, generator=g).cuda()))
    ps.append(torch.nn.Parameter(torch.randn(7, generator=g).cuda()))
    return ps


def _grads(ps, seed, steps=5, dead_last=True):
    g = torch.Generator().manual_seed(seed)
    out = [[torch.randn(*p.shape, generator=g).cuda() for p in ps] for _ in range(steps)]
    if dead_last:
        for gs in out:
            gs[-1] = None
    return out


def _set_grads(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else g.clone()


def _np64(t):
    return t.detach().double().cpu().numpy()


def _table(ps, steps=0):
    """A device segment table over the parameters that have a gradient, with fresh zero moments: (table, nsegs, live)."""
    from recguru_amd import hip, optim
    live = [(p, {"step": steps, "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}) for p in ps if p.grad is not None]
    tbl = np.array(optim._rows(live), dtype=hip.ADAM_SEG_DEV_DTYPE)
    return torch.from_numpy(tbl.view(np.uint8).copy()).cuda(), len(tbl), live


def _ctl():
    from recguru_amd import hip
    return torch.zeros(np.dtype(hip.ADAM_CTL_DTYPE).itemsize, device="cuda", dtype=torch.uint8)


def _read_ctl(ctl):
    from recguru_amd import hip
    return ctl.cpu().numpy().view(hip.ADAM_CTL_DTYPE)[0]


def _share(a, b):
    """max over the elements of |a - b| / (ATOL + RTOL |b|): the measured share of the bound."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / (ATOL + RTOL * np.abs(b)))) if a.size else 0.0


def _against_ref(opt, ref, capsys, what):
    """p, exp_avg, exp_avg_sq and step counts of every parameter against the restatement; prints the worst share of the bound."""
    worst = 0.0
    for g, rg in zip(opt.param_groups, ref.groups):
        for i, p in enumerate(g["params"]):
            st = opt.state.get(p)
            if st is None:
                assert rg["t"][i] == 0
                np.testing.assert_array_equal(_np64(p), rg["params"][i])
                continue
            assert st["step"] == rg["t"][i]
            for a, b in ((p, rg["params"][i]), (st["exp_avg"], rg["m"][i]), (st["exp_avg_sq"], rg["v"][i])):
                worst = max(worst, _share(_np64(a), b))
    with capsys.disabled():
        print("\n[adamw] %s: worst |gpu - f64| / (%.0e + %.0e |f64|) = %.3g" % (what, ATOL, RTOL, worst))
    assert worst <= 1.0, (what, worst)


# ---- the norm -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("many", [False, True])
def test_total_sq_within_the_declared_chain_bound_and_repeatable(many, capsys):
    from recguru_amd import hip
    ps = _params(11, many)
    gs = _grads(ps, 12, steps=1, dead_last=not many)[0]
    _set_grads(ps, gs)
    tbl, n, live = _table(ps)
    assert n == (257 if many else 6) and len(live) == (257 if many else 5)
    partial = torch.full((n,), float("nan"), device="cuda")
    ctl = _ctl()
    hip.grad_sqnorm_multi(tbl, n, partial, ctl, 0.0, False)
    first = ctl.cpu().numpy().copy()
    c = _read_ctl(ctl)
    exact = total_sq([g.cpu().numpy() for g in gs if g is not None])      # the parameter without a gradient is not in it
    chain = hip.sqnorm_chain(hip.ADAM_CHUNK, n)
    rel = abs(float(c["total_sq"]) - exact) / exact
    with capsys.disabled():
        print("\n[adamw] total_sq over %d segments: rel. error %.3g, bound (%d + 1) * 2^-24 = %.3g" % (n, rel, chain, (chain + 1) * U))
    assert rel <= (chain + 1) * U
    assert c["coef"] == 1.0 and c["skip"] == 0 and c["skipped"] == 0
    assert abs(float(c["norm"]) - math.sqrt(exact)) <= ((chain + 1) * U / 2 + U) * math.sqrt(exact)
    # per segment too: each partial is a chain of its own
    seg_exact = [total_sq([g.cpu().numpy().reshape(-1)[o:o + hip.ADAM_CHUNK]]) for g in gs if g is not None
                 for o in range(0, g.numel(), hip.ADAM_CHUNK)]
    np.testing.assert_allclose(partial.cpu().numpy().astype(np.float64), seg_exact, rtol=chain * U, atol=0)
    # the same bits on a second call (fixed order: no atomics), into fresh buffers
    partial2 = torch.zeros(n, device="cuda")
    ctl2 = _ctl()
    hip.grad_sqnorm_multi(tbl, n, partial2, ctl2, 0.0, False)
    assert torch.equal(partial.view(torch.int32), partial2.view(torch.int32))
    assert np.array_equal(first, ctl2.cpu().numpy())
    # max_norm: torch's coefficient, from the measured norm
    hip.grad_sqnorm_multi(tbl, n, partial, ctl, 0.1 * math.sqrt(exact), False)
    c = _read_ctl(ctl)
    want = 0.1 * math.sqrt(exact) / (math.sqrt(float(c["total_sq"])) + 1e-6)
    assert abs(float(c["coef"]) - want) <= U * want and c["skip"] == 0


# ---- neutral options ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ctl", [False, True])
def test_neutral_adam_multi_dev2_has_the_bits_of_adam_multi_dev(with_ctl):
    """No ctl and no decay; and a ctl whose max_norm is 1000 x the norm, where coef is exactly 1: p, m, v and the step counts after 3
    steps at atol = 0."""
    from recguru_amd import hip
    pa, pb = _params(21), _params(21)
    grads = _grads(pa, 22, steps=3)
    _set_grads(pa, grads[0])
    _set_grads(pb, grads[0])
    ta, n, la = _table(pa, steps=2)
    tb, nb, lb = _table(pb, steps=2)
    assert n == nb == 6
    ctl, partial = _ctl(), torch.zeros(n, device="cuda")
    for gs in grads:
        for (p, _), (q, _), g in zip(la, lb, [g for g in gs if g is not None]):
            p.grad.copy_(g)                                                  # same buffers: the tables stay valid
            q.grad.copy_(g)
        hip.adam_multi_dev(ta, n, LR, BETAS[0], BETAS[1], EPS)
        if with_ctl:
            hip.grad_sqnorm_multi(tb, n, partial, ctl, 1000.0 * math.sqrt(total_sq([g.cpu().numpy() for g in gs if g is not None])), False)
            assert _read_ctl(ctl)["coef"] == 1.0
        hip.adam_multi_dev2(tb, n, LR, BETAS[0], BETAS[1], EPS, 0.0, False, ctl if with_ctl else None)
    for (p, sa), (q, sb) in zip(la, lb):
        for a, b in ((p, q), (sa["exp_avg"], sb["exp_avg"]), (sa["exp_avg_sq"], sb["exp_avg_sq"])):
            assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))
    sa, sb = (t.cpu().numpy().view(hip.ADAM_SEG_DEV_DTYPE)["step"] for t in (ta, tb))
    assert sa.tolist() == sb.tolist() == [5] * n
    assert torch.equal(pa[-1], pb[-1]) and torch.equal(pa[-1], _params(21)[-1])      # the parameter without a gradient: untouched


def test_neutral_optimizer_takes_the_old_code_path(monkeypatch):
    from recguru_amd import hip
    from recguru_amd.optim import Adam
    calls = []
    for name in ("adam_multi_dev", "adam_multi_dev2", "grad_sqnorm_multi"):
        real = getattr(hip, name)
        monkeypatch.setattr(hip, name, (lambda real, name: lambda *a, **k: (calls.append(name), real(*a, **k))[1])(real, name))
    ps = _params(31)
    _set_grads(ps, _grads(ps, 32, steps=1)[0])
    Adam(ps, lr=LR, betas=BETAS).step()
    assert calls == ["adam_multi_dev"]
    del calls[:]
    Adam([{"params": ps[:2]}, {"params": ps[2:], "weight_decay": 0.1}], lr=LR, betas=BETAS, max_norm=1.0).step()
    assert calls == ["grad_sqnorm_multi", "adam_multi_dev2", "adam_multi_dev2"]      # one norm + finalize call, one update per group
    del calls[:]
    Adam(ps, lr=LR, betas=BETAS, weight_decay=0.1).step()
    assert calls == ["adam_multi_dev2"]                                              # decay alone needs no norm


# ---- each option against the restatement ---------------------------------------------------------------------------------------
OPTION_CASES = {
    "coupled_decay": dict(groups=[dict(weight_decay=0.05)]),
    "decoupled_decay": dict(groups=[dict(weight_decay=0.05, decoupled=True)]),
    "clip": dict(groups=[dict()], clip=True),
    "clip_and_coupled_decay": dict(groups=[dict(weight_decay=0.05)], clip=True),
    "clip_and_decoupled_decay": dict(groups=[dict(weight_decay=0.05, decoupled=True)], clip=True),
    "two_groups_one_norm": dict(groups=[dict(weight_decay=0.1), dict(weight_decay=0.01, decoupled=True, lr=3e-3)], clip=True),
    "clip_many_small": dict(groups=[dict(weight_decay=0.05)], clip=True, many=True),
}


@pytest.mark.parametrize("case", sorted(OPTION_CASES))
def test_option_against_the_restatement(case, capsys):
    """5 steps at lr = 1e-2, betas = (0.5, 0.9), randn gradients.  max_norm = 0.1 x the smallest of the five norms: the clamp is active
    by a factor >= 10 in every step, so f32 and f64 cannot disagree about it."""
    from recguru_amd.optim import Adam
    c = OPTION_CASES[case]
    many = c.get("many", False)
    ps = _params(41, many)
    grads = _grads(ps, 42, dead_last=not many)
    split = [ps] if len(c["groups"]) == 1 else [ps[:3], ps[3:]]
    gsplit = (lambda gs: [gs]) if len(c["groups"]) == 1 else (lambda gs: [gs[:3], gs[3:]])
    norms = [math.sqrt(total_sq([g.cpu().numpy() for g in gs if g is not None])) for gs in grads]
    max_norm = 0.1 * min(norms) if c.get("clip") else None
    opt = Adam([dict(params=sp, **kw) for sp, kw in zip(split, c["groups"])], lr=LR, betas=BETAS, eps=EPS, max_norm=max_norm)
    ref = RefAdam([dict(dict(lr=LR, betas=BETAS, eps=EPS), params=[_np64(p) for p in sp], **kw) for sp, kw in zip(split, c["groups"])],
                  max_norm=max_norm)
    for gs, nrm in zip(grads, norms):
        before = [None if g is None else g.clone() for g in gs]
        _set_grads(ps, gs)
        opt.step()
        ref.step(gsplit([None if g is None else g.cpu().numpy() for g in gs]))
        for p, g in zip(ps, before):                                         # p.grad is not rewritten by the clip
            assert (p.grad is None) if g is None else torch.equal(p.grad, g)
        if max_norm is not None:
            assert abs(float(opt.grad_norm()) - nrm) <= 80 * U * nrm
    assert opt.skipped_steps() == 0
    _against_ref(opt, ref, capsys, case)


# ---- skip ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_gradient_skips_the_step(bad, capsys):
    from recguru_amd import hip
    from recguru_amd.optim import Adam
    ps = _params(51)
    grads = _grads(ps, 52, steps=3)
    grads[1][2][17, 3] = bad                                                 # ONE element of one gradient
    kw = dict(weight_decay=0.05)
    opt = Adam(ps, lr=LR, betas=BETAS, eps=EPS, max_norm=1.0, skip_nonfinite=True, **kw)
    ref = RefAdam([dict(params=[_np64(p) for p in ps], lr=LR, betas=BETAS, eps=EPS, **kw)], max_norm=1.0, skip_nonfinite=True)
    snap = None
    for i, gs in enumerate(grads):
        if i == 1:
            snap = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in ps[:-1]]
        _set_grads(ps, gs)
        opt.step()
        ref.step([[None if g is None else g.cpu().numpy() for g in gs]])
        if i == 1:
            for p, (p0, m0, v0) in zip(ps[:-1], snap):
                st = opt.state[p]
                for a, b in ((p, p0), (st["exp_avg"], m0), (st["exp_avg_sq"], v0)):
                    assert torch.equal(a.detach().view(torch.int32), b.view(torch.int32))
                assert st["step"] == 2                                       # a skipped step counts as a step
            assert opt.skipped_steps() == 1
            tbl = opt._tables["all"]["dev"].cpu().numpy().view(hip.ADAM_SEG_DEV_DTYPE)
            assert tbl["step"].tolist() == [2] * 6                           # ... on the device as well
            assert not math.isfinite(float(opt.grad_norm()))
    assert opt.skipped_steps() == 1 and ref.skipped == 1 and ps[-1] not in opt.state
    _against_ref(opt, ref, capsys, "clean step after a skipped one (%s)" % bad)


# ---- state --------------------------------------------------------------------------------------------------------------------
def test_state_dict_roundtrip_keeps_the_bits():
    from recguru_amd.optim import Adam
    mk = lambda ps: Adam([{"params": ps[:3], "weight_decay": 0.1}, {"params": ps[3:], "weight_decay": 0.02, "decoupled": True}],
                         lr=LR, betas=BETAS, eps=EPS, max_norm=5.0, skip_nonfinite=True)
    ps = _params(61)
    grads = _grads(ps, 62, steps=3)
    opt = mk(ps)
    for gs in grads[:2]:
        _set_grads(ps, gs)
        opt.step()
    sd = opt.state_dict()
    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt2 = Adam([{"params": ps2[:3]}, {"params": ps2[3:]}], max_norm=5.0, skip_nonfinite=True)     # options come from the checkpoint
    opt2.load_state_dict(sd)
    assert [(g["weight_decay"], g["decoupled"], g["lr"]) for g in opt2.param_groups] == [(0.1, False, LR), (0.02, True, LR)]
    for o, pp in ((opt, ps), (opt2, ps2)):
        _set_grads(pp, grads[2])
        o.step()
    for a, b in zip(ps, ps2):
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))
        if a in opt.state:
            assert opt.state[a]["step"] == opt2.state[b]["step"] == 3
            assert torch.equal(opt.state[a]["exp_avg_sq"], opt2.state[b]["exp_avg_sq"])


def test_torch_adamw_checkpoint_loads_and_continues(capsys):
    """A torch.optim.AdamW state dict (weight_decay = 0.05) after two CPU steps; the next step here against the restatement started
    from that same state."""
    from recguru_amd.optim import Adam
    ps = _params(71)[:4]
    grads = _grads(ps, 72, steps=3, dead_last=False)
    tp = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    topt = torch.optim.AdamW(tp, lr=LR, betas=BETAS, eps=EPS, weight_decay=0.05)
    for gs in grads[:2]:
        for p, g in zip(tp, gs):
            p.grad = g.cpu().clone()
        topt.step()
    with torch.no_grad():
        for p, t in zip(ps, tp):
            p.copy_(t)
    opt = Adam(ps)
    opt.load_state_dict(topt.state_dict())
    g0 = opt.param_groups[0]
    assert (g0["weight_decay"], g0["decoupled"], g0["lr"], tuple(g0["betas"])) == (0.05, True, LR, BETAS)
    ref = RefAdam([dict(params=[_np64(t) for t in tp], lr=LR, betas=BETAS, eps=EPS, weight_decay=0.05, decoupled=True)])
    ref.groups[0]["m"] = [_np64(topt.state[t]["exp_avg"]) for t in tp]
    ref.groups[0]["v"] = [_np64(topt.state[t]["exp_avg_sq"]) for t in tp]
    ref.groups[0]["t"] = [2] * len(tp)
    _set_grads(ps, grads[2])
    opt.step()
    ref.step([[g.cpu().numpy() for g in grads[2]]])
    _against_ref(opt, ref, capsys, "step 3 behind a torch.optim.AdamW checkpoint")


# ---- driver level -------------------------------------------------------------------------------------------------------------
def test_recon_step_clips_and_decays_through_opt_rec(capsys):
    """Two-layer d = 128 MyAuto4Rec_c, B = 4, L = 16, f32 tier: one training.recon_step with param.clip_norm / param.weight_decay
    (decoupled) on opt_rec.  The parameters after it equal the restatement applied to the gradients and parameters read just before
    opt.step(), and opt.grad_norm() is the float64 norm of those gradients.  (Decoupled: on a first Adam step the update is
    lr * g / (|g| + eps), and a coupled g + wd * p that cancels to ~eps would be ill-conditioned in f32 -- the arithmetic of that form is
    held by the cases above.)  clip_norm comes from a first, unclipped pass over the same batch: 0.1 x its norm."""
    from recguru_amd import config, hip, models, ops, optim, synthetic, training as T
    B, L, d, H, N, V, k = 4, 16, 128, 4, 2, 300, 3
    ops.set_compute_dtype(torch.float32)
    args = make_args(d, H, k, L, V, V, N, B, weight_decay=0.05, decoupled_wd=True, clip_norm=0.0)
    torch.manual_seed(81)
    G = models.MyAuto4Rec_c("cuda", config.get_param(args, make_dirs=False), wf=None, enc_share=True, dec_rec=False).to(torch.float32).cuda()
    G.train()
    state0 = {kk: v.clone() for kk, v in G.state_dict().items()}
    bt = []
    for s in (82, 83):
        dm = synthetic.make_domain(B, V, L, k, seed=s, min_len=3)
        bt.append(tuple(torch.as_tensor(dm[n]).cuda() for n in ("enc_in", "dec_in", "dec_out", "n_items")))
    params = list(G.parameters())
    cap = {}

    def run(param):
        opt = optim.Adam(params, lr=1e-3, betas=(0.9, 0.98), eps=1e-9, **optim.options(param))
        real = opt.step

        def step():
            cap["p"] = [_np64(p) for p in params]
            cap["g"] = [None if p.grad is None else p.grad.detach().cpu().numpy().copy() for p in params]
            real()
        opt.step = step
        T.recon_step(G, opt, bt[0], bt[1], param, "cuda", T._NoDP(), params, True, "s_soft", "org")
        return opt
    run(config.get_param(args, make_dirs=False))
    norm0 = math.sqrt(total_sq(cap["g"]))
    assert norm0 > 0 and sum(g is not None for g in cap["g"]) > 10
    G.load_state_dict(state0)
    args.clip_norm = 0.1 * norm0
    param = config.get_param(args, make_dirs=False)
    assert param.clip_norm == args.clip_norm and param.weight_decay == 0.05 and param.decoupled_wd
    opt = run(param)
    assert opt.max_norm == param.clip_norm and not opt._neutral()
    norm = math.sqrt(total_sq(cap["g"]))
    assert 0.5 * norm0 < norm < 2 * norm0                                     # the clamp is active by a factor ~10
    nsegs = opt._tables["all"]["n"]
    chain = hip.sqnorm_chain(hip.ADAM_CHUNK, nsegs)
    got = float(opt.grad_norm())
    with capsys.disabled():
        print("\n[adamw] recon_step: %d segments, grad_norm %.9g vs f64 %.9g (rel %.3g, bound %.3g)"
              % (nsegs, got, norm, abs(got - norm) / norm, (chain + 1) * U))
    assert abs(got - norm) <= (chain + 1) * U * norm
    ref = RefAdam([dict(params=cap["p"], lr=1e-3, betas=(0.9, 0.98), eps=1e-9, weight_decay=0.05, decoupled=True)], max_norm=param.clip_norm)
    ref.step([cap["g"]])
    _against_ref(opt, ref, capsys, "recon_step with clip_norm and weight_decay on opt_rec")
    assert T.norm_of(opt) is not None and T.norm_of(optim.Adam(params)) is None


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_rg_err_invalid():
    from recguru_amd import hip
    ps = _params(91)[:2]
    _set_grads(ps, _grads(ps, 92, steps=1, dead_last=False)[0])
    tbl, n, live = _table(ps)
    before = [p.detach().clone() for p in ps]
    partial, ctl = torch.zeros(n, device="cuda"), _ctl()
    with pytest.raises(RuntimeError, match=r"rg_adam_multi_dev2 failed \(-1\): adam_multi_dev2: weight_decay < 0"):
        hip.adam_multi_dev2(tbl, n, LR, 0.5, 0.9, EPS, -0.1, False, None)
    with pytest.raises(RuntimeError, match=r"rg_adam_multi_dev2 failed \(-1\): adam_multi_dev2: nsegs < 1"):
        hip.adam_multi_dev2(tbl, 0, LR, 0.5, 0.9, EPS, 0.0, False, None)
    with pytest.raises(RuntimeError, match=r"rg_adam_multi_dev2 failed \(-1\): adam_multi_dev2: null segment table"):
        hip.adam_multi_dev2(None, 1, LR, 0.5, 0.9, EPS, 0.0, False, None)
    with pytest.raises(RuntimeError, match=r"rg_grad_sqnorm_multi failed \(-1\): grad_sqnorm_multi: max_norm < 0"):
        hip.grad_sqnorm_multi(tbl, n, partial, ctl, -1.0, False)
    with pytest.raises(RuntimeError, match=r"rg_grad_sqnorm_multi failed \(-1\): grad_sqnorm_multi: nsegs < 1"):
        hip.grad_sqnorm_multi(tbl, 0, partial, ctl, 1.0, False)
    with pytest.raises(RuntimeError, match=r"rg_grad_sqnorm_multi failed \(-1\): grad_sqnorm_multi: null partial buffer or control record"):
        hip.grad_sqnorm_multi(tbl, n, partial, None, 1.0, False)
    torch.cuda.synchronize()
    for p, b in zip(ps, before):                                             # nothing was launched
        assert torch.equal(p, b)
    assert _read_ctl(ctl)["total_sq"] == 0.0
