"""GPU tests of the weight average the Adam update keeps (rg_adam_multi_dev3, rg_ema_swap_multi in csrc/optim.hip; ema_decay /
ema_warmup, swap_ema() and averaged() in recguru_amd/optim.py), against the float64 restatement of tests/ema_ref.py (which
tests/test_ema_cpu.py holds to hand-computed values).

Parameters: 1, 3, 5, 64, 4 099 and 65 536 + 7 elements (two chunks of the segment table), a 131-element view that starts one element
into its storage (misaligned: the scalar walk) and a 7-element parameter that never gets a gradient.  Eight steps unless a test says
otherwise, lr = 1e-2, betas = (0.5, 0.9), randn gradients.

Bounds.  Bit equality wherever the same arithmetic runs twice.  The average against float64: rtol 1e-5 / atol 1e-6, the bound
tests/test_adamw_gpu.py holds the update to -- the average is a convex combination of those weights; each case prints its share."""
import numpy as np
import pytest
import torch

from ema_ref import RefEmaAdam, decay_at
from parity_util import make_args

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-6
LR, BETAS, EPS = 1e-2, (0.5, 0.9), 1e-8
SIZES = (1, 3, 5, 64, 4099, 65536 + 7)
VIEW, DEAD = len(SIZES), len(SIZES) + 1                 # indices of the misaligned view and of the parameter without a gradient
SPECIALS = [0x7fc00001, -0x3edcbb, 0x7f800001, -0x80000000, 0x00000001, -0x7f800001, 0x7fffffff, 0x00000000]
#           quiet NaN + payload, negative NaN + payload (0xffc12345), signalling NaN, -0.0, smallest denormal, negative denormal
#           (0x807fffff), NaN all ones, +0.0


@pytest.fixture(autouse=True)
def _restore_tier():
    from recguru_amd import ops
    yield
    ops.set_compute_dtype(torch.bfloat16)


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g).cuda()) for n in SIZES]
    base = torch.randn(132, generator=g).cuda()
    ps.append(torch.nn.Parameter(base[1:]))
    assert ps[VIEW].data_ptr() % 16 == 4
    ps.append(torch.nn.Parameter(torch.randn(7, generator=g).cuda()))
    return ps


def _clones(ps):
    """Fresh parameters with the same values and the same alignment (the view stays a view one element into its storage)."""
    out = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    base = torch.zeros(132, device="cuda")
    base[1:].copy_(ps[VIEW].detach())
    out[VIEW] = torch.nn.Parameter(base[1:])
    assert out[VIEW].data_ptr() % 16 == 4
    return out


def _grads(ps, seed, steps=8):
    g = torch.Generator().manual_seed(seed)
    out = [[torch.randn(*p.shape, generator=g).cuda() for p in ps] for _ in range(steps)]
    for gs in out:
        gs[DEAD] = None
    return out


def _set_grads(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else g.clone()


def _np64(t):
    return t.detach().double().cpu().numpy()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _share(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / (ATOL + RTOL * np.abs(b)))) if a.size else 0.0


def _ref(ps, **kw):
    opt_kw = {k: kw.pop(k) for k in ("max_norm", "skip_nonfinite", "ema_decay", "ema_warmup") if k in kw}
    return RefEmaAdam([dict(params=[_np64(p) for p in ps], lr=LR, betas=BETAS, eps=EPS, **kw)], **opt_kw)


def _np_grads(gs):
    return [[None if g is None else g.cpu().numpy() for g in gs]]


def _ema_share(opt, ref, ps):
    """Worst share of the bound over every average (and: which parameters have one agrees with the restatement)."""
    worst = 0.0
    for i, p in enumerate(ps):
        want = ref.groups[0]["ema"][i]
        st = opt.state.get(p)
        if want is None:
            assert st is None or "ema" not in st, i
            continue
        assert st["step"] == ref.groups[0]["t"][i]
        worst = max(worst, _share(_np64(st["ema"]), want))
    return worst


# ---- 1. weights and moments do not notice the average ----------------------------------------------------------------------------
CASES = {
    "neutral": dict(),
    "coupled_decay_and_clip": dict(weight_decay=0.05, max_norm=1.0),
    "decoupled_decay": dict(weight_decay=0.05, decoupled=True),
    "skip_one_nonfinite_step": dict(max_norm=1.0, skip_nonfinite=True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_weights_and_moments_have_the_bits_of_the_optimizer_without_the_average(case):
    from recguru_amd import hip
    from recguru_amd.optim import Adam
    pa, pb = _params(11), _params(11)
    grads = _grads(pa, 12)
    if case.startswith("skip"):
        grads[3][4][17] = float("inf")
    on = Adam(pa, lr=LR, betas=BETAS, eps=EPS, ema_decay=0.9, ema_warmup=True, **CASES[case])
    off = Adam(pb, lr=LR, betas=BETAS, eps=EPS, **CASES[case])
    assert off._neutral() == (case == "neutral") and not on._neutral()
    for gs in grads:
        _set_grads(pa, gs)
        _set_grads(pb, gs)
        on.step()
        off.step()
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert _same(a, b), (case, i)
        if i == DEAD:
            assert a not in on.state and b not in off.state
            continue
        sa, sb = on.state[a], off.state[b]
        assert sa["step"] == sb["step"] == 8 and "ema" in sa and "ema" not in sb
        assert _same(sa["exp_avg"], sb["exp_avg"]) and _same(sa["exp_avg_sq"], sb["exp_avg_sq"]), (case, i)
    if case.startswith("skip"):
        assert on.skipped_steps() == off.skipped_steps() == 1
    tbl = on._tables["all"]["dev"].cpu().numpy().view(hip.ADAM_SEG_DEV_DTYPE)
    assert tbl["step"].tolist() == [8] * (len(SIZES) + 2)                    # seven live parameters, one of them in two chunks


# ---- 2. the average against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("decay", [0.9, 0.999])
def test_average_against_the_restatement(decay, warmup, capsys):
    from recguru_amd.optim import Adam
    ps = _params(21)
    grads = _grads(ps, 22, steps=20)
    opt = Adam(ps, lr=LR, betas=BETAS, eps=EPS, ema_decay=decay, ema_warmup=warmup)
    ref = _ref(ps, ema_decay=decay, ema_warmup=warmup)
    worst = 0.0
    for gs in grads:
        _set_grads(ps, gs)
        opt.step()
        ref.step(_np_grads(gs))
        worst = max(worst, _ema_share(opt, ref, ps))
    wp = max(_share(_np64(p), r) for p, r in zip(ps, ref.groups[0]["params"]))
    with capsys.disabled():
        print("\n[ema] decay %g warmup %s, 20 steps: worst |gpu - f64| / (%.0e + %.0e |f64|): average %.3g, weights %.3g"
              % (decay, warmup, ATOL, RTOL, worst, wp))
    assert worst <= 1.0, worst
    assert ps[DEAD] not in opt.state
    # the average is not the weights: at these decays it trails them by far more than the bound
    assert _share(_np64(opt.state[ps[4]]["ema"]), _np64(ps[4])) > 100


# ---- 3. ema_decay = 0 -----------------------------------------------------------------------------------------------------------
def test_zero_decay_average_has_the_bits_of_the_weights():
    from recguru_amd.optim import Adam
    ps = _params(31)
    opt = Adam(ps, lr=LR, betas=BETAS, eps=EPS, ema_decay=0.0, weight_decay=0.01)
    for gs in _grads(ps, 32):
        _set_grads(ps, gs)
        opt.step()
        for i, p in enumerate(ps[:DEAD]):
            assert _same(opt.state[p]["ema"], p), i


# ---- 4. a skipped step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_skipped_step_leaves_the_average_and_counts(bad, capsys):
    from recguru_amd.optim import Adam
    ps = _params(41)
    grads = _grads(ps, 42, steps=4)
    grads[1][5][65536 + 3] = bad                                             # ONE element, in the second chunk of the big parameter
    opt = Adam(ps, lr=LR, betas=BETAS, eps=EPS, skip_nonfinite=True, ema_decay=0.999, ema_warmup=True)
    ref = _ref(ps, skip_nonfinite=True, ema_decay=0.999, ema_warmup=True)
    for i, gs in enumerate(grads):
        if i == 1:
            snap = [(p.detach().clone(),) + tuple(opt.state[p][k].clone() for k in ("exp_avg", "exp_avg_sq", "ema")) for p in ps[:DEAD]]
        _set_grads(ps, gs)
        opt.step()
        ref.step(_np_grads(gs))
        if i == 1:
            for p, (p0, m0, v0, e0) in zip(ps[:DEAD], snap):
                st = opt.state[p]
                assert _same(p, p0) and _same(st["exp_avg"], m0) and _same(st["exp_avg_sq"], v0) and _same(st["ema"], e0)
                assert st["step"] == 2                                       # a skipped step counts as a step
            assert opt.skipped_steps() == 1
        if i == 2:
            # step 3 of the count: d = 4/13, where a count that had not advanced would give 3/12
            assert decay_at(0.999, True, 3) == 4.0 / 13.0
            share = _ema_share(opt, ref, ps)
            with capsys.disabled():
                print("\n[ema] first step behind a skipped one (%s): share of the bound %.3g" % (bad, share))
            assert share <= 1.0
            stale = [0.25 * _np64(e0) + 0.75 * _np64(p) for p, (_, _, _, e0) in zip(ps[:DEAD], snap)]
            assert _share(_np64(opt.state[ps[4]]["ema"]), stale[4]) > 10     # ... and the bound tells the two apart
    assert ref.skipped == 1 and _ema_share(opt, ref, ps) <= 1.0


# ---- 5. late and absent gradients -------------------------------------------------------------------------------------------------
def test_late_and_absent_gradients(capsys):
    from recguru_amd.optim import Adam
    d = 0.9
    ps, pf = _params(51), _params(51)
    grads = _grads(ps, 52)
    full = [list(gs) for gs in grads]
    LATE, GONE = 1, 4
    for i, gs in enumerate(grads):
        if i < 2:
            gs[LATE] = None                                                  # its gradient appears from step 3
        if i >= 4:
            gs[GONE] = None                                                  # its gradient disappears behind step 4
    opt = Adam(ps, lr=LR, betas=BETAS, eps=EPS, ema_decay=d)
    ful = Adam(pf, lr=LR, betas=BETAS, eps=EPS, ema_decay=d)
    ref = _ref(ps, ema_decay=d)
    for i, (gs, fs) in enumerate(zip(grads, full)):
        before = ps[LATE].detach().clone()
        if i == 4:
            gone = (ps[GONE].detach().clone(), opt.state[ps[GONE]]["ema"].clone())
        _set_grads(ps, gs)
        _set_grads(pf, fs)
        opt.step()
        ful.step()
        ref.step(_np_grads(gs))
        if i < 2:
            assert ps[LATE] not in opt.state and _same(ps[LATE], before)
        if i == 2:
            st = opt.state[ps[LATE]]
            assert st["step"] == 1
            want = d * _np64(before) + (1.0 - d) * _np64(ps[LATE])           # started from its value before step 3
            assert _share(_np64(st["ema"]), want) <= 1.0
        if i >= 4:
            assert _same(ps[GONE], gone[0]) and _same(opt.state[ps[GONE]]["ema"], gone[1]) and opt.state[ps[GONE]]["step"] == 4
    share = _ema_share(opt, ref, ps)
    with capsys.disabled():
        print("\n[ema] late / absent gradients: share of the bound %.3g" % share)
    assert share <= 1.0
    for i in range(DEAD):                                                    # the others: the bits of a run where nothing is absent
        if i not in (LATE, GONE):
            assert _same(ps[i], pf[i]) and _same(opt.state[ps[i]]["ema"], ful.state[pf[i]]["ema"]), i
    assert ps[DEAD] not in opt.state
    dead = ps[DEAD].detach().clone()
    opt.swap_ema()
    assert _same(ps[DEAD], dead) and not _same(ps[0], pf[0])
    opt.swap_ema()
    assert _same(ps[DEAD], dead) and _same(ps[0], pf[0])


# ---- 6. swap ----------------------------------------------------------------------------------------------------------------------
def _plant(t, seed):
    """Random 32-bit words over the whole range (NaNs with payloads, infinities, denormals among them) with the special words in front."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(-2 ** 31, 2 ** 31, (t.numel(),), generator=g, dtype=torch.int64).to(torch.int32)
    k = min(len(SPECIALS), t.numel())
    w[:k] = torch.tensor(SPECIALS[seed % len(SPECIALS):] + SPECIALS[:seed % len(SPECIALS)], dtype=torch.int64).to(torch.int32)[:k]
    t.detach().view(torch.int32).copy_(w.cuda().reshape(t.shape))
    return w.cuda()


def test_swap_exchanges_raw_words_and_guards_the_optimizer():
    from recguru_amd.optim import Adam
    ps = _params(61)
    grads = _grads(ps, 62, steps=2)
    opt = Adam(ps, lr=LR, betas=BETAS, eps=EPS, ema_decay=0.9)
    _set_grads(ps, grads[0])
    opt.step()
    wp = [_plant(p, 2 * i) for i, p in enumerate(ps[:DEAD])]
    we = [_plant(opt.state[p]["ema"], 2 * i + 1) for i, p in enumerate(ps[:DEAD])]
    dead = ps[DEAD].detach().clone()
    assert opt.ema_swapped is False
    opt.swap_ema()
    assert opt.ema_swapped is True
    for i, p in enumerate(ps[:DEAD]):
        assert torch.equal(_bits(p).reshape(-1), we[i]) and torch.equal(_bits(opt.state[p]["ema"]).reshape(-1), wp[i]), i
    assert _same(ps[DEAD], dead)
    _set_grads(ps, grads[1])
    for call in (opt.step, opt.state_dict, lambda: opt.load_state_dict({"state": {}, "param_groups": []})):
        with pytest.raises(RuntimeError, match="averaged weights"):
            call()
    for i, p in enumerate(ps[:DEAD]):                                        # the refused calls wrote nothing
        assert torch.equal(_bits(p).reshape(-1), we[i]), i
    opt.swap_ema()
    assert opt.ema_swapped is False
    for i, p in enumerate(ps[:DEAD]):
        assert torch.equal(_bits(p).reshape(-1), wp[i]) and torch.equal(_bits(opt.state[p]["ema"]).reshape(-1), we[i]), i
    with pytest.raises(ZeroDivisionError):
        with opt.averaged():
            assert opt.ema_swapped and torch.equal(_bits(ps[4]).reshape(-1), we[4])
            1 / 0
    assert opt.ema_swapped is False
    for i, p in enumerate(ps[:DEAD]):
        assert torch.equal(_bits(p).reshape(-1), wp[i]) and torch.equal(_bits(opt.state[p]["ema"]).reshape(-1), we[i]), i


def test_swap_entry_point_on_a_hand_built_table():
    """rg_ema_swap_multi itself: three pairs -- aligned, misaligned (word walk), and an aligned one whose length leaves a word tail."""
    from recguru_amd import hip
    base = torch.zeros(4 * 1031, device="cuda")
    a = [base[0:1028], base[1033:1033 + 515], base[2064:2064 + 1027]]
    b = [torch.zeros(n, device="cuda") for n in (1028, 515, 1027)]
    assert a[1].data_ptr() % 16 == 4 and a[2].data_ptr() % 16 == 0
    wa = [_plant(t, i) for i, t in enumerate(a)]
    wb = [_plant(t, i + 3) for i, t in enumerate(b)]
    guard = base.clone()
    tbl = np.array([(x.data_ptr(), y.data_ptr(), x.numel()) for x, y in zip(a, b)], dtype=hip.EMA_PAIR_DTYPE)
    dev = torch.from_numpy(tbl.view(np.uint8).copy()).cuda()
    hip.ema_swap_multi(dev, 3)
    for i in range(3):
        assert torch.equal(_bits(a[i]), wb[i]) and torch.equal(_bits(b[i]), wa[i]), i
    moved = torch.zeros_like(base, dtype=torch.bool)
    for lo, n in ((0, 1028), (1033, 515), (2064, 1027)):
        moved[lo:lo + n] = True
    assert torch.equal(_bits(base)[~moved], _bits(guard)[~moved])            # nothing outside the three ranges
    hip.ema_swap_multi(dev, 3)
    for i in range(3):
        assert torch.equal(_bits(a[i]), wa[i]) and torch.equal(_bits(b[i]), wb[i]), i


# ---- 7. cached copies -------------------------------------------------------------------------------------------------------------
def _tiny(seed, k=3, **kw):
    """B = 4, L = 8, d_model = 128, 4 heads, 1 layer, 50 items."""
    from recguru_amd import config, models, synthetic
    B, L, d, H, N, V = 4, 8, 128, 4, 1, 50
    param = config.get_param(make_args(d, H, k, L, V, V, N, B, **kw), make_dirs=False)
    torch.manual_seed(seed)
    G = models.MyAuto4Rec_c("cuda", param, wf=None, enc_share=True, dec_rec=False).to(torch.float32).cuda()
    doms = [synthetic.make_domain(B, V, L, k, seed=s, min_len=3) for s in (2 * seed + 1, 2 * seed + 2)]
    bt = [tuple(torch.as_tensor(dm[n]).cuda() for n in ("enc_in", "dec_in", "dec_out", "n_items")) for dm in doms]
    return param, G, bt


def _outputs(G, bt, param):
    """Forward passes in eval mode (no dropout), per domain: the user embeddings (encoder) and the recommender decoder's states, whose
    kernels sum in a fixed order -- compared bit for bit -- and the reconstruction loss, which reads the reconstruction decoder's copies
    too but is summed with float atomics: it is run for its hand-outs and returned apart."""
    from recguru_amd import training as T
    out, losses = [], []
    with torch.no_grad():
        for dom, b in zip("ab", bt):
            out.append(T.get_user_embed(G, b[0], dom, param, "cuda", 0).float().clone())
            m_in = T.get_pad_mask(b[1], param.pad_index, "cuda")
            out.append(G.recommend_forward(b[0], b[1], dom, m_in.view(-1, param.rec_maxlen)).float().clone())
            mask = T.get_pad_mask(b[2], param.pad_index, "cuda")
            losses.append(float(T.loss_ae(G, b[0], b[1], b[2], b[3], True, b[2].shape[0], b[2].shape[1], param, mask, "cuda", dom)))
    return out, losses


def _which(xs, ys):
    """Indices of the outputs whose bits differ."""
    return [i for i, (x, y) in enumerate(zip(xs, ys)) if not _same(x, y)]


@pytest.mark.parametrize("tier", ["bf16", "f32"])
def test_cached_copies_follow_the_swap(tier, monkeypatch, capsys):
    import shadow_audit as A
    from recguru_amd import hip, models, ops, optim, training as T
    ops.set_compute_dtype(torch.bfloat16 if tier == "bf16" else torch.float32)
    audit = A.Audit(ops, hip, optim).install(monkeypatch)
    param, G, bt = _tiny(71)
    G.train()
    params = list(G.parameters())
    opt = optim.Adam(params, lr=1e-3, betas=(0.9, 0.98), eps=1e-9, ema_decay=0.9)
    for _ in range(3):
        T.recon_step(G, opt, bt[0], bt[1], param, "cuda", T._NoDP(), params, True, "s_soft", "org")
    G.eval()
    raw, raw_loss = _outputs(G, bt, param)
    n_avg = sum("ema" in st for st in opt.state.values())
    assert 10 < n_avg <= len(params)
    handed = sum(audit.handouts.values())
    opt.swap_ema()
    audit.sweep()                                                            # every current cache entry against the masters as they are NOW
    avg, avg_loss = _outputs(G, bt, param)                                   # ... and every hand-out of these passes (StaleError otherwise)
    assert sum(audit.handouts.values()) > handed and len(_which(raw, avg)) == len(raw)
    opt.swap_ema()
    audit.sweep()
    back, back_loss = _outputs(G, bt, param)
    assert _which(raw, back) == []
    np.testing.assert_allclose(back_loss, raw_loss, rtol=1e-6)
    # a copy of the model whose parameters were loaded with the averages computes the same bits as the model under averaged()
    G2 = models.MyAuto4Rec_c("cuda", param, wf=None, enc_share=True, dec_rec=False).to(torch.float32).cuda()
    G2.load_state_dict(G.state_dict())
    with torch.no_grad():
        for p, q in zip(params, G2.parameters()):
            st = opt.state.get(p)
            if st is not None and "ema" in st:
                q.copy_(st["ema"])
    G2.eval()
    want, want_loss = _outputs(G2, bt, param)
    with opt.averaged():
        got, got_loss = _outputs(G, bt, param)
    assert _which(got, want) == [] and _which(got, avg) == []
    np.testing.assert_allclose(got_loss, want_loss, rtol=1e-6)
    np.testing.assert_allclose(avg_loss, want_loss, rtol=1e-6)
    assert _which(_outputs(G, bt, param)[0], raw) == []
    with capsys.disabled():
        print("\n[ema] cached copies, %s tier: %s; %d of %d parameters averaged" % (tier, audit.report(), n_avg, len(params)))


# ---- 8. checkpoints ---------------------------------------------------------------------------------------------------------------
def test_checkpoint_roundtrip_keeps_the_bits_average_included():
    from recguru_amd.optim import Adam
    kw = dict(lr=LR, betas=BETAS, eps=EPS, weight_decay=0.05, max_norm=5.0, ema_decay=0.99, ema_warmup=True)
    ps = _params(81)
    grads = _grads(ps, 82)
    opt = Adam(ps, **kw)
    for gs in grads[:4]:
        _set_grads(ps, gs)
        opt.step()
    sd = opt.state_dict()
    assert all("ema" in st for st in sd["state"].values()) and sorted(sd["state"]) == list(range(DEAD))
    assert sd["state"][VIEW]["ema"].data_ptr() != opt.state[ps[VIEW]]["ema"].data_ptr()      # a copy, as exp_avg is
    ps2 = _clones(ps)
    opt2 = Adam(ps2, **kw)
    opt2.load_state_dict(sd)
    for gs in grads[4:]:
        for o, pp in ((opt, ps), (opt2, ps2)):
            _set_grads(pp, gs)
            o.step()
    for i, (a, b) in enumerate(zip(ps[:DEAD], ps2[:DEAD])):
        sa, sb = opt.state[a], opt2.state[b]
        assert sa["step"] == sb["step"] == 8
        assert _same(a, b) and _same(sa["ema"], sb["ema"]) and _same(sa["exp_avg"], sb["exp_avg"]) and _same(sa["exp_avg_sq"], sb["exp_avg_sq"]), i


def test_checkpoint_without_the_average_loads_and_starts_from_the_weights():
    from recguru_amd.optim import Adam
    d = 0.9
    ps = _params(91)
    grads = _grads(ps, 92, steps=3)
    plain = Adam(ps, lr=LR, betas=BETAS, eps=EPS)
    for gs in grads[:2]:
        _set_grads(ps, gs)
        plain.step()
    sd = plain.state_dict()
    assert not any("ema" in st for st in sd["state"].values())
    opt = Adam(ps, lr=LR, betas=BETAS, eps=EPS, ema_decay=d)
    opt.load_state_dict(sd)
    assert not any("ema" in st for st in opt.state.values())
    before = [p.detach().clone() for p in ps]
    _set_grads(ps, grads[2])
    opt.step()
    for i, p in enumerate(ps[:DEAD]):
        st = opt.state[p]
        assert st["step"] == 3
        assert _share(_np64(st["ema"]), d * _np64(before[i]) + (1.0 - d) * _np64(p)) <= 1.0, i
    # a torch.optim.Adam checkpoint too
    tp = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps[:3]]
    topt = torch.optim.Adam(tp, lr=LR, betas=BETAS, eps=EPS)
    for p, g in zip(tp, grads[0]):
        p.grad = g.cpu().clone()
    topt.step()
    qs = [torch.nn.Parameter(t.detach().cuda()) for t in tp]
    opt = Adam(qs, ema_decay=d)
    opt.load_state_dict(topt.state_dict())
    before = [q.detach().clone() for q in qs]
    _set_grads(qs, grads[1][:3])
    opt.step()
    for q, b in zip(qs, before):
        assert opt.state[q]["step"] == 2 and _share(_np64(opt.state[q]["ema"]), d * _np64(b) + (1.0 - d) * _np64(q)) <= 1.0


# ---- 9. option off ----------------------------------------------------------------------------------------------------------------
def test_option_off_never_reaches_the_new_entry_points(monkeypatch):
    from recguru_amd import hip
    from recguru_amd.optim import Adam, averaged

    def boom(*a, **k):
        raise AssertionError("the new entry points must not be reached with ema_decay off")
    monkeypatch.setattr(hip, "adam_multi_dev3", boom)
    monkeypatch.setattr(hip, "ema_swap_multi", boom)
    for kw in (dict(), dict(weight_decay=0.05, max_norm=1.0, skip_nonfinite=True)):
        ps, pr = _params(101), _params(101)
        opt = Adam(ps, lr=LR, betas=BETAS, eps=EPS, **kw)
        for gs in _grads(ps, 102, steps=2):
            _set_grads(ps, gs)
            opt.step()
            with averaged(opt):
                pass
            opt.swap_ema()
        assert opt.ema_swapped is False and not any("ema" in st for st in opt.state.values())
        assert not any("ema" in st for st in opt.state_dict()["state"].values())
        assert not _same(ps[0], pr[0])                                       # it did step
    with pytest.raises(AssertionError, match="must not be reached"):         # and the guard itself works
        ps = _params(101)
        _set_grads(ps, _grads(ps, 102, steps=1)[0])
        Adam(ps, ema_decay=0.5).step()


# ---- 10. driver -------------------------------------------------------------------------------------------------------------------
def test_recommendation_tune_evaluates_under_the_average(tmp_path, monkeypatch):
    from recguru_amd import ops, optim, synthetic, training as T
    ops.set_compute_dtype(torch.float32)
    param, G, _ = _tiny(111, ema_decay=0.9)
    param.result_path = str(tmp_path)
    assert param.ema_decay == 0.9 and param.n_bpr_neg == 5
    param.eval_step = 2
    B, L, V = 4, 8, 50
    loaders = []
    for s in (112, 113):
        dm = synthetic.make_domain(2 * B, V, L, param.n_bpr_neg, seed=s, min_len=3)
        loaders.append(synthetic.TensorLoader(dm, B, device="cuda"))
    made, log, seen = [], [], []

    class Recording(optim.Adam):
        def __init__(self, *a, **k):
            optim.Adam.__init__(self, *a, **k)
            made.append(self)

        def step(self):
            optim.Adam.step(self)
            p = next(q for g in self.param_groups for q in g["params"] if "ema" in self.state.get(q, {}))
            log.append((p, _bits(p).clone(), _bits(self.state[p]["ema"]).clone()))

    def fake_eval(model, loader, device, prm, k_val=None, sas=False, domain="a"):
        p = log[-1][0]
        seen.append((len(log), _bits(p).clone(), made[0].ema_swapped))
        names = ("ht_eval", "ndcg_eval", "mrr_eval", "ht_test", "ndcg_test", "mrr_test")
        return [{str(k): {n: [0.0] for n in names} for k in k_val} for _ in range(2)]
    monkeypatch.setattr(T, "Adam", Recording)
    monkeypatch.setattr(T, "evaluation_2", fake_eval)
    T.plot.reset()
    losses, result = T.recommendation_tune(G, loaders, object(), 5, param, "cuda", "a")
    assert len(losses) == 5 and len(made) == 1 and made[0].ema_decay == 0.9 and made[0].ema_warmup is False
    assert [n for n, _, _ in seen] == [2, 4]                                 # evaluated behind steps 2 and 4
    for n, words, swapped in seen:
        assert swapped is True
        assert torch.equal(words, log[n - 1][2]) and not torch.equal(words, log[n - 1][1])     # the average, not the raw weights
    p, words, avg = log[-1]
    assert made[0].ema_swapped is False and torch.equal(_bits(p), words) and torch.equal(_bits(made[0].state[p]["ema"]), avg)
    assert len(result[0]["10"]["ht_eval"]) == 2


def test_main_2_writes_the_averaged_weights_beside_the_raw_file(tmp_path, monkeypatch):
    """training.main_2 with phases 2 / 3 stubbed out: pre_model holds the raw weights as before, pre_model_ema the averages of the
    parameters phase 1 updated (raw values for the others), and the model is left with its raw weights.  Without the option there is
    no second file."""
    from recguru_amd import blocks, ops, optim, training as T
    ops.set_compute_dtype(torch.float32)
    zero = torch.zeros(4, dtype=torch.long)
    monkeypatch.setattr(T, "train_gan_all", lambda *a, **k: "history")
    for on in (True, False):
        param, G, bt = _tiny(131)
        param.model_path = str(tmp_path / ("on" if on else "off"))
        param.result_path = param.model_path
        (tmp_path / ("on" if on else "off")).mkdir()
        loaders = [[((b[0], b[1], b[2]), b[3], zero, zero)] * 4 for b in bt]
        inner = optim.Adam(G.parameters(), betas=(0.9, 0.98), eps=1e-9, **(dict(ema_decay=0.9) if on else {}))
        opt_rec = blocks.ScheduledOptim(inner, 1.0, param.d_model, 2)
        assert T.main_2(G, opt_rec, None, None, None, param, "cuda", loaders, None, None, None, phase1_steps=3) == "history"
        raw = torch.load(str(tmp_path / ("on" if on else "off") / "pre_model"), map_location="cuda", weights_only=True)
        now = G.state_dict()
        assert list(raw) == list(now) and all(_same(raw[k], now[k]) for k in raw if raw[k].dtype == torch.float32)
        if not on:
            assert sorted(p.name for p in (tmp_path / "off").iterdir()) == ["pre_model"]
            continue
        assert inner.ema_swapped is False
        avg = torch.load(str(tmp_path / "on" / "pre_model_ema"), map_location="cuda", weights_only=True)
        assert list(avg) == list(raw)
        names = {id(p): k for k, p in G.named_parameters()}
        n_avg = n_moved = 0
        for p in G.parameters():
            k, st = names[id(p)], inner.state.get(p)
            if st is not None and "ema" in st:
                n_avg += 1
                n_moved += not _same(avg[k], raw[k])                         # (a parameter whose gradient is all zeros does not move)
                assert _same(avg[k], st["ema"]), k
            else:
                assert _same(avg[k], raw[k]), k
        assert n_avg > 10 and n_moved > 10


# ---- 11. argument errors ----------------------------------------------------------------------------------------------------------
def test_argument_errors_are_rg_err_invalid():
    from recguru_amd import hip, optim
    ps = _params(121)[:3]
    _set_grads(ps, [torch.randn_like(p) for p in ps])
    live = [(p, {"step": 0, "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p), "ema": p.detach().clone()}) for p in ps]
    tbl = torch.from_numpy(np.array(optim._rows(live), dtype=hip.ADAM_SEG_DEV_DTYPE).view(np.uint8).copy()).cuda()
    ema = torch.from_numpy(np.array(optim._ema_rows(live), dtype=np.uint64).view(np.uint8).copy()).cuda()
    n = 3
    before = [[t.detach().clone() for t in (p, st["exp_avg"], st["exp_avg_sq"], st["ema"])] for p, st in live]
    tbl0 = tbl.clone()
    ok = dict(weight_decay=0.0, decoupled=False, ctl=None, ema_decay=0.9, ema_warmup=False)

    def call(t, e, nn, **kw):
        hip.adam_multi_dev3(t, e, nn, LR, 0.5, 0.9, EPS, **dict(ok, **kw))
    for args, kw, msg in (((tbl, None, n), {}, "null average table"), ((None, ema, n), {}, "null segment table"),
                          ((tbl, ema, 0), {}, "nsegs < 1"), ((tbl, ema, -2), {}, "nsegs < 1"),
                          ((tbl, ema, n), dict(weight_decay=-0.1), "weight_decay < 0"),
                          ((tbl, ema, n), dict(ema_decay=1.0), r"ema_decay outside \[0, 1\)"),
                          ((tbl, ema, n), dict(ema_decay=-0.01), r"ema_decay outside \[0, 1\)"),
                          ((tbl, ema, n), dict(ema_decay=1.5), r"ema_decay outside \[0, 1\)"),
                          ((tbl, ema, n), dict(ema_decay=float("nan")), r"ema_decay outside \[0, 1\)")):
        with pytest.raises(RuntimeError, match=r"rg_adam_multi_dev3 failed \(-1\): adam_multi_dev3: " + msg):
            call(*args, **kw)
    pairs = torch.from_numpy(np.array([(p.data_ptr(), st["ema"].data_ptr(), p.numel()) for p, st in live], dtype=hip.EMA_PAIR_DTYPE)
                             .view(np.uint8).copy()).cuda()
    with pytest.raises(RuntimeError, match=r"rg_ema_swap_multi failed \(-1\): ema_swap_multi: null pair table"):
        hip.ema_swap_multi(None, 3)
    with pytest.raises(RuntimeError, match=r"rg_ema_swap_multi failed \(-1\): ema_swap_multi: npairs < 1"):
        hip.ema_swap_multi(pairs, 0)
    torch.cuda.synchronize()
    for (p, st), b in zip(live, before):                                     # nothing was launched
        for t, t0 in zip((p, st["exp_avg"], st["exp_avg_sq"], st["ema"]), b):
            assert _same(t, t0)
    assert torch.equal(tbl, tbl0)
    call(tbl, ema, n)                                                        # the valid call does run: weights, average and counts move
    torch.cuda.synchronize()
    assert not _same(ps[2], before[2][0]) and not _same(live[2][1]["ema"], before[2][3])
    assert tbl.cpu().numpy().view(hip.ADAM_SEG_DEV_DTYPE)["step"].tolist() == [1, 1, 1]
