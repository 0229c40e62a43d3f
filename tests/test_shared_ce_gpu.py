"""Sampled softmax over one candidate list shared by the batch on the MI355X (csrc/shared_ce.hip, ops.SharedSoftmaxLoss,
models.SharedLogits, sampler.DeviceLoader(shared_negs=)): a float64 restatement (tests/shared_ce_ref.py) in every tier
and width, the two losses the objective reduces to, exact zeros, bit-identical repeats, batch invariance, the zero-count convention,
refusals, the model surface, the loader, a training loop and data-parallel normalisation.

Bounds are those of tests/test_full_softmax_gpu.py, whose kernels do the same arithmetic: the split-operand tiers (f32, bf16x3) hold
rtol 1e-3 / atol 1e-5 on the loss and 1e-3 max|ref| + 1e-5 on gradients; the bf16 tier holds BF16_BOUNDS (2e-2 of the loss, 6e-2 of
the largest gradient)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from shared_ce_ref import shared_ce_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TIERS = {"f32": torch.float32, "bf16x3": "bf16x3", "bf16": torch.bfloat16}
BF16_BOUNDS = {"loss_rel": 2e-2, "grad_rel_to_max": 6e-2}          # tests/test_full_softmax_gpu.py
B, L, ROWS = 48, 64, 2003


@pytest.fixture(autouse=True)
def _tier_reset():
    from recguru_amd import ops
    yield
    ops.set_compute_dtype(torch.bfloat16)


def _mask_of(lens):
    return (torch.arange(L)[None, :] >= (L - lens)[:, None]).to(torch.float32).reshape(-1)


def _problem(d, C, seed, rows=ROWS, biases=False, disjoint=False, lens=None):
    """h [B L, d], table [rows, d], targets, a sorted candidate list, a ragged left-padded mask with the sequences sorted by length --
    whole 16-row tiles dead as well as padded rows inside live tiles -- and, unless disjoint, >= 7 live rows whose target is a
    candidate (S[0] and S[C - 1] among them) and one live row whose target is the last row of the table."""
    g = torch.Generator().manual_seed(seed)
    if lens is None:
        lens = torch.sort(torch.randint(1, L + 1, (B,), generator=g))[0]
        lens[0] = 1
    mask = _mask_of(lens)
    tiles = mask.view(-1, 16)
    assert int((tiles.sum(1) == 0).sum()) > 0 and int(((tiles.sum(1) > 0) & (tiles.sum(1) < 16)).sum()) > 0
    h = torch.randn(B * L, d, generator=g) * 0.5
    table = torch.randn(rows, d, generator=g) * 0.3
    perm = torch.randperm(rows - 2, generator=g) + 1                     # 1 .. rows - 2
    cand = torch.sort(perm[:C])[0]
    live = torch.nonzero(mask).reshape(-1)
    if disjoint:
        pool = perm[C:]
        lab = pool[torch.randint(0, pool.numel(), (B * L,), generator=g)] * mask.long()
        assert not bool(torch.isin(lab, cand).any())
    else:
        lab = torch.randint(1, rows - 1, (B * L,), generator=g) * mask.long()
        pick = live[torch.randperm(live.numel(), generator=g)[:11]]
        lab[pick[:4]] = cand[0]
        lab[pick[4:8]] = cand[C - 1]
        lab[pick[8]] = cand[C // 2]
        lab[pick[9]] = rows - 1
        lab[pick[10]] = perm[C]                                          # a target outside S: the skip_row of the tests that take one
        hit = torch.isin(lab[live], cand)
        assert int(hit.sum()) >= 7 and bool((lab[live] == cand[0]).any()) and bool((lab[live] == cand[C - 1]).any())
        assert bool((lab[live] == rows - 1).any())
    cb = torch.randn(C, generator=g) if biases else None
    pb = torch.randn(B * L, generator=g) if biases else None
    dev = lambda t: None if t is None else t.cuda()
    return dict(h=dev(h), table=dev(table), lab=dev(lab), cand=dev(cand), mask=dev(mask), cb=dev(cb), pb=dev(pb), skip=int(perm[C]))


def _run(p, tier, skip_row=-1, fn=None):
    """loss, dh, dE of ops.shared_softmax_loss (or fn) in a tier; the bf16 tier's h is the rounded one, its table the f32 master."""
    from recguru_amd import ops
    ops.set_compute_dtype(TIERS[tier])
    hh = p["h"].to(ops.compute_dtype()).detach().requires_grad_(True)
    wp = torch.nn.Parameter(p["table"].clone())
    if fn is None:
        loss = ops.shared_softmax_loss(hh, wp, p["lab"], p["cand"], p["mask"], skip_row, p["cb"], p["pb"])
    else:
        loss = fn(ops, hh, wp)
    loss.backward()
    return float(loss.detach()), hh.grad.float(), wp.grad


def _hold(got, ref, tier, what):
    """got / ref = (loss, dh, dE); every figure is printed before it is judged."""
    lerr = abs(got[0] - ref[0])
    print("%s %s: loss %.9g ref %.9g |err| %.3g" % (what, tier, got[0], ref[0], lerr))
    if tier == "bf16":
        assert lerr <= BF16_BOUNDS["loss_rel"] * abs(ref[0]), (what, "loss", lerr)
    else:
        np.testing.assert_allclose(got[0], ref[0], rtol=1e-3, atol=1e-5, err_msg=what)
    for g, r, nm in ((got[1], ref[1], "dh"), (got[2], ref[2], "dE")):
        scale = float(r.abs().max())
        err = float((g.double() - r.double()).abs().max())
        print("%s %s: %s max|err| %.3g max|ref| %.3g" % (what, tier, nm, err, scale))
        if tier == "bf16":
            assert err <= BF16_BOUNDS["grad_rel_to_max"] * scale, (what, nm, err, scale)
        else:
            assert err <= 1e-3 * scale + 1e-5, (what, nm, err, scale)


def _ref(p, skip_row=-1):
    return shared_ce_ref(p["h"], p["table"], p["lab"], p["cand"], p["mask"], skip_row, p["cb"], p["pb"])[:3]


def _structure(p, got, skip_row):
    """dh of masked rows exactly 0; dE exactly 0 off the live targets and the candidates; dE[skip_row] without the target route."""
    loss, dh, dE = got
    assert float(dh[p["mask"] == 0].abs().max()) == 0.0
    touched = torch.zeros(p["table"].shape[0], dtype=torch.bool, device="cuda")
    touched[p["cand"]] = True
    touched[p["lab"][p["mask"] != 0]] = True
    assert int((~touched).sum()) > 0 and float(dE[~touched].abs().max()) == 0.0
    assert float(dE[p["table"].shape[0] - 1].abs().max()) > 0                    # the last row of the table, a target only


@pytest.mark.parametrize("C", [1, 17, 1001])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_float64_parity_bf16x3(d, C):
    biases = (d, C) == (128, 17)
    p = _problem(d, C, seed=100 + d + C, biases=biases)
    skip = p["skip"]                             # the target of a live row, not a candidate: nothing else reaches its row of dE
    got = _run(p, "bf16x3", skip_row=skip)
    ref = _ref(p, skip_row=skip)
    _hold(got, ref, "bf16x3", "d=%d C=%d" % (d, C))
    _structure(p, got, skip)
    # the target route into skip_row is what the two restatements differ by; the kernels leave that row untouched
    assert float(_ref(p)[2][skip].abs().max()) > 0 and float(ref[2][skip].abs().max()) == 0.0
    assert float(got[2][skip].abs().max()) == 0.0


@pytest.mark.parametrize("tier", list(TIERS))
def test_all_tiers(tier):
    p = _problem(128, 1001, seed=7)
    got = _run(p, tier)
    _hold(got, _ref(p), tier, "d=128 C=1001")
    _structure(p, got, -1)


@pytest.mark.parametrize("tier", ["bf16x3", "bf16"])
def test_single_candidate_equal_to_every_target_is_exactly_zero(tier):
    p = _problem(128, 1, seed=11)
    y = int(p["cand"][0])
    p["lab"] = torch.full_like(p["lab"], y) * p["mask"].long()
    loss, dh, dE = _run(p, tier)
    assert loss == 0.0 and float(dh.abs().max()) == 0.0 and float(dE.abs().max()) == 0.0


@pytest.mark.parametrize("tier", ["bf16x3", "bf16"])
def test_every_row_as_candidates_is_the_full_loss(tier):
    p = _problem(128, 17, seed=13)
    p["cand"] = torch.arange(ROWS, device="cuda")
    got = _run(p, tier)
    full = _run(p, tier, fn=lambda ops, hh, wp: ops.full_softmax_loss(hh, wp, p["lab"], p["mask"]))
    _hold(got, full, tier, "S = all rows vs full_softmax_loss")
    _hold(got, _ref(p), tier, "S = all rows vs float64")


@pytest.mark.parametrize("tier", list(TIERS))
def test_disjoint_candidates_is_the_per_position_loss(tier):
    p = _problem(128, 30, seed=17, disjoint=True)
    n = B * L
    neg = p["cand"].view(1, 30).expand(n, 30).contiguous()
    got = _run(p, tier)
    per = _run(p, tier, fn=lambda ops, hh, wp: ops.sampled_softmax_loss(hh, wp, p["lab"], neg, p["mask"], 30))
    _hold(got, per, tier, "disjoint S vs sampled_softmax_loss")
    _hold(got, _ref(p), tier, "disjoint S vs float64")


def _lens_with_sums(seed):
    """Sorted lengths from 1 whose first half sums to 256 and whose whole sums to 1024: the mask counts of the half and of the whole
    batch are powers of two, so 1 / count and the rescale by their ratio are exact in f32."""
    g = torch.Generator().manual_seed(seed)

    def part(lo, hi, total, first=None):
        v = torch.randint(lo, hi + 1, (B // 2,), generator=g)
        if first is not None:
            v[0] = first
        while int(v.sum()) != total:
            i = int(torch.randint(0 if first is None else 1, B // 2, (1,), generator=g))
            step = 1 if int(v.sum()) < total else -1
            if lo <= int(v[i]) + step <= hi:
                v[i] += step
        return torch.sort(v)[0]
    return torch.cat([part(1, 21, 256, first=1), part(21, 48, 768)])


def _raw(p, tier, sl=None):
    """hip-level forward + candidate route on the first sl rows: lse, dh, candidate part of the table gradient, loss sum."""
    from recguru_amd import hip, ops
    ops.set_compute_dtype(TIERS[tier])
    cut = (lambda t: t) if sl is None else (lambda t: t[:sl].contiguous())
    h, lab, mask = cut(p["h"].to(ops.compute_dtype())), cut(p["lab"]), cut(p["mask"])
    n = h.shape[0]
    sums = torch.zeros(2, device="cuda")
    sums[1] = mask.sum()
    live = hip.live_tiles(mask, n)
    table = p["table"].to(ops.compute_dtype())
    lse, wc, dh, coef = hip.shared_ce_fwd(h, table, lab, p["cand"], mask, live, sums, train=True)
    dE = torch.zeros(p["table"].shape, device="cuda")
    hip.shared_ce_bwd(h, table.shape[0], lab, p["cand"], mask, live, wc, lse, coef, sums, torch.ones(1, device="cuda"), dE,
                      target_route=False)
    torch.cuda.synchronize()
    return lse, dh.float(), dE, sums.clone(), mask


@pytest.mark.parametrize("tier", ["bf16x3", "bf16"])
def test_repeats_and_batch_invariance(tier):
    lens = _lens_with_sums(19)
    assert int(lens[:B // 2].sum()) == 256 and int(lens.sum()) == 1024 and bool((lens[1:] >= lens[:-1]).all()) and int(lens[0]) == 1
    p = _problem(128, 1001, seed=19, lens=lens)
    a, b = _raw(p, tier), _raw(p, tier)
    live = a[4] != 0
    assert torch.equal(a[0][live], b[0][live]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert float(a[2].abs().max()) > 0
    la, lb = _run(p, tier), _run(p, tier)
    assert la[0] == lb[0] and torch.equal(la[1], lb[1])
    # the first half of the sequences alone: a position's lse does not depend on which workgroup or wave walks it
    half = _raw(p, tier, sl=B // 2 * L)
    hl = half[4] != 0
    assert int(hl.sum()) == 256
    assert torch.equal(half[0][hl], a[0][:B // 2 * L][hl])
    # dh = v * (mask / count) with v a function of the row alone: 256 -> 1024 is a factor of exactly 1/4 (a power of two: it commutes
    # with the rounding of either storage type, no subnormals at these magnitudes), so one multiply reproduces the bits
    want = a[1][:B // 2 * L]
    resc = half[1] * 0.25
    w64, r64 = want.cpu().numpy().astype(np.float64), resc.cpu().numpy().astype(np.float64)
    ulp = np.spacing(np.abs(want.cpu().numpy())).astype(np.float64)
    print("batch invariance %s: max |diff| in f32 ulps %.3g" % (tier, float((np.abs(r64 - w64) / ulp).max())))
    assert (np.abs(r64 - w64) <= ulp).all()
    assert torch.equal(resc, want)


def _worker(args, env=None, timeout=600):
    e = dict(os.environ)
    e.pop("RG_DETERMINISTIC", None)
    e.update(env or {})
    p = subprocess.run([sys.executable, os.path.join(HERE, "shared_ce_worker.py")] + args, env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=timeout)
    assert p.returncode == 0, p.stdout.decode()[-3000:]


def test_deterministic_library_repeats_the_whole_table_gradient(tmp_path):
    out = str(tmp_path / "det.npz")
    _worker(["det", out], {"RG_DETERMINISTIC": "1"})
    r = np.load(out)
    assert int(r["det_fault"]) == 0
    for tier in ("bf16x3", "bf16"):
        for k in ("loss", "dh", "dE"):
            assert np.array_equal(r["%s.%s.0" % (k, tier)], r["%s.%s.1" % (k, tier)]), (tier, k)
        assert np.isfinite(r["dE.%s.0" % tier]).all() and np.abs(r["dE.%s.0" % tier]).max() > 0


@pytest.mark.parametrize("tier", ["bf16x3", "bf16"])
def test_no_live_row(tier):
    """mask all zero, C = 1, a table of two rows: what ops.full_softmax_loss returns for the same mask (the zero-count convention of
    tests/test_dead_rows_gpu.py), and no row of S or of the table read out of bounds."""
    g = torch.Generator().manual_seed(23)
    n = B * L
    p = dict(h=(torch.randn(n, 128, generator=g) * 0.5).cuda(), table=torch.randn(2, 128, generator=g).cuda(),
             lab=torch.ones(n, dtype=torch.long).cuda(), cand=torch.tensor([1]).cuda(), mask=torch.zeros(n).cuda(), cb=None, pb=None)
    got = _run(p, tier)
    full = _run(p, tier, fn=lambda ops, hh, wp: ops.full_softmax_loss(hh, wp, p["lab"], p["mask"]))
    assert np.array_equal(np.float32(got[0]), np.float32(full[0]), equal_nan=True)
    assert torch.equal(got[1], full[1]) and torch.equal(got[2], full[2])
    assert float(got[1].abs().max()) == 0.0 and float(got[2].abs().max()) == 0.0


def test_refusals():
    from recguru_amd import hip
    n = 64
    mask = torch.ones(n, device="cuda")
    lab = torch.ones(n, dtype=torch.long, device="cuda")
    sums = torch.tensor([0.0, float(n)], device="cuda")
    live = hip.live_tiles(mask, n)

    def call(d, cand, rows=50):
        h = torch.zeros(n, d, device="cuda", dtype=torch.bfloat16)
        table = torch.zeros(rows, d, device="cuda", dtype=torch.bfloat16)
        return hip.shared_ce_fwd(h, table, lab, torch.tensor(cand, dtype=torch.long, device="cuda"), mask, live, sums, train=True)
    torch.cuda.synchronize()
    assert not hip.shared_ce_supported(96, torch.zeros(1, dtype=torch.bfloat16)) and hip.shared_ce_supported(128, torch.zeros(1))
    with pytest.raises(RuntimeError, match=r"rg_shared_ce_fwd failed \(-2\): shared_ce_fwd: d must be 64, 128 or 256"):
        call(96, [1, 2, 3])
    with pytest.raises(RuntimeError, match=r"rg_shared_ce_fwd failed \(-1\): shared_ce_fwd: C must be in \[1, 2\^31\)"):
        call(128, [])
    with pytest.raises(RuntimeError, match=r"rg_shared_ce_fwd failed \(-1\): shared_ce_fwd: cand must be strictly ascending \(cand\[2\] = 4 after 7\)"):
        call(128, [1, 7, 4, 9])
    with pytest.raises(RuntimeError, match=r"rg_shared_ce_fwd failed \(-1\): shared_ce_fwd: cand must be strictly ascending \(cand\[1\] = 7 after 7\)"):
        call(128, [7, 7, 9])
    with pytest.raises(RuntimeError, match=r"rg_shared_ce_fwd failed \(-1\): shared_ce_fwd: cand\[2\] = 50 is outside the table rows \[0, 50\)"):
        call(128, [1, 7, 50])
    # the refusals launched nothing: the stream is clean and a supported call still answers (all-zero operands: lse = log(1 + 3))
    torch.cuda.synchronize()
    lse, wc, dh, coef = call(128, [2, 7, 9])
    torch.cuda.synchronize()
    np.testing.assert_allclose(lse.cpu().numpy(), np.log(4.0), rtol=1e-6)
    np.testing.assert_allclose(float(sums[0]), n * np.log(4.0), rtol=1e-5)


def _model_case(kind):
    from parity_util import make_args
    from recguru_amd import synthetic
    from recguru_amd.config import get_param
    from recguru_amd.models import MyAuto4Rec, MyAuto4Rec_c
    d, H, N, Bm, Lm, V, k = 128, 4, 1, 8, 32, 500, 5
    param = get_param(make_args(d, H, k, Lm, V, V, N, Bm), make_dirs=False)
    torch.manual_seed(3)
    if kind == "cross":
        model = MyAuto4Rec_c("cuda", param).to(torch.float32).to("cuda")
    else:
        model = MyAuto4Rec(param.vocab_size, d, 0, param.d_ff, param.d_k, param.d_v, H, N, "cuda", param).to(torch.float32).to("cuda")
    dm = synthetic.make_domain(Bm, V, Lm, k, seed=6, min_len=3)
    enc, din, dout, neg = (torch.as_tensor(dm[nm]).cuda() for nm in ("enc_in", "dec_in", "dec_out", "n_items"))
    g = torch.Generator().manual_seed(8)
    live_targets = torch.unique(dout[dout != 0])
    cand = torch.unique(torch.cat([torch.randint(1, V + 1, (60,), generator=g).cuda(), live_targets[:3]]))     # three accidental hits
    return param, model, enc, din, dout, neg, cand


@pytest.mark.parametrize("kind", ["cross", "single"])
def test_model_level(kind):
    from recguru_amd import ops, training
    from recguru_amd.models import SampledLogits, SharedLogits, check_recon_handle
    ops.set_compute_dtype(torch.float32)
    param, model, enc, din, dout, neg, cand = _model_case(kind)
    Bm, Lm = dout.shape
    if kind == "cross":
        mask = training.get_pad_mask(dout, param.pad_index, "cuda")
        fwd = lambda n_items: model(enc, din, dout, n_items, "a", mask)
        states = lambda: model.get_dec_out(enc, din, "a", mask)[0]
        table, skip = model.src_emb_a.weight, -1
    else:
        mask = (din != 0).view(-1).to(torch.float32)
        fwd = lambda n_items: model(enc, din, dout, n_items)
        states = lambda: model.get_dec_out(enc, din)[0]
        table, skip = model.src_emb.weight, 0
    logits = fwd(cand)
    assert isinstance(logits, SharedLogits) and check_recon_handle(logits, True) is logits
    assert isinstance(fwd(neg), SampledLogits)
    with pytest.raises(NotImplementedError, match="per-position negatives"):
        logits.bpr(mask)
    dense = logits.dense()
    assert tuple(dense.shape) == (Bm, Lm, 1 + cand.numel())
    hits = cand.view(1, 1, -1) == dout.unsqueeze(-1)
    assert int(hits.sum()) > 0 and bool(torch.isinf(dense[..., 1:][hits]).all()) and bool(torch.isfinite(dense[..., 1:][~hits]).all())
    # the loss: the restatement fed with the model's own decoder states
    model.zero_grad()
    if kind == "cross":
        loss = training.loss_ae(model, enc, din, dout, cand, True, Bm, Lm, param, mask, "cuda", "a")
    else:
        loss = check_recon_handle(logits, True).loss(mask)
    loss.backward()
    total = table.grad.detach().clone()
    model.zero_grad()
    h = states()
    ref_loss, ref_dh, ref_dE, _ = shared_ce_ref(h.detach().reshape(-1, h.shape[-1]), table.detach(), dout.reshape(-1), cand, mask, skip)
    np.testing.assert_allclose(float(loss.detach()), ref_loss, rtol=1e-3, atol=1e-5)
    # the table's gradient = the loss's own two routes (restated) + what reaches it through h (the model's backward fed with the
    # restated dh)
    h.backward(ref_dh.to(h.dtype).view(h.shape))
    want = table.grad.detach().double() + ref_dE
    scale = float(want.abs().max())
    err = float((total.double() - want).abs().max())
    print("model %s: src_emb grad max|err| %.3g max|ref| %.3g" % (kind, err, scale))
    assert err <= 1e-3 * scale + 1e-5
    assert float(ref_dE.abs().max()) > 0.05 * scale                 # the loss's own routes are a visible part of it


def _users(n, V, Ls, seed):
    from recguru_amd import synthetic
    return synthetic.make_users(n, V, Ls, seed=seed)[:3]


def test_loader():
    from recguru_amd import hip, sampler
    V, Ls = 700, 16
    seqs, val, test = _users(64, V, Ls, 1)
    dom = sampler.DeviceDomain(seqs, val, test, V, "cuda")

    def batches(shared, seed=5, rank=0, nb=3):
        ld = sampler.DeviceLoader(dom, 8, Ls, Ls, V + 1, Ls * 3, seed=seed, shuffle=False, rank=rank, world=2, shared_negs=shared)
        return [b for b, _ in zip(ld, range(nb))]
    a, a2, other = batches(64), batches(64), batches(64, rank=1)
    for (seqs_t, n_items, v, t) in a:
        assert n_items.dim() == 1 and n_items.dtype == torch.int64 and n_items.is_cuda and 1 <= n_items.numel() <= 64
        assert bool((n_items[1:] > n_items[:-1]).all()) and int(n_items.min()) >= 1 and int(n_items.max()) <= V
        assert seqs_t[0].shape == (8, Ls)
    assert not torch.equal(a[0][1], a[1][1])
    assert all(torch.equal(x[1], y[1]) for x, y in zip(a, a2))
    assert not torch.equal(a[0][1], other[0][1])                        # the seed carries the rank
    assert max(b[1].numel() for b in a) > 32                            # 64 draws over 700 ids: mostly distinct
    # shared_negs = 0: the per-user draws, the sampler called directly with the batch's seed
    plain = batches(0)
    users = torch.arange(0, 64, 2, device="cuda")
    for i, (seqs_t, n_items, v, t) in enumerate(plain):
        u = users[i * 8:(i + 1) * 8].contiguous()
        want = hip.sample_negatives(dom.excl, dom.excl_off, u, Ls * 3, V, sampler.batch_seed(5, 0, i), None)
        assert n_items.shape == (8, Ls * 3) and torch.equal(n_items, want)
        enc, di, do = hip.assemble_batch(dom.items, dom.offsets, u, Ls, Ls, V + 1)
        assert torch.equal(seqs_t[0], enc) and torch.equal(seqs_t[1], di) and torch.equal(seqs_t[2], do)
        assert torch.equal(a[i][0][0], enc)                             # the sequences do not depend on the option
    # the alias table is used when the domain has one: zero-frequency items are never drawn
    wf = np.zeros(V + 1)
    wf[1:101] = 1.0
    domf = sampler.DeviceDomain(seqs, val, test, V, "cuda", wf=wf)
    s = domf.shared_candidates(64, 77)
    assert s.dim() == 1 and int(s.max()) <= 100 and bool((s[1:] > s[:-1]).all())


def test_training_with_shared_negatives_moves_the_loss(tmp_path):
    from parity_util import make_args
    from recguru_amd import ops, sampler, training
    from recguru_amd.config import get_param
    from recguru_amd.models import MyAuto4Rec_c
    from recguru_amd.optim import Adam
    ops.set_compute_dtype(torch.bfloat16)
    Bt, Lt, V = 64, 32, 2000
    param = get_param(make_args(64, 2, 8, Lt, V, V, 1, Bt, result_path=str(tmp_path)), make_dirs=False)
    assert param.dropout_rate == 0.0
    torch.manual_seed(0)
    ops.manual_seed(0, 0)
    model = MyAuto4Rec_c("cuda", param).to(torch.float32).to("cuda")
    data = []
    for seed in (1, 2):
        seqs, val, test = _users(4 * Bt, V, Lt, seed)
        dom = sampler.DeviceDomain(seqs, val, test, V, "cuda")
        data.append(sampler.DeviceLoader(dom, Bt, Lt, Lt, V + 1, Lt * 8, seed=seed, shuffle=True, shared_negs=256))
    assert next(iter(data[0]))[1].dim() == 1
    opt = Adam(model.parameters(), lr=3e-3)
    losses = training.train_recon_x(model, opt, 30, data, param, "cuda", neg_sample=True, loss_type="s_soft", opt_type="org",
                                    log_every=0, verbose=False)
    la = np.array([[float(a), float(b)] for a, b in losses])
    assert la.shape == (30, 2) and np.isfinite(la).all()
    print("shared-negatives training: first 5 mean %s last 5 mean %s" % (la[:5].mean(0), la[-5:].mean(0)))
    assert (la[-5:].mean(0) < la[:5].mean(0)).all()
    assert all(torch.isfinite(q).all() for q in model.parameters())


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_data_parallel_normalisation(tmp_path):
    one = str(tmp_path / "one.npz")
    _worker(["one", one])
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.pop("RG_DETERMINISTIC", None)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "shared_ce_worker.py"), "dp", str(tmp_path / "dp.npz")],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            p.kill()
            o, _ = p.communicate()
        logs.append(o.decode()[-3000:])
    assert all(p.returncode == 0 for p in procs), "\n----\n".join(logs)
    a, b = np.load(one), np.load(str(tmp_path / "dp.npz"))
    np.testing.assert_allclose(float(b["loss"]), float(a["loss"]), rtol=1e-5, atol=1e-7)
    Bw = 64
    d = a["dh"].shape[-1]
    np.testing.assert_allclose(b["dh"], a["dh"].reshape(Bw, -1, d)[0::2].reshape(b["dh"].shape), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(b["dE"], a["dE"], rtol=1e-5, atol=1e-7)
