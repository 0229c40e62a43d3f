"""Full-catalogue softmax reconstruction loss on the MI355X (csrc/full_ce.hip, ops.FullSoftmaxLoss, models.FullLogits; quirk Q15):
parity with the reference's own logits, loss and gradients (tests/golden/full_case{1,2}.npz) in every tier, a catalogue of 100 001
classes against a float64 restatement, bit-identical repeats in both libraries, a training loop and data-parallel normalisation."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_util import load_case, make_state, arrays_to_manifest, sample

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("full_case1", "full_case2")
TIERS = {"f32": torch.float32, "bf16x3": "bf16x3", "bf16": torch.bfloat16}
# bf16 tier: operands of both products rounded to 8 significant bits (h, W and the probabilities fed back to the matrix pipe);
# errors relative to the largest magnitude of the compared array
BF16_BOUNDS = {"loss_rel": 2e-2, "dense_rel_to_max": 2e-2, "grad_rel_to_max": 6e-2}


@pytest.fixture(autouse=True)
def _tier_reset():
    from recguru_amd import ops
    yield
    ops.set_compute_dtype(torch.bfloat16)


def _param(z):
    from parity_util import make_args
    from recguru_amd.config import get_param
    B, L, d, H, N, Va, Vb, k = [int(x) for x in z["meta"]]
    return get_param(make_args(d, H, k, L, Va, Vb, N, B, decoder_neg=False), make_dirs=False)


def _load(module, z, tag):
    man = arrays_to_manifest(z[tag + ".keys"], z[tag + ".shapes"], z[tag + ".ndim"])
    st = {k: torch.as_tensor(v) for k, v in make_state(man, int(z[tag + ".seed"])).items()}
    r = module.load_state_dict(st, strict=False)
    assert all(k.endswith(".pe") for k in r.missing_keys) and not r.unexpected_keys
    return module.to("cuda")


def _close(got, ref, tier, what, kind, floor=1e-12):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    if tier == "bf16":
        err = np.abs(got - ref).max() / max(np.abs(ref).max(), floor)
        assert err <= BF16_BOUNDS[kind], (what, err)
    else:
        np.testing.assert_allclose(got, ref, rtol=1e-3, atol=1e-5 * max(1.0, np.abs(ref).max()), err_msg=what)


def _grads(prefix, module, z, tier):
    # bf16: an array whose reference gradient is ~0 (a bias behind a softmax) is judged against 1 % of the module's largest gradient
    floor = 0.01 * max(float(np.abs(v).max()) for k, v in z.items() if k.startswith(prefix))
    n = 0
    for k, p in module.named_parameters():
        if prefix + k in z:
            # (a parameter this package leaves without a gradient -- the cross-attention's WQ / WK under its uniform rows -- has a
            # zero one in the reference)
            n += 1
            if p.grad is None:
                assert np.abs(z[prefix + k]).max() <= 1e-6, k
                continue
            _close(sample(p.grad.detach().cpu().numpy()), z[prefix + k], tier, prefix + k, "grad_rel_to_max", floor)
    assert n == sum(1 for k in z if k.startswith(prefix))
    return n


@pytest.mark.parametrize("tier", list(TIERS))
@pytest.mark.parametrize("case", CASES)
def test_cross_domain_golden_parity(case, tier):
    from recguru_amd import ops, training as T
    from recguru_amd.models import FullLogits, MyAuto4Rec_c
    ops.set_compute_dtype(TIERS[tier])
    z = load_case(case)
    param = _param(z)
    G = _load(MyAuto4Rec_c("cuda", param, wf=None, enc_share=True, dec_rec=False).to(torch.float32), z, "G")
    for dom in "ab":
        enc, di, do = (torch.as_tensor(z["%s.%s" % (nm, dom)]).cuda() for nm in ("enc_in", "dec_in", "dec_out"))
        mask = T.get_pad_mask(do, param.pad_index, "cuda")
        G.zero_grad()
        B, L = do.shape
        loss = T.loss_ae(G, enc, di, do, None, False, B, L, param, mask, "cuda", domain=dom)
        logits = G(enc, di, do, None, dom, mask)
        assert isinstance(logits, FullLogits)
        _close(logits.dense().cpu().numpy(), z["logits.%s" % dom], tier, "logits." + dom, "dense_rel_to_max")
        _close(float(loss.detach()), float(z["loss.%s" % dom]), tier, "loss." + dom, "loss_rel")
        loss.backward()
        _grads("gradG.%s." % dom, G, z, tier)
        assert ("gradG.%s.projection_%s.weight" % (dom, dom)) in z


@pytest.mark.parametrize("tier", list(TIERS))
@pytest.mark.parametrize("case", CASES)
def test_single_domain_golden_parity(case, tier):
    from recguru_amd import auto_training as A, ops
    from recguru_amd.models import MyRec
    ops.set_compute_dtype(TIERS[tier])
    z = load_case(case)
    param = _param(z)
    R = _load(MyRec("cuda", param).to(torch.float32), z, "R")
    enc, di, do = (torch.as_tensor(z["%s.a" % nm]).cuda() for nm in ("enc_in", "dec_in", "dec_out"))
    mask = (di != param.pad_index).view(-1).to(torch.float32)
    B, L = do.shape
    R.zero_grad()
    loss = A.loss_ae(R, enc, di, do, None, False, B, L, param, mask)
    _close(R(enc, di, do, None, recon=True).dense().cpu().numpy(), z["logits.s"], tier, "logits.s", "dense_rel_to_max")
    _close(float(loss.detach()), float(z["loss.s"]), tier, "loss.s", "loss_rel")
    loss.backward()
    _grads("gradR.", R, z, tier)
    row0 = R.AutoEnc.src_emb.weight.grad[0].cpu().numpy()
    assert np.abs(z["gradR_src_emb_row0"]).max() > 0 and np.abs(row0).max() > 0       # the pad row takes the product's gradient
    _close(row0, z["gradR_src_emb_row0"], tier, "src_emb.grad[0]", "grad_rel_to_max")


def _against_float64(B, L, d, C, min_len, seed, lo, hi):
    """ops.full_softmax_loss in the bf16x3 tier against a chunked float64 restatement: ragged left-padded rows (whole padded 16-row
    tiles and padded rows inside live tiles), the last class -- inside the tail chunk -- as the label of some live rows."""
    from recguru_amd import ops
    ops.set_compute_dtype("bf16x3")
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(min_len, L + 1, (B,), generator=g)
    mask = (torch.arange(L)[None, :] >= (L - lens)[:, None]).to(torch.float32).reshape(-1).cuda()
    h = (torch.randn(B * L, d, generator=g) * 0.5).cuda()
    w = (torch.randn(C, d, generator=g) * 0.3).cuda()
    lab = (torch.randint(0, C, (B * L,), generator=g).cuda() * mask.long())
    live = torch.nonzero(mask).reshape(-1)
    assert lo < live.numel() < hi
    lab[live[:7]] = C - 1
    hh = h.clone().requires_grad_(True)
    wp = torch.nn.Parameter(w.clone())
    loss = ops.full_softmax_loss(hh, wp, lab, mask)
    loss.backward()
    cnt = float(mask.sum())
    w64 = w.double()
    tot, dh_ref, dw_ref = 0.0, torch.zeros(B * L, d, dtype=torch.float64, device="cuda"), torch.zeros_like(w64)
    for s in range(0, live.numel(), 1024):
        ix = live[s:s + 1024]
        z = h[ix].double() @ w64.T
        lse = torch.logsumexp(z, 1)
        tot += float((lse - z.gather(1, lab[ix][:, None])[:, 0]).sum())
        p = torch.softmax(z, 1)
        p[torch.arange(ix.numel(), device="cuda"), lab[ix]] -= 1.0
        p /= cnt
        dh_ref[ix] = p @ w64
        dw_ref += p.T @ h[ix].double()
    np.testing.assert_allclose(loss.item(), tot / cnt, rtol=1e-3, atol=1e-5)
    dead = mask == 0
    assert float(hh.grad[dead].abs().max()) == 0.0
    for got, ref, nm in ((hh.grad, dh_ref, "dh"), (wp.grad, dw_ref, "dW")):
        scale = float(ref.abs().max())
        err = float((got.double() - ref).abs().max())
        assert err <= 1e-3 * scale + 1e-5, (nm, err, scale)
    assert float(wp.grad[C - 1].abs().max()) > 0


def test_large_catalogue_against_float64():
    """~20 k live rows x C = 100 001 x d = 128: the class tail, dh and dW at scale, padded rows with zero dh and no contribution."""
    _against_float64(B=200, L=200, d=128, C=100001, min_len=5, seed=3, lo=15000, hi=25000)


@pytest.mark.parametrize("d", [64, 256])
def test_other_widths_against_float64(d):
    """d = 64 and d = 256 (one 16-row tile per wave; ~150 KB of LDS per workgroup in this tier) at a catalogue of 1 001 classes."""
    _against_float64(B=48, L=64, d=d, C=1001, min_len=1, seed=9 + d, lo=300, hi=3000)


def _worker(args, env=None, timeout=600):
    e = dict(os.environ)
    e.pop("RG_DETERMINISTIC", None)
    e.update(env or {})
    p = subprocess.run([sys.executable, os.path.join(HERE, "full_softmax_worker.py")] + args, env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=timeout)
    assert p.returncode == 0, p.stdout.decode()[-3000:]


@pytest.mark.parametrize("det", [False, True])
def test_repeat_runs_are_bit_identical(tmp_path, det):
    out = str(tmp_path / "det.npz")
    _worker(["det", out], {"RG_DETERMINISTIC": "1"} if det else None)
    r = np.load(out)
    assert int(r["det_fault"]) == 0
    for tier in ("bf16x3", "bf16"):
        for k in ("loss", "dh", "dw"):
            a, b = r["%s.%s.0" % (k, tier)], r["%s.%s.1" % (k, tier)]
            assert np.array_equal(a, b), (tier, k)
        assert np.isfinite(r["dw.%s.0" % tier]).all() and np.abs(r["dw.%s.0" % tier]).max() > 0


def test_train_with_the_full_loss_decreases_it(tmp_path):
    from parity_util import make_args
    from recguru_amd import auto_training as A, ops, synthetic
    from recguru_amd.config import get_param
    from recguru_amd.models import MyRec
    from recguru_amd.optim import Adam
    ops.set_compute_dtype(torch.bfloat16)
    B, L, V = 32, 20, 300
    param = get_param(make_args(64, 2, 8, L, V, V, 1, B, decoder_neg=False, result_path=str(tmp_path)), make_dirs=False)
    torch.manual_seed(0)
    model = MyRec("cuda", param).to("cuda")
    dm = synthetic.make_domain(B, V, L, 8, seed=4, min_len=3)
    seqs = tuple(torch.as_tensor(dm[n]) for n in ("enc_in", "dec_in", "dec_out"))
    n_items = torch.as_tensor(dm["n_items"])
    data = [[(seqs, n_items, n_items[:, :1], n_items[:, :1])]]
    opt = Adam(model.parameters(), lr=3e-3)
    losses, _ = A.train(model, opt, 0, data, param, "cuda", neg_sample=False, loss_type="s_soft", opt_type="org",
                        epochs=8, verbose=False)
    assert len(losses) == 8 and all(np.isfinite(losses))
    assert losses[-1] < losses[0] - 0.1, losses
    assert all(torch.isfinite(p).all() for p in model.parameters())


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
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "full_softmax_worker.py"), "dp", str(tmp_path / "dp.npz")],
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
    B = 64
    d = a["dh"].shape[-1]
    np.testing.assert_allclose(b["dh"], a["dh"].reshape(B, -1, d)[0::2].reshape(b["dh"].shape), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(b["dw"], a["dw"], rtol=1e-5, atol=1e-7)
