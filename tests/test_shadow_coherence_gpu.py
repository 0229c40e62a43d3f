"""Every cached weight copy and tile list against a fresh recompute, under the shipped drivers (tests/shadow_audit.py).

The auditor wraps ops.shadow / shadow_cat / bias_cat / pad_rows_cat, hip.live_tiles / first_live and Adam.step; whatever they hand
out is compared BIT FOR BIT with a plain-torch restatement from the current f32 masters (or the current row mask).  One Adam step is
below the bf16 tier's loss bounds, so no loss-curve test can see a copy that is one step old; these can.  Scenarios a-i of the
issue, then the negative controls: three ways of breaking the cache's state machine that the auditor must report.

Models are the smallest that take the fused paths (d = 128, H = 4, one block, L = 16, B = 8, 300 items) unless a scenario says why not.
"""
import gc
import os
import time

import pytest
import torch

import shadow_audit as A
from golden_util import load_case
from parity_util import curve_loaders, curve_meta, make_args, state_of

pytestmark = pytest.mark.gpu
TIERS = {"f32": torch.float32, "bf16": torch.bfloat16, "bf16x3": "bf16x3", "mixed": "mixed"}


@pytest.fixture
def audit(monkeypatch, capsys, request):
    from recguru_amd import hip, ops, optim
    a = A.Audit(ops, hip, optim).install(monkeypatch)
    a.notes = []
    t0 = time.perf_counter()
    yield a
    torch.cuda.synchronize()
    with capsys.disabled():
        print("\n[shadow_audit] %s: %s%s | %.2f s" % (request.node.name, a.report(), "".join(" | " + n for n in a.notes),
                                                     time.perf_counter() - t0))


def _small(seed, d=128, H=4, N=1, L=16, B=8, V=300, k=3, dropout=0.0):
    from recguru_amd import config, models, synthetic
    param = config.get_param(make_args(d, H, k, L, V, V, N, B, dropout=dropout), make_dirs=False)
    torch.manual_seed(seed)
    G = models.MyAuto4Rec_c("cuda", param, wf=None, enc_share=True, dec_rec=False).to(torch.float32).cuda()
    D = models.Discriminator(d, 1, param.dis_dim).to(torch.float32).cuda()
    D.eval()
    bt = []
    for s in (2 * seed + 1, 2 * seed + 2):
        dm = synthetic.make_domain(B, V, L, k, seed=s)
        bt.append(tuple(torch.as_tensor(dm[n]).cuda() for n in ("enc_in", "dec_in", "dec_out", "n_items")))
    return param, G, D, bt


def _fwd_bwd(G, bt, param, domains="ab"):
    """Forward and backward of the reconstruction loss (no optimizer step): every form a training pass reads is handed out."""
    from recguru_amd import ops, training as T
    ops.release_grads(list(G.parameters()))
    for dom, b in zip("ab", bt):
        if dom in domains:
            mask = T.get_pad_mask(b[2], param.pad_index, "cuda")
            T.loss_ae(G, b[0], b[1], b[2], b[3], True, b[2].shape[0], b[2].shape[1], param, mask, "cuda", dom).backward()


def _forward(G, bt, param):
    from recguru_amd import training as T
    with torch.no_grad():
        return T.get_user_embed(G, bt[0][0], "a", param, "cuda", 0)


def _gan_iteration(G, D, opt_d, opt_g, bt, param):
    from recguru_amd import training as T
    B, L = bt[0][0].shape
    T.critic_iteration(G, D, bt[0][0], bt[1][0], opt_d, param, "cuda", T._NoDP())
    T.generator_iteration(G, D, bt[0] + (B, L), bt[1] + (B, L), opt_g, param, "cuda", T._NoDP())


def _layer0(G):
    """(Wq, Wk, Wv, Wo, W1, W2, bq, bk, bv) of the first encoder layer."""
    lay = G.encoder.layers[0]
    att, ffn = lay.enc_self_attn, lay.pos_ffn
    return (att.WQ.weight, att.WK.weight, att.WV.weight, att.linear.weight, ffn.l1.weight, ffn.l2.weight,
            att.WQ.bias, att.WK.bias, att.WV.bias)


# ------------------------------------------------------------------------------------------------------------------------------
# a. the drivers of test_loss_curves_replay under the auditor
# ------------------------------------------------------------------------------------------------------------------------------
def _curve_models(z):
    from recguru_amd import config, models
    m = curve_meta(z)
    res = "/tmp/rg_shadow_audit_%d" % os.getpid()
    os.makedirs(res, exist_ok=True)
    param = config.get_param(make_args(m["d"], m["H"], m["k"], m["L"], m["V_a"], m["V_b"], m["N"], m["B"], result_path=res))
    G = models.MyAuto4Rec_c("cuda", param, wf=None, enc_share=True, dec_rec=False).to(torch.float32)
    G.load_state_dict(state_of(z, "G"), strict=False)
    D = models.Discriminator(param.d_model, 1, param.dis_dim).to(torch.float32)
    D.load_state_dict(state_of(z, "D"))
    D.eval()
    return m, param, G.cuda(), D.cuda()


@pytest.mark.parametrize("tier", ["bf16", "bf16x3", "mixed", "f32"])
def test_driver_replay(tier, audit):
    """curves1 as test_loss_curves_replay runs it -- 20 train_recon_x steps, then train_gan_all with three optimizers in turn -- plus
    one critic_phase(overlap=True), whose encoder passes take their copies on the side stream.  Losses are not compared here."""
    from recguru_amd import blocks, ops, training as T
    from recguru_amd.optim import Adam
    ops.set_compute_dtype(TIERS[tier])
    z = load_case("curves1")
    m, param, G, D = _curve_models(z)
    ld = curve_loaders(z)
    T.plot.reset()
    opt_rec = blocks.ScheduledOptim(Adam(G.parameters(), betas=(0.9, 0.98), eps=1e-09), 1.0, m["d"], m["warmup"])
    opt_gen = Adam(G.parameters(), lr=0.0001, betas=(0.5, 0.9))
    opt_dis = Adam(D.parameters(), lr=0.0001, betas=(0.5, 0.9))
    T.train_recon_x(G, opt_rec, m["phase1_steps"], [ld["ae_a"], ld["ae_b"]], param, "cuda", neg_sample=True, loss_type="s_soft",
                    opt_type="schedule", log_every=0)
    torch.manual_seed(m["alpha_seed"])
    hist = T.train_gan_all(G, D, [ld["ae_a"], ld["ae_b"]], opt_dis, opt_gen, "cuda", param, m["iterations"], None,
                           [ld["rec0"], ld["rec1"]], None, domain="a", overlap=False)
    assert len(hist) == 5 and len(hist.phase3) == 5
    seqs = [(ld["ae_a"][i][0][0].cuda(), ld["ae_b"][i][0][0].cuda()) for i in range(3)]
    before = sum(audit.handouts.values())
    T.critic_phase(G, D, seqs, opt_dis, param, "cuda", T._NoDP(), overlap=True)
    torch.cuda.synchronize()
    assert sum(audit.handouts.values()) > before
    assert audit.steps == 20 + 5 * (T.CRITIC_ITERS + 1) + 5 + 3
    if tier == "bf16":
        # the fixture's 256 rows never reach the head-major attention form (bf16, B x L >= 4096), the one reader of the pad rows: two
        # more steps of the same driver at B = L = 64
        p2, G2, _, bt = _small(1, L=64, B=64, k=2)
        zero = torch.zeros(64, dtype=torch.long)
        loaders = [[((b[0], b[1], b[2]), b[3], zero, zero)] * 3 for b in bt]
        T.train_recon_x(G2, Adam(G2.parameters(), lr=1e-3), 2, loaders, p2, "cuda", log_every=0)
        assert audit.steps == 20 + 5 * (T.CRITIC_ITERS + 1) + 5 + 3 + 2
    h = audit.handouts
    if tier == "bf16":
        for form in ("plain", "transposed", "packed", "cat", "cat_t", "bias_cat", "pad_rows"):
            assert h[form] > 0 and audit.audited[form] > 0, (form, dict(h))
    else:
        for form in ("transposed", "cat", "cat_t", "bias_cat"):
            assert h[form] > 0, (form, dict(h))
    if tier in ("bf16x3", "mixed"):
        assert h["presplit"] + h["presplit_t"] > 0, dict(h)
    if tier == "mixed":
        assert audit.dtypes[("mixed", torch.bfloat16)] > 0 and audit.dtypes[("mixed", torch.float32)] > 0, dict(audit.dtypes)
    assert audit.paths["refresh"] > 0 and audit.paths["lazy"] > 0, dict(audit.paths)
    assert audit.swept > 0


# ------------------------------------------------------------------------------------------------------------------------------
# b. width 256
# ------------------------------------------------------------------------------------------------------------------------------
def test_width_256(audit):
    """d = 256, H = 8, dropout on: the packed weights of csrc/fused256.hip, the 768-wide fused QKV copy whose column slices go out as
    strided operands, and the unfused discriminator chain (the fused critic kernel is instantiated for d = 128)."""
    from recguru_amd import ops, training as T
    from recguru_amd.optim import Adam
    param, G, D, bt = _small(3, d=256, H=8, dropout=0.5)
    G.train()
    D.train()
    opt = Adam(G.parameters(), lr=1e-3)
    opt_d, opt_g = Adam(D.parameters(), lr=1e-3, betas=(0.5, 0.9)), Adam(G.parameters(), lr=1e-3, betas=(0.5, 0.9))
    for _ in range(2):                                                          # the second round reads what the first one's steps refreshed
        T.recon_step(G, opt, bt[0], bt[1], param, "cuda", T._NoDP(), list(G.parameters()))
        _gan_iteration(G, D, opt_d, opt_g, bt, param)
    torch.cuda.synchronize()
    h = audit.handouts
    for form in ("plain", "transposed", "cat", "cat_t", "bias_cat"):
        assert h[form] > 0, (form, dict(h))
    assert h["packed"] > 0, dict(h)                                           # csrc/fused256.hip reads fragment-packed weights
    audit.notes.append("packed hand-outs at d=256: %d" % h["packed"])
    assert audit.steps == 6 and audit.paths["refresh"] > 0


# ------------------------------------------------------------------------------------------------------------------------------
# c. the lifetime promise of ops.shadow
# ------------------------------------------------------------------------------------------------------------------------------
def _lifetime(audit, tier):
    """Copies taken before a step keep their bits through it; the next call returns ANOTHER buffer with the new weights, which in
    turn keeps its bits through the second step.  (Nothing is claimed about the first copies after the second step.)"""
    from recguru_amd import ops
    from recguru_amd.optim import Adam
    ops.set_compute_dtype(TIERS[tier])
    param, G, D, bt = _small(5)
    Wq, Wk, Wv, Wo, W1, W2, bq, bk, bv = _layer0(G)
    opt = Adam(G.parameters(), lr=1e-2)
    H = param.num_heads

    def take():
        out = {}
        for name, (tr, pk) in (("plain", (False, False)), ("transposed", (True, False)), ("packed", (False, True)), ("packed_t", (True, True))):
            if name == "plain" and ops.compute_dtype() == torch.float32:
                continue                                                        # f32 storage: the plain form is the master itself
            out[name] = ops.shadow(Wo, tr, pack=pk)
        if tier in ("bf16x3", "mixed"):
            out["presplit"] = ops.shadow(W1, pack=True, split=True)
            out["presplit_t"] = ops.shadow(W2, True, pack=True, split=True)
        out["cat"] = ops.shadow_cat((Wq, Wk, Wv))
        out["cat_t"] = ops.shadow_cat((Wq, Wk, Wv), transpose=True)
        out["bias_cat"] = ops.bias_cat((bq, bk, bv))
        out["pad_rows"] = ops.pad_rows_cat((bq, bk, bv), H)
        return out

    first = take()
    bits = {k: A.raw(v).clone() for k, v in first.items()}
    for k, v in first.items():
        audit.hold(v, "%s taken before step 1" % k)
    _fwd_bwd(G, bt, param)
    assert all(p.grad is not None for p in (Wq, Wk, Wv, Wo, W1, W2, bq, bk, bv))
    opt.step()                                                                  # the auditor's first check of the held copies
    for k, v in first.items():
        assert torch.equal(A.raw(v), bits[k]), "%s changed under the first step" % k
    second = take()                                                             # audited: the new weights
    for k in first:
        assert second[k].data_ptr() != first[k].data_ptr(), "%s: the buffer handed out before the step was handed out again" % k
        assert not torch.equal(A.raw(second[k]), bits[k]), "%s: the step moved nothing" % k
        audit.hold(second[k], "%s taken after step 1" % k)
    bits2 = {k: A.raw(v).clone() for k, v in second.items()}
    _fwd_bwd(G, bt, param)
    opt.step()                                                                  # the second check: the copies taken after step 1
    for k, v in second.items():
        assert torch.equal(A.raw(v), bits2[k]), "%s changed under the second step" % k
    third = take()
    for k in second:
        assert third[k].data_ptr() != second[k].data_ptr()
    return sorted(first)


@pytest.mark.parametrize("tier", ["bf16", "bf16x3", "f32"])
def test_lifetime_promise(tier, audit):
    forms = _lifetime(audit, tier)
    audit.notes.append("forms held: " + ",".join(forms))
    assert audit.steps == 2 and audit.paths["refresh"] > 0 and audit.paths["lazy"] > 0


# ------------------------------------------------------------------------------------------------------------------------------
# d. edits from outside the optimizer
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["bf16", "bf16x3"])
def test_outside_edits(tier, audit):
    """Between two passes a parameter is rewritten by something that is not Adam.step; the next hand-out must be current.  Writes
    through p.data (or a raw pointer) do not move _version: followed by ops.bump(p) they are seen -- the contract ops.shadow states."""
    from recguru_amd import ops
    from recguru_amd.optim import Adam, AdamW
    ops.set_compute_dtype(TIERS[tier])
    param, G, D, bt = _small(7)
    Wq, Wk, Wv, Wo, W1, W2, bq, bk, bv = _layer0(G)
    edited = (Wq, Wo, W2, bk, G.src_emb_a.weight)                               # a cat member, packed forms, a bias, the plain table
    gen = torch.Generator(device="cuda").manual_seed(1)

    def passes():
        n = sum(audit.audited.values())
        _forward(G, bt, param)
        _fwd_bwd(G, bt, param)
        return sum(audit.audited.values()) - n

    assert passes() > 0
    with torch.no_grad():
        for p in edited:
            p.mul_(1.25)
    assert passes() >= 4                                                        # the edited ones were rebuilt and compared again
    sd = {k: (v * 0.5 if v.dtype == torch.float32 and not k.endswith(".pe") else v) for k, v in G.state_dict().items()}
    G.load_state_dict(sd)
    assert passes() >= 4
    for p in edited:
        p.data.copy_(torch.randn(p.shape, device="cuda", generator=gen) * 0.1)
        ops.bump(p)
    assert passes() >= 4
    for p in edited:
        p.data = torch.randn(p.shape, device="cuda", generator=gen) * 0.1
    assert passes() >= 4
    # a step that skip_nonfinite skips: an inf gradient is data, not a fault
    opt = Adam(G.parameters(), lr=1e-2, skip_nonfinite=True)
    _fwd_bwd(G, bt, param)
    Wo.grad[0, 0] = float("inf")
    masters = [p.detach().clone() for p in edited]
    copy = A.raw(ops.shadow(Wo, pack=True, split=True)).clone()
    opt.step()
    assert opt.skipped_steps() == 1 and opt.state[Wo]["step"] == 1 and opt.state[Wq]["step"] == 1
    for p, m in zip(edited, masters):
        assert torch.equal(A.raw(p), A.raw(m))
    assert torch.equal(A.raw(ops.shadow(Wo, pack=True, split=True)), copy)
    assert passes() > 0
    # a clipped AdamW step (the option path, _step_options)
    optw = AdamW(G.parameters(), lr=1e-2, max_norm=0.5)
    _fwd_bwd(G, bt, param)
    optw.step()
    assert not torch.equal(A.raw(Wo), A.raw(masters[1]))
    assert passes() >= 4
    assert audit.steps == 2


def test_replaced_data_at_a_recycled_address(audit):
    """p.data replaced TWICE between two hand-outs.  The first replacement frees the old storage, and the allocator may hand its
    block to the second tensor: address, _version and bump count are then those recorded with the cached copy.  A cache entry that
    did not keep the storage it was made from alive served the old weights here; with it alive the address cannot come back."""
    from recguru_amd import ops
    param, G, D, bt = _small(19)
    Wq, Wk, Wv, Wo, W1, W2, bq, bk, bv = _layer0(G)
    gen = torch.Generator(device="cuda").manual_seed(2)
    cases = ((Wo, "shadow", (Wo,), A.TRANSPOSE, lambda: ops.shadow(Wo, True)),
             (W1, "shadow", (W1,), A.PACK, lambda: ops.shadow(W1, pack=True)),
             (Wk, "cat", (Wq, Wk, Wv), 0, lambda: ops.shadow_cat((Wq, Wk, Wv))),
             (bv, "bias_cat", (bq, bk, bv), 0, lambda: ops.bias_cat((bq, bk, bv))),
             (bq, "pad_rows", (bq, bk, bv), param.num_heads, lambda: ops.pad_rows_cat((bq, bk, bv), param.num_heads)))
    recycled = 0
    for p, kind, ps, mode, take in cases:
        take()
        ptr, ver = p.data_ptr(), A.version_of(p)
        for _ in range(4):
            p.data = torch.randn(p.shape, device="cuda", generator=gen) * 0.1  # the storage the copy was made from is released ...
            p.data = torch.randn(p.shape, device="cuda", generator=gen) * 0.1  # ... and its block may be handed out again
            if p.data_ptr() == ptr:
                break
        recycled += A.version_of(p) == ver
        dtype = torch.float32 if kind == "bias_cat" else ops.compute_dtype()
        ok, idx = A.same_bits(take(), A.restate(kind, ps, mode, dtype))
        assert ok, "%s of a parameter whose data was replaced twice holds old weights (first differing raw index %s; address recycled: %s)" % (
            kind, idx, A.version_of(p) == ver)
    audit.notes.append("replaced p.data came back at the old address with the old version in %d of %d cases" % (recycled, len(cases)))


# ------------------------------------------------------------------------------------------------------------------------------
# e. changing parameter subsets
# ------------------------------------------------------------------------------------------------------------------------------
def test_changing_subsets(audit, monkeypatch):
    """Three optimizers over overlapping subsets and requires_grad toggled so that refresh_shadows meets more subset signatures than
    _REFRESH_CACHE holds (16): an entry is evicted, then the first signature comes back."""
    from recguru_amd import ops
    from recguru_amd.optim import Adam
    param, G, D, bt = _small(9, N=2)
    named = list(G.named_parameters())
    toggled = [p for n, p in named if n.startswith("encoder.") and n.endswith(("linear.weight", "l1.weight", "l2.weight"))]
    assert len(toggled) == 6
    opts = [Adam([p for n, p in named], lr=1e-2),
            Adam([p for n, p in named if n.startswith(("encoder.", "src_emb"))], lr=1e-2),
            Adam([p for n, p in named if n.startswith(("encoder.", "decoder_a."))], lr=1e-2)]
    sigs, real = [], ops.refresh_shadows

    def refresh(params):
        real(params)
        for s in ops._REFRESH_CACHE:
            if s not in sigs:
                sigs.append(s)

    monkeypatch.setattr(ops, "refresh_shadows", refresh)

    def iteration(pattern, opt):
        for i, p in enumerate(toggled):
            p.requires_grad = bool(pattern >> i & 1)
        _fwd_bwd(G, bt, param)
        opt.step()
        _forward(G, bt, param)

    _fwd_bwd(G, bt, param)                                                      # fills the cache: the first refresh has something to rewrite
    _forward(G, bt, param)
    for it in range(20):
        iteration(1 + 3 * it, opts[it % 3])
    assert len(sigs) >= 17, len(sigs)
    assert len(ops._REFRESH_CACHE) <= 16 and sigs[0] not in ops._REFRESH_CACHE  # evicted
    n = len(sigs)
    iteration(1, opts[0])                                                       # the first subset again: its entry was evicted, so it is rebuilt
    iteration(1, opts[0])
    assert sigs[0] in ops._REFRESH_CACHE or len(sigs) == n + 1
    audit.notes.append("first signature %s" % ("rebuilt after eviction" if len(sigs) == n else "came back as a new one"))
    for p in toggled:
        p.requires_grad = True
    iteration(63, opts[0])
    audit.notes.append("%d distinct refresh signatures" % len(sigs))
    assert audit.paths["refresh"] > 0


# ------------------------------------------------------------------------------------------------------------------------------
# f. identity reuse
# ------------------------------------------------------------------------------------------------------------------------------
def test_identity_reuse(audit):
    """A model is dropped and another of the same shapes built, 30 times: id() and the data pointer of a collected parameter come
    back in a later one, and the cache must not serve the dead model's copy (it did once in ~25 runs of the suite, before the
    weak-reference check in ops.shadow)."""
    dead_ids, dead_ptrs, reused_id, reused_ptr = set(), set(), 0, 0
    for rnd in range(30):
        param, G, D, bt = _small(100 + rnd)
        ps = list(G.parameters())
        reused_id += any(id(p) in dead_ids for p in ps)
        reused_ptr += any(p.data_ptr() in dead_ptrs for p in ps)
        _forward(G, bt, param)
        if rnd % 3 == 0:
            _fwd_bwd(G, bt, param, domains="a")
        dead_ids.update(id(p) for p in ps)
        dead_ptrs.update(p.data_ptr() for p in ps)
        del G, D, ps, param, bt
        gc.collect()
    audit.notes.append("rounds with a reused id(): %d, with a reused data_ptr: %d of 30%s"
                       % (reused_id, reused_ptr, "" if reused_id + reused_ptr else " -- VACUOUS in this environment"))
    assert reused_id + reused_ptr > 0, "no parameter identity was ever reused: the scenario tested nothing"
    assert audit.audited["plain"] >= 30 and audit.audited["cat"] >= 30
    audit.notes.append("packed copies audited: %d" % (audit.audited["packed"] + audit.audited["packed_t"]))


# ------------------------------------------------------------------------------------------------------------------------------
# g. tier switches on a live model
# ------------------------------------------------------------------------------------------------------------------------------
def test_tier_switches(audit):
    from recguru_amd import ops
    from recguru_amd.optim import Adam
    param, G, D, bt = _small(11)
    opt = Adam(G.parameters(), lr=1e-2)
    visits = []
    for tier in ("bf16", "bf16x3", "mixed", "f32", "bf16"):
        ops.set_compute_dtype(TIERS[tier])
        audit.retain = []
        _fwd_bwd(G, bt, param)
        opt.step()
        _forward(G, bt, param)
        _fwd_bwd(G, bt, param)
        visits.append((tier, audit.retain))                                     # kept alive: no address of the visit can be reused
    audit.retain = None
    masters = set(p.data_ptr() for p in G.parameters())
    first = set(t.data_ptr() for t in visits[0][1]) - masters
    again = set(t.data_ptr() for t in visits[4][1]) - masters
    assert first and again and not (first & again), "a copy cached during the first bf16 visit was served on the second"
    assert audit.steps == 5 and audit.handouts["presplit"] + audit.handouts["presplit_t"] > 0
    audit.notes.append("copies handed out per visit: " + " ".join("%s=%d" % (t, len(r)) for t, r in visits))


# ------------------------------------------------------------------------------------------------------------------------------
# h. evaluation after training
# ------------------------------------------------------------------------------------------------------------------------------
def _eval_loader(bt, val):
    return [((b[0], b[1], val), (b[0], b[1], val.flip(0)), b[3], b[3]) for b in bt]


@pytest.mark.parametrize("tier", ["bf16", "f32"])
def test_evaluation_after_training(tier, audit):
    """The ranking and top-K paths of both model families after optimizer steps: each is handed the current item table."""
    from recguru_amd import auto_training as at, models, ops, training as T
    from recguru_amd.optim import Adam
    ops.set_compute_dtype(TIERS[tier])
    param, G, D, bt = _small(13)
    B, L = bt[0][0].shape
    val = torch.arange(1, B + 1, device="cuda")
    param.eval_steps, param.candidate_size = 2, bt[0][3].shape[1]
    among = torch.arange(5, 120, device="cuda")

    def evaluate_cross():
        n = audit.handouts["plain"]
        T.get_scores(G, bt[0][0], bt[0][1], val, bt[0][3], param, False, "a", "cuda")
        T.evaluation_2(G, _eval_loader(bt[:1], val), "cuda", param, k_val=[5], domain="a")
        T.recommend(G, bt[0][0], bt[0][1], 10, param, domain="a", device="cuda")
        T.recommend(G, bt[0][0], bt[0][1], 10, param, domain="a", device="cuda", among=among)
        T.evaluation_full(G, _eval_loader(bt[:1], val), "cuda", param, k_val=[5], domain="a")
        T.evaluation_full(G, _eval_loader(bt[:1], val), "cuda", param, k_val=[5], domain="a", among=among)
        G.train()
        assert audit.handouts["plain"] - n >= 6 + 4 + 2                          # six entry points, the embedding look-ups besides

    opt = Adam(G.parameters(), lr=1e-2)
    evaluate_cross()
    for _ in range(3):
        T.recon_step(G, opt, bt[0], bt[1], param, "cuda", T._NoDP(), list(G.parameters()))
        evaluate_cross()                                                        # after one step, after two, after three
    R = models.MyRec("cuda", param, None, dec_rec=False, fix_enc=False, sas=False, pos_train=False).to(torch.float32).cuda()
    optr = Adam(R.parameters(), lr=1e-2)
    b = bt[0]

    def evaluate_single():
        n = audit.handouts["plain"]
        at.get_scores(R, b[0], b[1], val, b[3], param)
        at.evaluation(R, _eval_loader(bt[:1], val), "cuda", param, k_val=[5])
        at.recommend(R, b[0], b[1], 10, param)
        at.recommend(R, b[0], b[1], 10, param, among=among)
        at.evaluation_full(R, _eval_loader(bt[:1], val), "cuda", param, k_val=[5])
        at.evaluation_full(R, _eval_loader(bt[:1], val), "cuda", param, k_val=[5], among=among)
        R.train()
        assert audit.handouts["plain"] - n >= 6

    evaluate_single()
    for _ in range(2):
        optr.zero_grad()
        mask = T.get_pad_mask(b[2], 0, "cuda")
        at.loss_ae(R, b[0], b[1], b[2], b[3], True, B, L, param, mask).backward()
        optr.step()
        evaluate_single()
    assert audit.steps == 5
    if tier == "bf16":
        assert audit.paths["refresh"] > 0 and audit.audited["plain"] >= 8


# ------------------------------------------------------------------------------------------------------------------------------
# i. tile lists
# ------------------------------------------------------------------------------------------------------------------------------
def _mask_loop(hip, B=128, L=128, rounds=40):
    """40 masks through hip.live_tiles / first_live: fresh allocations after the previous one was freed, the same tensor edited in
    place by torch ops, reshape(-1) views of one [B, L] mask.  Returns (number of shared-list checks, in-place edits)."""
    M = B * L
    gen = torch.Generator(device="cuda").manual_seed(3)
    shared = edits = 0
    m = None
    for r in range(rounds):
        kind = r % 4
        if kind == 0 or m is None:                                              # freshly allocated, the previous one freed first
            m = None
            lens = torch.randint(0, L + 1, (B,), device="cuda", generator=gen)
            m = (torch.arange(L, device="cuda")[None, :] >= (L - lens)[:, None]).float()       # left-padded
        elif kind == 1:                                                         # edited in place: whole sequences die
            m[torch.randint(0, B, (B // 2,), device="cuda", generator=gen)] = 0
            edits += 1
        elif kind == 2:                                                         # edited in place: dead rows come alive
            m.view(-1)[torch.randint(0, M, (64,), device="cuda", generator=gen)] = 1
            edits += 1
        a = hip.live_tiles(m.reshape(-1), M)
        f = hip.first_live(m.reshape(-1), B, L)
        b = hip.live_tiles(m.reshape(-1), M)                                    # another view object of the unedited mask
        g = hip.first_live(m.view(M), B, L)
        assert a.data_ptr() == b.data_ptr() and f.data_ptr() == g.data_ptr(), "views of one unedited mask did not share a list"
        shared += 1
        if r % 5 == 0:                                                          # other extents of the same storage
            hip.live_tiles(m.reshape(-1), M - 7)
            hip.first_live(m.reshape(-1), B // 2, L)
    m = torch.zeros(M, device="cuda")
    assert int(hip.live_tiles(m, M)[0]) == 0 and int(hip.first_live(m, B, L)[0]) == L
    m.fill_(1)
    assert int(hip.live_tiles(m, M)[0]) == M // 16 and int(hip.first_live(m, B, L)[B - 1]) == 0
    return shared, edits


@pytest.mark.parametrize("tier", ["bf16", "bf16x3"])
def test_tile_lists(tier, audit):
    """B x L = 16384 = hip.COMPACT_MIN_ROWS, left-padded: ops._live hands the backward real lists.  Then the mask loop."""
    from recguru_amd import hip, ops, training as T
    from recguru_amd.optim import Adam
    ops.set_compute_dtype(TIERS[tier])
    assert 128 * 128 >= hip.COMPACT_MIN_ROWS
    param, G, D, bt = _small(15, L=128, B=128, k=2)
    opt = Adam(G.parameters(), lr=1e-3)
    T.recon_step(G, opt, bt[0], bt[1], param, "cuda", T._NoDP(), list(G.parameters()))
    torch.cuda.synchronize()
    n_live, n_first = audit.lists["live"], audit.lists["first"]
    assert n_live > 0 and n_first > 0, dict(audit.lists)
    shared, edits = _mask_loop(hip)
    assert shared == 40 and edits == 20 and audit.lists["live"] >= n_live + 80
    audit.notes.append("lists in the training step: live %d first %d; mask loop: 40 masks, %d in-place edits" % (n_live, n_first, edits))


# ------------------------------------------------------------------------------------------------------------------------------
# negative controls: the auditor can fail
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sweeping", [False, True])
def test_control_bump_is_a_noop(sweeping, audit, monkeypatch):
    """Without ops.bump the raw-pointer update moves no version: the copy of the previous step is served.  With the sweep off the
    first hand-out after the step reports it, one step old; with it on the sweep after the step does."""
    from recguru_amd import ops
    from recguru_amd.optim import Adam
    param, G, D, bt = _small(17)
    opt = Adam(G.parameters(), lr=1e-2)
    _fwd_bwd(G, bt, param)
    opt.step()
    _fwd_bwd(G, bt, param)                                                      # coherent so far
    audit.sweeping = sweeping
    monkeypatch.setattr(ops, "bump", lambda p: None)
    if sweeping:
        with pytest.raises(A.StaleError) as e:
            opt.step()
        assert e.value.where.startswith("sweep")
    else:
        opt.step()
        with pytest.raises(A.StaleError) as e:
            _forward(G, bt, param)
        assert e.value.where == "hand-out"
    assert e.value.age == 1 and e.value.index is not None and e.value.key is not None
    audit.notes.append("reported: " + str(e.value)[:160])


def test_control_refresh_turn_held(audit, monkeypatch):
    """Both refreshes write the same generation of buffers: the copy handed out after step 1 is overwritten by step 2 -- the
    lifetime scenario fails at its second check."""
    from recguru_amd import ops
    real = ops.refresh_shadows

    def refresh(params):
        real(params)
        for ent in ops._REFRESH_CACHE.values():
            ent["turn"] = 0

    monkeypatch.setattr(ops, "refresh_shadows", refresh)
    with pytest.raises(A.StaleError, match="after optimizer step 2.*held copy .* taken after step 1") as e:
        _lifetime(audit, "bf16")
    audit.notes.append("reported: " + str(e.value)[:160])


def test_control_live_list_keyed_without_version(audit):
    """hip._LIVE keyed by the address alone (a .data view has a version counter of its own, always 0): the list of the mask before
    an in-place edit is served after it."""
    from recguru_amd import hip
    real = audit._orig["live_tiles"]
    audit._orig["live_tiles"] = lambda rowmask, M: real(rowmask.data, M)
    with pytest.raises(A.StaleError) as e:
        _mask_loop(hip)
    assert e.value.kind == "live" and e.value.index is not None
    audit.notes.append("reported: " + str(e.value)[:160])
