"""tests/shadow_audit.py held to itself on the CPU: the layouts the restatements claim, on inputs small enough to check by hand."""
import pytest
import torch

import shadow_audit as A


def _w(N, K, seed=0):
    return torch.randn(N, K, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("N,K", [(16, 32), (64, 96), (384, 128), (128, 512)])
def test_pack_layout_and_roundtrip(N, K):
    m = _w(N, K, N + K)
    b = A.pack(m)
    assert b.shape == (N // 16, K // 32, 64, 8)
    assert torch.equal(A.unpack(b), m)                                           # pack followed by unpack is the identity
    for nb, kb, g, i in [(0, 0, 0, 0), (N // 16 - 1, K // 32 - 1, 3, 15), (N // 32, K // 64, 2, 7), (0, K // 32 - 1, 1, 9)]:
        assert torch.equal(b[nb, kb, 16 * g + i], m[16 * nb + i, 32 * kb + 8 * g:32 * kb + 8 * g + 8])     # lane 16 g + i


def test_pack_rejects_ragged_shapes():
    with pytest.raises(AssertionError):
        A.pack(torch.zeros(24, 32))
    with pytest.raises(AssertionError):
        A.pack(torch.zeros(32, 48))


def test_split_reconstructs_to_2_pow_minus_16():
    v = _w(64, 96, 1)
    hi, lo = A.split(v)
    assert hi.dtype == lo.dtype == torch.bfloat16
    assert float(((hi.float() + lo.float()) - v).abs().max() / v.abs().max()) < 2 ** -16
    s = A.presplit(v)                                                            # 2 KB slot: hi parts, then lo parts
    assert s.shape == (4, 3, 2, 64, 8) and s.numel() * 2 == v.numel() * 4
    assert torch.equal(s[:, :, 0], A.pack(v).to(torch.bfloat16))
    assert torch.equal(A.unpack(s[:, :, 0].float() + s[:, :, 1].float()), hi.float() + lo.float())


def test_restate_forms():
    q, k, v = _w(32, 64, 2), _w(32, 64, 3), _w(32, 64, 4)
    bf = torch.bfloat16
    assert torch.equal(A.restate("shadow", [q], 0, bf), q.to(bf))
    assert torch.equal(A.restate("shadow", [q], A.TRANSPOSE, bf), q.t().contiguous().to(bf))
    assert torch.equal(A.restate("shadow", [q], A.PACK, bf), A.pack(q).to(bf))
    assert torch.equal(A.restate("shadow", [q], A.PACK | A.TRANSPOSE, torch.float32), A.pack(q.t().contiguous()))
    assert torch.equal(A.restate("shadow", [q], A.PACK | A.SPLIT, torch.float32), A.presplit(q))
    cat = torch.cat([q, k, v], 0)
    assert torch.equal(A.restate("cat", [q, k, v], 0, torch.float32), cat)       # f32 tier, no transpose: the concatenation itself
    assert torch.equal(A.restate("cat", [q, k, v], A.TRANSPOSE, bf), cat.t().contiguous().to(bf))
    bq, bk, bv = torch.arange(64.0), torch.arange(64.0) + 100, torch.arange(64.0) + 200
    assert torch.equal(A.restate("bias_cat", [bq, bk, bv], 0, torch.float32), torch.cat([bq, bk, bv]))
    rows = A.restate("pad_rows", [bq, bk, bv], 2, bf)
    assert rows.shape == (7, 32) and rows.dtype == bf
    assert torch.equal(rows[1], bq[32:].to(bf)) and torch.equal(rows[2], bk[:32].to(bf)) and torch.equal(rows[5], bv[32:].to(bf))
    assert not rows[6].any()                                                     # the zero row
    names = [A.form_name("shadow", m) for m in (0, 1, 2, 3, 6, 7)] + [A.form_name("cat", 0), A.form_name("cat", 1)]
    assert names == ["plain", "transposed", "packed", "packed_t", "presplit", "presplit_t", "cat", "cat_t"]


def test_same_bits_reads_a_presplit_buffer_as_halves():
    v = _w(32, 64, 5)
    want = A.presplit(v)
    got = want.reshape(-1).view(torch.float32).reshape(32, 64)                   # how the cache types the buffer
    assert A.same_bits(got, want) == (True, None)
    bad = got.clone()
    bad.view(-1).view(torch.int16)[77] ^= 1
    assert A.same_bits(bad, want) == (False, 77)
    assert A.same_bits(torch.zeros(3), torch.zeros(4)) == (False, 3)
    assert A.same_bits(torch.tensor([0.0]), torch.tensor([-0.0])) == (False, 0)   # bits, not values


def test_live_list_hand_made_masks():
    m = torch.zeros(40)                                                          # M = 40: tiles 0..2, the last one ragged (8 rows)
    m[17] = 0.5
    m[39] = -2.0
    assert A.restate_live(m, 40).tolist() == [2, 1, 2, 0]
    assert A.restate_live(torch.zeros(40), 40).tolist() == [0, 2, 1, 0]          # all dead: from the far end backwards
    assert A.restate_live(torch.ones(40), 40).tolist() == [3, 0, 1, 2]           # all live
    m = torch.zeros(64)
    m[0] = 1
    m[63] = 1
    assert A.restate_live(m, 64).tolist() == [2, 0, 3, 2, 1]
    assert A.restate_live(m, 33).tolist() == [1, 0, 2, 1]                        # only the first 33 rows count
    assert A.restate_live(m, 64).dtype == torch.int32
    assert A.restate_live(torch.tensor([float("nan")]), 1).tolist() == [1, 0]    # != 0, as the kernel tests it


def test_first_live_hand_made_masks():
    m = torch.tensor([[0, 0, 1, 1], [1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 7]], dtype=torch.float32)
    f = A.restate_first(m, 4, 4)
    assert f.dtype == torch.int32 and f.tolist() == [2, 0, 4, 3]
    assert A.restate_first(m.reshape(-1), 4, 4).tolist() == [2, 0, 4, 3]         # a flat view of the mask
    assert A.restate_first(torch.ones(2, 5), 2, 5).tolist() == [0, 0]
    assert A.restate_first(torch.zeros(2, 5), 2, 5).tolist() == [5, 5]


def test_stale_error_names_what_it_found():
    e = A.StaleError("shadow", "packed_t", ("shadow", (1,), 3, torch.bfloat16), 1, 12, "hand-out")
    s = str(e)
    assert "packed_t" in s and "1 optimizer step(s) old" in s and "index 12" in s and "hand-out" in s and e.age == 1
    assert "not the bits of any" in str(A.StaleError("cat", "cat", None, None, 0, "sweep"))


# ------------------------------------------------------------------------------------------------------------------------------
# the auditor's own state machine, on the real ops cache with the cast kernel replaced by its restatement (CPU parameters take
# the lazy path only: refresh_shadows leaves them alone)
# ------------------------------------------------------------------------------------------------------------------------------
class _FakeAdam(object):
    """An optimizer that writes through p.data (no _version bump, like the raw-pointer update) and then bumps."""

    def __init__(self, params):
        self.param_groups = [{"params": list(params)}]

    def step(self):
        from recguru_amd import ops
        for p in self.param_groups[0]["params"]:
            if p.grad is not None:
                p.data.add_(0.37 * p.grad)
                ops.bump(p)


@pytest.fixture
def cpu_audit(monkeypatch):
    import types
    from recguru_amd import hip, ops

    def cast(src, dtype, transpose=False):
        out = A.restate("shadow", [src], int(transpose), dtype)
        if int(transpose) & A.SPLIT:
            out = out.reshape(-1).view(torch.float32).reshape(src.shape[::-1] if int(transpose) & 1 else src.shape)
        return out

    monkeypatch.setattr(hip, "cast", cast)
    fake_optim = types.SimpleNamespace(Adam=_FakeAdam)
    ops.set_compute_dtype(torch.bfloat16)
    monkeypatch.setattr(_FakeAdam, "step", _FakeAdam.step)                       # restored after the auditor's wrapper
    return A.Audit(ops, hip, fake_optim).install(monkeypatch), ops, hip


def _params(n=3, seed=0):
    ps = [torch.nn.Parameter(_w(32, 64, seed + i)) for i in range(n)]
    for p in ps:
        p.grad = torch.ones_like(p)
    return ps


def test_audit_counts_dedups_and_sweeps(cpu_audit):
    audit, ops, hip = cpu_audit
    q, k, v = _params()
    b = [torch.nn.Parameter(torch.arange(64.0) + i) for i in range(3)]
    opt = _FakeAdam([q, k, v])
    for rnd in range(2):
        for _ in range(2):                                                       # the second round of calls is deduplicated
            ops.shadow(q), ops.shadow(q, True), ops.shadow(q, pack=True), ops.shadow(q, True, pack=True, split=True)
            ops.shadow_cat((q, k, v)), ops.shadow_cat((q, k, v), transpose=True), ops.bias_cat(b), ops.pad_rows_cat(b, 2)
        opt.step()
    assert audit.steps == 2 and audit.swept_old > 0 and audit.swept >= 2         # the small concatenations stay current
    for form in ("plain", "transposed", "packed", "packed_t", "cat", "cat_t", "bias_cat", "pad_rows"):
        assert audit.handouts[form] == 4 and audit.audited[form] == 2, (form, audit.audited)     # once per round (bias_cat in round 2: by the sweep)
    assert audit.paths["lazy"] == 12 and audit.paths["refresh"] == 0
    assert "plain=2/4" in audit.report()
    ops.set_compute_dtype("bf16x3")
    hip_split = ops.shadow(q, pack=True, split=True)
    assert hip_split.dtype == torch.float32 and audit.handouts["presplit"] == 1
    assert ops.shadow(q) is not None and audit.paths["alias"] == 1               # f32 storage, plain: the master itself


def test_audit_dates_a_copy_the_optimizer_did_not_bump(cpu_audit, monkeypatch):
    audit, ops, hip = cpu_audit
    q, = _params(1)
    opt = _FakeAdam([q])
    ops.shadow(q, True)
    opt.step()
    ops.shadow(q, True)                                                          # bumped: rebuilt, current
    monkeypatch.setattr(ops, "bump", lambda p: None)
    with pytest.raises(A.StaleError) as e:                                       # the sweep after the step finds it first ...
        opt.step()
    assert e.value.age == 1 and e.value.where.startswith("sweep")
    audit.sweeping = False                                                       # ... and without the sweep the next hand-out does
    with pytest.raises(A.StaleError) as e:
        ops.shadow(q, True)
    assert e.value.age == 1 and e.value.form == "transposed" and e.value.index == 0 and e.value.where == "hand-out"
    opt.step()
    with pytest.raises(A.StaleError) as e:
        ops.shadow(q, True)
    assert e.value.age == 2


def test_audit_tells_a_reused_identity_from_a_seen_one(cpu_audit):
    audit, ops, hip = cpu_audit
    q, = _params(1)
    ops.shadow(q)
    n = audit.audited["plain"]
    ops.shadow(q)
    assert audit.audited["plain"] == n
    key = ("shadow", (id(q),), 0, torch.bfloat16)
    stamp = audit._seen[key][0]
    other = torch.nn.Parameter(q.detach().clone())
    audit._seen[key] = (stamp, (A.weakref.ref(other),), True)                          # the same key and stamp, another object
    ops.shadow(q)
    assert audit.audited["plain"] == n + 1


def test_audit_holds_a_copy_for_one_step(cpu_audit):
    audit, ops, hip = cpu_audit
    q, = _params(1)
    opt = _FakeAdam([q])
    s = ops.shadow(q, pack=True)
    audit.hold(s, "packed copy of q")
    opt.step()                                                                   # untouched: fine
    opt.step()                                                                   # released after the second step
    s.zero_()
    opt.step()
    t = ops.shadow(q, pack=True)
    audit.hold(t, "packed copy of q")
    t.zero_()                                                                    # what a refresh into the SAME generation does
    with pytest.raises(A.StaleError, match="held copy"):
        opt.step()


def test_audit_catches_a_list_cached_without_the_mask_version(cpu_audit, monkeypatch):
    audit, ops, hip = cpu_audit
    cache = {}

    def live_tiles(rowmask, M):                                                  # keyed by the address alone
        if rowmask.data_ptr() not in cache:
            cache[rowmask.data_ptr()] = torch.cat([A.restate_live(rowmask, M), torch.zeros(5, dtype=torch.int32)])
        return cache[rowmask.data_ptr()]

    audit._orig["live_tiles"] = live_tiles
    audit._orig["first_live"] = lambda m, B, L: A.restate_first(m, B, L)
    m = torch.ones(64)
    m[:32] = 0
    assert hip.live_tiles(m, 64)[:5].tolist() == [2, 2, 3, 1, 0]
    assert hip.live_tiles(m.reshape(-1), 64).data_ptr() == hip.live_tiles(m, 64).data_ptr()
    assert hip.first_live(m, 4, 16).tolist() == [16, 16, 0, 0]
    m[0] = 1                                                                     # an in-place edit: _version moves, the address does not
    with pytest.raises(A.StaleError) as e:
        hip.live_tiles(m, 64)
    assert e.value.kind == "live" and e.value.index == 0 and audit.lists["live"] == 4 and audit.lists["first"] == 1
