"""Host restatements of every cached weight copy and tile list, and the auditor that holds the caches to them.

The kernels never read a parameter: they read the copies ops.shadow / shadow_cat / bias_cat / pad_rows_cat keep per parameter
version (and ops.refresh_shadows rewrites after every optimizer step), and the tile lists hip.live_tiles / first_live keep per
mask version.  The invariant: at every moment a cached object is HANDED TO A CALLER its bits equal a recomputation from the current
f32 masters (or the current row mask).  The recomputation below is plain torch -- none of the cast / list kernels, none of the
functions under audit -- and every comparison is torch.equal on the raw integer view: no tolerance anywhere.

Pure torch: importable without a GPU (tests/test_shadow_audit_cpu.py holds the restatements to themselves).
"""
import collections
import weakref

import torch

TRANSPOSE, PACK, SPLIT = 1, 2, 4          # the cast-mode bits (include/recguru_hip.h RG_CAST_*)
KEEP_STEPS = 3                            # how many optimizer steps back a stale copy is dated


# ------------------------------------------------------------------------------------------------------------------------------
# restatements
# ------------------------------------------------------------------------------------------------------------------------------
def raw(t):
    """The flat raw-integer view of a tensor: int16 for bf16, int32 for f32 and int32."""
    t = t.detach().contiguous().reshape(-1)
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16)
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    assert t.dtype in (torch.int16, torch.int32), t.dtype
    return t


def same_bits(got, want):
    """(equal, first differing index or None) of two tensors' raw views.  A presplit copy is an f32-typed buffer of bf16 halves:
    when the element sizes differ both sides are read as int16."""
    a, b = raw(got), raw(want)
    if a.dtype != b.dtype:
        a, b = a.view(torch.int16), b.view(torch.int16)
    if a.numel() != b.numel():
        return False, min(a.numel(), b.numel())
    if torch.equal(a, b):
        return True, None
    return False, int(torch.nonzero(a != b)[0])


def pack(m):
    """[N, K] -> [N / 16, K / 32, 64, 8]: block (n / 16, k / 32) holds 64 lanes x 8 elements, lane 16 g + i = M[16 nb + i][32 kb + 8 g .. + 8]."""
    N, K = m.shape
    assert N % 16 == 0 and K % 32 == 0, (N, K)
    return m.reshape(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).reshape(N // 16, K // 32, 64, 8).contiguous()


def unpack(blocks):
    """The inverse of pack(): [N / 16, K / 32, 64, 8] -> [N, K]."""
    nb, kb = blocks.shape[:2]
    return blocks.reshape(nb, kb, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(nb * 16, kb * 32).contiguous()


def split(v):
    """(hi, lo) = (bf16(v), bf16(v - hi)): the bf16x3 tier's operand split."""
    hi = v.to(torch.bfloat16)
    return hi, (v - hi.float()).to(torch.bfloat16)


def presplit(m):
    """[N, K] f32 -> bf16 [N / 16, K / 32, 2, 64, 8]: per fragment the 64 lanes' hi parts (1 KB), then their lo parts (1 KB)."""
    hi, lo = split(pack(m))
    return torch.stack([hi, lo], 2).contiguous()


def _form(w, mode, dtype):
    m = w.t().contiguous() if mode & TRANSPOSE else w.contiguous()
    if mode & SPLIT:
        assert mode & PACK and dtype == torch.float32
        return presplit(m)
    if mode & PACK:
        return pack(m).to(dtype)
    return m.to(dtype)


def restate(kind, params, mode, dtype):
    """The expected tensor of a cached form.  kind: "shadow" (one 2-D parameter), "cat" (torch.cat(params, 0) first), "bias_cat",
    "pad_rows" (mode = H).  mode: TRANSPOSE | PACK | SPLIT.  params: the f32 masters."""
    ps = [p.detach() for p in params]
    if kind == "shadow":
        w = ps[0]
        return _form(w.reshape(w.shape[0], -1) if w.dim() > 1 else w.reshape(1, -1), mode, dtype)
    if kind == "cat":
        return _form(torch.cat(ps, 0), mode, dtype)
    if kind == "bias_cat":
        return torch.cat(ps)
    if kind == "pad_rows":
        H = int(mode)
        rows = [p.reshape(H, 32) for p in ps] + [torch.zeros(1, 32, device=ps[0].device, dtype=ps[0].dtype)]
        return torch.cat(rows, 0).to(dtype)
    raise ValueError(kind)


def form_name(kind, mode):
    if kind == "shadow":
        if mode & SPLIT:
            return "presplit_t" if mode & TRANSPOSE else "presplit"
        if mode & PACK:
            return "packed_t" if mode & TRANSPOSE else "packed"
        return "transposed" if mode & TRANSPOSE else "plain"
    if kind == "cat":
        return "cat_t" if mode & TRANSPOSE else "cat"
    return kind


def restate_live(rowmask, M):
    """int32 [1 + nt], nt = ceil(M / 16): the count of 16-row tiles holding a row with rowmask != 0, their indices ascending, then
    the dead tiles from the far end backwards (list[nt] is the smallest dead index)."""
    nt = (M + 15) // 16
    m = rowmask.detach().reshape(-1)[:M]
    tail = torch.zeros(nt * 16 - M, device=m.device, dtype=torch.bool)
    live = torch.cat([m != 0, tail]).reshape(nt, 16).any(1)
    idx = torch.arange(nt, device=m.device, dtype=torch.int32)
    return torch.cat([live.sum().to(torch.int32).reshape(1), idx[live], idx[~live].flip(0)])


def restate_first(rowmask, B, L):
    """int32 [B]: the first position of each sequence with rowmask != 0, L if it has none."""
    m = rowmask.detach().reshape(-1)[:B * L].reshape(B, L) != 0
    pos = torch.arange(L, device=m.device, dtype=torch.int32).expand(B, L)
    return torch.where(m, pos, torch.full_like(pos, L)).min(1).values.to(torch.int32)


# ------------------------------------------------------------------------------------------------------------------------------
# the auditor
# ------------------------------------------------------------------------------------------------------------------------------
class StaleError(AssertionError):
    """A cached object did not hold the bits of its restatement.  kind / form / key name it, age is the number of optimizer steps
    the bits are old (None: the bits of none of the last KEEP_STEPS steps), index the first differing raw element."""

    def __init__(self, kind, form, key, age, index, where):
        self.kind, self.form, self.key, self.age, self.index, self.where = kind, form, key, age, index, where
        old = "not the bits of any of the last %d optimizer steps" % KEEP_STEPS if age is None else "%d optimizer step(s) old" % age
        super(StaleError, self).__init__("%s: %s %s (key %r) is not its restatement: %s; first differing raw index %s"
                                         % (where, kind, form, key, old, index))


def version_of(p):
    """The auditor's own statement of a parameter's identity: address, autograd version, optimizer generation."""
    return (p.data_ptr(), p._version, getattr(p, "_rg_gen", 0))


def _stamp_of(p):
    """version_of() and the storage object behind p: a replaced p.data is another storage even where the allocator gave it the
    address of the one it freed (only the auditor's own once-per-version bookkeeping uses this)."""
    return version_of(p) + (p.untyped_storage()._cdata,)


class Audit(object):
    """Wraps the six hand-out functions and Adam.step (install() with a monkeypatch: module attributes only, nothing in the
    product).  Every returned object is compared with its restatement on the stream it was handed out on; each distinct (cache
    key, version, buffer address, optimizer step) once.  After each optimizer step every _SHADOWS entry whose recorded version is
    current is swept, and every tensor registered with hold() is held to the lifetime promise of ops.shadow."""

    def __init__(self, ops, hip, optim, sweeping=True):
        self.ops, self.hip, self.optim = ops, hip, optim
        self.sweeping = sweeping                     # False: the hand-out check alone (the negative controls show it suffices)
        self.steps = 0
        self.handouts = collections.Counter()        # every hand-out, per form
        self.audited = collections.Counter()         # the compared ones (distinct key / version / buffer / step), per form
        self.paths = collections.Counter()           # of the compared weight copies: "lazy" | "refresh" | "alias"
        self.dtypes = collections.Counter()          # (tier, storage dtype of the request) per hand-out
        self.lists = collections.Counter()           # "live" / "first" hand-outs compared
        self.retain = None                           # a list: every handed-out tensor is kept alive in it
        self.swept = 0
        self.swept_old = 0                           # entries left in the cache with an old version (rebuilt lazily)
        self._seen = {}
        self._hist = {}                              # id(p) -> (weakref, deque of master clones, newest last)
        self._holds = []
        self._orig = {}

    # ---- installation ------------------------------------------------------------------------------------------------
    def install(self, monkeypatch):
        ops, hip, optim = self.ops, self.hip, self.optim
        for name in ("shadow", "shadow_cat", "bias_cat", "pad_rows_cat"):
            self._orig[name] = getattr(ops, name)
        for name in ("live_tiles", "first_live"):
            self._orig[name] = getattr(hip, name)
        self._orig["step"] = optim.Adam.step
        o = self._orig

        def shadow(p, transpose=False, pack=False, split=False):
            out = o["shadow"](p, transpose, pack, split)
            mode = int(bool(transpose)) | (PACK if pack else 0) | (SPLIT if (split and pack and hip.SPLIT_OPERANDS) else 0)
            self._handout("shadow", (p,), mode, ops.compute_dtype(), out)
            return out

        def shadow_cat(ps, transpose=False):
            out = o["shadow_cat"](ps, transpose)
            self._handout("cat", tuple(ps), int(bool(transpose)), ops.compute_dtype(), out)
            return out

        def bias_cat(ps):
            out = o["bias_cat"](ps)
            self._handout("bias_cat", tuple(ps), 0, torch.float32, out)
            return out

        def pad_rows_cat(ps, H):
            out = o["pad_rows_cat"](ps, H)
            self._handout("pad_rows", tuple(ps), int(H), ops.compute_dtype(), out)
            return out

        def live_tiles(rowmask, M):
            out = o["live_tiles"](rowmask, M)
            nt = (M + 15) // 16
            self._list("live", (rowmask.data_ptr(), rowmask._version, M), out[:1 + nt], restate_live(rowmask, M))
            return out

        def first_live(rowmask, B, L):
            out = o["first_live"](rowmask, B, L)
            self._list("first", (rowmask.data_ptr(), rowmask._version, B, L), out, restate_first(rowmask, B, L))
            return out

        audit = self

        def step(opt, *a, **k):
            audit._snapshot(opt)
            r = o["step"](opt, *a, **k)
            audit.steps += 1
            audit._after_step()
            return r

        monkeypatch.setattr(ops, "shadow", shadow)
        monkeypatch.setattr(ops, "shadow_cat", shadow_cat)
        monkeypatch.setattr(ops, "bias_cat", bias_cat)
        monkeypatch.setattr(ops, "pad_rows_cat", pad_rows_cat)
        monkeypatch.setattr(hip, "live_tiles", live_tiles)
        monkeypatch.setattr(hip, "first_live", first_live)
        monkeypatch.setattr(optim.Adam, "step", step)
        return self

    # ---- hand-outs ---------------------------------------------------------------------------------------------------
    def _tier(self):
        return self.ops.compute_tier()

    def _handout(self, kind, ps, mode, dtype, out):
        form = form_name(kind, mode)
        self.handouts[form] += 1
        if kind in ("shadow", "cat"):
            self.dtypes[(("mixed" if self.ops.mixed() else self._tier()), dtype)] += 1
        if self.retain is not None:
            self.retain.append(out)
        key = (kind, tuple(id(p) for p in ps), mode, dtype)
        stamp = (tuple(_stamp_of(p) for p in ps), out.data_ptr(), self.steps)
        seen = self._seen.get(key)
        if seen is not None and seen[0] == stamp and all(r() is p for r, p in zip(seen[1], ps)):
            if seen[2]:
                return
            # compared by the sweep after this step and handed out now for the first time: counted, not compared twice
        else:
            self._compare(kind, form, key, ps, mode, dtype, out, "hand-out")
        self._seen[key] = (stamp, tuple(weakref.ref(p) for p in ps), True)
        self.audited[form] += 1
        if kind in ("shadow", "cat"):
            self.paths[self._path(ps, out)] += 1

    def _path(self, ps, out):
        ptr = out.data_ptr()
        if any(ptr == p.data_ptr() for p in ps):
            return "alias"                                   # f32 tier, plain form: the master itself
        for ent in self.ops._REFRESH_CACHE.values():
            for outs, _, _ in ent["gens"]:
                if any(ptr == d.data_ptr() for d in outs):
                    return "refresh"
        return "lazy"

    def _compare(self, kind, form, key, ps, mode, dtype, out, where):
        ok, idx = same_bits(out, restate(kind, ps, mode, dtype))
        if not ok:
            raise StaleError(kind, form, key, self._age(kind, ps, mode, dtype, out), idx, where)

    def _age(self, kind, ps, mode, dtype, out):
        """How many optimizer steps old the bits of `out` are: the masters of k steps ago restated and compared."""
        for age in range(1, KEEP_STEPS + 1):
            old, any_old = [], False
            for p in ps:
                h = self._hist.get(id(p))
                if h is not None and h[0]() is p and len(h[1]) >= age:
                    old.append(h[1][-age])
                    any_old = True
                else:
                    old.append(p.detach())
            if not any_old:
                break
            if same_bits(out, restate(kind, old, mode, dtype))[0]:
                return age
        return None

    def _list(self, kind, key, got, want):
        self.lists[kind] += 1
        ok, idx = same_bits(got, want)
        if not ok:
            raise StaleError(kind, "tile list" if kind == "live" else "first-live vector", key, None, idx, "hand-out")

    # ---- optimizer steps ---------------------------------------------------------------------------------------------
    def _snapshot(self, opt):
        for g in opt.param_groups:
            for p in g["params"]:
                if p.grad is None:
                    continue
                h = self._hist.get(id(p))
                if h is None or h[0]() is not p:
                    h = self._hist[id(p)] = (weakref.ref(p), collections.deque(maxlen=KEEP_STEPS))
                h[1].append(p.detach().clone())

    def _after_step(self):
        # the lifetime promise: a copy handed out before this step is still what it was; after the second step it is released
        keep = []
        for t, bits, at, label in self._holds:
            if self.steps - at <= 1:
                ok, idx = same_bits(t, bits)
                if not ok:
                    raise StaleError("held copy", label, None, None, idx, "after optimizer step %d, %d step(s) after the hand-out"
                                     % (self.steps, self.steps - at))
                keep.append((t, bits, at, label))
        self._holds = keep
        if self.sweeping:
            self.sweep()

    def hold(self, t, label):
        """Hold a handed-out copy to the lifetime promise: its bits must not change in the next optimizer step."""
        self._holds.append((t, raw(t).clone(), self.steps, label))

    def sweep(self):
        """Every _SHADOWS entry whose recorded version is current against its restatement."""
        for key, ent in list(self.ops._SHADOWS.items()):
            ps = tuple(r() for r in ent[2])
            if any(p is None for p in ps):
                continue
            if key[-1] == "cat":
                kind, mode, dtype, cur = "cat", int(bool(key[1])), key[2], tuple(version_of(p) for p in ps)
            elif key[-1] == "bias_cat":
                kind, mode, dtype, cur = "bias_cat", 0, torch.float32, tuple(version_of(p) for p in ps)
            elif key[-1] == "pad_rows":
                kind, mode, dtype, cur = "pad_rows", (ent[1].shape[0] - 1) // 3, key[1], tuple(version_of(p) for p in ps)
            else:
                kind, mode, dtype, cur = "shadow", int(key[1]), key[2], version_of(ps[0])
            if ent[0] != cur:
                self.swept_old += 1
                continue
            akey = (kind, tuple(id(p) for p in ps), mode, dtype)
            self._compare(kind, form_name(kind, mode), akey, ps, mode, dtype, ent[1], "sweep after optimizer step %d" % self.steps)
            self._seen[akey] = ((tuple(_stamp_of(p) for p in ps), ent[1].data_ptr(), self.steps), tuple(weakref.ref(p) for p in ps), False)
            self.swept += 1

    # ---- report ------------------------------------------------------------------------------------------------------
    def report(self):
        forms = " ".join("%s=%d/%d" % (k, self.audited[k], self.handouts[k]) for k in sorted(self.handouts))
        return ("steps %d | audited/handed out: %s | lazy %d refresh %d alias %d | lists live %d first %d | swept %d (old, left to the "
                "lazy path: %d)" % (self.steps, forms or "-", self.paths["lazy"], self.paths["refresh"], self.paths["alias"],
                                    self.lists["live"], self.lists["first"], self.swept, self.swept_old))
