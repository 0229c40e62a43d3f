"""Adam on the GPU through rg_adam_multi_dev (include/recguru_hip.h), with torch.optim.Adam's semantics as the
reference configures it (train_gan.py:126-134, gan_training.py:359,920): no amsgrad, parameters whose .grad is None
are skipped, per-parameter step counts.

Options beyond the reference, all off by default (csrc/optim.hip):
  weight_decay, decoupled   torch.optim.Adam(weight_decay=) (coupled: g += wd * p) or torch.optim.AdamW (p *= 1 - lr * wd), per group.
  max_norm                  torch.nn.utils.clip_grad_norm_ over every live parameter of every group -- EXCEPT that p.grad is not
                            rewritten: the clipped gradient exists only inside the update (one write pass less).  Code that reads
                            p.grad after step() sees the unclipped values.
  skip_nonfinite            a step whose squared gradient norm is inf or NaN writes nothing to p, exp_avg or exp_avg_sq.  A SKIPPED
                            STEP COUNTS AS A STEP: the per-parameter step counts advance as usual, so that st["step"], the host mirror
                            of the device counters, stays exact without a read-back.  The only effect is on the bias corrections of the
                            first few steps after a skip.
  ema_decay, ema_warmup     an exponential moving average of the weights, kept by the update launch itself (rg_adam_multi_dev3;
                            DESIGN.md 6i): st["ema"] <- d_t * st["ema"] + (1 - d_t) * p_new after every update of p, with
                            d_t = ema_decay, or min(ema_decay, (1 + t) / (10 + t)) under ema_warmup (t: p's own step count after the
                            update).  THE AVERAGE FOLLOWS A PARAMETER'S OWN UPDATES: it is created, as a copy of the parameter, when the
                            parameter first has a gradient under this optimizer (before that first update); a step in which the parameter
                            has no gradient leaves its average untouched; a parameter that never had one has no average.  A step that
                            skip_nonfinite skips leaves the average alone too (and counts, as above).  ema_decay = None is off, 0.0 is
                            valid (the average then equals the weights).  swap_ema() / averaged() exchange weights and averages in
                            place, for evaluation and for saving; while they are exchanged step(), state_dict() and load_state_dict()
                            raise RuntimeError.
With every option neutral step() is the code path it was: one hip.adam_multi_dev launch per group.
"""
import contextlib

import torch

from . import hip, ops


def _key(live):
    return tuple((p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"])
                 + ((st["ema"].data_ptr(),) if "ema" in st else ()) for p, st in live)


def _rows(live):
    rows = []
    for p, st in live:                                    # st["step"]: updates this parameter has had so far
        n = p.numel()
        for off in range(0, n, hip.ADAM_CHUNK):
            rows.append((p.data_ptr() + 4 * off, p.grad.data_ptr() + 4 * off, st["exp_avg"].data_ptr() + 4 * off,
                         st["exp_avg_sq"].data_ptr() + 4 * off, min(hip.ADAM_CHUNK, n - off), st["step"]))
    return rows


def _ema_rows(live):
    """The average's address for every row of _rows(live), in the same order."""
    return [st["ema"].data_ptr() + 4 * off for p, st in live for off in range(0, p.numel(), hip.ADAM_CHUNK)]


def _upload(arr, dev):
    """A numpy table as (pinned host bytes, device bytes); the host tensor must outlive the asynchronous copy."""
    import numpy as np
    host = torch.from_numpy(arr.view(np.uint8).copy()).pin_memory()
    return host, host.to(dev, non_blocking=True)


def options(param, critic=False):
    """Constructor keywords from the run's configuration (config.get_param: weight_decay, decoupled_wd, clip_norm, skip_nonfinite,
    ema_decay, ema_warmup).  Decay, clipping and the weight average go to the reconstruction / recommender optimizers; critic=True (the
    W-GAN pair, whose balance the gradient penalty sets) takes skip_nonfinite alone.  ema_decay / ema_warmup appear only when
    param.ema_decay > 0.  A configuration object without the attributes gives the neutral set."""
    kw = {"skip_nonfinite": bool(getattr(param, "skip_nonfinite", False))}
    if not critic:
        kw.update(weight_decay=float(getattr(param, "weight_decay", 0.0)), decoupled=bool(getattr(param, "decoupled_wd", False)),
                  max_norm=float(getattr(param, "clip_norm", 0.0)) or None)
        ema = float(getattr(param, "ema_decay", 0.0) or 0.0)
        if ema > 0:
            kw.update(ema_decay=ema, ema_warmup=bool(getattr(param, "ema_warmup", False)))
    return kw


def norm_of(opt):
    """The last measured gradient norm of an optimizer (or of the one a ScheduledOptim wraps) as a device scalar, None when it
    does not clip."""
    opt = getattr(opt, "_optimizer", opt)
    return opt.grad_norm() if getattr(opt, "max_norm", None) else None


def has_average(opt):
    """True when the optimizer (or the one a ScheduledOptim wraps) keeps an average of its weights."""
    return getattr(getattr(opt, "_optimizer", opt), "ema_decay", None) is not None


@contextlib.contextmanager
def averaged(*opts):
    """with averaged(opt_a, opt_b, ...): the parameters of every given optimizer (or of the one a ScheduledOptim wraps) hold their
    averages inside the block and their raw weights again behind it, also when the block raises.  An optimizer without an average
    (ema_decay=None, another class, None) is left alone: nothing is launched for it."""
    opts = [getattr(o, "_optimizer", o) for o in opts if o is not None]
    opts = [o for o in opts if getattr(o, "ema_decay", None) is not None]
    with contextlib.ExitStack() as stack:
        for o in opts:
            stack.enter_context(o.averaged())
        yield


class Adam(object):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, max_norm=None,
                 skip_nonfinite=False, ema_decay=None, ema_warmup=False):
        """params: an iterable of parameters, or a list of torch-style group dicts {"params": [...], and optionally "lr", "betas",
        "eps", "weight_decay", "decoupled"}.  max_norm and skip_nonfinite belong to the optimizer: one norm over all groups; so do
        ema_decay (None: off; 0 <= ema_decay < 1) and ema_warmup."""
        params = list(params)
        if not params or not isinstance(params[0], dict):
            params = [{"params": params}]
        self.param_groups = []
        for g in params:
            extra = set(g) - {"params", "lr", "betas", "eps", "weight_decay", "decoupled"}
            if extra:
                raise ValueError("recguru_amd.optim.Adam: unknown group option(s) %s" % sorted(extra))
            grp = {"params": [p for p in g["params"]], "lr": g.get("lr", lr), "betas": tuple(g.get("betas", betas)), "eps": g.get("eps", eps),
                   "weight_decay": float(g.get("weight_decay", weight_decay)), "decoupled": bool(g.get("decoupled", decoupled))}
            if grp["weight_decay"] < 0:
                raise ValueError("recguru_amd.optim.Adam: weight_decay < 0")
            self.param_groups.append(grp)
        if max_norm is not None and max_norm < 0:
            raise ValueError("recguru_amd.optim.Adam: max_norm < 0")
        self.max_norm = None if not max_norm else float(max_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        if ema_decay is not None:
            ema_decay = float(ema_decay)
            if not 0.0 <= ema_decay < 1.0:                # (NaN fails both comparisons)
                raise ValueError("recguru_amd.optim.Adam: ema_decay must be None or in [0, 1), got %r" % ema_decay)
        self.ema_decay = ema_decay
        self.ema_warmup = bool(ema_warmup)
        self.ema_swapped = False                          # True: the parameters hold the averages and st["ema"] the raw weights
        self._pairs = None                                # device rg_ema_pair table of swap_ema(), cached per set of buffers
        self.state = {}
        self._tables = {}
        self._ctl = None                                  # device rg_adam_ctl of the option path; survives table rebuilds (the skipped counter)

    def zero_grad(self, set_to_none=True):
        """p.grad = None for every parameter (so step() skips what the next backward does not touch), but the
        gradient buffers are kept, zeroed in a few multi-tensor launches and re-adopted by the in-place
        accumulating backward (ops.release_grads)."""
        for g in self.param_groups:
            if set_to_none:
                ops.release_grads(g["params"])
            else:
                for p in g["params"]:
                    if p.grad is not None:
                        p.grad.zero_()

    def state_dict(self):
        """{"state": {parameter index: {"step", "exp_avg", "exp_avg_sq"}}, "param_groups": [...]} -- torch.optim.Adam's layout; with
        ema_decay on, "ema" beside exp_avg for every parameter that has an average."""
        self._not_swapped("state_dict()")
        params = [p for g in self.param_groups for p in g["params"]]
        idx = {id(p): i for i, p in enumerate(params)}
        return {"state": {idx[id(p)]: dict({"step": st["step"], "exp_avg": st["exp_avg"].clone(), "exp_avg_sq": st["exp_avg_sq"].clone()},
                                           **({"ema": st["ema"].clone()} if "ema" in st else {}))
                          for p, st in self.state.items()},
                "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]}

    def load_state_dict(self, sd):
        """A checkpoint of this class or of torch.optim.Adam / AdamW.  "ema" is restored when this optimizer keeps an average; a
        checkpoint without it loads, and the average then starts from the weights at the parameter's next live step."""
        self._not_swapped("load_state_dict()")
        params = [p for g in self.param_groups for p in g["params"]]
        self.state = {}
        for i, st in sd["state"].items():
            p = params[int(i)]
            self.state[p] = {"step": int(st["step"]), "exp_avg": st["exp_avg"].to(p.device, torch.float32).clone(),
                             "exp_avg_sq": st["exp_avg_sq"].to(p.device, torch.float32).clone()}
            if self.ema_decay is not None and st.get("ema") is not None:
                self.state[p]["ema"] = st["ema"].to(p.device, torch.float32).clone().contiguous()
        for g, gs in zip(self.param_groups, sd.get("param_groups", [])):
            # only what step() implements is taken over; a torch.optim.Adam checkpoint that relies on anything else must not load
            # silently into different semantics
            if gs.get("amsgrad", False) or gs.get("maximize", False):
                raise ValueError("recguru_amd.optim.Adam: amsgrad / maximize are not implemented (checkpoint asks for %s)"
                                 % {k: gs[k] for k in ("amsgrad", "maximize") if gs.get(k)})
            if float(gs.get("weight_decay", 0) or 0) < 0:
                raise ValueError("recguru_amd.optim.Adam: weight_decay < 0")
            g.update({k: gs[k] for k in ("lr", "betas", "eps") if k in gs})
            if "weight_decay" in gs:
                g["weight_decay"] = float(gs["weight_decay"] or 0)
            if "decoupled" in gs:                         # this class's own state_dict
                g["decoupled"] = bool(gs["decoupled"])
            if "decoupled_weight_decay" in gs:            # torch.optim.Adam / AdamW (torch >= 2.7 writes the key)
                g["decoupled"] = bool(gs["decoupled_weight_decay"])
        self._tables = {}                                 # device tables are rebuilt from the restored state
        self._pairs = None

    def grad_norm(self):
        """The global gradient norm the last step() measured (before clipping), a float32 device scalar; no host wait.  None before the
        first step with an option on (only the option path measures a norm)."""
        if self._ctl is None:
            return None
        return self._ctl[8:12].view(torch.float32)[0].clone()

    def skipped_steps(self):
        """Number of steps skip_nonfinite has skipped.  Reads the device counter back: the one call here that waits for the GPU."""
        if self._ctl is None:
            return 0
        return int(self._ctl[24:32].view(torch.int64)[0].item())

    def _neutral(self):
        return (self.max_norm is None and not self.skip_nonfinite and self.ema_decay is None
                and not any(g["weight_decay"] for g in self.param_groups))

    def _not_swapped(self, what):
        if self.ema_swapped:
            raise RuntimeError("recguru_amd.optim.Adam: %s while the parameters hold the averaged weights (swap_ema() back first)" % what)

    def _live(self, g):
        live = []
        for p in g["params"]:
            if p.grad is None:
                continue
            st = self.state.get(p)
            if st is None:
                st = {"step": 0, "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
                self.state[p] = st
            if not p.grad.is_contiguous():
                p.grad = p.grad.contiguous()
            if self.ema_decay is not None and "ema" not in st:
                st["ema"] = p.detach().clone(memory_format=torch.contiguous_format)      # the weights before this parameter's first update here
            live.append((p, st))
        return live

    @torch.no_grad()
    def step(self):
        """One rg_adam_multi_dev launch per parameter group over a DEVICE-RESIDENT segment table listing (chunks of) the
        parameters that have a gradient.  The table -- pointers, chunk sizes and the per-parameter step counts, which the
        kernel itself advances -- is uploaded (from pinned memory) only when that set of parameters or one of their
        buffers changes; in steady state an optimizer step moves nothing across PCIe and never blocks the host."""
        import numpy as np
        self._not_swapped("step()")
        if not self._neutral():
            return self._step_options()
        for gi, g in enumerate(self.param_groups):
            b1, b2 = g["betas"]
            live = self._live(g)
            if not live:
                continue
            # every pointer baked into the table, and the host-side step counts: state restored or edited from outside
            # (load_state_dict, a replaced exp_avg_sq, an edited step) changes the key and rebuilds the table from the host values
            key = _key(live)
            cache = self._tables.get(gi)
            if cache is None or cache["key"] != key:
                tbl = np.array(_rows(live), dtype=hip.ADAM_SEG_DEV_DTYPE)
                host = torch.from_numpy(tbl.view(np.uint8).copy()).pin_memory()
                cache = {"key": key, "n": len(tbl), "dev": host.to(live[0][0].device, non_blocking=True), "host": host}
                self._tables[gi] = cache
            hip.adam_multi_dev(cache["dev"], cache["n"], g["lr"], b1, b2, g["eps"])
            for p, st in live:
                st["step"] += 1                           # host mirror of the device counters (used when the table is rebuilt)
                ops.bump(p)
            cache["key"] = _key(live)                     # the key the NEXT step expects (the device counters advanced with the host's)
            ops.refresh_shadows([p for p, _ in live])

    def _step_options(self):
        """step() with an option on.  ONE segment table for all groups (group after group, so that a group's update launch walks a
        slice of it) and beside it the partial-sum buffer; the control record is allocated once.  Launches: the norm over the whole
        table and its finalize (rg_grad_sqnorm_multi), then one rg_adam_multi_dev2 per group -- rg_adam_multi_dev3 with ema_decay on, over
        the same table and a device array of the averages' addresses that is built, cached and dropped with it.  Nothing is uploaded in
        steady state and nothing waits: clip coefficient and skip verdict stay on the device."""
        import numpy as np
        lives = [self._live(g) for g in self.param_groups]
        flat = [x for live in lives for x in live]
        if not flat:
            return
        dev = flat[0][0].device
        key = tuple(_key(live) for live in lives)
        cache = self._tables.get("all")
        if cache is None or cache["key"] != key:
            rows, spans = [], []
            for live in lives:
                r = _rows(live)
                spans.append((len(rows), len(r)))
                rows += r
            if not rows:                                  # live parameters without elements: nothing to launch
                return
            tbl = np.array(rows, dtype=hip.ADAM_SEG_DEV_DTYPE)
            host = torch.from_numpy(tbl.view(np.uint8).copy()).pin_memory()
            cache = {"key": key, "n": len(tbl), "spans": spans, "dev": host.to(dev, non_blocking=True), "host": host,
                     "partial": torch.empty(len(tbl), device=dev, dtype=torch.float32)}
            if self.ema_decay is not None:
                cache["ema_host"], cache["ema"] = _upload(np.array([a for live in lives for a in _ema_rows(live)], dtype=np.uint64), dev)
            self._tables = {"all": cache}
        if self._ctl is None or self._ctl.device != dev:
            self._ctl = torch.zeros(np.dtype(hip.ADAM_CTL_DTYPE).itemsize, device=dev, dtype=torch.uint8)
        ctl = None
        if self.max_norm is not None or self.skip_nonfinite:
            ctl = self._ctl
            hip.grad_sqnorm_multi(cache["dev"], cache["n"], cache["partial"], ctl, self.max_norm or 0.0, self.skip_nonfinite)
        rec = np.dtype(hip.ADAM_SEG_DEV_DTYPE).itemsize
        for g, live, (first, n) in zip(self.param_groups, lives, cache["spans"]):
            if n and self.ema_decay is not None:
                hip.adam_multi_dev3(cache["dev"][first * rec:], cache["ema"][first * 8:], n, g["lr"], g["betas"][0], g["betas"][1], g["eps"],
                                    g["weight_decay"], g["decoupled"], ctl, self.ema_decay, self.ema_warmup)
            elif n:
                hip.adam_multi_dev2(cache["dev"][first * rec:], n, g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"],
                                    g["decoupled"], ctl)
            for p, st in live:
                st["step"] += 1                           # also on a skipped step: the device counters advance too
                ops.bump(p)
        cache["key"] = tuple(_key(live) for live in lives)
        ops.refresh_shadows([p for p, _ in flat])

    @torch.no_grad()
    def swap_ema(self):
        """Exchange weights and averages of every parameter that has an average, in ONE rg_ema_swap_multi launch over a cached device
        table of (parameter, average) chunks, and let every cached operand copy follow (ops.bump, ops.refresh_shadows).  Word for
        word: two calls restore every bit.  ema_swapped tells which side the parameters hold.  Without ema_decay: nothing."""
        import numpy as np
        if self.ema_decay is None:
            return
        both = [(p, st["ema"]) for g in self.param_groups for p in g["params"] for st in (self.state.get(p),)
                if st is not None and "ema" in st and p.numel()]
        self.ema_swapped = not self.ema_swapped
        if not both:
            return
        key = tuple((p.data_ptr(), e.data_ptr(), p.numel()) for p, e in both)
        if self._pairs is None or self._pairs["key"] != key:
            rows = [(p.data_ptr() + 4 * off, e.data_ptr() + 4 * off, min(hip.ADAM_CHUNK, p.numel() - off))
                    for p, e in both for off in range(0, p.numel(), hip.ADAM_CHUNK)]
            host, dev = _upload(np.array(rows, dtype=hip.EMA_PAIR_DTYPE), both[0][0].device)
            self._pairs = {"key": key, "n": len(rows), "host": host, "dev": dev}
        hip.ema_swap_multi(self._pairs["dev"], self._pairs["n"])
        for p, _ in both:
            ops.bump(p)
        ops.refresh_shadows([p for p, _ in both])

    @contextlib.contextmanager
    def averaged(self):
        """with opt.averaged(): the parameters hold their averages inside the block and their raw weights again behind it, also when
        the block raises."""
        self._not_swapped("averaged()")
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()


class AdamW(Adam):
    """torch.optim.AdamW: Adam with decoupled weight decay, 1e-2 by default."""
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, decoupled=True, max_norm=None,
                 skip_nonfinite=False, ema_decay=None, ema_warmup=False):
        super(AdamW, self).__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled=decoupled,
                                    max_norm=max_norm, skip_nonfinite=skip_nonfinite, ema_decay=ema_decay, ema_warmup=ema_warmup)
