"""A float64 restatement of the weight average recguru_amd.optim.Adam keeps (ema_decay / ema_warmup), on top of tests/adamw_ref.RefAdam.

The rule (include/recguru_hip.h: rg_adam_multi_dev3; recguru_amd/optim.py):
  start    a parameter's average is created when the parameter first has a gradient, as a copy of the parameter BEFORE that update;
  update   after every update of the parameter, with t its own step count counted from 1 (after this update),
               d_t = min(ema_decay, (1 + t) / (10 + t))  under ema_warmup,   d_t = ema_decay  otherwise
               e <- d_t * e + (1 - d_t) * p_new
  absent   a step in which the parameter has no gradient leaves its average (and its t) alone; a parameter that never had a gradient
           has no average (None here);
  skip     a step that skip_nonfinite skips writes nothing, the average included -- and t still advances, so the next step's warm-up
           factor is that of the advanced count.
"""
import numpy as np

from adamw_ref import RefAdam


def decay_at(ema_decay, ema_warmup, t):
    """d_t of the rule above for a parameter's step count t (counted from 1)."""
    return min(ema_decay, (1.0 + t) / (10.0 + t)) if ema_warmup else ema_decay


class RefEmaAdam(RefAdam):
    """RefAdam that keeps g["ema"]: per parameter a float64 array, or None while the parameter has had no gradient."""
    def __init__(self, groups, max_norm=None, skip_nonfinite=False, ema_decay=0.0, ema_warmup=False):
        RefAdam.__init__(self, groups, max_norm=max_norm, skip_nonfinite=skip_nonfinite)
        self.ema_decay, self.ema_warmup = float(ema_decay), bool(ema_warmup)
        for g in self.groups:
            g["ema"] = [None] * len(g["params"])

    def step(self, grads):
        for g, gg in zip(self.groups, grads):
            for i, gr in enumerate(gg):
                if gr is not None and g["ema"][i] is None:
                    g["ema"][i] = g["params"][i].copy()                      # the weights before the first update
        skipped = self.skipped
        norm = RefAdam.step(self, grads)
        if self.skipped == skipped:                                          # not a skipped step
            for g, gg in zip(self.groups, grads):
                for i, gr in enumerate(gg):
                    if gr is None:
                        continue
                    d = decay_at(self.ema_decay, self.ema_warmup, g["t"][i])
                    g["ema"][i][...] = d * g["ema"][i] + (1.0 - d) * g["params"][i]
        return norm
