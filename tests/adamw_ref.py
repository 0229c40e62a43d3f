"""A float64 restatement of recguru_amd.optim.Adam's update with its options, for the tests to hold the kernels to.

The formulas are torch's:
  torch.nn.utils.clip_grad_norm_(params, max_norm):  total = sqrt(sum over every gradient of sum(g^2));
      coef = min(1, max_norm / (total + 1e-6));  g <- coef * g                      (clip_grad.py: clip_coef_clamped)
  torch.optim.Adam(weight_decay=wd), per parameter with its own step count t (counted from 1):
      g <- g + wd * p                                                               (after the clip: the clip runs before step())
      m <- b1 * m + (1 - b1) * g;   v <- b2 * v + (1 - b2) * g * g
      p <- p - lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)               (adam.py: _single_tensor_adam)
  torch.optim.AdamW(weight_decay=wd):  p <- p * (1 - lr * wd) first, g unchanged, then the same update
                                                                                    (adamw.py / decoupled_weight_decay)
and the library's own rule where torch has none:
  skip_nonfinite:  when sum(g^2) is inf or NaN nothing is written to p, m or v, and every live parameter's t still advances
      (a skipped step counts as a step).
A parameter whose gradient is None enters neither the norm nor the update, and its t does not advance.
"""
import math

import numpy as np


def total_sq(grads):
    """sum of g^2 in float64 over the given (float32 or float64) gradient arrays; None entries are skipped."""
    return float(sum(np.sum(np.asarray(g, dtype=np.float64) ** 2) for g in grads if g is not None))


def clip_coef(tsq, max_norm):
    if not max_norm:
        return 1.0
    return min(1.0, max_norm / (math.sqrt(tsq) + 1e-6))


class RefAdam(object):
    """groups: list of dicts {"params": [float64 arrays, updated in place], "lr", "betas", "eps", "weight_decay", "decoupled"}."""
    def __init__(self, groups, max_norm=None, skip_nonfinite=False):
        self.groups = groups
        self.max_norm, self.skip_nonfinite = max_norm, skip_nonfinite
        self.skipped = 0
        for g in groups:
            g.setdefault("weight_decay", 0.0)
            g.setdefault("decoupled", False)
            g.setdefault("eps", 1e-8)
            g["params"] = [np.array(p, dtype=np.float64) for p in g["params"]]
            g["m"] = [np.zeros_like(p) for p in g["params"]]
            g["v"] = [np.zeros_like(p) for p in g["params"]]
            g["t"] = [0] * len(g["params"])

    def step(self, grads):
        """grads: per group a list of arrays (or None) matching params.  Returns the measured norm."""
        with np.errstate(over="ignore", invalid="ignore"):
            tsq = total_sq([x for gg in grads for x in gg])
        coef = clip_coef(tsq, self.max_norm) if self.max_norm else 1.0
        skip = self.skip_nonfinite and not math.isfinite(tsq)
        self.skipped += int(skip)
        for g, gg in zip(self.groups, grads):
            b1, b2 = g["betas"]
            lr, eps, wd = g["lr"], g["eps"], g["weight_decay"]
            for i, gr in enumerate(gg):
                if gr is None:
                    continue
                g["t"][i] += 1
                if skip:
                    continue
                t = g["t"][i]
                p, m, v = g["params"][i], g["m"][i], g["v"][i]
                ge = coef * np.asarray(gr, dtype=np.float64)
                if wd and not g["decoupled"]:
                    ge = ge + wd * p
                if wd and g["decoupled"]:
                    p *= 1.0 - lr * wd
                m[...] = b1 * m + (1 - b1) * ge
                v[...] = b2 * v + (1 - b2) * ge * ge
                p -= lr / (1 - b1 ** t) * m / (np.sqrt(v) / math.sqrt(1 - b2 ** t) + eps)
        return math.sqrt(tsq) if tsq >= 0 else float("nan")
