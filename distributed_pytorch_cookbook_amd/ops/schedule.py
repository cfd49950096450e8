"""Learning-rate schedule: linear warmup, then constant / linear / cosine decay to a floor.

With ``L = base_lr``, ``m = L * min_lr_ratio``, ``W = warmup_steps``, ``T = decay_steps`` and
``t`` the 1-based index of the update being applied (the ``t`` of AdamW's bias corrections):

    t <= W:    lr = L * t / W
    constant:  lr = L
    linear:    lr = L - (L - m) * q            q = min(1, (t - W) / (T - W))
    cosine:    lr = m + (L - m) * 0.5 * (1 + cos(pi * q))

which is ``torch.optim.lr_scheduler.LambdaLR(opt, lambda k: f(k + 1) / L)`` stepped once after
every optimizer step.  This file is the definition in f64 (CPU and host-AdamW paths, logging);
``csrc/misc.hip:adamw_sched_lr`` evaluates the same expressions in f32 inside ``adamw_kernel``
from the device step counter, so a replayed HIP graph applies a new rate every step.  With the
loss scaler ``t`` counts applied steps: a skipped step does not advance the schedule (torch's
``scheduler.step()`` would).
"""
from __future__ import annotations

import math

KINDS = {"constant": 1, "linear": 2, "cosine": 3}  # the kernel's AdamArgs.sched_kind (0 = none)


class LRSchedule:
    def __init__(self, kind: str, base_lr: float, warmup_steps: int = 0, decay_steps: int = 0,
                 min_lr_ratio: float = 0.1):
        if kind not in KINDS:
            raise ValueError(f"lr schedule {kind!r}: one of {sorted(KINDS)}")
        self.kind, self.base_lr = kind, float(base_lr)
        self.warmup_steps, self.decay_steps = int(warmup_steps), int(decay_steps)
        self.min_lr_ratio = float(min_lr_ratio)
        if self.warmup_steps < 0:
            raise ValueError("warmup_steps must be >= 0")
        if kind != "constant" and self.decay_steps <= self.warmup_steps:
            raise ValueError(f"lr schedule {kind!r} needs decay_steps ({self.decay_steps}) > "
                             f"warmup_steps ({self.warmup_steps})")

    @property
    def code(self) -> int:
        return KINDS[self.kind]

    @property
    def min_lr(self) -> float:
        return self.base_lr * self.min_lr_ratio

    def lr_at(self, t) -> float:
        """The rate of update ``t`` (1-based)."""
        L, m, W, T = self.base_lr, self.min_lr, self.warmup_steps, self.decay_steps
        t = float(t)
        if 0 < W and t <= W:  # (t = 0, before the first update, is the start of the ramp)
            return L * t / W
        if self.kind == "constant":
            return L
        q = min(1.0, (t - W) / (T - W))
        if self.kind == "linear":
            return L - (L - m) * q
        return m + (L - m) * 0.5 * (1.0 + math.cos(math.pi * q))

    def params(self) -> dict:
        """What a checkpoint records (``FlatAdamW.state_dict``)."""
        return {"kind": self.kind, "base_lr": self.base_lr, "warmup_steps": self.warmup_steps,
                "decay_steps": self.decay_steps, "min_lr_ratio": self.min_lr_ratio}

    def __eq__(self, other):
        return isinstance(other, LRSchedule) and self.params() == other.params()

    def __repr__(self):
        return "LRSchedule({kind!r}, {base_lr}, warmup_steps={warmup_steps}, decay_steps={decay_steps}, " \
               "min_lr_ratio={min_lr_ratio})".format(**self.params())
