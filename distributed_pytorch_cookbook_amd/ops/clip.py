"""Global-norm gradient clipping over flat gradient buffers (``--max_grad_norm``).

``torch.nn.utils.clip_grad_norm_`` semantics -- ``coef = min(1, max_norm / (norm + 1e-6))``,
a non-finite norm propagates -- without its per-parameter walk and without a host read, so a
captured step replays it:

* ``begin()`` zeroes two device accumulators;
* ``add(grad, replicated)`` adds one flat f32 buffer's sum of squares (``dpc_grad_sumsq``: one
  streaming read, per-block partials summed in a fixed order, no floating-point atomics -- the
  result is bitwise reproducible, so replicas that hold identical gradients compute identical
  coefficients) into ``sumsq[0]`` (gradients that differ per rank: FSDP shards, pipeline
  stages) or ``sumsq[1]`` (gradients every rank holds identically: all-reduced DDP buckets,
  FSDP's replicated 1-D parameters -- counted once);
* ``reduce(transport)`` sums ``sumsq[0]`` over the ranks that hold the other pieces;
* ``finish(pre_scale, pre_scale_t)`` runs the one-thread ``dpc_clip_coef``: the norm of the TRUE
  gradient -- the flat buffer times the factors AdamW folds in anyway, 1/W on the host and the
  loss scaler's 1/scale on the device -- the coefficient, and ``scale_t = coef * pre_scale_t``,
  the device scalar handed to ``FlatAdamW.step`` as ``grad_scale_t``.  The gradient buffer is
  never rewritten: AdamW already multiplies ``grad_scale * *grad_scale_ptr`` in.

Host tensors (the gloo engine tests, CPU runs) take a pure-torch path: f64 sums, same formulas.
"""
from __future__ import annotations

import torch

from . import _lib


class GradClipper:
    def __init__(self, max_norm: float, device):
        if not max_norm > 0.0:
            raise ValueError(f"max_norm must be positive, got {max_norm}")
        dev = torch.device(device)
        self.device = dev
        self.max_norm = float(max_norm)
        self.native = dev.type == "cuda"
        # everything a step touches exists before any capture starts
        self.sumsq = torch.zeros(2, device=dev, dtype=torch.float32 if self.native else torch.float64)
        self.partials = torch.zeros(_lib.SUMSQ_MAX_BLOCKS, device=dev, dtype=torch.float32)
        self.norm_t = torch.zeros((), device=dev, dtype=torch.float32)
        self.coef_t = torch.ones((), device=dev, dtype=torch.float32)
        self.scale_t = torch.ones((), device=dev, dtype=torch.float32)

    @torch.no_grad()
    def begin(self) -> None:
        self.sumsq.zero_()

    @torch.no_grad()
    def add(self, grad: torch.Tensor, replicated: bool) -> None:
        """sumsq[replicated] += sum(grad ** 2) for one flat buffer (any length, 4-byte aligned)."""
        slot = 1 if replicated else 0
        if self.native:
            if not (grad.is_cuda and grad.dtype == torch.float32 and grad.is_contiguous()):
                raise TypeError("GradClipper.add: a contiguous f32 buffer on the clipper's device, got "
                                f"{grad.dtype} on {grad.device} (contiguous={grad.is_contiguous()})")
            _lib.call("dpc_grad_sumsq", _lib.GradSumsqArgs(
                g=grad.data_ptr() if grad.numel() else None, n=grad.numel(),
                partials=self.partials.data_ptr(), sumsq=self.sumsq.data_ptr(), slot=slot), grad.device)
            return
        self.sumsq[slot] += grad.detach().double().pow(2).sum().to(self.sumsq.device)

    @torch.no_grad()
    def reduce(self, transport) -> None:
        """SUM all-reduce of the per-rank accumulator over ``transport``'s group (once per step)."""
        if transport is None or not transport.active or transport.size == 1:
            return
        transport.all_reduce(self.sumsq[0:1])

    @torch.no_grad()
    def finish(self, pre_scale: float = 1.0, pre_scale_t: torch.Tensor | None = None) -> dict:
        """Norm, coefficient and AdamW's scalar from the accumulators.  The true gradient is
        ``buffer * pre_scale * pre_scale_t``; returns ``{"grad_scale_t": scale_t}``."""
        if self.native:
            _lib.call("dpc_clip_coef", _lib.ClipCoefArgs(
                sumsq=self.sumsq.data_ptr(), pre_scale_ptr=_lib.ptr(pre_scale_t),
                norm=self.norm_t.data_ptr(), coef=self.coef_t.data_ptr(), scale=self.scale_t.data_ptr(),
                max_norm=self.max_norm, pre_scale=float(pre_scale)), self.device)
            return {"grad_scale_t": self.scale_t}
        ps = 1.0 if pre_scale_t is None else pre_scale_t.detach().to(self.device, torch.float64)
        norm = (self.sumsq[0] + self.sumsq[1]).sqrt() * float(pre_scale) * ps
        coef = torch.clamp(self.max_norm / (norm + 1e-6), max=1.0)  # (NaN stays NaN)
        self.norm_t.copy_(norm)
        self.coef_t.copy_(coef)
        self.scale_t.copy_(coef * ps)
        return {"grad_scale_t": self.scale_t}

    def opt_kwargs(self, opt) -> dict:
        """``grad_scale_t`` on the optimizer's device (a host-resident optimizer -- FSDP
        ``--cpu_offload`` -- gets a host copy, as ``GradScaler.opt_kwargs`` gives: that path
        synchronises anyway)."""
        dev = opt.param.device
        return {"grad_scale_t": self.scale_t if dev == self.device else self.scale_t.to(dev)}
