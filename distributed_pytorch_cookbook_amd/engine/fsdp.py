"""FSDP engine (recipe ``main-fsdp.py``): sharded store + sharded AdamW.

Reference: ``/root/reference/main-fsdp.py:42-202``.  Differences by design: generation
runs on every rank (the reference ran it on rank 0 only through an FSDP module, an
unmatched-collective hang, ``main-fsdp.py:184-188``); the final state dict is gathered
unit by unit to rank 0 only instead of materialising the full model on every GPU
(``main-fsdp.py:194``).
"""
from __future__ import annotations

import os

import torch

from ..ops.optim import FlatAdamW
from ..parallel import comm
from ..parallel.fsdp import FSDPStore
from ..utils.profiling import mark
from .base import Engine, GraphedStep

# A/B switch (bench/offload.py): the synchronous offload step (D2H, host AdamW, H2D in turn)
_OFFLOAD_SYNC = os.environ.get("DPC_OFFLOAD_SYNC", "0") == "1"


class FSDPEngine(Engine):
    name = "fsdp"
    collective_generate = True

    def __init__(self, model, device, lr: float, group=None, prefetch: int = 1,
                 reshard_after_forward: bool = True, cpu_offload: bool = False, compute_dtype=None,
                 reduce_dtype=torch.float32, grad_scaler: bool = False, graph: bool = False,
                 comm_kind: str | None = None, force_sharded: bool = False, max_grad_norm: float = 0.0,
                 weight_decay: float = 1e-2, betas=(0.9, 0.999), lr_schedule=None):
        self.device = torch.device(device)
        self.model = model
        self.dp_group = group
        self.dp_world = comm.world_size(group)
        self.dp_rank = comm.rank(group)
        self.is_logger = comm.rank() == 0
        self.store = FSDPStore(model, device, group=group, compute_dtype=compute_dtype,
                               prefetch=prefetch, reshard_after_forward=reshard_after_forward,
                               cpu_offload=cpu_offload, reduce_dtype=reduce_dtype, comm_kind=comm_kind,
                               force_sharded=force_sharded)
        st = self.store
        grad = st.grads_host if st.cpu_offload else st.grads
        okw = self._opt_kwargs(weight_decay, betas, lr_schedule)
        self.opt = FlatAdamW(st.master, grad, lr=lr, shadow=st.shadow, **okw)
        self.opt_rep = FlatAdamW(st.rep_master, st.rep_grads, lr=lr, **okw)  # replicated 1-D params
        self._make_scaler_clipper(grad_scaler, max_grad_norm)
        # The shards differ per rank: the skip flag and the shards' squared norm are reduced over
        # the group; the replicated 1-D gradients are all-reduced by finish_grads and counted
        # once.  The norm is taken on the device gradients (--cpu_offload: before they are
        # consumed on the host), over the whole of st.grads: its padding (units are padded to
        # W x 64 elements) and the slots of the 1-D parameters inside the units are zero --
        # zero_grad clears the buffer, the unit gradient buffers start as zeros, the kernels
        # write parameter views only and the 1-D gradients live in rep_grads -- so nothing is
        # excluded (tests/test_grad_clip_cpu.py checks the norm against the unsharded engine's)
        self.parts = [(self.opt, st.grads, False), (self.opt_rep, st.rep_grads, True)]
        self.reduce_flag, self.flag_group, self.norm_tp = True, group, st.tp
        # unit by unit: AdamW of the units already reduce-scattered on the compute stream while
        # the remaining reduce-scatters are still on the comm stream
        self.may_overlap = st.sharded and st.tp.active and not st.cpu_offload
        # HIP-graph "compile" of the whole sharded step (gathers, reduce-scatters, AdamW);
        # not with --cpu_offload, whose optimizer runs on the host
        self.graph = (graph and self.device.type == "cuda" and not st.cpu_offload
                      and (not st.sharded or st.tp.capturable()))
        self._stepper = GraphedStep(self, [self.opt, self.opt_rep])

    def _step_body(self, batch, targets):
        st = self.store
        st.zero_grad()
        with mark("fwd"):  # (unit all-gathers enqueued inside: "comm:all_gather")
            out = self.model(**batch, targets=targets)
        with mark("bwd"):  # (re-gathers and reduce-scatters enqueued inside)
            self._scaled(out.loss).backward()
        if st.cpu_offload:
            self._finish_and_step_on_host()
        else:
            self._finish_and_step()
        return out.loss.detach()

    def _finish_and_step_on_host(self):
        """--cpu_offload: the sharded optimizer lives on the host."""
        st = self.store
        with mark("comm:finish_grads"):
            st.finish_grads()
        with mark("optim"):
            if self.scaler is None and self.clipper is None and not _OFFLOAD_SYNC:
                # pipelined host AdamW: overlaps the next step's forward (FSDPStore.host_step)
                st.host_step(self.opt, grad_scale=1.0 / self.dp_world)
                self.opt_rep.step(grad_scale=1.0 / self.dp_world)
                return
            st.grads_host.copy_(st.grads, non_blocking=True)
            torch.cuda.current_stream().synchronize()  # grads_host D2H landed
            self._step_all()  # (the clipper reads the device gradients: ``parts``)

    def full_state_dict(self):
        return self.store.gather_full(self.store.master, dst_rank=0)

    def load_model_state(self, sd):
        self.store.wait_host()
        self.store.load_full(sd, self.store.master)
        self.store.refresh_shadow()

    def train_state(self):
        st = self.store
        m = st.gather_full(self.opt.exp_avg, dst_rank=0, rep_flat=self.opt_rep.exp_avg)
        v = st.gather_full(self.opt.exp_avg_sq, dst_rank=0, rep_flat=self.opt_rep.exp_avg_sq)
        s = self.opt.lr_schedule
        return {"optimizer": {"step": self.opt.step_count, "exp_avg": m, "exp_avg_sq": v,
                              "format": "canonical", "applied_step": self.opt.applied_steps,
                              "lr_schedule": s.params() if s is not None else None},
                **self._scaler_state()}

    def load_train_state(self, st):
        self.store.wait_host()
        o = st["optimizer"]
        for opt in (self.opt, self.opt_rep):
            opt.set_steps(o["step"], o.get("applied_step"))
        if isinstance(o.get("exp_avg"), dict):
            self.store.load_full(o["exp_avg"], self.opt.exp_avg, rep_flat=self.opt_rep.exp_avg)
            self.store.load_full(o["exp_avg_sq"], self.opt.exp_avg_sq, rep_flat=self.opt_rep.exp_avg_sq)
        self._load_scaler_state(st)

    @property
    def step_count(self):
        return self.opt.step_count
