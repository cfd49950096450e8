"""Single-device and data-parallel engines (recipes ``main-single.py`` / ``main-ddp.py``).

Reference step (``/root/reference/main-single.py:85-101``, ``main-ddp.py:110-126``):
zero_grad -> autocast forward -> cross-entropy -> GradScaler backward -> step.  Here:
memset of the flat gradient buffer -> fused forward with the loss inside the head ->
backward (DDP bucket all-reduces fire from inside it) -> wait for the last buckets ->
one fused AdamW launch (which also folds in the 1/W average and refreshes the bf16
weights).  No GradScaler: bf16 needs none.  With ``graph=True`` the
whole single-GPU step is captured once into a HIP graph and replayed (the cookbook's
meaning of "compile", replacing torch.compile/Inductor).
"""
from __future__ import annotations

import torch

from ..ops.optim import FlatAdamW
from ..parallel import comm
from ..parallel.ddp import DDPStore
from ..parallel.store import LocalStore
from ..utils.profiling import mark
from .base import Engine, GraphedStep


class DataParallelEngine(Engine):
    name = "ddp"

    def __init__(self, model, device, lr: float, group=None, bucket_mb: float = 128.0,
                 reduce_dtype=torch.float32, overlap: bool = True, compute_dtype=None,
                 graph: bool = False, comm_kind: str | None = None, grad_scaler: bool = False,
                 force_ddp_store: bool = False, max_grad_norm: float = 0.0,
                 weight_decay: float = 1e-2, betas=(0.9, 0.999), lr_schedule=None):
        self.device = torch.device(device)
        self.model = model
        self.dp_group = group
        self.dp_world = comm.world_size(group)
        self.dp_rank = comm.rank(group)
        self.is_logger = comm.rank() == 0
        if self.dp_world > 1 or force_ddp_store:
            # (force_ddp_store: the bucketed store and its transport at one rank -- tests)
            self.store = DDPStore(model, device, group=group, bucket_mb=bucket_mb,
                                  reduce_dtype=reduce_dtype, overlap=overlap, compute_dtype=compute_dtype,
                                  comm_kind=comm_kind)
        else:
            self.store = LocalStore(model, device, compute_dtype=compute_dtype)
        self.opt = FlatAdamW(self.store.master, self.store.grads, lr=lr, shadow=self.store.shadow,
                             **self._opt_kwargs(weight_decay, betas, lr_schedule))
        self._make_scaler_clipper(grad_scaler, max_grad_norm)
        # all-reduced gradients are identical on every rank, so are the skip flag and the norm
        # (its sum has a fixed order: ops/clip.py) -- no collective for either
        self.parts = [(self.opt, self.store.grads, True)]
        tp = getattr(self.store, "tp", None)
        self.may_overlap = tp is not None and tp.active and self.store.master.is_cuda
        # HIP-graph "compile": at one rank, or across ranks when the gradient all-reduces ride
        # the capturable native RCCL transport
        self.graph = graph and self.device.type == "cuda" and (self.dp_world == 1 or (tp is not None and tp.capturable()))
        self._stepper = GraphedStep(self, [self.opt])

    # ------------------------------------------------------------------ training
    def _step_body(self, batch, targets):
        self.store.zero_grad()
        with mark("fwd"):
            out = self.model(**batch, targets=targets)
        with mark("bwd"):  # (the DDP bucket all-reduces are enqueued from inside it: "comm:*")
            self._scaled(out.loss).backward()
        self._finish_and_step()
        return out.loss.detach()

    # ------------------------------------------------------------------ state
    def full_state_dict(self):
        return self.store.state_dict()

    def load_model_state(self, sd):
        self.store.load_state_dict(sd)

    def train_state(self):
        return {"optimizer": {k: (v.detach().cpu() if torch.is_tensor(v) else v)
                              for k, v in self.opt.state_dict().items()}, **self._scaler_state()}

    def load_train_state(self, st):
        self.opt.load_state_dict({k: (v.to(self.device) if torch.is_tensor(v) else v)
                                  for k, v in st["optimizer"].items()})
        self._load_scaler_state(st)

    @property
    def step_count(self):
        return self.opt.step_count
