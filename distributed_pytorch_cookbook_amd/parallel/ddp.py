"""Data parallel: bucketed gradient all-reduce over RCCL, overlapped with backward.

Reference: ``DistributedDataParallel(sp_model, device_ids=[device_id])``
(``/root/reference/main-ddp.py:55``) -- rank-0 broadcast of the parameters in the
constructor, fp32 gradient buckets (1 MiB first, then 25 MiB) all-reduced by the C++
Reducer as autograd hooks fire, averaged by the world size.

MI355X-first design:
* gradients already live in ONE flat f32 buffer (``LocalStore``), unit by unit, so a
  bucket is a contiguous slice -- nothing is copied into or out of bucket storage;
* buckets are whole units taken in backward order (head, layer L-1, ..., layer 0,
  embeddings) up to ``bucket_mb``; the fused layer's backward calls ``post_backward``
  the moment its weight gradients are written, and the bucket's all-reduce is enqueued
  right then on RCCL's stream while the next layer's backward runs on the compute stream;
* sizes are chosen for xGMI (7 point-to-point links per GPU, ring collectives are
  per-link bound): fewer, larger buckets (default 128 MiB) keep RCCL at its bus
  bandwidth instead of paying per-call latency 25x per step;
* the 1/W average is folded into the AdamW kernel (``grad_scale``), so no extra pass;
* optional bf16 reduction (``reduce_dtype``) halves the bytes on the links;
* the all-reduces go through the engine's ``Transport`` (``parallel/transport.py``): by
  default the native C++ RCCL communicator on its own high-priority HIP stream, ordered with
  events (capturable into the step's HIP graph); torch's process group for ``--comm torch``
  and the gloo CPU tests.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from ..utils.profiling import mark
from .store import LocalStore
from .transport import Transport, make_transport


class DDPStore(LocalStore):
    def __init__(self, model, device, group=None, bucket_mb: float = 128.0,
                 reduce_dtype: torch.dtype = torch.float32, overlap: bool = True,
                 compute_dtype=None, units=None, broadcast_src: int | None = None,
                 transport: Transport | None = None, comm_kind: str | None = None):
        super().__init__(model, device, compute_dtype=compute_dtype, units=units)
        self.group = group
        self.tp = transport if transport is not None else make_transport(group, self.master.device, comm_kind)
        self.world = self.tp.size
        self.reduce_dtype = reduce_dtype
        self.overlap = overlap
        if self.tp.active:
            # the reference DDP constructor's rank-0 parameter broadcast (distributed.py:864)
            src = broadcast_src if broadcast_src is not None else 0
            with torch.no_grad():
                self.tp.broadcast(self.master, src=src)
            self.refresh_shadow()
        # buckets of whole units in backward order
        cap = int(bucket_mb * 2**20 / 4)
        self.buckets = []  # (lo, hi, [units])
        cur = []
        for u in reversed(self.units):
            sl = self.unit_slice(u)
            if cur and (sum(self.unit_slice(x).stop - self.unit_slice(x).start for x in cur)
                        + sl.stop - sl.start) > cap:
                self.buckets.append(cur)
                cur = []
            cur.append(u)
        if cur:
            self.buckets.append(cur)
        self.bucket_of = {}
        for bi, us in enumerate(self.buckets):
            for u in us:
                self.bucket_of[u] = bi
        self._ready = [0] * len(self.buckets)
        self._works = {}
        self._tmp = {}
        self.accum_steps = 1

    def _range(self, bi):
        us = self.buckets[bi]
        lo = min(self.unit_slice(u).start for u in us)
        hi = max(self.unit_slice(u).stop for u in us)
        return lo, hi

    def _launch(self, bi):
        if not self.tp.active or bi in self._works:
            return
        lo, hi = self._range(bi)
        g = self.grads[lo:hi]
        if self.reduce_dtype != torch.float32:
            t = g.to(self.reduce_dtype)
            self._tmp[bi] = t
            self._works[bi] = self.tp.all_reduce(t, async_op=True)
        else:
            self._works[bi] = self.tp.all_reduce(g, async_op=True)

    def post_backward(self, u):
        if not self.tp.active:
            return
        bi = self.bucket_of[u]
        self._ready[bi] += 1
        # with gradient accumulation (pipeline micro-batches) a unit's backward runs
        # accum_steps times; the bucket is final after the last one
        if self.overlap and self._ready[bi] >= self.accum_steps * len(self.buckets[bi]):
            self._launch(bi)  # (once: _launch skips a bucket already in flight)

    def reset_step_state(self):
        self._works.clear()
        self._tmp.clear()
        self._ready = [0] * len(self.buckets)

    def finish_grads(self, ready=None):
        """Complete the step's all-reduces: every bucket not launched yet (overlap off, or left
        partial) is enqueued, then bucket by bucket, in launch order, the current stream is
        ordered after its all-reduce (no host sync), a reduce-dtype temporary is copied back and
        ``ready(lo, hi)`` hears of the bucket's range -- AdamW of the buckets already reduced can
        run while the last ones (the embeddings, whose backward comes last) are still on the comm
        stream.  An inactive transport reports the whole buffer once, as ``LocalStore`` does."""
        if not self.tp.active:
            return super().finish_grads(ready)
        for bi in range(len(self.buckets)):
            self._launch(bi)
        for bi in range(len(self.buckets)):
            with mark("comm:wait_bucket"):
                self._works[bi].wait()
            lo, hi = self._range(bi)
            if bi in self._tmp:
                self.grads[lo:hi].copy_(self._tmp[bi])
            if ready is not None:
                ready(lo, hi)
        self.reset_step_state()

    @property
    def grad_scale(self) -> float:
        return 1.0 / self.world
