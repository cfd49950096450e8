"""Worker of the two-rank gradient-clipping test: both ranks run the real HIP kernels on cuda:0
and talk over the peer-access transport (``--comm ipc``), the step captured into a HIP graph.
Importable by spawned children."""
from __future__ import annotations

import time

import torch

from dist_workers_gpu import LR, S, _init, full_batch, make_model, shard

STEP_TIMEOUT = 60.0  # seconds a single step may take before the worker gives up


def _finish_step(tp, what):
    """Wait for the step's device work under its own time limit (polling an event: a step that
    ends returns at once), then ask the transport whether a bounded wait gave up."""
    ev = torch.cuda.Event()
    ev.record()
    limit = time.monotonic() + STEP_TIMEOUT
    while not ev.query():
        if time.monotonic() > limit:
            raise RuntimeError(f"{what}: not finished after {STEP_TIMEOUT} s")
        time.sleep(0.002)
    tp.nc.check()


def ipc_clip_worker(rank, world, out, kind, steps, max_norm):
    info = _init()
    assert info.device.type == "cuda"
    from distributed_pytorch_cookbook_amd.engine.fsdp import FSDPEngine
    from distributed_pytorch_cookbook_amd.engine.pipeline import PipelineEngine

    m = make_model()
    if kind == "fsdp":
        eng = FSDPEngine(m, "cuda", lr=LR, prefetch=1, graph=True, comm_kind="ipc", max_grad_norm=max_norm)
        tp, dp, rep = eng.store.tp, world, rank
    else:  # "pipe-<schedule>"
        eng = PipelineEngine(m, "cuda", lr=LR, pp=world, dp=1, num_microbatches=4, schedule=kind.split("-")[1],
                             bucket_mb=0.2, seq_len=S - 1, graph=True, comm_kind="ipc", max_grad_norm=max_norm)
        tp, dp, rep = eng.pp_tp, 1, 0
    assert tp.kind == "ipc", tp.kind
    norms = []
    for s in range(steps):  # (the first failure raises: nothing more is started on the device)
        eng.train_step(*shard(*full_batch(step=s), rep, dp))
        _finish_step(tp, f"{kind} step {s} on rank {rank}")
        norms.append(eng.grad_norm.detach().cpu().clone())
    assert eng._stepper.graph is not None, "the two-rank step was not captured"
    torch.save({"norms": torch.stack(norms)}, f"{out}.{rank}")
