"""Worker bodies of the gradient-clipping engine tests (gloo; importable by spawned children).

The tiny model of ``dist_workers.py`` has flat-gradient norms near 0.5 on its first steps, so
``MAX_NORM = 0.25`` clips on every step (each test asserts ``norm > 0.3`` first)."""
from __future__ import annotations

import torch

from dist_workers import LR, S, full_batch, make_model, shard

MAX_NORM = 0.25


def build(kind, world, max_grad_norm=MAX_NORM, grad_scaler=False, **kw):
    """(engine, dp, replica index of this rank) for an engine kind of the cross-engine tests."""
    from distributed_pytorch_cookbook_amd.engine.data_parallel import DataParallelEngine
    from distributed_pytorch_cookbook_amd.engine.fsdp import FSDPEngine
    from distributed_pytorch_cookbook_amd.engine.pipeline import PipelineEngine
    from distributed_pytorch_cookbook_amd.parallel import comm

    if max_grad_norm is not None:
        kw["max_grad_norm"] = max_grad_norm
    m = make_model()
    if kind in ("single", "ddp"):
        eng = DataParallelEngine(m, "cpu", lr=LR, bucket_mb=0.05, grad_scaler=grad_scaler, **kw)
        return eng, world, comm.rank()
    if kind == "fsdp":
        eng = FSDPEngine(m, "cpu", lr=LR, grad_scaler=grad_scaler, **kw)
        return eng, world, comm.rank()
    if kind in ("pipe-1f1b", "pipe-zb"):
        eng = PipelineEngine(m, "cpu", lr=LR, pp=world, dp=1, num_microbatches=4, schedule=kind[5:],
                             bucket_mb=0.01, seq_len=S, grad_scaler=grad_scaler, **kw)
        return eng, 1, 0
    if kind == "pipe_ddp":
        eng = PipelineEngine(m, "cpu", lr=LR, pp=2, dp=world // 2, num_microbatches=2, schedule="1f1b",
                             bucket_mb=0.01, seq_len=S, grad_scaler=grad_scaler, **kw)
        return eng, world // 2, eng.replica
    raise ValueError(kind)


def run_steps(eng, dp, idx, steps):
    """Per step: the reported norm and coefficient, the flat gradient the optimizer consumed
    (the buffer survives the step) and the first moment after it."""
    rec = []
    for s in range(steps):
        b, t = shard(*full_batch(step=s), idx, dp)
        eng.train_step(b, t)
        rec.append({"norm": float(eng.grad_norm), "coef": float(eng.clipper.coef_t),
                    "grads": eng.store.grads.clone(), "exp_avg": eng.opt.exp_avg.clone(),
                    "exp_avg_sq": eng.opt.exp_avg_sq.clone()})
    return rec


def single_clipped(steps=2, **kw):
    """The one-process clipped engine on the full batch: (state dict, per-step records)."""
    eng, dp, idx = build("single", 1, **kw)
    rec = run_steps(eng, dp, idx, steps)
    return {k: v.clone() for k, v in eng.full_state_dict().items()}, rec


def worker_clip(rank, world, out, kind, steps, grad_scaler):
    from distributed_pytorch_cookbook_amd.parallel import comm

    comm.init_dist(force_cpu=True)
    eng, dp, idx = build(kind, world, grad_scaler=grad_scaler)
    assert eng.clipper is not None
    rec = run_steps(eng, dp, idx, steps)
    if kind != "ddp":  # (sharded / staged buffers: only the norms are compared)
        rec = [{"norm": r["norm"], "coef": r["coef"]} for r in rec]
    sd = eng.full_state_dict()
    torch.save({"rec": rec, "dp": dp}, f"{out}.{rank}")
    if rank == 0:
        torch.save({k: v.clone() for k, v in sd.items()}, out)
