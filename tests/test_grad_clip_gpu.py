"""Global-norm gradient clipping on the GPU: the sum-of-squares and coefficient kernels
(ops/csrc/misc.hip, ops/clip.py), the three engines with the step captured into a HIP graph, and
two ranks sharing the GPU over the peer-access transport."""
import contextlib
import math

import pytest
import torch

from kernel_checks import assert_guards_intact, guarded

from distributed_pytorch_cookbook_amd.engine.data_parallel import DataParallelEngine
from distributed_pytorch_cookbook_amd.engine.fsdp import FSDPEngine
from distributed_pytorch_cookbook_amd.engine.pipeline import PipelineEngine
from distributed_pytorch_cookbook_amd.ops import _lib
from distributed_pytorch_cookbook_amd.ops.clip import GradClipper

pytestmark = pytest.mark.gpu

TRIP = _lib.SUMSQ_TRIP  # elements one trip of the whole (capped) grid covers


def guarded_clipper(max_norm=1.0):
    """A clipper whose accumulators and partials sit between guard bands."""
    cl = GradClipper(max_norm, "cuda")
    cl.sumsq = guarded(2, torch.float32, "cuda", fill=0.0)
    cl.partials = guarded(_lib.SUMSQ_MAX_BLOCKS, torch.float32, "cuda", fill=float("nan"))
    return cl


# ---------------------------------------------------------------- sum of squares: edges
# 2 * TRIP + 7: a wrapped grid-stride loop, a vector tail and a scalar tail.  Error bound: at most a
# few serial adds per accumulator at these sizes plus a tree of about 20 levels -- below 3e-6 in
# f32; 1e-5 leaves room for the square root.
@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("n", [0, 1, 3, 4, 255, 1025, 4099, 2 * TRIP + 7])
def test_sumsq_edges(n, offset):
    g = torch.Generator(device="cuda").manual_seed(n + int(offset))
    x = guarded(n, torch.float32, "cuda", offset=offset, fill=torch.randn(n, device="cuda", generator=g))
    assert n == 0 or x.data_ptr() % 16 == (4 if offset else 0)
    before = x.view(torch.int32).clone()
    cl = guarded_clipper()
    side = torch.cuda.Stream() if n in (4099, 2 * TRIP + 7) else None  # (two cases on a side stream)
    if side is not None:
        side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
        cl.begin()
        cl.add(x, replicated=False)
        first = cl.sumsq.clone()
        cl.begin()
        cl.add(x, replicated=False)
        second = cl.sumsq.clone()
        cl.add(x, replicated=True)  # the other accumulator; the first one stays
        both = cl.sumsq.clone()
    if side is not None:
        torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want = x.double().pow(2).sum().item()
    got = first[0].item()
    print(f"n={n} offset={offset}: sumsq {got!r} f64 {want!r}")
    assert first[1].item() == 0.0
    assert abs(math.sqrt(got) - math.sqrt(want)) <= 1e-5 * math.sqrt(want)
    if n == 0:
        assert got == 0.0
    assert torch.equal(first.view(torch.int32), second.view(torch.int32)), "two launches differ"
    assert both[0].item() == got and both[1].item() == got
    assert torch.equal(x.view(torch.int32), before), "the input was written"
    assert_guards_intact(x, cl.sumsq, cl.partials, what=f"sumsq n={n}")
    # every block of the launch stored its partial (0 for a block without elements); the slots
    # beyond the grid keep their fill
    head = min(n, 3 if offset else 0)  # elements before the first 16-byte boundary
    blocks = min(_lib.SUMSQ_MAX_BLOCKS, max(1, -(-((n - head) // 4) // (TRIP // 4 // _lib.SUMSQ_MAX_BLOCKS))))
    assert torch.isfinite(cl.partials[:blocks]).all() and torch.isnan(cl.partials[blocks:]).all()
    if n == 2 * TRIP + 7:
        assert blocks == _lib.SUMSQ_MAX_BLOCKS


@pytest.mark.parametrize("where", [7, -5])
def test_sumsq_infinity_stays_infinity(where):
    """An infinite element gives an infinite sum, not NaN (torch: norm inf, coef 0) -- also in the
    last vector, which the lanes past the end load again and must drop, not multiply by 0."""
    x = torch.randn(4099, device="cuda")
    x[where] = float("inf")
    cl = GradClipper(1.0, "cuda")
    cl.begin()
    cl.add(x, replicated=False)
    cl.finish(1.0)
    assert cl.sumsq[0].item() == float("inf") and cl.norm_t.item() == float("inf") and cl.coef_t.item() == 0.0


def test_sumsq_rejects_what_it_cannot_sum():
    cl = GradClipper(1.0, "cuda")
    with pytest.raises(TypeError):
        cl.add(torch.ones(8, device="cuda", dtype=torch.bfloat16), replicated=False)
    with pytest.raises(TypeError):
        cl.add(torch.ones(8, 2, device="cuda")[:, 0], replicated=False)


# ---------------------------------------------------------------- coefficient
def torch_coef(norm, max_norm):
    return torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (norm + 1e-6), max=1.0)


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("vec,max_norm", [([3.0, 4.0], 1.0), ([3.0, 4.0], 10.0), ([0.0, 0.0], 1.0),
                                          ([3.0, float("nan")], 1.0), ([float("inf"), 4.0], 1.0)])
def test_clip_coef(vec, max_norm, scaled):
    """Above max_norm, below it, exactly zero (coef 1), a NaN (coef NaN, as torch's clamp gives) and
    an infinity (coef 0, as torch gives); with ``scaled`` the buffer holds 1024 x the true
    gradient and the device factor 1/1024 undoes it."""
    cl = guarded_clipper(max_norm)
    v = torch.tensor(vec, device="cuda")
    inv = torch.tensor(1.0 / 1024.0, device="cuda") if scaled else None
    cl.begin()
    cl.add(v[:1] * (1024.0 if scaled else 1.0), replicated=False)
    cl.add(v[1:] * (1024.0 if scaled else 1.0), replicated=True)
    kw = cl.finish(0.5, inv)
    torch.cuda.synchronize()
    norm = (v.double().norm() * 0.5).float().cpu()
    want = torch_coef(norm, max_norm)
    got_norm, got, scale = cl.norm_t.cpu(), cl.coef_t.cpu(), kw["grad_scale_t"].cpu()
    print(f"{vec} max {max_norm} scaled {scaled}: norm {got_norm.item()!r} coef {got.item()!r} torch {want.item()!r}")
    assert_guards_intact(cl.sumsq, cl.partials)
    if torch.isnan(norm):
        assert torch.isnan(got_norm) and torch.isnan(got) and torch.isnan(scale)
        return
    assert got_norm.item() == norm.item() or abs(got_norm.item() - norm.item()) <= 1e-6 * norm.item()
    assert abs(got.item() - want.item()) <= 1e-6 * want.item()
    assert scale.item() == got.item() * (1.0 / 1024.0 if scaled else 1.0)
    if vec == [0.0, 0.0] or max_norm == 10.0:
        assert got.item() == 1.0


# ---------------------------------------------------------------- engines, captured step
from test_engines_gpu import batch, make  # noqa: E402  (model and batches of the engine tests)


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.fixture(scope="module")
def n0():
    """Gradient norm of the first step of an unclipped engine."""
    eng = DataParallelEngine(make(), "cuda", lr=1e-3)
    eng.train_step(*batch(0))
    return eng.store.grads.double().norm().item()


def build(kind, max_norm):
    if kind == "ddp-eager":
        return DataParallelEngine(make(), "cuda", lr=1e-3, graph=False, max_grad_norm=max_norm)
    if kind == "ddp-graph":
        return DataParallelEngine(make(), "cuda", lr=1e-3, graph=True, max_grad_norm=max_norm)
    if kind == "fsdp-graph":
        return FSDPEngine(make(), "cuda", lr=1e-3, graph=True, max_grad_norm=max_norm)
    if kind == "fsdp-offload":  # host-resident optimizer: the norm comes from the device gradients
        return FSDPEngine(make(), "cuda", lr=1e-3, cpu_offload=True, max_grad_norm=max_norm)
    return PipelineEngine(make(), "cuda", lr=1e-3, pp=1, dp=1, num_microbatches=4, seq_len=127, graph=True,
                          max_grad_norm=max_norm)


@pytest.mark.parametrize("kind", ["ddp-eager", "ddp-graph", "fsdp-graph", "pipe-graph", "fsdp-offload"])
def test_engine_clips_every_step(n0, kind):
    """Four steps (eager, capture + replay, two replays).  The gradient buffer still holds the
    step's gradient afterwards: the reported norm is its norm, clipping is active, and the first
    moment follows m = 0.9 m + 0.1 coef_s g_s with the coefficient of THAT step -- a coefficient
    frozen at capture time fails on the replays."""
    max_norm = n0 / 4
    eng = build(kind, max_norm)
    pairs = [(eng.opt, eng.store.grads)]
    if kind.startswith("fsdp"):
        pairs.append((eng.opt_rep, eng.store.rep_grads))
    ms = [torch.zeros_like(g, dtype=torch.float64) for _, g in pairs]
    for s in range(4):
        eng.train_step(*batch(s))
        torch.cuda.synchronize()
        gs = [g.double() for _, g in pairs]
        norm = math.sqrt(sum(g.pow(2).sum().item() for g in gs)) / eng.dp_world
        got = float(eng.grad_norm)
        print(f"{kind} step {s}: grad_norm {got!r} buffer norm {norm!r} max_norm {max_norm!r}")
        assert abs(got - norm) <= 1e-5 * norm
        assert got > 2 * max_norm
        coef = max_norm / (got + 1e-6)
        assert abs(float(eng.clipper.coef_t) - coef) <= 1e-5 * coef
        for i, (opt, _) in enumerate(pairs):
            ms[i] = 0.9 * ms[i] + 0.1 * coef * gs[i]
            assert rel(opt.exp_avg.cpu(), ms[i].cpu()) <= 1e-5, (s, i)
    if kind.endswith("-graph"):
        assert eng._stepper.graph is not None, "the clipped step was not captured"
    assert eng.step_count == 4


# ---------------------------------------------------------------- two ranks share the GPU (--comm ipc)
@pytest.fixture(scope="module")
def ipc_ref():
    """One-process clipped reference on the workers' model: (max_norm, norms of 3 steps)."""
    import dist_workers_gpu as w

    eng = DataParallelEngine(w.make_model(), "cuda", lr=w.LR)
    eng.train_step(*w.full_batch(step=0))
    max_norm = eng.store.grads.double().norm().item() / 4
    eng = DataParallelEngine(w.make_model(), "cuda", lr=w.LR, max_grad_norm=max_norm)
    norms = []
    for s in range(3):
        eng.train_step(*w.full_batch(step=s))
        norms.append(float(eng.grad_norm))
    return max_norm, norms


@pytest.mark.parametrize("kind", ["fsdp", "pipe-1f1b"])
def test_ipc_two_ranks_report_one_norm(tmp_path, ipc_ref, kind):
    """FSDP shards (+ replicated 1-D parameters) and two pipeline stages, the squared norm
    all-reduced inside the captured step: both ranks report the same norm bit for bit, and it is
    the one-process engine's (to 1e-3: the backward's atomics reorder sums run to run)."""
    from clip_workers_gpu import ipc_clip_worker
    from dist_helpers import run_workers

    max_norm, want = ipc_ref
    out = tmp_path / f"{kind}.pt"
    run_workers(ipc_clip_worker, 2, str(out), kind, 3, max_norm, timeout=110)
    a, b = (torch.load(f"{out}.{r}", weights_only=True)["norms"] for r in range(2))
    print(f"{kind}: rank norms {a.tolist()} / {b.tolist()} reference {want}")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (a, b)
    for s in range(3):
        assert want[s] > 2 * max_norm
        assert abs(a[s].item() - want[s]) <= 1e-3 * want[s], (s, a[s].item(), want[s])
