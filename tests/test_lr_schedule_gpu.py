"""Learning-rate schedule on the GPU: the rate ``adamw_kernel`` computes from the step counter
(ops/csrc/misc.hip: adamw_sched_lr), the three engines with the step captured into a HIP graph --
every replay a different rate -- and two ranks sharing the GPU over the peer-access transport."""
import math

import pytest
import torch

from kernel_checks import assert_elem_bound, assert_guards_intact, guarded

from distributed_pytorch_cookbook_amd.engine.data_parallel import DataParallelEngine
from distributed_pytorch_cookbook_amd.engine.fsdp import FSDPEngine
from distributed_pytorch_cookbook_amd.engine.pipeline import PipelineEngine
from distributed_pytorch_cookbook_amd.ops.optim import FlatAdamW
from distributed_pytorch_cookbook_amd.ops.schedule import LRSchedule

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, BF = torch.float32, torch.bfloat16
KINDS = ["constant", "linear", "cosine"]


def bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


# ---------------------------------------------------------------- the rate the kernel used
@pytest.mark.parametrize("mode", ["host_t", "device_t", "skipped_step"])
@pytest.mark.parametrize("kind", KINDS)
def test_kernel_rate_step_by_step(kind, mode):
    """p = 1, g = 0, weight_decay = 1: the moments stay 0 and p_new = p_old (1 - lr), so
    lr = 1 - p_new / p_old (in f64) is the rate the kernel used.  n = 1028: 257 float4 groups,
    two workgroups and a tail.  Bound 2^-21: one rounding of the product (2^-24 relative), one of
    1 - lr (2^-25) and a few ulp of the f32 cos / divide in the rate (<= 8 x 2^-24 x 0.25);
    adjacent steps of these schedules differ by more than 1e-2.
    host_t: t is a kernel argument, the step issued as two sub-range launches; device_t: t is read
    from the device counter (what a captured step does); skipped_step: the loss scaler's flag skips
    attempt 5 -- p unchanged, and the next rate is lr_at(applied), not lr_at(attempted)."""
    n = 1028
    s = LRSchedule(kind, 0.25, 3, 9, 0.1)
    p = guarded(n, F32, dev, fill=1.0)
    g = guarded(n, F32, dev, fill=0.0)
    sh = guarded(n, BF, dev, fill=7.0)
    opt = FlatAdamW(p, g, weight_decay=1.0, shadow=sh, lr_schedule=s)
    opt.exp_avg = guarded(n, F32, dev, fill=0.0)
    opt.exp_avg_sq = guarded(n, F32, dev, fill=0.0)
    if mode == "device_t":
        opt.device_step = True
    applied, attempt = 0, 0
    while applied < 11:
        attempt += 1
        skip = mode == "skipped_step" and attempt == 5
        skip_t = torch.full((), 1.0 if skip else 0.0, device=dev) if mode == "skipped_step" else None
        before = p.clone()
        opt.begin_step(skip_t)
        if mode == "host_t":
            opt.update(0, 516, skip_t=skip_t)
            opt.update(516, n, skip_t=skip_t)
        else:
            opt.update(0, n, skip_t=skip_t)
        if skip:
            assert torch.equal(bits(p), bits(before))
            continue
        applied += 1
        got = 1.0 - p.double() / before.double()
        want = s.lr_at(applied)
        err = (got - want).abs().max().item()
        print(f"{kind} {mode} t={applied}: lr_at {want!r} recovered {got[0].item()!r} worst |diff| {err:.3e}")
        assert err <= 2.0 ** -21, (applied, err)
        assert (got.max() - got.min()).item() == 0.0  # one rate for every element and launch
        assert opt.last_lr == want and opt.applied_steps == applied
    assert attempt == (12 if mode == "skipped_step" else 11) and opt.step_count == attempt
    assert torch.count_nonzero(opt.exp_avg) == 0 and torch.count_nonzero(opt.exp_avg_sq) == 0
    assert torch.equal(bits(sh), bits(p.bfloat16()))
    assert_guards_intact(p, g, sh, opt.exp_avg, opt.exp_avg_sq)
    for a, b in ((1, 2), (2, 3)) + (((3, 4), (5, 6), (8, 9)) if kind != "constant" else ()):
        assert abs(s.lr_at(a) - s.lr_at(b)) > 1e-2


def test_reloaded_optimizer_continues_at_the_applied_count():
    """With the loss scaler's skip flag the device counter is only ever added to: an optimizer
    restored from a checkpoint (5 attempts, 4 applied) runs its next update at lr_at(5), not at
    lr_at(1) from a counter left at zero."""
    n = 1028
    s = LRSchedule("linear", 0.25, 3, 9, 0.1)
    p, g = torch.ones(n, device=dev), torch.zeros(n, device=dev)
    opt = FlatAdamW(p, g, weight_decay=1.0, lr_schedule=s)
    for attempt in range(1, 6):
        skip_t = torch.full((), 1.0 if attempt == 2 else 0.0, device=dev)
        opt.begin_step(skip_t)
        opt.update(0, n, skip_t=skip_t)
    sd = opt.state_dict()
    assert (sd["step"], sd["applied_step"]) == (5, 4)
    p2 = p.clone()
    new = FlatAdamW(p2, torch.zeros(n, device=dev), weight_decay=1.0, lr_schedule=s)
    new.load_state_dict(sd)
    assert new.step_count == 5 and new.applied_steps == 4 and new.last_lr == s.lr_at(4)
    skip_t = torch.zeros((), device=dev)
    new.begin_step(skip_t)
    new.update(0, n, skip_t=skip_t)
    got = 1.0 - p2.double() / p.double()
    assert (got - s.lr_at(5)).abs().max().item() <= 2.0 ** -21
    assert new.applied_steps == 5 and abs(s.lr_at(5) - s.lr_at(1)) > 1e-2


# ---------------------------------------------------------------- full AdamW with a schedule
def _adam64(p, m, v, g, t, lr, b1, b2, eps, wd):
    p = p * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1 - b2 ** t) + eps
    return p - (lr / (1 - b1 ** t)) * m / denom, m, v


@pytest.mark.parametrize("variant", ["plain", "device_step"])
@pytest.mark.parametrize("n", [4, 2052, 4096 + 12])
def test_scheduled_adamw_subrange_edges(n, variant):
    """The setup and bound of test_kernel_edges_gpu.py::test_adamw_subrange_edges (|p| >= 0.5,
    three steps with new gradients, updates on sub-ranges, 4 ulp of |p64|), cosine with W = 1,
    T = 3; the f64 reference uses lr_at(t).  device_step: the second step is skipped on the device,
    so the third runs at lr_at(2)."""
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.999, 1e-8, 1e-2
    s = LRSchedule("cosine", lr, 1, 3, 0.1)
    ranges = [r for r in ((0, n), (4, n - 4), (1028, 1032)) if 0 <= r[0] < r[1] <= n]
    for lo, hi in ranges:
        torch.manual_seed(n + lo)
        p0 = torch.randn(n, device=dev)
        p0 = torch.where(p0 >= 0, p0 + 0.5, p0 - 0.5)
        p = guarded(n, F32, dev, fill=p0)
        g = guarded(n, F32, dev, fill=0.0)
        sh = guarded(n, BF, dev, fill=7.0)
        opt = FlatAdamW(p, g, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, shadow=sh, lr_schedule=s)
        opt.exp_avg = guarded(n, F32, dev, fill=0.0)
        opt.exp_avg_sq = guarded(n, F32, dev, fill=0.0)
        p64 = p0.double()
        m64, v64 = torch.zeros_like(p64), torch.zeros_like(p64)
        t_dev = 0
        for step in range(3):
            g.normal_()
            skip_t = None if variant == "plain" else torch.full((), 1.0 if step == 1 else 0.0, device=dev)
            opt.begin_step(skip_t)
            opt.update(lo, hi, skip_t=skip_t)
            if not (variant == "device_step" and step == 1):
                t_dev += 1
                pn, mn, vn = _adam64(p64, m64, v64, g.double(), t_dev, s.lr_at(t_dev), b1, b2, eps, wd)
                p64[lo:hi], m64[lo:hi], v64[lo:hi] = pn[lo:hi], mn[lo:hi], vn[lo:hi]
        assert opt.applied_steps == t_dev == (3 if variant == "plain" else 2)
        inside = torch.zeros(n, dtype=torch.bool, device=dev)
        inside[lo:hi] = True
        assert_elem_bound(p[inside], p64[inside], 4 * 2.0 ** -23 * p64[inside].abs(), what=f"param [{lo},{hi})",
                          family="scheduled adamw (fraction of 4 ulp)")
        assert torch.equal(bits(sh[inside]), bits(p[inside].bfloat16()))
        assert (opt.exp_avg[inside] != 0).all() and (opt.exp_avg_sq[inside] != 0).all()
        out = ~inside
        assert torch.equal(p[out], p0[out])
        assert torch.count_nonzero(opt.exp_avg[out]) == 0 and torch.count_nonzero(opt.exp_avg_sq[out]) == 0
        assert torch.equal(sh[out].float(), torch.full_like(sh[out], 7.0).float())
        assert_guards_intact(p, g, sh, opt.exp_avg, opt.exp_avg_sq)


# ---------------------------------------------------------------- kind 0 is today's kernel
@pytest.mark.parametrize("device_step", [False, True])
def test_constant_schedule_is_bit_identical_to_none(device_step):
    n = 2052
    torch.manual_seed(1)
    p0 = torch.randn(n, device=dev)
    grads = [torch.randn(n, device=dev) for _ in range(3)]
    res = []
    for s in (None, LRSchedule("constant", 1e-3, 0, 0, 0.1)):
        p, g = p0.clone(), torch.zeros(n, device=dev)
        opt = FlatAdamW(p, g, lr=1e-3, shadow=torch.zeros(n, device=dev, dtype=BF))
        opt.set_lr_schedule(s)
        opt.device_step = device_step
        for gr in grads:
            g.copy_(gr)
            opt.step()
        res.append((p, opt.exp_avg, opt.exp_avg_sq, opt.shadow))
    assert not torch.equal(res[0][0], p0)
    for a, b in zip(*res):
        assert torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------- engines, every step a different rate
from test_engines_gpu import batch, make  # noqa: E402  (model and batches of the engine tests)

SCHED = LRSchedule("cosine", 1e-3, 2, 5, 0.1)


def build(kind):  # (as test_grad_clip_gpu.py::build)
    kw = {"lr": 1e-3, "lr_schedule": SCHED}
    if kind == "ddp-eager":
        return DataParallelEngine(make(), "cuda", graph=False, **kw)
    if kind == "ddp-graph":
        return DataParallelEngine(make(), "cuda", graph=True, **kw)
    if kind == "fsdp-graph":
        return FSDPEngine(make(), "cuda", graph=True, **kw)
    if kind == "fsdp-offload":  # host-resident optimizer: runtime.adamw_host with lr_at(step)
        return FSDPEngine(make(), "cuda", cpu_offload=True, **kw)
    return PipelineEngine(make(), "cuda", pp=1, dp=1, num_microbatches=4, seq_len=127, graph=True, **kw)


def f32(x):
    return torch.tensor(x, dtype=F32).double().item()


def adam64_as_handed(opt, p, m, v, g, t, lr, device_t):
    """One AdamW step in f64 on the numbers the update is handed: the f32 snapshot of parameter
    and moments, the f32 gradient, beta / eps / weight_decay as the f32 values the kernel (and the
    native host pass) receive -- 1 - 0.999f is 1.29e-5 below 0.001 -- and the bias corrections
    from the device counter (``device_t``: powers of the f32 betas) or as the host forms them
    (from the decimal betas, rounded to f32).  The rate is lr_at(t) in f64."""
    b1, b2, eps, wd = f32(opt.betas[0]), f32(opt.betas[1]), f32(opt.eps), f32(opt.weight_decay)
    if device_t:
        bc1, bc2s = 1 - b1 ** t, math.sqrt(1 - b2 ** t)
    else:
        bc1, bc2s = f32(1.0 - opt.betas[0] ** t), f32(math.sqrt(1.0 - opt.betas[1] ** t))
    p = p * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    return p - (lr / bc1) * m / (v.sqrt() / bc2s + eps)


ENGINES = ["ddp-eager", "ddp-graph", "fsdp-graph", "pipe-graph", "fsdp-offload"]
RATES = [SCHED.lr_at(t) for t in range(1, 6)]
_runs = {}


def run_engine(kind):
    """Five steps (eager, capture + replay, three replays) of a scheduled engine, once per kind.
    Before each step parameter and moments of every optimizer are snapshot; after it the gradient
    buffer still holds the step's gradient; one f64 AdamW step from those with lr_at(s + 1) is the
    reference.  Per step and optimizer: the elements over the bound
    4 x 2^-23 |p64| + 2^-20 |p64 - p_before|, the worst error as a multiple of it, whether a rate
    frozen at capture time (lr_at(2)) would be far outside it, and the rate the step used --
    p_new = p_before - lr u is linear in lr, so lr_eff = <p_before - p_new, u> / <u, u>."""
    if kind in _runs:
        return _runs[kind]
    eng = build(kind)
    opts = [o for o, _, _ in eng.parts]
    assert len(opts) == (2 if kind.startswith("fsdp") else 1) and all(o.lr_schedule == SCHED for o in opts)
    wait = getattr(eng.store, "wait_host", lambda: None)
    recs = []
    for s in range(5):
        wait()
        torch.cuda.synchronize()
        snap = [(o.param.double(), o.exp_avg.double(), o.exp_avg_sq.double()) for o in opts]
        eng.train_step(*batch(s))
        wait()
        torch.cuda.synchronize()
        lr = RATES[s]
        assert abs(eng.lr - lr) <= 2.0 ** -23 * lr and eng.lr == opts[0].last_lr
        for i, (o, (p0, m0, v0)) in enumerate(zip(opts, snap)):
            g = o.grad.double() / eng.dp_world
            device_t = o.device_step and o.param.is_cuda
            p64 = adam64_as_handed(o, p0, m0, v0, g, s + 1, lr, device_t)
            assert (p64 - p0).abs().max() > 0.1 * lr  # the step moved something
            bound = 4 * 2.0 ** -23 * p64.abs() + 2.0 ** -20 * (p64 - p0).abs()
            ratio = (o.param.double() - p64).abs() / bound.clamp_min(1e-300)
            u = (p0 - p64) / lr
            lr_eff = ((p0 - o.param.double()) @ u / (u @ u)).item()
            frozen = adam64_as_handed(o, p0, m0, v0, g, s + 1, RATES[1], device_t)
            rec = {"step": s, "opt": i, "device_t": device_t, "worst": ratio.max().item(),
                   "over": int((ratio > 1).sum()), "numel": ratio.numel(), "lr": lr, "lr_eff": lr_eff,
                   "frozen_outside": ((frozen - p64).abs() > 100 * bound).float().mean().item()}
            print(f"{kind}: {rec}")
            recs.append(rec)
    assert eng.step_count == 5
    if kind.endswith("-graph"):
        assert eng._stepper.graph is not None, "the scheduled step was not captured"
        with pytest.raises(RuntimeError, match="captured"):
            eng.set_lr_schedule(None)
    _runs[kind] = recs
    return recs


@pytest.mark.parametrize("kind", ENGINES)
def test_engine_applies_a_new_rate_every_step(kind):
    """The rate every step used, recovered from the parameters (``run_engine``), is lr_at(s + 1)
    to 2^-15 relative; the five rates differ by 22 % or more, and a rate frozen at capture time
    would leave more than half of the elements over 100 x the element bound of the test below.
    2^-15 allows what an f32 bias correction 1 - b2^t can lose at t >= 2 (half an ulp of b2^t,
    2^-25, over 1.998e-3, doubled for a power one ulp off, halved by the square root: 1.5e-5 on
    the size of the update) plus about 1e-6 for the f32 operations of the update."""
    assert min(abs(a - b) / max(a, b) for i, a in enumerate(RATES) for b in RATES[i + 1:]) >= 0.22
    for r in run_engine(kind):
        assert abs(r["lr_eff"] - r["lr"]) <= 2.0 ** -15 * r["lr"], r
        if r["step"] >= 2:
            assert r["frozen_outside"] > 0.5, r


@pytest.mark.parametrize("kind", ENGINES)
def test_engine_step_within_the_element_bound(kind):
    """Every element of every step within 4 x 2^-23 |p64| + 2^-20 |p64 - p_before| of the f64 step
    (the project's AdamW bound plus 2^-20 of the update for its roughly 8 f32 operations).

    The f64 reference takes beta, eps and weight_decay as the f32 values the update is handed
    (``adam64_as_handed``).  The bound leaves no room for an f32 ``1 - beta2^t`` from the device
    counter nor for a first moment that keeps the rounding error of its cancelling terms: the
    kernel and the host pass avoid both (docs/LR_SCHEDULE.md, Accuracy)."""
    bad = [r for r in run_engine(kind) if r["over"]]
    assert not bad, bad


# ---------------------------------------------------------------- two ranks share the GPU (--comm ipc)
def close(sd_a, sd_b, tol=5e-2, lr=1e-3, steps=3):  # (test_ipc_gpu.py's comparison)
    assert list(sd_a) == list(sd_b)
    bad = {}
    for k in sd_b:
        scale = max(sd_b[k].norm().item(), lr * steps * sd_b[k].numel() ** 0.5)
        e = (sd_a[k] - sd_b[k]).norm().item() / scale
        if e >= tol:
            bad[k] = round(e, 4)
    assert not bad, bad


def test_ipc_two_ranks_follow_one_schedule(tmp_path):
    """FSDP over the peer-access transport, the step captured on both ranks: both report
    lr_at(1..4), and the gathered state is the one-rank scheduled run's."""
    import dist_workers_gpu as w
    from dist_helpers import run_workers
    from lr_workers_gpu import STEPS, ipc_lr_worker, schedule

    s = schedule()
    eng = DataParallelEngine(w.make_model(), "cuda", lr=w.LR, lr_schedule=s)
    for st in range(STEPS):
        eng.train_step(*w.full_batch(step=st))
    ref = {k: v.float().cpu() for k, v in eng.full_state_dict().items()}
    assert eng.lr == s.lr_at(STEPS)
    out = tmp_path / "fsdp.pt"
    run_workers(ipc_lr_worker, 2, str(out), timeout=110)
    lrs = [torch.load(f"{out}.{r}", weights_only=True)["lrs"] for r in range(2)]
    print(f"rank rates {lrs}")
    assert lrs[0] == lrs[1] == [s.lr_at(t) for t in range(1, STEPS + 1)]
    close(torch.load(out, weights_only=True), ref, lr=w.LR, steps=STEPS)
