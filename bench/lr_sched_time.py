"""``adamw_kernel`` with and without a learning-rate schedule (``ops/schedule.py``: the rate is
then computed inside the kernel, per thread, from the step counter) on the same flat buffers --
f32 parameters, gradients and both moments read, parameters and moments written (28 bytes per
element) plus the bf16 compute copy (2 more).
Sizes: the parameter counts of GPT-2 small and GPT-2 XL.  Per size the variants (no schedule,
with the step host-passed and read from the device counter -- the captured step's path, which
also forms the bias corrections on the device; cosine, the same two ways) are warmed
up, then timed with HIP events in alternating rounds of about ``--window_ms`` each; one JSON
line per size with the median (and spread) per launch and the ratios to the unscheduled kernel.

    python bench/lr_sched_time.py [--sizes 124439808,1557611200] [--rounds 5] [--window_ms 200]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_pytorch_cookbook_amd.ops.optim import FlatAdamW  # noqa: E402
from distributed_pytorch_cookbook_amd.ops.schedule import LRSchedule  # noqa: E402


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters  # ms per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="124439808,1557611200")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window_ms", type=float, default=200.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lr_sched_time.py times a HIP kernel: no GPU found")
    sched = LRSchedule("cosine", 6e-4, 2000, 100000, 0.1)
    for n in (int(x) for x in a.sizes.split(",")):
        p, g = torch.randn(n, device="cuda"), torch.randn(n, device="cuda")
        opt = FlatAdamW(p, g, lr=6e-4, shadow=torch.empty(n, device="cuda", dtype=torch.bfloat16))
        opt.step_count = 50000  # mid-decay: the cosine branch
        opt.step_t.fill_(50000.0)

        def run(s, device_step):
            opt.lr_schedule, opt.device_step = s, device_step
            opt.update(0, n)

        fns = {"none": lambda: run(None, False), "none_device_t": lambda: run(None, True),
               "cosine_host_t": lambda: run(sched, False), "cosine_device_t": lambda: run(sched, True)}
        iters = {}
        for name, fn in fns.items():  # warm-up, and the launches that fill one window
            timed(fn, 3)
            iters[name] = max(10, min(5000, int(a.window_ms / timed(fn, 10))))
        ms = {name: [] for name in fns}
        for _ in range(a.rounds):  # alternating: drift hits all alike
            for name, fn in fns.items():
                ms[name].append(timed(fn, iters[name]))
        med = {name: statistics.median(v) for name, v in ms.items()}
        rec = {"n": n, "bytes": 30 * n, "rounds": a.rounds, "finite": bool(torch.isfinite(p).all())}
        for name in fns:
            rec[name] = {"ms": round(med[name], 5), "min_ms": round(min(ms[name]), 5),
                         "max_ms": round(max(ms[name]), 5), "iters": iters[name],
                         "tb_per_s": round(30 * n / med[name] / 1e9, 3)}
        rec["spread_none"] = round((max(ms["none"]) - min(ms["none"])) / med["none"], 5)
        for name in ("none_device_t", "cosine_host_t", "cosine_device_t"):
            rec[f"ratio_{name}"] = round(med[name] / med["none"], 5)
        # the schedule alone on the device-counter path (both form the bias corrections there)
        rec["ratio_cosine_device_t_to_none_device_t"] = round(med["cosine_device_t"] / med["none_device_t"], 5)
        print(json.dumps(rec), flush=True)
        del opt, p, g


if __name__ == "__main__":
    main()
