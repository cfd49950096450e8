"""Gradient clipping's sum-of-squares pass (``dpc_grad_sumsq``: streaming kernel + one-block
finalize) against the loss scaler's non-finite check (``dpc_amp_check``) on the same flat f32
buffer -- both are one read of the same bytes.  Sizes: the parameter counts of GPT-2 small and
GPT-2 XL.  Per size the two are warmed up, then timed with HIP events in alternating rounds of
about ``--window_ms`` each; one JSON line per size with the median (and spread) per launch, the
bytes/s of the median and the ratio sumsq / amp_check.

    python bench/clip_time.py [--sizes 124439808,1557611200] [--rounds 5] [--window_ms 200]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_pytorch_cookbook_amd.ops.amp import GradScaler  # noqa: E402
from distributed_pytorch_cookbook_amd.ops.clip import GradClipper  # noqa: E402


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
        raise SystemExit("clip_time.py times HIP kernels: no GPU found")
    clipper, scaler = GradClipper(1.0, "cuda"), GradScaler("cuda")
    for n in (int(x) for x in a.sizes.split(",")):
        g = torch.randn(n, device="cuda")
        fns = {"sumsq": lambda: clipper.add(g, replicated=False), "amp_check": lambda: scaler.check(g)}
        clipper.begin()
        clipper.add(g, replicated=False)
        err = abs(float(clipper.sumsq[0].sqrt()) / float(g.double().norm()) - 1.0)
        iters = {}
        for name, fn in fns.items():  # warm-up, and the launches that fill one window
            timed(fn, 3)
            iters[name] = max(10, min(5000, int(a.window_ms / timed(fn, 10))))
        ms = {name: [] for name in fns}
        for _ in range(a.rounds):  # alternating: drift hits both alike
            for name, fn in fns.items():
                ms[name].append(timed(fn, iters[name]))
        med = {name: statistics.median(v) for name, v in ms.items()}
        rec = {"n": n, "bytes": 4 * n, "rounds": a.rounds, "norm_rel_err": err}
        for name in fns:
            rec[name] = {"ms": round(med[name], 5), "min_ms": round(min(ms[name]), 5),
                         "max_ms": round(max(ms[name]), 5), "iters": iters[name],
                         "tb_per_s": round(4 * n / med[name] / 1e9, 3)}
        rec["ratio"] = round(med["sumsq"] / med["amp_check"], 4)
        print(json.dumps(rec), flush=True)
        del g


if __name__ == "__main__":
    main()
