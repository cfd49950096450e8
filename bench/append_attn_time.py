"""One layer's append-attention call alone (``ops.attention.append_attention``) at GPT-2 small's
heads: a block of n new tokens against a cache that holds ``start``, batch 1 and 8 -- the kernel
with the planner's split count, with one split, and with any counts given by ``--splits``; beside
them the same math on the materialised torch path (the op's retained fallback, on the same
tensors).  The kernel's launches are captured back to back in one HIP graph as a decode step runs
them; the torch path reads the length on the host, so it is timed eagerly between two events (its
calls take hundreds of microseconds and more, far above the launch rate).  Median of the rounds,
us per call.  One JSON line per (batch, start, n, variant).

    python bench/append_attn_time.py [--splits 2 4 8] [--blocks 8 128 512] [--starts 512 4096 16000]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_pytorch_cookbook_amd.ops import attention as A  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--head_dim", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--blocks", type=int, nargs="+", default=[8, 128, 512])
    ap.add_argument("--starts", type=int, nargs="+", default=[512, 4096, 16000])
    ap.add_argument("--splits", type=int, nargs="*", default=[], help="further forced split counts")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("append_attn_time.py times HIP kernels: no GPU found")
    torch.manual_seed(0)
    H, hd = a.heads, a.head_dim
    E = H * hd
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def timed(run, iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        run()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / iters * 1e3  # us per call

    def graphed(fn):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(a.iters):
                fn()
        return g.replay, a.iters

    def eager(fn):
        iters = max(2, a.iters // 10)
        return (lambda: [fn() for _ in range(iters)]), iters

    for N in a.batches:
        for start in a.starts:
            for n in a.blocks:
                Smax = start + n + 68
                kc = torch.randn(N, Smax, E, device="cuda").bfloat16()
                vc = torch.randn(N, Smax, E, device="cuda").bfloat16()
                qkv = torch.randn(N * n, 3 * E, device="cuda").bfloat16()
                length = torch.full((1,), start, device="cuda", dtype=torch.int64)
                plan = A.append_splits(N, H, n, Smax, cus)
                variants = [(f"plan {plan}", graphed, lambda: A.append_attention(qkv, kc, vc, length, n, H, hd))]
                for k in sorted({1, *a.splits} - {plan}):
                    variants.append((f"split {k}", graphed,
                                     lambda k=k: A.append_attention(qkv, kc, vc, length, n, H, hd, splits=k)))
                variants.append(("torch", eager, lambda: A._append_torch(qkv, kc, vc, start, n, H, hd, hd ** -0.5)))
                ref = None
                for name, how, fn in variants:
                    o = fn().float()
                    ref = o if ref is None else ref
                    run, iters = how(fn)
                    timed(run, iters)
                    us = [timed(run, iters) for _ in range(a.rounds)]
                    print(json.dumps({"batch": N, "start": start, "n": n, "variant": name,
                                      "us_per_call": round(statistics.median(us), 2), "min_us": round(min(us), 2),
                                      "max_us": round(max(us), 2),
                                      "max_diff_vs_first": round((o - ref).abs().max().item(), 5)}), flush=True)


if __name__ == "__main__":
    main()
