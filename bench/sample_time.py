"""The sampler kernel's own time (``dpc_sample``: one workgroup per row of bf16 logits) at GPT-2's
vocabulary, for one parameter set per run so that a kernel-stats profile of the run is that set's
time.  Timed with HIP events over back-to-back launches on the same logits (L2-resident, as they
are behind the LM head of a decode step); one JSON line with the time per launch.

    python bench/sample_time.py [--rows 8] [--vocab 50257] [--temperature 0.8 --top_k 50 --top_p 0.9]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_pytorch_cookbook_amd.models.fused import vocab_ld  # noqa: E402
from distributed_pytorch_cookbook_amd.ops.sample import sample_logits  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=50257)
    ap.add_argument("--scale", type=float, default=3.0, help="standard deviation of the random logits")
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--top_k", type=int, default=50)
    ap.add_argument("--top_p", type=float, default=0.9)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_time.py times a HIP kernel: no GPU found")
    torch.manual_seed(0)
    N, V = a.rows, a.vocab
    buf = torch.full((N, vocab_ld(V)), 1e4, dtype=torch.bfloat16, device="cuda")
    buf[:, :V] = (torch.randn(N, V, device="cuda") * a.scale).bfloat16()
    logits = buf[:, :V]
    counters = torch.zeros(N, dtype=torch.int64, device="cuda")
    tok = torch.zeros(N, 1, dtype=torch.int64, device="cuda")

    def run():
        sample_logits(logits, temperature=a.temperature, top_k=a.top_k, top_p=a.top_p, seed=0, counters=counters,
                      out_tok=tok)

    def timed(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            run()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / iters * 1e3  # us per launch

    timed(10)
    us = [timed(a.iters) for _ in range(a.rounds)]
    print(json.dumps({"rows": N, "vocab": V, "temperature": a.temperature, "top_k": a.top_k, "top_p": a.top_p,
                      "us_per_launch": round(statistics.median(us), 2), "min_us": round(min(us), 2),
                      "max_us": round(max(us), 2), "iters": a.iters, "rounds": a.rounds}))


if __name__ == "__main__":
    main()
