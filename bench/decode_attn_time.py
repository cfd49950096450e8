"""One layer's decode-attention call alone (``ops.attention.decode_attention``) at GPT-2 small's
heads, batch 1 and 8, over cache lengths: the one-workgroup kernel where it can run
(``dpc_decode_attn``, caches up to 16384 rows), the split kernel with one split, with the
planner's count, and with any counts given by ``--splits`` (how DECODE_SPLIT_MIN_KEYS is chosen).
Timed with HIP events over back-to-back launches after a warm-up, the launches captured in one
HIP graph as the decode step runs them (issued eagerly, a 10 us call measures the host's launch
rate); a cache of a few MB stays in L2 / MALL between launches, as it does not between the
layers of a real step.  Beside each time:
the K/V bytes the call must read, computed from the shape, and those bytes over the time.  One
JSON line per (batch, length, variant).

    python bench/decode_attn_time.py [--splits 2 4 8 16] [--lengths 1000 4000 16000 32000] [--kv_dtype fp8]

``--kv_dtype fp8``: the same calls over a 1-byte e4m3 cache (always the split kernel's fp8 twin;
half the K/V bytes).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_pytorch_cookbook_amd.ops import _lib  # noqa: E402
from distributed_pytorch_cookbook_amd.ops import attention as A  # noqa: E402


def one_workgroup(qkv, kc, vc, length, H, hd):
    """``dpc_decode_attn`` whatever the planner says (the routing of a plan of 1)."""
    N, E = qkv.shape[0], H * hd
    o = torch.empty(N, E, device=qkv.device, dtype=torch.bfloat16)
    args = _lib.DecodeAttnArgs(qkv=qkv.data_ptr(), kc=kc.data_ptr(), vc=vc.data_ptr(), o=o.data_ptr(),
                               len=length.data_ptr(), ldqkv=qkv.stride(0), ldo=E, N=N, H=H, hd=hd,
                               Smax=kc.shape[1], scale=hd ** -0.5, per_seq=0)
    _lib.call("dpc_decode_attn", args, qkv.device)
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--head_dim", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--lengths", type=int, nargs="+", default=[1000, 4000, 16000, 32000])
    ap.add_argument("--splits", type=int, nargs="*", default=[], help="further forced split counts")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kv_dtype", default="bf16", choices=["bf16", "fp8"])
    a = ap.parse_args()
    fp8 = a.kv_dtype == "fp8"
    if not torch.cuda.is_available():
        raise SystemExit("decode_attn_time.py times HIP kernels: no GPU found")
    torch.manual_seed(0)
    H, hd = a.heads, a.head_dim
    E = H * hd
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def graph_of(fn, iters):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(iters):
                fn()
        return g

    def timed(g, iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        g.replay()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / iters * 1e3  # us per call

    for N in a.batches:
        for L in a.lengths:
            Smax = L + 68  # the capacity bench/generate.py gives a context of L
            kc = torch.randn(N, Smax, E, device="cuda").bfloat16()
            vc = torch.randn(N, Smax, E, device="cuda").bfloat16()
            if fp8:
                kc, vc = A.kv_quantize_ref(kc, 1.0), A.kv_quantize_ref(vc, 1.0)
            qkv = torch.randn(N, 3 * E, device="cuda").bfloat16()
            length = torch.full((1,), L - 1, device="cuda", dtype=torch.int64)  # L keys with the new one
            plan = A.decode_splits(N, H, Smax, cus)
            variants = [("split 1", lambda: A.decode_attention(qkv, kc, vc, length, H, hd, splits=1)),
                        (f"plan {plan}", lambda: A.decode_attention(qkv, kc, vc, length, H, hd))]
            if Smax <= A.DECODE_MAX_S and not fp8:
                variants.insert(0, ("one workgroup", lambda: one_workgroup(qkv, kc, vc, length, H, hd)))
            for k in a.splits:
                variants.append((f"split {k}", lambda k=k: A.decode_attention(qkv, kc, vc, length, H, hd, splits=k)))
            ref = None
            kv_bytes = 2 * N * L * E * kc.element_size()
            for name, fn in variants:
                o = fn().float()
                ref = o if ref is None else ref
                g = graph_of(fn, a.iters)
                timed(g, a.iters)
                us = [timed(g, a.iters) for _ in range(a.rounds)]
                med = statistics.median(us)
                print(json.dumps({"kv_dtype": a.kv_dtype, "batch": N, "keys": L, "variant": name, "us_per_call": round(med, 2),
                                  "min_us": round(min(us), 2), "max_us": round(max(us), 2), "kv_bytes": kv_bytes,
                                  "kv_bytes_per_s": round(kv_bytes / (med * 1e-6)),
                                  "max_diff_vs_first": round((o - ref).abs().max().item(), 5)}), flush=True)


if __name__ == "__main__":
    main()
