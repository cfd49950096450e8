"""One Linear of 1..64 rows alone, at the shapes of a GPT-2 small / GPT-2 XL decode step (QKV, the
out-projection with bias and f32 residual, the up-projection with bias and GELU, the
down-projection with bias and f32 residual, the LM head over the padded vocabulary): the skinny
kernel (``dpc_gemm_skinny``, csrc/skinny_gemm.hip) with the planner's plan -- and with every
instantiated plan under ``--plans`` (how ``ops/gemm.py:skinny_plan`` is chosen) -- against the
training dispatcher's path (``gemm``: what ``linear_fwd`` runs with DPC_SKINNY=0) and, at 16 rows
or fewer, the few-row kernel (``dpc_gemv``).  Timed with HIP events over back-to-back launches
captured in one HIP graph, as the decode step runs them, after a warm-up replay; the median of
``--rounds`` replays.  The layers' weights differ from call to call in a real step, so each call of
the graph uses its own copy of the weight (``--copies``, together larger than L2 and the
Infinity Cache): a weight that stayed in cache would flatter every variant.  Beside each time the
weight bytes the product must read and those bytes over the time.  One JSON line per
(shape, rows, variant).

``--weight_dtype fp8``: beside what bf16 weights run at that row count, the fp8-weight kernel
(``dpc_gemm_wq8``, csrc/wq_gemm.hip) on a quantised copy of every weight copy, under both plans;
its weight bytes are half.  ``--weight_dtype fp4``: the fp8-weight kernel and the MXFP4-weight kernel
(``dpc_gemm_wq4``, csrc/wq4_gemm.hip, a quarter of the bytes) side by side; the copies are then
counted so that the fp4 ones alone exceed the caches.

``--norm``: the products that consume a LayerNorm (QKV, up-projection, LM head) on the f32 residual
stream: ``layernorm_fwd`` then ``linear_fwd`` (two launches) against ``linear_fwd(norm=)``
(``dpc_ln_linear``, csrc/ln_linear.hip, one launch), at the row counts that kernel takes, on bf16
weights or with ``--weight_dtype fp8`` on the quantised ones.

    python bench/skinny_time.py [--rows 1 8 16 17 32 48 64] [--models gpt2-small gpt2-xl] [--plans]
                                [--weight_dtype fp8|fp4] [--norm]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_pytorch_cookbook_amd.ops import gemm as G  # noqa: E402
from distributed_pytorch_cookbook_amd.ops.norm import layernorm_fwd  # noqa: E402

DIMS = {"gpt2-small": 768, "gpt2-xl": 1600}
VOCAB, VOCAB_LD = 50257, 50304


def shapes(D):
    """(name, Nw, N, K, bias, act, residual -> f32 out)"""
    return [("qkv", 3 * D, 3 * D, D, True, 0, False), ("out", D, D, D, True, 0, True),
            ("up_gelu", 4 * D, 4 * D, D, True, G.ACT_GELU, False), ("down_res", D, D, 4 * D, True, 0, True),
            ("lm_head", VOCAB, VOCAB_LD, D, False, 0, False)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 8, 16, 17, 32, 48, 64])
    ap.add_argument("--models", nargs="+", default=list(DIMS))
    ap.add_argument("--plans", action="store_true", help="also every instantiated (columns, waves) plan")
    ap.add_argument("--weight_dtype", default="bf16", choices=["bf16", "fp8", "fp4"],
                    help="fp8: also dpc_gemm_wq8; fp4: also dpc_gemm_wq8 and dpc_gemm_wq4")
    ap.add_argument("--norm", action="store_true",
                    help="instead: LayerNorm + Linear (two launches) against dpc_ln_linear (one), on the products "
                         "that consume a LayerNorm, with the weights of --weight_dtype")
    ap.add_argument("--cache_mb", type=int, default=768, help="weight copies cover at least this much")
    ap.add_argument("--min_calls", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("skinny_time.py times HIP kernels: no GPU found")
    torch.manual_seed(0)
    dev = "cuda"
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def timed(g, calls):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        g.replay()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / calls * 1e3  # us per call

    for model in a.models:
        D = DIMS[model]
        for name, Nw, N, K, has_bias, act, has_res in shapes(D):
            if a.norm and has_res:  # (no LayerNorm feeds the out- and down-projections)
                continue
            w_bytes = Nw * K * 2
            copies = max(a.min_calls, -(-a.cache_mb * 2**20 // (w_bytes // 4 if a.weight_dtype == "fp4" else w_bytes)))
            ws = [(torch.randn(Nw, K, device=dev) / K ** 0.5).bfloat16() for _ in range(copies)]
            qs = [G.quantize_weight(w) for w in ws] if a.weight_dtype != "bf16" else None
            q4s = [G.quantize_weight(w, "fp4") for w in ws] if a.weight_dtype == "fp4" else None
            bias = torch.randn(Nw, device=dev) if has_bias else None
            for M in a.rows:
                x = torch.randn(M, K, device=dev).bfloat16()
                res = torch.randn(M, N, device=dev) if has_res else None
                odt = torch.float32 if has_res else torch.bfloat16
                out = torch.empty(M, N, device=dev, dtype=odt)
                variants = [("dispatcher", lambda w: G.gemm(x, w, bias=bias, act=act, residual=res, out=out))]
                if M <= G._GEMV_ROWS:
                    variants.append(("gemv", lambda w: G._linear_fwd_few_rows(x, w, bias, act, res, out, odt)))
                plan = G.skinny_plan(M, N, K, cus)
                for pl in ((plan,) + tuple(p for p in G.SKINNY_PLANS if a.plans and p != plan)):
                    variants.append((f"skinny {pl[0]}x{pl[1]}" + (" (plan)" if pl == plan else ""),
                                     lambda w, pl=pl: G._linear_fwd_skinny(x, w, bias, act, res, out, odt, plan=pl)))
                variants = [(vname, fn, ws, w_bytes) for vname, fn in variants]
                if a.norm:
                    # the LayerNorm's consumers only, on the f32 residual stream: one fused launch
                    # against LayerNorm then what linear_fwd runs at that row count
                    if not G.ln_linear_ok(M, K, (qs or ws)[0]):
                        continue
                    xf, gamma, beta = torch.randn(M, K, device=dev), torch.rand(K, device=dev) + 0.5, torch.randn(K, device=dev)
                    norm = (gamma, beta, 1e-5)
                    variants = [("ln + linear", lambda w: G.linear_fwd(layernorm_fwd(xf, *norm)[0], w, bias=bias, act=act, out=out),
                                 qs or ws, w_bytes // (2 if qs else 1)),
                                ("ln_linear", lambda w: G.linear_fwd(xf, w, bias=bias, act=act, out=out, norm=norm),
                                 qs or ws, w_bytes // (2 if qs else 1))]
                elif qs is not None:
                    for pl in G.SKINNY_PLANS:
                        variants.append((f"fp8 {pl[0]}x{pl[1]}" + (" (plan)" if pl == plan else ""),
                                         lambda w, pl=pl: G._linear_fwd_wq8(x, w, bias, act, res, out, odt, plan=pl),
                                         qs, w_bytes // 2))
                    for pl in (G.SKINNY_PLANS if q4s is not None else ()):
                        variants.append((f"fp4 {pl[0]}x{pl[1]}" + (" (plan)" if pl == plan else ""),
                                         lambda w, pl=pl: G._linear_fwd_wq4(x, w, bias, act, res, out, odt, plan=pl),
                                         q4s, w_bytes // 4 + w_bytes // 64))
                ref = None
                for vname, fn, weights, nbytes in variants:
                    o = fn(weights[0]).float().clone()
                    ref = o if ref is None else ref
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        for w in weights:
                            fn(w)
                    timed(g, copies)
                    us = [timed(g, copies) for _ in range(a.rounds)]
                    med = statistics.median(us)
                    print(json.dumps({"model": model, "shape": name, "N": N, "K": K, "rows": M, "variant": vname,
                                      "us_per_call": round(med, 2), "min_us": round(min(us), 2),
                                      "max_us": round(max(us), 2), "weight_bytes": nbytes,
                                      "weight_bytes_per_s": round(nbytes / (med * 1e-6)),
                                      "max_diff_vs_first": round((o - ref).abs().max().item(), 5)}), flush=True)
            del ws, qs, q4s


if __name__ == "__main__":
    main()
