"""GEMM with fused epilogues -- the matmul behind every ``nn.Linear`` of ``models.gpt``.

``gemm`` computes ``C = epilogue(alpha * A @ B^T)`` where A is ``[M, K]`` and B is
``[N, K]`` logically; each operand may be stored k-contiguous ("kmaj") or
m/n-contiguous, so the forward (``x @ W^T``), the input gradient (``dy @ W``) and the
weight gradient (``dy^T @ x``) of a Linear are all one kernel family without transpose
copies (reference: ``/root/reference/models/gpt.py:29-30,60-64,219`` -- every Linear).

Epilogue order (identical in the HIP kernel and the torch reference below)::

    v = acc * alpha (* alpha_t) + bias[n]
    v = v * act'(aux_in)            if act_bwd (ACT_MUL: v * aux_in -- act' precomputed)
    aux_out = bf16(v)               if aux_out (pre-activation saved for backward;
                                    bf16(act'(v)) with aux_deriv, for a later ACT_MUL)
    v = act(v)                      if act
    v = v + residual                if residual
    C = C + v                       if accumulate (f32 C only)

On a HIP device with bf16 operands this runs ``dpc_gemm`` (MFMA, ``csrc/gemm.hip``);
on CPU (or fp32 operands, the explicit ``--disable_amp`` precision mode) it runs the
same math with torch ops -- that expression is also the numerics oracle of the tests.
"""
from __future__ import annotations

import atexit
import json
import math
import os

import torch
import torch.nn.functional as F

from . import _lib

ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
# input-gradient epilogues only: the act' operand holds act'(z) already (written by a forward
# epilogue with aux_deriv=True), multiplied in as is (csrc/common.h:Act)
ACT_MUL = 3
ACTS = {None: ACT_NONE, "none": ACT_NONE, "relu": ACT_RELU, "gelu": ACT_GELU}


def act_code(act) -> int:
    if isinstance(act, int):
        return act
    return ACTS[act]


def act_fwd_ref(v: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_RELU:
        return F.relu(v)
    if act == ACT_GELU:
        return F.gelu(v, approximate="tanh")
    return v


def act_grad_ref(z: torch.Tensor, act: int) -> torch.Tensor:
    z = z.float()
    if act == ACT_RELU:
        return (z > 0).float()
    if act == ACT_GELU:
        k0, k1 = math.sqrt(2.0 / math.pi), 0.044715
        u = k0 * (z + k1 * z * z * z)
        t = torch.tanh(u)
        return 0.5 * (1 + t) + 0.5 * z * (1 - t * t) * k0 * (1 + 3 * k1 * z * z)
    if act == ACT_MUL:
        return z
    return torch.ones_like(z)


# ---------------------------------------------------------------- measured per-shape choices
# The dispatcher's built-in policy (csrc/gemm_plan.h) was fitted to GPT-2 small; on other shapes
# the best tile / pipeline depends on wave quantisation (tiles vs 256 CUs), the epilogue's
# traffic and K.  ``gemm_tuned.json`` (next to this file) maps a product's signature to the
# implementation measured fastest for it on MI355X; ``DPC_GEMM_TUNE=1`` measures every
# signature missing from the table the first time it runs eagerly (never inside a HIP-graph
# capture: outputs are cloned, candidates timed with HIP events, best of 3 x 5 launches) and
# writes the merged table to ``DPC_GEMM_TUNE_OUT`` (default: the in-package file) at exit.
_TUNE_PATH = os.environ.get("DPC_GEMM_TABLE_PATH") or os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "gemm_tuned.json")
_TUNE = os.environ.get("DPC_GEMM_TUNE", "0") == "1"
_USE_TABLE = os.environ.get("DPC_GEMM_TABLE", "1") == "1"
# 0 = the dispatcher's policy, else an id of the implementation table (csrc/gemm_plan.h:GEMM_IMPLS)
_CANDIDATES = (0, 2, 3, 4, 10, 16, 17, 19, 20, 21, 22, 23, 24, 25, 26)
_TUNE_MAX_OUT_BYTES = 16 << 30  # (the GPT-2 small LM-head logits are 6.6 GB)


def _load_table(path: str = _TUNE_PATH) -> dict:
    try:
        with open(path) as f:
            return {k: int(v) for k, v in json.load(f).get("impl", {}).items()}
    except (OSError, ValueError):
        return {}


_table: dict = _load_table() if _USE_TABLE else {}
_tuned_new: dict = {}
_near_cache: dict = {}
_NEAR = os.environ.get("DPC_GEMM_NEAR", "1") == "1"  # 0: exact signatures only (A/B)


def _near(key: str):
    """The table's choice for the closest measured product that differs from ``key`` only in its
    token dimension (M of a forward / input-gradient product, K of a weight gradient) by at most
    25 % -- e.g. 8 x 8191 = 65528 rows at S = 8192 against the 65472 (64 x 1023) the table was
    measured at; the best tile / pipeline depends on the other dimensions and the epilogue."""
    if key in _near_cache:
        return _near_cache[key]
    dims, rest = key.split(":", 1)
    M, N, K = (int(v) for v in dims.split("x"))
    best = None
    for k2, v in _table.items():
        d2, r2 = k2.split(":", 1)
        if r2 != rest:
            continue
        M2, N2, K2 = (int(x) for x in d2.split("x"))
        if N2 != N:
            continue
        if K2 == K and M2 != M:
            diff = abs(M2 - M) / M
        elif M2 == M and K2 != K:
            diff = abs(K2 - K) / K
        else:
            continue
        if diff <= 0.25 and (best is None or diff < best[0]):
            best = (diff, v)
    _near_cache[key] = best[1] if best else None
    return _near_cache[key]


def _save_table() -> None:
    if not _tuned_new:
        return
    path = os.environ.get("DPC_GEMM_TUNE_OUT", _TUNE_PATH)
    merged = _load_table(path) if os.path.exists(path) else _load_table()
    merged.update(_tuned_new)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"device": "MI355X (gfx950)", "impl": dict(sorted(merged.items()))}, f, indent=1)


if _TUNE:
    atexit.register(_save_table)


# Split-K workspace of the weight-gradient products (f32, per device and stream): the v7 kernel
# stores every k-range's partial tile there with plain stores and one reduction pass sums the
# slabs into the gradient, instead of f32 atomics into it -- GPT-2 small's split layer weight
# gradients ran 276-380 us with the atomics (bench/gemm_one.py --splits, scripts/
# wgrad_split_sweep.sh).  Allocated once, outside any graph capture, and kept alive (a captured
# step graph holds its address).  DPC_GEMM_WS_MB=0 turns it off (atomics).
# One workspace per device serves the compute stream -- and the private stream a HIP-graph
# capture records it from, so a captured step uses the same buffer as its eager warm-up; a
# stream that runs GEMMs CONCURRENTLY with it (the optional weight-gradient side stream,
# models/fused.py) registers itself and gets its own.
_WS_BYTES = int(float(os.environ.get("DPC_GEMM_WS_MB", "1024")) * 2**20)
_ws: dict = {}
_side_streams: set = set()


def register_side_stream(stream) -> None:
    """Give ``stream`` (which runs GEMMs concurrently with the compute stream) its own split-K
    workspace."""
    _side_streams.add(stream.cuda_stream)


def _workspace(device):
    if _WS_BYTES <= 0:
        return None
    sid = torch.cuda.current_stream(device).cuda_stream
    key = (device.index, sid) if sid in _side_streams else device.index
    t = _ws.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        t = torch.empty(_WS_BYTES // 4, dtype=torch.float32, device=device)
        _ws[key] = t
    return t


def _sig(M, N, K, a_kmaj, b_kmaj, out_f32, bias, act, act_bwd, aux_out, residual, colsum,
         accumulate) -> str:
    flags = "".join(c for c, on in (("b", bias is not None), ("x", aux_out is not None),
                                     ("r", residual is not None), ("c", colsum is not None),
                                     ("a", accumulate)) if on)
    # (ACT_MUL keys as GELU': same product and epilogue traffic, one table entry for both)
    act_bwd = ACT_GELU if act_bwd == ACT_MUL else act_bwd
    return (f"{M}x{N}x{K}:{'k' if a_kmaj else 'm'}{'k' if b_kmaj else 'm'}:"
            f"{'f' if out_f32 else 'h'}:{act}{act_bwd}:{flags}")


def _tune(args, out, aux_out, colsum, device) -> int:
    """Time every candidate implementation on clones of the outputs; return the fastest."""
    scratch = {"C": out.clone()}
    if aux_out is not None:
        scratch["aux_out"] = aux_out.clone()
    if colsum is not None:
        scratch["colsum"] = colsum.clone()
    saved = {k: getattr(args, k) for k in scratch}
    for k, t in scratch.items():
        setattr(args, k, t.data_ptr())
    best, best_t = 0, float("inf")
    try:
        for impl in _CANDIDATES:
            args.impl = impl
            try:
                _lib.call("dpc_gemm", args, device)
                torch.cuda.synchronize(device)
            except RuntimeError:
                continue
            t_min = float("inf")
            for _ in range(3):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(5):
                    _lib.call("dpc_gemm", args, device)
                e.record()
                e.synchronize()
                t_min = min(t_min, s.elapsed_time(e))
            if t_min < best_t:
                best, best_t = impl, t_min
    finally:
        for k, v in saved.items():
            setattr(args, k, v)
    return best


def _check_operand(t: torch.Tensor, rows: int, cols: int, name: str) -> None:
    if t.dim() != 2 or t.shape[0] != rows or t.shape[1] != cols:
        raise ValueError(f"{name}: expected shape ({rows}, {cols}), got {tuple(t.shape)}")
    if t.stride(1) != 1:
        raise ValueError(f"{name}: inner dimension must be contiguous (stride {t.stride()})")
    if t.dtype != torch.bfloat16:
        raise ValueError(f"{name}: expected bf16, got {t.dtype}")
    if t.data_ptr() % 16 or t.stride(0) % 8:
        raise ValueError(f"{name}: base must be 16-B aligned and row stride a multiple of 8")
    # 16-B chunk reads may touch up to roundup8(cols) elements of the last row
    need = (t.storage_offset() + (rows - 1) * t.stride(0) + ((cols + 7) // 8) * 8) * t.element_size()
    if rows > 0 and need > t.untyped_storage().nbytes():
        raise ValueError(f"{name}: storage too small for 16-B chunked reads (pad the row)")


def gemm(
    a: torch.Tensor,
    b: torch.Tensor,
    *,
    a_kmaj: bool = True,
    b_kmaj: bool = True,
    out: torch.Tensor | None = None,
    out_dtype: torch.dtype = torch.bfloat16,
    bias: torch.Tensor | None = None,
    act=ACT_NONE,
    act_bwd=ACT_NONE,
    aux_in: torch.Tensor | None = None,
    aux_out: torch.Tensor | None = None,
    residual: torch.Tensor | None = None,
    alpha: float = 1.0,
    alpha_t: torch.Tensor | None = None,
    accumulate: bool = False,
    colsum: torch.Tensor | None = None,
    aux_deriv: bool = False,
) -> torch.Tensor:
    act, act_bwd = act_code(act), act_code(act_bwd)
    if aux_deriv and (aux_out is None or act != ACT_GELU):
        raise ValueError("gemm: aux_deriv needs aux_out and act='gelu'")
    Ma, Ka = (a.shape[0], a.shape[1]) if a_kmaj else (a.shape[1], a.shape[0])
    Nb, Kb = (b.shape[0], b.shape[1]) if b_kmaj else (b.shape[1], b.shape[0])
    # logical sizes; an operand may be stored smaller than them (rows / k-rows beyond its
    # stored extent read as zeros), e.g. the lm_head over a 64-padded vocabulary
    M = out.shape[0] if out is not None else Ma
    N = out.shape[1] if out is not None else Nb
    K = max(Ka, Kb)
    if Ma > M or Nb > N or (Ka != K and a_kmaj) or (Kb != K and b_kmaj):
        raise ValueError(f"gemm: incompatible operands A{tuple(a.shape)} B{tuple(b.shape)} -> ({M},{N},{K})")
    if out is None:
        if accumulate:
            raise ValueError("gemm: accumulate needs an out tensor")
        out = torch.empty((M, N), device=a.device, dtype=out_dtype)
    if out.shape != (M, N) or out.stride(1) != 1:
        raise ValueError(f"gemm: bad out {tuple(out.shape)} stride {out.stride()}")
    if accumulate and out.dtype != torch.float32:
        raise ValueError("gemm: accumulate requires an f32 output")
    if act_bwd and aux_in is None:
        raise ValueError("gemm: act_bwd needs aux_in")

    if a.is_cuda and a.dtype == torch.bfloat16:
        _check_operand(a, a.shape[0], a.shape[1], "A")
        _check_operand(b, b.shape[0], b.shape[1], "B")
        for t, nm, dt in ((residual, "residual", torch.float32), (bias, "bias", torch.float32),
                          (colsum, "colsum", torch.float32),
                          (aux_in, "aux_in", torch.bfloat16), (aux_out, "aux_out", torch.bfloat16)):
            if t is not None and (t.dtype != dt or t.stride(-1) != 1):
                raise ValueError(f"gemm: {nm} must be contiguous-last {dt}")
        if out.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("gemm: out must be f32 or bf16")
        # the workspace: split-K slabs of plain f32 products, and the per-tile partial column
        # sums of the input-gradient epilogue (act' + bias-gradient column sums)
        ws = (_workspace(a.device) if ((out.dtype == torch.float32 and bias is None and residual is None
                                          and aux_in is None and aux_out is None and colsum is None
                                          and not act and not act_bwd)
                                         or (colsum is not None and act_bwd)) else None)
        args = _lib.GemmArgs(
            A=a.data_ptr(), B=b.data_ptr(), C=out.data_ptr(),
            bias=_lib.ptr(bias), residual=_lib.ptr(residual), aux_in=_lib.ptr(aux_in),
            aux_out=_lib.ptr(aux_out), alpha_ptr=_lib.ptr(alpha_t), colsum=_lib.ptr(colsum),
            lda=a.stride(0), ldb=b.stride(0), ldc=out.stride(0),
            ldr=residual.stride(0) if residual is not None else 0,
            ld_aux_in=aux_in.stride(0) if aux_in is not None else 0,
            ld_aux_out=aux_out.stride(0) if aux_out is not None else 0,
            M=M, N=N, K=K, alpha=float(alpha), act=act, act_bwd=act_bwd,
            out_f32=int(out.dtype == torch.float32), accumulate=int(accumulate),
            a_kmaj=int(a_kmaj), b_kmaj=int(b_kmaj),
            a_r=a.shape[0], a_c=a.shape[1], b_r=b.shape[0], b_c=b.shape[1],
            ws=_lib.ptr(ws), ws_bytes=0 if ws is None else ws.numel() * 4,
            aux_deriv=int(aux_deriv),
        )
        if (_table or _TUNE) and _lib.forced_gemm_impl < 0:
            key = _sig(M, N, K, a_kmaj, b_kmaj, out.dtype == torch.float32, bias, act, act_bwd,
                       aux_out, residual, colsum, accumulate)
            impl = _table.get(key)
            if impl is None and not _TUNE and _NEAR:
                impl = _near(key)
            if (impl is None and _TUNE and not torch.cuda.is_current_stream_capturing()
                    and out.numel() * out.element_size() <= _TUNE_MAX_OUT_BYTES):
                impl = _tune(args, out, aux_out, colsum, a.device)
                _table[key] = _tuned_new[key] = impl
            args.impl = impl or 0
        _lib.call("dpc_gemm", args, a.device)
        return out
    if a.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32 and out.dtype == torch.float32:
        return _gemm_f32(a, b, a_kmaj, b_kmaj, out, M, N, K, bias, act, act_bwd, aux_in, aux_out,
                         residual, alpha, alpha_t, accumulate, colsum, aux_deriv)
    return _gemm_ref(a, b, a_kmaj, b_kmaj, out, bias, act, act_bwd, aux_in, aux_out, residual,
                     alpha, alpha_t, accumulate, colsum, aux_deriv)


def _gemm_f32(a, b, a_kmaj, b_kmaj, out, M, N, K, bias, act, act_bwd, aux_in, aux_out, residual,
              alpha, alpha_t, accumulate, colsum, aux_deriv=False):
    """f32 operands (the --disable_amp path): ``dpc_gemm_f32`` on the f32 matrix cores
    (csrc/gemm_f32.hip), same fused epilogue as the bf16 kernels."""
    for t, nm in ((a, "A"), (b, "B"), (out, "out")):
        if t.stride(-1) != 1:
            raise ValueError(f"gemm f32: {nm} inner dimension must be contiguous")
    aux = [t for t in (aux_in, aux_out) if t is not None]
    aux_f32 = bool(aux) and aux[0].dtype == torch.float32
    for t, nm in ((residual, "residual"), (bias, "bias"), (colsum, "colsum")):
        if t is not None and (t.dtype != torch.float32 or t.stride(-1) != 1):
            raise ValueError(f"gemm f32: {nm} must be contiguous-last f32")
    for t in aux:
        if t.dtype != (torch.float32 if aux_f32 else torch.bfloat16) or t.stride(-1) != 1:
            raise ValueError("gemm f32: aux_in / aux_out must share one dtype (f32 or bf16)")
    args = _lib.GemmArgs(
        A=a.data_ptr(), B=b.data_ptr(), C=out.data_ptr(),
        bias=_lib.ptr(bias), residual=_lib.ptr(residual), aux_in=_lib.ptr(aux_in),
        aux_out=_lib.ptr(aux_out), alpha_ptr=_lib.ptr(alpha_t), colsum=_lib.ptr(colsum),
        lda=a.stride(0), ldb=b.stride(0), ldc=out.stride(0),
        ldr=residual.stride(0) if residual is not None else 0,
        ld_aux_in=aux_in.stride(0) if aux_in is not None else 0,
        ld_aux_out=aux_out.stride(0) if aux_out is not None else 0,
        M=M, N=N, K=K, alpha=float(alpha), act=act, act_bwd=act_bwd, out_f32=1,
        accumulate=int(accumulate), a_kmaj=int(a_kmaj), b_kmaj=int(b_kmaj),
        a_r=a.shape[0], a_c=a.shape[1], b_r=b.shape[0], b_c=b.shape[1], aux_f32=int(aux_f32),
        aux_deriv=int(aux_deriv),
    )
    _lib.call("dpc_gemm_f32", args, a.device)
    return out


def _pad_to(x: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    if x.shape[0] == rows and x.shape[1] == cols:
        return x
    out = torch.zeros(rows, cols, dtype=x.dtype, device=x.device)
    out[:x.shape[0], :x.shape[1]] = x
    return out


def _gemm_ref(a, b, a_kmaj, b_kmaj, out, bias, act, act_bwd, aux_in, aux_out, residual,
              alpha, alpha_t, accumulate, colsum=None, aux_deriv=False):
    am = (a if a_kmaj else a.t()).float()
    bm = (b if b_kmaj else b.t()).float()
    M, N = out.shape
    K = max(am.shape[1], bm.shape[1])
    v = _pad_to(am, M, K) @ _pad_to(bm, N, K).t()
    v = v * alpha
    if alpha_t is not None:
        v = v * alpha_t.float()
    if bias is not None:
        v = v + bias.float()
    if act_bwd:
        v = v * act_grad_ref(aux_in, act_bwd)
    if colsum is not None:
        colsum.add_(v.sum(0))
    if aux_out is not None:
        aux_out.copy_(act_grad_ref(v, act) if aux_deriv else v)
    v = act_fwd_ref(v, act)
    if residual is not None:
        v = v + residual.float()
    if accumulate:
        out.add_(v)
    else:
        out.copy_(v)
    return out


# ---------------------------------------------------------------- Linear-shaped helpers
def linear_fwd(x, w, *, bias=None, act=None, residual=None, aux_out=None, out=None,
               out_dtype=torch.bfloat16, aux_deriv=False):
    """y = act(x @ w^T + bias) (+ residual); x [M, K], w [N, K] (nn.Linear layout).
    ``aux_out`` receives the pre-activation, or act'(pre-activation) with ``aux_deriv``."""
    if (x.is_cuda and x.shape[0] <= _GEMV_ROWS and aux_out is None and x.dtype == torch.bfloat16
            and w.dtype == torch.bfloat16):
        return _linear_fwd_few_rows(x, w, bias, act_code(act), residual, out, out_dtype)
    return gemm(x, w, a_kmaj=True, b_kmaj=True, bias=bias, act=act, residual=residual,
                aux_out=aux_out, out=out, out_dtype=out_dtype, aux_deriv=aux_deriv)


# decode-shaped products (a handful of rows): the MFMA tile kernels would launch N / 256
# workgroups on a 256-CU chip and the weight stream is the whole cost, so these run the
# few-row kernel (csrc/decode.hip: dpc_gemv -- vector-ALU dot products at the memory rate,
# bias / activation / f32 residual fused into the same launch: one launch per Linear of the
# decode step instead of the library GEMV plus up to three elementwise launches)
_GEMV_ROWS = 16
_GEMV_NATIVE = os.environ.get("DPC_GEMV", "1") == "1"  # 0: the library product (A/B only)


def _gemv_ok(x, w, bias, residual, out, N):
    return (x.stride(1) == 1 and w.stride(1) == 1 and x.shape[1] % 8 == 0 and x.stride(0) % 8 == 0
            and w.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
            and (bias is None or (bias.dtype == torch.float32 and bias.is_contiguous()))
            and (residual is None or (residual.dtype == torch.float32 and residual.stride(1) == 1))
            and out.stride(1) == 1 and w.shape[0] <= N)


def _linear_fwd_few_rows(x, w, bias, act, residual, out, out_dtype):
    M, K = x.shape
    Nw = w.shape[0]
    if out is None:
        out = torch.empty(M, Nw, device=x.device, dtype=out_dtype)
    N = out.shape[1]
    if _GEMV_NATIVE and _gemv_ok(x, w, bias, residual, out, N) and out.dtype in (torch.float32, torch.bfloat16):
        args = _lib.GemvArgs(
            x=x.data_ptr(), w=w.data_ptr(), bias=_lib.ptr(bias), residual=_lib.ptr(residual),
            y=out.data_ptr(), ldx=x.stride(0), ldw=w.stride(0),
            ldr=residual.stride(0) if residual is not None else 0, ldy=out.stride(0),
            M=M, N=N, Nw=Nw, K=K, act=act, y_f32=int(out.dtype == torch.float32))
        _lib.call("dpc_gemv", args, x.device)
        return out
    # operands the kernel does not take (unaligned rows, K % 8): the library product
    v = torch.mm(x, w.t()) if bias is None else torch.addmm(bias.to(x.dtype), x, w.t())
    if act:
        v = act_fwd_ref(v, act)
    if residual is not None:
        v = residual + v.to(residual.dtype)
    out[:, :Nw].copy_(v)
    if N > Nw:
        out[:, Nw:].zero_()
    return out


def linear_dgrad(dy, w, *, act_bwd=None, aux_in=None, out=None, out_dtype=torch.bfloat16,
                 alpha_t=None, colsum=None):
    """dx = (dy @ w) * act'(aux_in); dy [M, N], w [N, K] -> dx [M, K]; colsum += sum_m dx."""
    return gemm(dy, w, a_kmaj=True, b_kmaj=False, act_bwd=act_bwd, aux_in=aux_in, out=out,
                out_dtype=out_dtype, alpha_t=alpha_t, colsum=colsum)


def linear_wgrad(dy, x, *, out, accumulate=True, alpha_t=None):
    """dW (+)= dy^T @ x; dy [T, N], x [T, K] -> dW [N, K] (f32 gradient buffer)."""
    return gemm(dy, x, a_kmaj=False, b_kmaj=False, out=out, accumulate=accumulate,
                alpha_t=alpha_t)
