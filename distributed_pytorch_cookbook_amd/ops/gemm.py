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
               out_dtype=torch.bfloat16, aux_deriv=False, norm=None):
    """y = act(x @ w^T + bias) (+ residual); x [M, K], w [N, K] (nn.Linear layout).
    ``aux_out`` receives the pre-activation, or act'(pre-activation) with ``aux_deriv``.
    ``w`` a ``QWeight`` (fp8 weight bytes and per-row scales): ``dpc_gemm_wq8`` for up to 64 rows,
    ``ValueError`` for anything that kernel does not take; an ``MxWeight`` (MXFP4 bytes and block
    scales): ``dpc_gemm_wq4`` on the same terms, and no ``norm=``.
    ``norm=(gamma, beta, eps)``: x is the f32 residual stream and the product takes
    bf16(LayerNorm(x)) in the same launch (``dpc_ln_linear``, w bf16 or a ``QWeight``); operands
    that kernel does not take (``ln_linear_ok``) are a ``ValueError``, never two launches."""
    if norm is not None:
        if aux_out is not None:
            raise ValueError("linear_fwd (norm=): no aux_out")
        return _linear_fwd_ln(x, w, norm, bias, act_code(act), residual, out, out_dtype)
    if isinstance(w, QWeight):
        if aux_out is not None:
            raise ValueError("linear_fwd (fp8 weights): no aux_out")
        return _linear_fwd_wq8(x, w, bias, act_code(act), residual, out, out_dtype)
    if isinstance(w, MxWeight):
        if aux_out is not None:
            raise ValueError("linear_fwd (fp4 weights): no aux_out")
        return _linear_fwd_wq4(x, w, bias, act_code(act), residual, out, out_dtype)
    if x.is_cuda and aux_out is None and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16:
        M = x.shape[0]
        if M <= _GEMV_ROWS:
            return _linear_fwd_few_rows(x, w, bias, act_code(act), residual, out, out_dtype)
        N = w.shape[0] if out is None else out.shape[-1]
        if _SKINNY_NATIVE and M <= _SKINNY_ROWS and N <= _SKINNY_MAX_N:
            if out is None:
                out = torch.empty(M, w.shape[0], device=x.device, dtype=out_dtype)
            if _skinny_ok(x, w, bias, residual, out):
                return _linear_fwd_skinny(x, w, bias, act_code(act), residual, out, out_dtype)
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


# 17 .. _SKINNY_ROWS rows (decode at batch 17-64, blocks of draft tokens, chunked-prefill tails, the
# LM head on that many last rows): still a stream of the weights, but with enough rows per weight
# byte for the matrix cores -- csrc/skinny_gemm.hip: dpc_gemm_skinny, one workgroup per strip of
# NB output columns with its waves splitting K, the same fused epilogue as dpc_gemv.  The training
# dispatcher would give these products N / 256 workgroups.
_SKINNY_MAX_ROWS = 64  # what the kernel takes
# what linear_fwd sends it (docs/GENERATION.md, measured per shape on the MI355X): every row count
# the kernel takes, but no product wider than _SKINNY_MAX_N columns -- the LM head over the
# vocabulary gives the dispatcher 197 tiles, and from 32 (GPT-2 XL) or 48 (GPT-2 small) rows on
# the dispatcher is the faster of the two there
_SKINNY_ROWS = 64
_SKINNY_MAX_N = 32768
_SKINNY_NATIVE = os.environ.get("DPC_SKINNY", "1") == "1"  # 0: the dispatcher, as before (A/B only)
SKINNY_PLANS = ((16, 8), (32, 4))  # the instantiated (columns, waves) per workgroup


def skinny_plan(M: int, N: int, K: int, cus: int):
    """(NB, waves) of one workgroup of the skinny kernel, from the shape alone (a captured graph
    replays the same launch).  Every workgroup reads all of x (from L2), so a wider strip divides
    that traffic -- at NB = 16 and M = 64 it is four times the weight bytes -- but also the
    workgroup count: 32 columns while that still leaves a workgroup for every second one of ``cus``
    compute units (measured: GPT-2 XL's QKV and up-projection, 150 and 200 strips of 32, run 16
    to 22 % faster that way at every row count; GPT-2 small's up-projection, 96 strips, 19 %
    slower), else 16 columns, whose eight waves split K further."""
    nb, nw = SKINNY_PLANS[1]
    return (nb, nw) if 2 * -(-N // nb) >= cus else SKINNY_PLANS[0]


def _skinny_ok(x, w, bias, residual, out):
    return (x.dim() == 2 and w.dim() == 2 and out.dim() == 2 and 0 < w.shape[0] and w.shape[1] == x.shape[1]
            and out.shape[0] == x.shape[0] and out.dtype in (torch.float32, torch.bfloat16)
            and _gemv_ok(x, w, bias, residual, out, out.shape[1])
            and (residual is None or (residual.shape[0] >= x.shape[0] and residual.shape[1] >= w.shape[0])))


def _linear_fwd_skinny(x, w, bias, act, residual, out, out_dtype, plan=None):
    """``dpc_gemm_skinny`` on operands it takes (``_skinny_ok``; anything else raises).  ``plan``:
    one of SKINNY_PLANS instead of the planner's choice (tests, measurements)."""
    M, K = x.shape
    Nw = w.shape[0]
    if out is None:
        out = torch.empty(M, Nw, device=x.device, dtype=out_dtype)
    if not (0 < M <= _SKINNY_MAX_ROWS and _skinny_ok(x, w, bias, residual, out)):
        raise ValueError("linear_fwd (skinny): operands the kernel does not take")
    N = out.shape[1]
    nb, nw = plan or skinny_plan(M, N, K, torch.cuda.get_device_properties(x.device).multi_processor_count)
    args = _lib.SkinnyArgs(
        x=x.data_ptr(), w=w.data_ptr(), bias=_lib.ptr(bias), residual=_lib.ptr(residual),
        y=out.data_ptr(), ldx=x.stride(0), ldw=w.stride(0),
        ldr=residual.stride(0) if residual is not None else 0, ldy=out.stride(0),
        M=M, N=N, Nw=Nw, K=K, act=act, y_f32=int(out.dtype == torch.float32), nb=nb, nw=nw)
    _lib.call("dpc_gemm_skinny", args, x.device)
    return out


# Weight-only FP8 (e4m3) Linears of the decode step (csrc/wq_gemm.hip): the weight stream at one
# byte per element.  One f32 scale per output row, scale[n] = amax_k |w[n, k]| / 448 (1.0 for a row
# of zeros), byte = fp8_rne(clamp(float(w) * float32(1 / scale[n]), -448, 448)); the kernel widens
# the bytes to bf16 in registers (exact), runs the bf16 MFMA and applies scale[n] to the summed
# accumulator ahead of the bias.  dpc_gemm_wq8 takes every row count 1..64 and every width (the LM
# head included): there is no other path behind a QWeight.
FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0


class QWeight:
    """An fp8 weight: ``q`` [N, K] float8_e4m3fn, ``scale`` [N] f32, w ~ q * scale[:, None]."""
    __slots__ = ("q", "scale", "shape")

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        if q.dim() != 2 or q.dtype != FP8 or scale.dtype != torch.float32 or scale.shape != (q.shape[0],):
            raise ValueError("QWeight: q [N, K] float8_e4m3fn and scale [N] float32")
        self.q, self.scale, self.shape = q, scale, q.shape


def weight_scales(w: torch.Tensor):
    """(scale, inv) [N] f32 of ``quantize_weight``: amax / 448 per row (1.0 for a zero row) and its
    f32 reciprocal."""
    amax = w.abs().amax(dim=1).float()
    scale = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    return scale, 1.0 / scale


def weight_quantize_ref(w: torch.Tensor, inv: torch.Tensor) -> torch.Tensor:
    """The torch twin of ``dpc_wq_quantize``, bit for bit: ``ops/attention.py:kv_quantize_ref``'s
    expression with one ``inv`` per row."""
    return (w.float() * inv[:, None]).clamp(-FP8_MAX, FP8_MAX).to(FP8)


def _quantize_weight_fp8(w: torch.Tensor) -> QWeight:
    """``quantize_weight`` (below) with its default ``dtype="fp8"``."""
    if not (w.dim() == 2 and w.is_cuda and w.dtype == torch.bfloat16 and w.stride(1) == 1 and w.shape[1] % 16 == 0
            and w.shape[0] > 0 and w.stride(0) % 8 == 0 and w.stride(0) >= w.shape[1] and w.data_ptr() % 16 == 0):
        raise ValueError("quantize_weight: a CUDA bf16 [N, K] weight with K % 16 == 0 and 16-B aligned rows")
    N, K = w.shape
    scale, inv = weight_scales(w)
    q = torch.empty(N, K, device=w.device, dtype=FP8)
    _lib.call("dpc_wq_quantize", _lib.WqQuantArgs(w=w.data_ptr(), inv=inv.data_ptr(), q=q.data_ptr(),
                                                  ldw=w.stride(0), ldq=K, N=N, K=K), w.device)
    return QWeight(q, scale)


def _wq_ok(x, w, bias, residual, out):
    q = w.q
    return (x.dim() == 2 and out.dim() == 2 and x.is_cuda and q.is_cuda and x.dtype == torch.bfloat16
            and q.shape[1] == x.shape[1] and x.shape[1] % 16 == 0 and out.shape[0] == x.shape[0]
            and out.dtype in (torch.float32, torch.bfloat16) and x.stride(1) == 1 and q.stride(1) == 1
            and x.stride(0) % 8 == 0 and x.stride(0) >= x.shape[1] and q.stride(0) % 16 == 0
            and q.stride(0) >= q.shape[1] and x.data_ptr() % 16 == 0 and q.data_ptr() % 16 == 0
            and w.scale.is_cuda and w.scale.is_contiguous()
            and (bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() >= q.shape[0]))
            and (residual is None or (residual.dtype == torch.float32 and residual.stride(1) == 1
                                      and residual.shape[0] >= x.shape[0] and residual.shape[1] >= q.shape[0]))
            and out.stride(1) == 1 and 0 < q.shape[0] <= out.shape[1])


def _linear_fwd_wq8(x, w, bias, act, residual, out, out_dtype, plan=None):
    """``dpc_gemm_wq8`` (csrc/wq_gemm.hip) on a ``QWeight``; operands the kernel does not take raise.
    The plan is ``skinny_plan``'s, or ``plan``: one of SKINNY_PLANS (tests, measurements)."""
    M, K = x.shape
    Nw = w.shape[0]
    if M > _SKINNY_MAX_ROWS:
        raise ValueError(f"linear_fwd (fp8 weights): at most {_SKINNY_MAX_ROWS} rows, not {M}")
    if out is None:
        out = torch.empty(M, Nw, device=x.device, dtype=out_dtype)
    if not (M > 0 and _wq_ok(x, w, bias, residual, out)):
        raise ValueError("linear_fwd (fp8 weights): operands the kernel does not take (CUDA bf16 x, K % 16 == 0, "
                         "16-B aligned rows, f32 bias / residual)")
    N = out.shape[1]
    nb, nw = plan or skinny_plan(M, N, K, torch.cuda.get_device_properties(x.device).multi_processor_count)
    args = _lib.WqArgs(
        x=x.data_ptr(), q=w.q.data_ptr(), scale=w.scale.data_ptr(), bias=_lib.ptr(bias), residual=_lib.ptr(residual),
        y=out.data_ptr(), ldx=x.stride(0), ldw=w.q.stride(0),
        ldr=residual.stride(0) if residual is not None else 0, ldy=out.stride(0),
        M=M, N=N, Nw=Nw, K=K, act=act, y_f32=int(out.dtype == torch.float32), nb=nb, nw=nw)
    _lib.call("dpc_gemm_wq8", args, x.device)
    return out


# Weight-only MXFP4 Linears of the decode step (csrc/wq4_gemm.hip): the weight stream at half a byte
# per element.  OCP MXFP4: e2m1 elements (0, .5, 1, 1.5, 2, 3, 4, 6 and a sign), two per byte, and one
# e8m0 scale byte, 2^(byte - 127), per block of 32 consecutive k of a row.  mx_quantize_ref below is
# the definition of the format.  The kernel turns each byte and its block's scale into two bf16 by
# one convert, exactly, and runs the bf16 MFMA: activations are not quantised and no scale meets
# the accumulator.  dpc_gemm_wq4 takes every row count 1..64 and every width: there is no other
# path behind an MxWeight.
MX_BLOCK = 32
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
_E2M1_STEPS = ((0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False), (3.5, True), (5.0, False))


class MxWeight:
    """An MXFP4 weight: ``q`` [N, K / 2] uint8 (element 2j in the low nibble of byte j), ``scale``
    [N, K / 32] uint8 (e8m0), ``shape`` (N, K); w ~ ``mx_dequantize(q, scale)``."""
    __slots__ = ("q", "scale", "shape")

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        if (q.dim() != 2 or q.dtype != torch.uint8 or scale.dtype != torch.uint8 or q.shape[1] % (MX_BLOCK // 2)
                or scale.shape != (q.shape[0], q.shape[1] // (MX_BLOCK // 2))):
            raise ValueError("MxWeight: q [N, K / 2] uint8 and scale [N, K / 32] uint8, K % 32 == 0")
        self.q, self.scale, self.shape = q, scale, torch.Size((q.shape[0], 2 * q.shape[1]))


def mx_quantize_ref(w: torch.Tensor):
    """(q [N, K / 2] uint8, scale [N, K / 32] uint8) of a finite ``w`` [N, K], K % 32 == 0: the
    definition of the format and the torch twin of ``dpc_wq4_quantize``, bit for bit.  Per block of
    32 consecutive k of a row: the exponent e is the smallest integer with 6 * 2^e >= amax, read off
    frexp(amax) = (m, x) as x - 3 for m <= .75, else x - 2, clamped to [-125, 125] (every
    dequantised value is then a finite, normal bf16), 0 for a block of zeros; the scale byte is
    e + 127.  |w| * 2^-e is rounded to the nearest of the e2m1 magnitudes, ties to the even code
    (the compares of ``_E2M1_STEPS``), and saturates at 6 -- which only the upper clamp can reach;
    the sign goes in bit 3.  Element 2j sits in the low nibble of byte j, the order in which
    v_cvt_scalef32_pk_bf16_fp4's byte selector yields ascending k."""
    N, K = w.shape
    if K % MX_BLOCK:
        raise ValueError(f"mx_quantize_ref: K % {MX_BLOCK} == 0, not K = {K}")
    f = w.float().reshape(N, K // MX_BLOCK, MX_BLOCK)
    amax = f.abs().amax(dim=2)
    m, x = torch.frexp(amax)
    e = torch.where(amax > 0, x - torch.where(m <= 0.75, 3, 2), torch.zeros_like(x)).clamp(-125, 125)
    v = f.abs() * ((127 - e) << 23).to(torch.int32).view(torch.float32)[:, :, None]  # * 2^-e, exact
    code = torch.zeros_like(v, dtype=torch.int32)
    for t, closed in _E2M1_STEPS:
        code += (v >= t) if closed else (v > t)
    code = (code | (torch.signbit(f).to(torch.int32) << 3)).view(N, K // 2, 2)
    return (code[:, :, 0] | (code[:, :, 1] << 4)).to(torch.uint8), (e + 127).to(torch.uint8)


def mx_dequantize(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """[N, K] f32 of an MXFP4 weight: sign * e2m1 magnitude * 2^(scale - 127), exact."""
    N = q.shape[0]
    code = torch.stack((q & 0xF, q >> 4), dim=2).view(N, -1).long()
    mag = torch.tensor(_E2M1, device=q.device)[code & 7] * (1.0 - 2.0 * (code >> 3))
    s = (scale.to(torch.int32) << 23).view(torch.float32)
    return (mag.view(N, -1, MX_BLOCK) * s[:, :, None]).view(N, -1)


def quantize_weight(w: torch.Tensor, dtype: str = "fp8"):
    """``w`` [N, K] bf16 on the GPU with 16-B aligned rows, quantised for the few-row Linears.
    ``dtype="fp8"`` (K % 16 == 0): a ``QWeight``, the scales by torch (set-up, once per weight), the
    bytes by ``dpc_wq_quantize``.  ``dtype="fp4"`` (K % 32 == 0): an ``MxWeight``, codes and scales by
    ``dpc_wq4_quantize``."""
    if dtype == "fp8":
        return _quantize_weight_fp8(w)
    if dtype != "fp4":
        raise ValueError(f"quantize_weight: dtype must be 'fp8' or 'fp4', not {dtype!r}")
    if not (w.dim() == 2 and w.is_cuda and w.dtype == torch.bfloat16 and w.stride(1) == 1 and w.shape[1] % MX_BLOCK == 0
            and w.shape[0] > 0 and w.stride(0) % 8 == 0 and w.stride(0) >= w.shape[1] and w.data_ptr() % 16 == 0):
        raise ValueError("quantize_weight: a CUDA bf16 [N, K] weight with K % 32 == 0 and 16-B aligned rows")
    N, K = w.shape
    q = torch.empty(N, K // 2, device=w.device, dtype=torch.uint8)
    scale = torch.empty(N, K // MX_BLOCK, device=w.device, dtype=torch.uint8)
    _lib.call("dpc_wq4_quantize", _lib.Wq4QuantArgs(w=w.data_ptr(), q=q.data_ptr(), scale=scale.data_ptr(),
                                                    ldw=w.stride(0), ldq=K // 2, N=N, K=K), w.device)
    return MxWeight(q, scale)


def _wq4_ok(x, w, bias, residual, out):
    q, K = w.q, w.shape[1]
    return (x.dim() == 2 and out.dim() == 2 and x.is_cuda and q.is_cuda and x.dtype == torch.bfloat16
            and x.shape[1] == K and out.shape[0] == x.shape[0]
            and out.dtype in (torch.float32, torch.bfloat16) and x.stride(1) == 1 and q.stride(1) == 1
            and x.stride(0) % 8 == 0 and x.stride(0) >= K and q.stride(0) % 16 == 0
            and x.data_ptr() % 16 == 0 and q.data_ptr() % 16 == 0
            and w.scale.is_cuda and w.scale.is_contiguous()
            and (bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() >= q.shape[0]))
            and (residual is None or (residual.dtype == torch.float32 and residual.stride(1) == 1
                                      and residual.shape[0] >= x.shape[0] and residual.shape[1] >= q.shape[0]))
            and out.stride(1) == 1 and 0 < q.shape[0] <= out.shape[1])


def _linear_fwd_wq4(x, w, bias, act, residual, out, out_dtype, plan=None):
    """``dpc_gemm_wq4`` (csrc/wq4_gemm.hip) on an ``MxWeight``; operands the kernel does not take
    raise.  The plan is ``skinny_plan``'s, or ``plan``: one of SKINNY_PLANS (tests, measurements)."""
    M = x.shape[0]
    Nw, K = w.shape
    if M > _SKINNY_MAX_ROWS:
        raise ValueError(f"linear_fwd (fp4 weights): at most {_SKINNY_MAX_ROWS} rows, not {M}")
    if out is None:
        out = torch.empty(M, Nw, device=x.device, dtype=out_dtype)
    if not (M > 0 and _wq4_ok(x, w, bias, residual, out)):
        raise ValueError("linear_fwd (fp4 weights): operands the kernel does not take (CUDA bf16 x [M, K] with the "
                         "weight's K, 16-B aligned rows, f32 bias / residual)")
    N = out.shape[1]
    nb, nw = plan or skinny_plan(M, N, K, torch.cuda.get_device_properties(x.device).multi_processor_count)
    args = _lib.Wq4Args(
        x=x.data_ptr(), q=w.q.data_ptr(), scale=w.scale.data_ptr(), bias=_lib.ptr(bias), residual=_lib.ptr(residual),
        y=out.data_ptr(), ldx=x.stride(0), ldw=w.q.stride(0),
        ldr=residual.stride(0) if residual is not None else 0, ldy=out.stride(0),
        M=M, N=N, Nw=Nw, K=K, act=act, y_f32=int(out.dtype == torch.float32), nb=nb, nw=nw)
    _lib.call("dpc_gemm_wq4", args, x.device)
    return out


# LayerNorm fused into the Linear that consumes it (csrc/ln_linear.hip): every workgroup of the
# few-row split normalises the f32 rows into LDS as bf16 and reads its MFMA B operand from there,
# so LN + Linear is one launch.  The kernel takes up to _LN_LINEAR_MAX_ROWS rows while the image
# [M][K + pad] and the partials fit a workgroup's LDS.
_LN_LINEAR_MAX_ROWS = 32
_LN_LINEAR_LDS = 160 * 1024
# The row count up to which the one-token step uses it (models/fused.py:ln_linear_step), and the
# widest product it takes there.  0: the step keeps its separate LayerNorm launches.  Measured on
# the MI355X (docs/GENERATION.md): the graphed GPT-2 small step is 5.9 % (bf16 weights) and 2.9 %
# (e4m3) faster at batch 1 with the fused layers, the GPT-2 XL step 1.0 % and 0.8 % SLOWER, at a
# run-to-run spread of 0.1 %; the step changes only if it gains on both.  The LM head over the
# vocabulary loses as a single product at one row with either weight type: no width above
# LN_LINEAR_MAX_N is fused at any setting of the row count.
LN_LINEAR_ROWS = 0
LN_LINEAR_MAX_N = 32768


def _ln_image_ld(K: int) -> int:
    """Row stride of the LDS image in elements (ln_linear.hip:lnl_ld): an odd number of 16-B units."""
    return K + (8 if (K // 8) % 2 == 0 else 16)


def ln_linear_ok(M: int, K: int, w) -> bool:
    """Whether ``linear_fwd(x [M, K] f32, w, norm=...)`` takes these shapes (shapes and weight type
    only: alignment and the epilogue operands are checked at the call)."""
    fp8 = isinstance(w, QWeight)
    if not fp8 and not (torch.is_tensor(w) and w.dim() == 2 and w.dtype == torch.bfloat16):
        return False
    return (0 < M <= _LN_LINEAR_MAX_ROWS and K > 0 and K % (16 if fp8 else 8) == 0 and w.shape[1] == K
            and w.shape[0] > 0 and M * _ln_image_ld(K) * 2 + 8192 * -(-M // 16) <= _LN_LINEAR_LDS)


def _linear_fwd_ln(x, w, norm, bias, act, residual, out, out_dtype, plan=None):
    """``dpc_ln_linear`` (csrc/ln_linear.hip); operands the kernel does not take raise.  The plan is
    ``skinny_plan``'s, or ``plan``: one of SKINNY_PLANS (tests, measurements)."""
    gamma, beta, eps = norm
    fp8 = isinstance(w, QWeight)
    wt = w.q if fp8 else w
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 2 and x.dtype == torch.float32):
        raise ValueError("linear_fwd (norm=): x must be a CUDA f32 [M, K] tensor (the residual stream)")
    if not (fp8 or (torch.is_tensor(w) and w.dtype == torch.bfloat16)):
        raise ValueError("linear_fwd (norm=): w must be bf16 or a QWeight")
    M, K = x.shape
    if not 0 < M <= _LN_LINEAR_MAX_ROWS:
        raise ValueError(f"linear_fwd (norm=): 1 to {_LN_LINEAR_MAX_ROWS} rows, not {M}")
    if K % (16 if fp8 else 8) or wt.dim() != 2 or wt.shape[1] != K:
        raise ValueError(f"linear_fwd (norm=): K % {16 if fp8 else 8} == 0 and w [N, K], not K = {K}, w {tuple(wt.shape)}")
    if not ln_linear_ok(M, K, w):
        raise ValueError(f"linear_fwd (norm=): {M} rows of K = {K} do not fit the LDS image")
    Nw = wt.shape[0]
    if out is None:
        out = torch.empty(M, Nw, device=x.device, dtype=out_dtype)
    lw = 16 if fp8 else 8
    if not (x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.stride(0) >= K and x.data_ptr() % 16 == 0
            and wt.is_cuda and wt.stride(1) == 1 and wt.stride(0) % lw == 0 and wt.stride(0) >= K
            and wt.data_ptr() % 16 == 0 and (not fp8 or (w.scale.is_cuda and w.scale.is_contiguous()))
            and all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == K
                    and t.data_ptr() % 16 == 0 for t in (gamma, beta))
            and (bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() >= Nw))
            and (residual is None or (residual.dtype == torch.float32 and residual.stride(1) == 1
                                      and residual.shape[0] >= M and residual.shape[1] >= Nw))
            and out.dim() == 2 and out.shape[0] == M and out.stride(1) == 1 and Nw <= out.shape[1]
            and out.dtype in (torch.float32, torch.bfloat16)):
        raise ValueError("linear_fwd (norm=): operands the kernel does not take (16-B aligned rows, f32 gamma / beta "
                         "[K] / bias / residual, bf16 or f32 out)")
    N = out.shape[1]
    nb, nw = plan or skinny_plan(M, N, K, torch.cuda.get_device_properties(x.device).multi_processor_count)
    args = _lib.LnLinearArgs(
        x=x.data_ptr(), gamma=gamma.data_ptr(), beta=beta.data_ptr(), w=wt.data_ptr(),
        scale=w.scale.data_ptr() if fp8 else None, bias=_lib.ptr(bias), residual=_lib.ptr(residual),
        y=out.data_ptr(), ldx=x.stride(0), ldw=wt.stride(0),
        ldr=residual.stride(0) if residual is not None else 0, ldy=out.stride(0),
        M=M, N=N, Nw=Nw, K=K, eps=float(eps), act=act, y_f32=int(out.dtype == torch.float32), nb=nb, nw=nw)
    _lib.call("dpc_ln_linear", args, x.device)
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
