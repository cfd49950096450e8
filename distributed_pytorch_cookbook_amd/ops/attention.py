"""Causal self-attention core (softmax(q k^T * scale + masks) v) on the fused QKV buffer.

Semantics follow ``/root/reference/models/gpt.py:68-105``: causal mask (key j > query i
is excluded), optional key-padding mask (``True`` = padded key, excluded), softmax in
f32, output heads merged back to ``[T, H*hd]``.  One deliberate difference: a query row
whose every key is masked yields 0 here (the reference's finfo.min / -1e9 arithmetic
yields an ill-defined average); such rows occur for all-padding sequences and, under the
causal mask, for the queries inside a run of left padding.  For such a row every path
(bf16, f32, torch) gives o = +0 and lse = +inf, and the backward gives exact zeros for
its dq; dk and dv of a padded key are exact zeros too, however far its score lies above
the row's lse (the kernels select the zero, they do not multiply by it).
Precision of the f32 path: the forward sums each score q . k in f64 (one f32 rounding
per pair of products), so o stays within 1e-5 of its largest element of the f64 result
even when raw scores reach several hundred -- where plain f32 math, and this kernel
with one f32 accumulator, were 1e-5 to 4e-5 off.  It costs the f32 forward about 2 x
(tests/test_attention_scores_gpu.py and csrc/attention_f32.hip have the measurements).
The backward forms P from f32-accumulated scores; its gradients are held to 1e-4.

HIP path (bf16, head_dim 32, 64, 128 or 256 natively): ``dpc_attn_fwd`` / ``dpc_attn_bwd`` flash
kernels (``csrc/attention.hip``; 256 has kernels of its own there) -- O(S) memory, f32
log-sum-exp saved for the backward.
f32 operands (``--disable_amp``) run ``dpc_attn_fwd_f32`` / ``dpc_attn_bwd_f32``
(``csrc/attention_f32.hip``, f32 matrix cores; head_dim 32, 64 or 128), also O(S).
head_dim 32 is the reference default config (``/root/reference/main-single.py:160``); other
head sizes up to the dtype's largest kernel are zero-padded to the next kernel size on the way
in (16 -> 32, 48 -> 64, 96 -> 128, and for bf16 160 -> 256; the scale is the true head_dim's).
The reference's ``SelfAttention`` takes any ``--head_dim``
(``/root/reference/models/gpt.py:44-66``): bf16 sizes above 256 and f32 sizes above 128 run the
reference math on the device (O(S^2) memory, correct but slow) rather than refusing.
The fp8 KV cache and ``append_attention`` have kernels at 32, 64 and 128 only (``HD_KERNELS``).
CPU / fp32 path: the same math with torch ops (test oracle).
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib

HD_KERNELS = (32, 64, 128)  # every dtype and kernel family: f32, the fp8 cache, append attention
HD_KERNEL = 128  # the largest
HD_KERNELS_BF16 = HD_KERNELS + (256,)  # the bf16 flash forward / backward only


def kernel_head_dim(head_dim: int, dtype: torch.dtype | None = None) -> int | None:
    """The kernel size a head of ``head_dim`` runs at (itself for 32 / 64 / 128, and 256 for
    bf16; else padded up); None above the largest kernel of ``dtype`` (the device then runs the
    reference math)."""
    for k in (HD_KERNELS_BF16 if dtype == torch.bfloat16 else HD_KERNELS):
        if head_dim <= k:
            return k
    return None


def _use_hip(t: torch.Tensor, head_dim: int | None = None) -> bool:
    """bf16 -> csrc/attention.hip; f32 (--disable_amp) -> csrc/attention_f32.hip; head sizes
    past the dtype's largest kernel -> the reference math (on whatever device ``t`` is on)."""
    if head_dim is not None and kernel_head_dim(head_dim, t.dtype) is None:
        return False
    return t.is_cuda and t.dtype in (torch.bfloat16, torch.float32)


def _suffix(t: torch.Tensor) -> str:
    return "_f32" if t.dtype == torch.float32 else ""


def _check_span(t: torch.Tensor, S: int, *lds: int) -> None:
    """The bf16 kernels address one sequence's rows with 32-bit offsets (attention.hip:rows_rsrc):
    (S + 256) rows of every strided operand must span < 4 GiB."""
    if t.dtype != torch.float32 and (S + 256) * max(lds) * t.element_size() >= 0xFFFFFFFF:
        raise ValueError(f"attention: one sequence's rows span >= 4 GiB (S={S}, row strides {lds}); "
                         "split the sequence or run the reference path")


def split_qkv(qkv: torch.Tensor, heads: int, head_dim: int):
    """Views q, k, v [T, H*hd] out of the fused [T, 3*H*hd] projection."""
    hd = heads * head_dim
    return qkv[:, :hd], qkv[:, hd:2 * hd], qkv[:, 2 * hd:]


def attention_ref(qkv, N, S, heads, head_dim, pad_mask=None, causal=True, scale=None):
    """Reference math; returns (o [T, H*hd] in qkv.dtype, lse [N*H, S] f32)."""
    scale = 1.0 / math.sqrt(head_dim) if scale is None else scale
    q, k, v = split_qkv(qkv, heads, head_dim)
    q = q.float().reshape(N, S, heads, head_dim).transpose(1, 2)
    k = k.float().reshape(N, S, heads, head_dim).transpose(1, 2)
    v = v.float().reshape(N, S, heads, head_dim).transpose(1, 2)
    s = (q @ k.transpose(-1, -2)) * scale
    allowed = torch.ones(S, S, dtype=torch.bool, device=qkv.device)
    if causal:
        allowed = torch.tril(allowed)
    allowed = allowed.expand(N, 1, S, S)
    if pad_mask is not None:
        allowed = allowed & ~pad_mask.bool()[:, None, None, :]
    s = s.masked_fill(~allowed, float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p = torch.where(l > 0, e / l.clamp_min(1e-30), torch.zeros_like(e))
    o = (p @ v).transpose(1, 2).reshape(N * S, heads * head_dim)
    lse = torch.where(l > 0, m + torch.log(l.clamp_min(1e-30)), torch.full_like(l, float("inf")))
    return o.to(qkv.dtype), lse.reshape(N * heads, S)


def _pad_heads(x: torch.Tensor, T: int, heads: int, head_dim: int, kd: int) -> torch.Tensor:
    """[T, H*hd] (strided view ok) -> contiguous [T, H*kd] with zero padding."""
    out = torch.zeros(T, heads, kd, device=x.device, dtype=x.dtype)
    out[:, :, :head_dim] = x.reshape(T, heads, head_dim)
    return out.reshape(T, heads * kd)


def attention_fwd(qkv: torch.Tensor, N: int, S: int, heads: int, head_dim: int,
                  pad_mask: torch.Tensor | None = None, causal: bool = True,
                  out: torch.Tensor | None = None):
    """qkv [T = N*S, 3*H*hd] -> (o [T, H*hd], lse [N*H, S] f32)."""
    T = N * S
    if not _use_hip(qkv, head_dim):
        o, lse = attention_ref(qkv, N, S, heads, head_dim, pad_mask, causal)
        if out is not None:
            out.copy_(o)
            o = out
        return o, lse
    scale = 1.0 / math.sqrt(head_dim)
    kd = kernel_head_dim(head_dim, qkv.dtype)
    if head_dim != kd:
        q, k, v = split_qkv(qkv, heads, head_dim)
        qkv_p = torch.cat([_pad_heads(t, T, heads, head_dim, kd) for t in (q, k, v)], dim=1)
        o_p, lse = _attn_fwd_hip(qkv_p, N, S, heads, kd, pad_mask, causal, scale, None)
        o = o_p.reshape(T, heads, kd)[:, :, :head_dim].reshape(T, heads * head_dim)
        if out is not None:
            out.copy_(o)
            o = out
        return o.contiguous() if out is None else o, lse
    return _attn_fwd_hip(qkv, N, S, heads, kd, pad_mask, causal, scale, out)


def _check(t, T, cols, name, dtype=torch.bfloat16):
    if t.shape[0] != T or t.stride(1) != 1 or t.dtype != dtype:
        raise ValueError(f"attention: bad {name} {tuple(t.shape)} {t.stride()} {t.dtype}")
    if t.data_ptr() % 16 or t.stride(0) % (16 // t.element_size()) or t.shape[1] < cols:
        raise ValueError(f"attention: {name} must be 16-B aligned with 16-B aligned rows")


def _attn_fwd_hip(qkv, N, S, heads, kd, pad_mask, causal, scale, out):
    T = N * S
    hd = heads * kd
    dt = qkv.dtype
    _check(qkv, T, 3 * hd, "qkv", dt)
    if out is None:
        out = torch.empty(T, hd, device=qkv.device, dtype=dt)
    _check(out, T, hd, "out", dt)
    lse = torch.empty(N * heads, S, device=qkv.device, dtype=torch.float32)
    pad = None
    if pad_mask is not None:
        pad = pad_mask.to(torch.uint8).contiguous()
        assert pad.shape == (N, S)
    q, k, v = split_qkv(qkv, heads, kd)
    args = _lib.AttnArgs(
        q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), o=out.data_ptr(), lse=lse.data_ptr(),
        pad=_lib.ptr(pad), ld_qkv=qkv.stride(0), ld_o=out.stride(0), ld_dqkv=0,
        N=N, S=S, H=heads, scale=float(scale), causal=int(causal), hd=kd,
    )
    _check_span(qkv, S, qkv.stride(0), out.stride(0))
    _lib.call("dpc_attn_fwd" + _suffix(qkv), args, qkv.device)
    return out, lse


def attention_bwd(dout: torch.Tensor, qkv: torch.Tensor, o: torch.Tensor, lse: torch.Tensor,
                  N: int, S: int, heads: int, head_dim: int,
                  pad_mask: torch.Tensor | None = None, causal: bool = True,
                  dqkv: torch.Tensor | None = None) -> torch.Tensor:
    """Gradient w.r.t. the fused qkv buffer: returns dqkv [T, 3*H*hd] (qkv dtype)."""
    T = N * S
    if not _use_hip(qkv, head_dim):
        with torch.enable_grad():
            x = qkv.detach().float().requires_grad_(True)
            o_ref, _ = attention_ref(x, N, S, heads, head_dim, pad_mask, causal)
            (g,) = torch.autograd.grad(o_ref, x, dout.float())
        if dqkv is not None:
            dqkv.copy_(g)
            return dqkv
        return g.to(qkv.dtype)
    scale = 1.0 / math.sqrt(head_dim)
    kd = kernel_head_dim(head_dim, qkv.dtype)
    if head_dim != kd:
        q, k, v = split_qkv(qkv, heads, head_dim)
        qkv_p = torch.cat([_pad_heads(t, T, heads, head_dim, kd) for t in (q, k, v)], dim=1)
        o_p = _pad_heads(o, T, heads, head_dim, kd)
        do_p = _pad_heads(dout, T, heads, head_dim, kd)
        g_p = _attn_bwd_hip(do_p, qkv_p, o_p, lse, N, S, heads, kd, pad_mask, causal, scale, None)
        g = g_p.reshape(T, 3, heads, kd)[..., :head_dim].reshape(T, 3 * heads * head_dim)
        if dqkv is not None:
            dqkv.copy_(g)
            return dqkv
        return g.contiguous()
    return _attn_bwd_hip(dout, qkv, o, lse, N, S, heads, kd, pad_mask, causal, scale, dqkv)


def _attn_bwd_hip(dout, qkv, o, lse, N, S, heads, kd, pad_mask, causal, scale, dqkv):
    T = N * S
    hd = heads * kd
    dt = qkv.dtype
    dout = dout.to(dt)
    _check(qkv, T, 3 * hd, "qkv", dt)
    _check(o, T, hd, "o", dt)
    _check(dout, T, hd, "dout", dt)
    if o.stride(0) != dout.stride(0):
        dout = dout.contiguous()
        o = o.contiguous()
        if o.stride(0) != dout.stride(0):
            raise ValueError("attention_bwd: o and dout need equal row strides")
    if dqkv is None:
        dqkv = torch.empty(T, 3 * hd, device=qkv.device, dtype=dt)
    _check(dqkv, T, 3 * hd, "dqkv", dt)
    # [delta | lse in log2 units] rows (the dQ kernel writes both, the dK / dV kernel reads them)
    delta = torch.empty(2, N * heads, S, device=qkv.device, dtype=torch.float32)
    pad = None
    if pad_mask is not None:
        pad = pad_mask.to(torch.uint8).contiguous()
    q, k, v = split_qkv(qkv, heads, kd)
    dq, dk, dv = split_qkv(dqkv, heads, kd)
    args = _lib.AttnArgs(
        q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), o=o.data_ptr(), lse=lse.data_ptr(),
        pad=_lib.ptr(pad), dout=dout.data_ptr(), dq=dq.data_ptr(), dk=dk.data_ptr(),
        dv=dv.data_ptr(), delta=delta.data_ptr(),
        ld_qkv=qkv.stride(0), ld_o=o.stride(0), ld_dqkv=dqkv.stride(0),
        N=N, S=S, H=heads, scale=float(scale), causal=int(causal), hd=kd,
    )
    _check_span(qkv, S, qkv.stride(0), o.stride(0))
    _lib.call("dpc_attn_bwd" + _suffix(qkv), args, qkv.device)
    return dqkv


DECODE_MAX_S = 16384  # csrc/decode.hip (the one-workgroup kernel): LDS score buffer
DECODE_MAX_SPLITS = 64  # csrc/decode_split.hip: DS_MAX_SPLITS
# the fewest keys of cache capacity worth a workgroup of the split kernel (docs/GENERATION.md has
# the measurement); at least 160, so that caches of up to 319 rows plan one split
DECODE_SPLIT_MIN_KEYS = 256


def decode_supported(head_dim: int) -> bool:
    """Head sizes the decode kernels take (16-B chunks of a row, at most 32 per row)."""
    return head_dim > 0 and head_dim % 8 == 0 and head_dim <= 256


def decode_splits(N: int, H: int, Smax: int, cus: int) -> int:
    """How many workgroups share one (sequence, head)'s keys: enough to give each of ``cus``
    compute units one, with at least DECODE_SPLIT_MIN_KEYS of the cache capacity each."""
    want = -(-cus // max(1, N * H))
    return max(1, min(want, Smax // DECODE_SPLIT_MIN_KEYS, DECODE_MAX_SPLITS))


def decode_split_keys_per_pass(head_dim: int) -> int:
    """Keys one workgroup of the split kernel covers per pass; a split's range starts at a
    multiple of it (``csrc/decode_split.hip``)."""
    return int(_lib.lib().dpc_decode_split_keys_per_pass(int(head_dim)))


FP8 = torch.float8_e4m3fn  # the 1-byte KV cache's element (OCP e4m3, what gfx950 converts in hardware)
FP8_MAX = 448.0


def decode_fp8_keys_per_pass(head_dim: int) -> int:
    """``decode_split_keys_per_pass`` of the fp8 kernel (a key row takes hd / 16 lanes)."""
    return int(_lib.lib().dpc_decode_fp8_keys_per_pass(int(head_dim)))


def kv_fp8_supported(head_dim: int) -> bool:
    """Head sizes with an fp8-cache decode and append kernel."""
    return head_dim in HD_KERNELS


def kv_quantize_ref(x: torch.Tensor, scale: float) -> torch.Tensor:
    """The torch twin of the kernels' quantisation, bit for bit: the f32 product with
    float32(1 / scale), clamped to +-448 ahead of the convert (e4m3fn has no infinity: an
    overflowing convert gives NaN), rounded to nearest even."""
    inv = torch.tensor(1.0 / scale, dtype=torch.float32, device=x.device)
    return (x.float() * inv).clamp(-FP8_MAX, FP8_MAX).to(FP8)


def _kv_scales(k_scale, v_scale, what):
    k_scale, v_scale = float(k_scale), float(v_scale)
    if not (math.isfinite(k_scale) and math.isfinite(v_scale) and k_scale > 0 and v_scale > 0):
        raise ValueError(f"{what}: k_scale and v_scale must be positive and finite")
    return dict(k_scale=k_scale, k_inv=1.0 / k_scale, v_scale=v_scale, v_inv=1.0 / v_scale)


def _check_fp8(what, qkv, kc, vc, N, Smax, E, head_dim, length):
    """An fp8 cache pair takes CUDA bf16 qkv and the bf16 kernels' layout at head_dim 32 / 64 / 128;
    there is no torch path."""
    if kc.dtype != vc.dtype:
        raise ValueError(f"{what}: kc and vc must share a dtype")
    if not (qkv.is_cuda and qkv.dtype == torch.bfloat16 and kc.is_cuda and vc.is_cuda):
        raise ValueError(f"{what}: an fp8 cache needs CUDA bf16 qkv")
    if (qkv.stride(1) != 1 or kc.shape != (N, Smax, E) or vc.shape != kc.shape or not kc.is_contiguous()
            or not vc.is_contiguous() or not kv_fp8_supported(head_dim) or qkv.stride(0) % 8
            or qkv.data_ptr() % 16 or kc.data_ptr() % 16 or vc.data_ptr() % 16
            or length.dtype != torch.int64 or not length.is_cuda):
        raise ValueError(f"{what}: unsupported layout")


def kv_cache_store_fp8(qkv, kc, vc, length, n, heads, head_dim, per_seq=False, k_scale=1.0, v_scale=1.0):
    """The k and v columns of ``n`` rows per sequence of qkv [N*n, 3*H*hd] (bf16) quantised into the
    fp8 cache rows ``length[s] + i`` (``length`` device int64 [1], or [N] with ``per_seq``; rows at
    or past S_max are not written): ``dpc_kv_store_fp8`` (``csrc/append_attn.hip``).  The stored
    byte is ``kv_quantize_ref``'s."""
    N, Smax, E = kc.shape[0], kc.shape[1], heads * head_dim
    if kc.dtype != FP8 or vc.dtype != FP8:
        raise ValueError("kv_cache_store_fp8: kc and vc must be float8_e4m3fn")
    if length.numel() != (N if per_seq else 1) or qkv.shape[0] != N * n or qkv.shape[1] < 3 * E:
        raise ValueError("kv_cache_store_fp8: qkv must hold n rows of 3*H*hd per sequence, length [N] or [1]")
    _check_fp8("kv_cache_store_fp8", qkv, kc, vc, N, Smax, E, head_dim, length)
    _lib.call("dpc_kv_store_fp8", _lib.AppendAttnFp8Args(
        qkv=qkv.data_ptr(), kc=kc.data_ptr(), vc=vc.data_ptr(), len=length.data_ptr(), ldqkv=qkv.stride(0),
        N=N, n=n, H=heads, hd=head_dim, Smax=Smax, per_seq=int(bool(per_seq)), nsplit=1,
        **_kv_scales(k_scale, v_scale, "kv_cache_store_fp8")), qkv.device)


def decode_attention(qkv, kc, vc, length, heads, head_dim, scale=None, per_seq=False, splits=None,
                     k_scale=1.0, v_scale=1.0):
    """One new token per sequence against a KV cache: appends its key / value at
    ``length`` (device int64 [1], cached tokens so far) and returns o [N, H*hd].
    ``per_seq``: ``length`` is int64 [N], one per sequence (a ragged batch); a sequence whose
    cache is full (``length[n] >= S_max``) appends nothing and gets a zero output row.

    qkv [N, 3*H*hd]; kc, vc [N, S_max, H*hd].  HIP path, the length read on the device so that
    the call can be graph-captured: ``decode_splits`` workgroups per (sequence, head) over
    contiguous key ranges, partials combined by a second launch (``dpc_decode_attn_split``,
    ``csrc/decode_split.hip``; any ``S_max``); a plan of one split with ``S_max <= DECODE_MAX_S``
    runs ``dpc_decode_attn`` (``csrc/decode.hip``).  ``splits``: that many splits of the split
    kernel, 1 included (tests, timing); the torch path ignores it.

    An fp8 cache (``kc``, ``vc`` float8_e4m3fn; CUDA bf16 qkv, head_dim 32, 64 or 128) holds
    ``x / scale`` per tensor (``k_scale``, ``v_scale``): the new row is stored quantised
    (``kv_quantize_ref``) and takes part as stored, so the result is the softmax over the
    dequantised cache as it stands after the write.  It always runs the split kernel's fp8 twin
    (``dpc_decode_attn_split_fp8``), a plan of one split included; there is no torch path.
    """
    scale = 1.0 / math.sqrt(head_dim) if scale is None else scale
    N, E = qkv.shape[0], heads * head_dim
    Smax = kc.shape[1]
    if length.numel() != (N if per_seq else 1):
        raise ValueError("decode_attention: length must be [N] with per_seq, [1] without")
    if kc.dtype == FP8 or vc.dtype == FP8:
        _check_fp8("decode_attention", qkv, kc, vc, N, Smax, E, head_dim, length)
        plan = int(splits) if splits is not None else decode_splits(
            N, heads, Smax, torch.cuda.get_device_properties(qkv.device).multi_processor_count)
        if not 1 <= plan <= DECODE_MAX_SPLITS:
            raise ValueError("decode_attention: unsupported layout")
        o = torch.empty(N, E, device=qkv.device, dtype=torch.bfloat16)
        ws = torch.empty(N * heads * plan * (head_dim + 2), device=qkv.device, dtype=torch.float32) if plan > 1 else None
        _lib.call("dpc_decode_attn_split_fp8", _lib.DecodeSplitFp8Args(
            qkv=qkv.data_ptr(), kc=kc.data_ptr(), vc=vc.data_ptr(), o=o.data_ptr(), len=length.data_ptr(),
            ldqkv=qkv.stride(0), ldo=E, N=N, H=heads, hd=head_dim, Smax=Smax, scale=scale,
            per_seq=int(bool(per_seq)), ws=_lib.ptr(ws), nsplit=plan,
            **_kv_scales(k_scale, v_scale, "decode_attention")), qkv.device)
        return o
    if not (qkv.is_cuda and qkv.dtype == torch.bfloat16):
        if per_seq:
            o = torch.zeros(N, E, device=qkv.device, dtype=qkv.dtype)
            for n, pos in enumerate(length.tolist()):
                if 0 <= pos < Smax:
                    o[n:n + 1] = decode_attention(qkv[n:n + 1], kc[n:n + 1], vc[n:n + 1], length[n:n + 1],
                                                  heads, head_dim, scale)
            return o
        pos = int(length)
        q, k, v = split_qkv(qkv, heads, head_dim)
        kc[:, pos] = k
        vc[:, pos] = v
        qf = q.float().reshape(N, heads, 1, head_dim)
        kf = kc[:, :pos + 1].float().reshape(N, pos + 1, heads, head_dim).transpose(1, 2)
        vf = vc[:, :pos + 1].float().reshape(N, pos + 1, heads, head_dim).transpose(1, 2)
        p = torch.softmax((qf @ kf.transpose(-1, -2)) * scale, -1)
        return (p @ vf).reshape(N, E).to(qkv.dtype)
    if splits is None:
        plan = decode_splits(N, heads, Smax, torch.cuda.get_device_properties(qkv.device).multi_processor_count)
        split_kernel = plan > 1 or Smax > DECODE_MAX_S
    else:
        plan, split_kernel = int(splits), True
    if (qkv.stride(1) != 1 or kc.shape != (N, Smax, E) or vc.shape != kc.shape or not kc.is_contiguous()
            or not vc.is_contiguous() or kc.dtype != torch.bfloat16 or vc.dtype != torch.bfloat16
            or not decode_supported(head_dim) or not 1 <= plan <= DECODE_MAX_SPLITS
            or qkv.stride(0) % 8 or qkv.data_ptr() % 16 or length.dtype != torch.int64):
        raise ValueError("decode_attention: unsupported layout")
    o = torch.empty(N, E, device=qkv.device, dtype=torch.bfloat16)
    common = dict(qkv=qkv.data_ptr(), kc=kc.data_ptr(), vc=vc.data_ptr(), o=o.data_ptr(),
                  len=length.data_ptr(), ldqkv=qkv.stride(0), ldo=E, N=N, H=heads,
                  hd=head_dim, Smax=Smax, scale=scale, per_seq=int(bool(per_seq)))
    if not split_kernel:
        _lib.call("dpc_decode_attn", _lib.DecodeAttnArgs(**common), qkv.device)
        return o
    # the partials live like o: allocated per call, so a capture keeps them in the graph's pool
    ws = torch.empty(N * heads * plan * (head_dim + 2), device=qkv.device, dtype=torch.float32) if plan > 1 else None
    _lib.call("dpc_decode_attn_split", _lib.DecodeSplitArgs(ws=_lib.ptr(ws), nsplit=plan, **common), qkv.device)
    return o


APPEND_MAX_SPLITS = 64  # csrc/append_attn.hip: APPEND_MAX_SPLITS
APPEND_SPLIT_MIN_TILES = 4  # the fewest key tiles of cache capacity worth a workgroup of their own


def append_attn_tiles(head_dim: int = 64):
    """(QB, KT) of ``csrc/append_attn.hip``: query rows per workgroup and keys per tile; a split's
    range starts at a multiple of KT."""
    qb, kt = ctypes.c_int(), ctypes.c_int()
    _lib.lib().dpc_append_attn_tiles(int(head_dim), ctypes.byref(qb), ctypes.byref(kt))
    return qb.value, kt.value


def append_splits(N: int, H: int, n: int, Smax: int, cus: int) -> int:
    """How many workgroups share the keys of one query tile of one (sequence, head): 1 when the
    query tiles alone give each of ``cus`` compute units a workgroup, else enough to, with at least
    APPEND_SPLIT_MIN_TILES key tiles of the cache capacity each.  Planned from the capacity, never
    from the device length: the launch shape is the same on every replay."""
    qb, kt = append_attn_tiles()
    wgs = max(1, N * H * -(-n // qb))
    want = -(-cus // wgs)
    return max(1, min(want, -(-Smax // kt) // APPEND_SPLIT_MIN_TILES, APPEND_MAX_SPLITS))


def _append_torch(qkv, kc, vc, start, n, heads, head_dim, scale):
    """The materialised path at one shared ``start`` (host int): f32 scores [N, H, m, start + m] over
    the up-cast cache prefix, m = the new tokens that fit the capacity; the rest get zero rows."""
    N, Smax, E = kc.shape
    o = torch.zeros(N, n, E, device=qkv.device, dtype=qkv.dtype)
    m = min(n, Smax - start) if 0 <= start < Smax else 0
    if m <= 0:
        return o.reshape(N * n, E)
    L = start + m
    q3 = qkv[:, :3 * E].reshape(N, n, 3, E)[:, :m]  # (qkv may be wider than 3 E, or strided)
    kc[:, start:L] = q3[:, :, 1]
    vc[:, start:L] = q3[:, :, 2]
    q = q3[:, :, 0].float().reshape(N, m, heads, head_dim).transpose(1, 2)   # [N, H, m, hd]
    k = kc[:, :L].float().reshape(N, L, heads, head_dim).transpose(1, 2)     # [N, H, L, hd]
    v = vc[:, :L].float().reshape(N, L, heads, head_dim).transpose(1, 2)
    sc = (q @ k.transpose(-1, -2)) * scale                                   # [N, H, m, L]
    qi = torch.arange(m, device=qkv.device)[:, None] + start                 # query i sees keys <= start + i
    sc = sc.masked_fill(torch.arange(L, device=qkv.device)[None, :] > qi, float("-inf"))
    o[:, :m] = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(N, m, E).to(qkv.dtype)
    return o.reshape(N * n, E)


def append_attention(qkv, kc, vc, length, n, heads, head_dim, scale=None, per_seq=False, splits=None,
                     k_scale=1.0, v_scale=1.0):
    """A block of ``n`` new tokens per sequence against a KV cache that may already hold tokens:
    token i of sequence s sits at position p = length[s] + i (``length`` device int64 [1], or [N]
    with ``per_seq``); its key / value go to cache row p and its output row is the softmax over
    cache rows 0..p.  A token with p >= S_max is not written and gets a zero row.  ``length`` is
    not advanced.  Returns o [N*n, H*hd].

    qkv [N*n, 3*H*hd] token-major; kc, vc [N, S_max, H*hd].  HIP path (CUDA bf16, head_dim 32, 64
    or 128): ``dpc_append_attn`` (``csrc/append_attn.hip``), the length read on the device so that
    the call can be graph-captured; ``append_splits`` workgroups share the keys of a query tile,
    their partials combined by a further launch.  ``splits``: that many, 1 included (tests, timing).
    Anything else runs the materialised torch path, which reads the length on the host.

    An fp8 cache (float8_e4m3fn, ``k_scale`` / ``v_scale`` as in ``decode_attention``): the block's
    rows are stored quantised first (``dpc_append_attn_fp8``) and every key, the block's own
    included, is read back from the cache; HIP only."""
    scale = 1.0 / math.sqrt(head_dim) if scale is None else scale
    N, Smax, E = kc.shape[0], kc.shape[1], heads * head_dim
    if length.numel() != (N if per_seq else 1):
        raise ValueError("append_attention: length must be [N] with per_seq, [1] without")
    if qkv.shape[0] != N * n or qkv.shape[1] < 3 * E:
        raise ValueError("append_attention: qkv must hold n rows of 3*H*hd per sequence")
    if not scale > 0:  # the kernel takes the tile maximum on raw scores and scales it afterwards
        raise ValueError("append_attention: scale must be positive")
    fp8 = kc.dtype == FP8 or vc.dtype == FP8
    if fp8:
        _check_fp8("append_attention", qkv, kc, vc, N, Smax, E, head_dim, length)
    if not (qkv.is_cuda and qkv.dtype == torch.bfloat16 and head_dim in HD_KERNELS):
        if not per_seq:
            return _append_torch(qkv, kc, vc, int(length), n, heads, head_dim, scale)
        rows = qkv[:, :3 * E].reshape(N, n, 3 * E)
        return torch.cat([_append_torch(rows[s], kc[s:s + 1], vc[s:s + 1], pos, n, heads, head_dim, scale)
                          for s, pos in enumerate(length.tolist())])
    if splits is None:
        plan = append_splits(N, heads, n, Smax, torch.cuda.get_device_properties(qkv.device).multi_processor_count)
    else:
        plan = int(splits)
    if (qkv.stride(1) != 1 or kc.shape != (N, Smax, E) or vc.shape != kc.shape
            or not kc.is_contiguous() or not vc.is_contiguous() or kc.dtype != (FP8 if fp8 else torch.bfloat16)
            or vc.dtype != kc.dtype or not 1 <= plan <= APPEND_MAX_SPLITS or N * heads > 65535
            or qkv.stride(0) % 8 or qkv.data_ptr() % 16 or length.dtype != torch.int64 or not length.is_cuda):
        raise ValueError("append_attention: unsupported layout")
    o = torch.empty(N * n, E, device=qkv.device, dtype=torch.bfloat16)
    # the partials live like o: allocated per call, so a capture keeps them in the graph's pool
    ws = torch.empty(N * n * heads * plan * (head_dim + 4), device=qkv.device, dtype=torch.float32) if plan > 1 else None
    common = dict(qkv=qkv.data_ptr(), kc=kc.data_ptr(), vc=vc.data_ptr(), o=o.data_ptr(), len=length.data_ptr(),
                  ldqkv=qkv.stride(0), ldo=E, N=N, n=n, H=heads, hd=head_dim, Smax=Smax, scale=scale,
                  per_seq=int(bool(per_seq)), ws=_lib.ptr(ws), nsplit=plan)
    if fp8:
        _lib.call("dpc_append_attn_fp8", _lib.AppendAttnFp8Args(
            **common, **_kv_scales(k_scale, v_scale, "append_attention")), qkv.device)
    else:
        _lib.call("dpc_append_attn", _lib.AppendAttnArgs(**common), qkv.device)
    return o
