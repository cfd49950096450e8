"""Checks that see what a kernel gets wrong at its edges (no fixtures; used on CPU and GPU).

* ``guarded`` / ``assert_guards_intact``: an output view inside a larger buffer of sentinel bits;
  anything a kernel writes outside the view (before it, after it, or in the gap after a row when
  the leading dimension is larger than the row) changes the sentinel and is reported.
* ``row_col_err`` / ``assert_local_close``: the worst per-row and per-column relative error
  instead of one Frobenius ratio over the whole output, with a tolerance measured inside the
  test from an *ideal* kernel (plain f32 PyTorch on the same rounded inputs, rounded to the
  output dtype) against the f64 reference -- never from the code under test.
* ``gemm_elem_bound``: an analytic per-element bound for f32-accumulated products.
* ``observed`` / ``KERNEL_CHECKS_REPORT``: how much of each tolerance a run used (see below).
"""
from __future__ import annotations

import atexit
import json
import math
import os

import torch

# margins of assert_local_close (x the ideal kernel's own worst row / column error)
MARGIN = 2.0       # GEMM, LayerNorm, cross-entropy, elementwise: summation order only
MARGIN_ATTN = 3.0  # flash attention rounds P to bf16 (measured 1.3x the ideal floor)
# dk on the score cases of tests/attn_cases.py only (test_attention_scores_gpu.py; MARGIN_ATTN holds
# everywhere else, the other checks of that file included: measured there 2.0 x fwd, 2.2 x dq,
# 1.8 x dv).  The backward rounds dS to bf16 as the MFMA operand of dK^T += Q^T dS
# (attention.hip: acc_frag(dp, ss)); the ideal kernel keeps it in f32.  The cases' q has one
# coordinate at 16, 32 x its others, so that column of dk collects every query's dS rounding at
# weight 16 while the row's other columns stay small.  Plain f32 math from the IDEAL's o and lse
# with nothing but dS rounded to bf16 gives the kernel's figure (worst dk row 2.3e-2 / 1.6e-2 /
# 1.4e-2 against the kernel's 2.6e-2 / 1.6e-2 / 1.3e-2 at rising 5 hd 32 S 576, falling 12 hd 32
# S 320, rising 5 hd 64 S 320 causal; ideal floor 4e-3).  Per element the worst case is the spike
# key's column 0 (|dk| = 133, where bf16 steps by 1.0: the ideal's own error 0.21 is under the
# half ulp; the kernel's f32 value is off by 0.8 through delta = rowsum(dO o) from its own o, whose
# P for the one dominant key was rounded to bf16 at up to 2^3 against a kept max).
# Measured on the MI355X over the 96 cases: 6.95 x the ideal's worst row, 5.83 x its largest
# element error; the constants are those x 1.5.
MARGIN_ATTN_DK_ROWS = 10.4
MARGIN_ATTN_DK_ELEM = 8.7
# dq and dk of the f32 attention at the edge lengths (test_gemm_forms_gpu.py: test_attention_f32_edges;
# its forward measured 0.78 x and dv 1.82 x the ideal floor, inside MARGIN).  attention_f32.hip's
# forward sums its scores in f64, so the o and lse it hands the backward are those of the exact
# scores, while the backward forms the scores again with one f32 accumulator over head_dim and
# P = exp2(s c - lse log2(e)) from them.  The ideal takes one and the same f32 s in both directions:
# its score rounding drops out of P = exp(s - lse), its P sums to 1 over a row like the P inside
# its o, and delta = rowsum(dO o) meets dP = dO V^T with matching roundings.  In the kernel the two
# roundings are independent, which shows where dS = P (dP - delta) is a near-cancellation over few
# terms: the last key of a causal sequence, seen by one query (dk of token 199 at hd 32, S 200:
# |dk row| 1e-3 against a typical 0.8, error 2.5e-6 of it against the ideal's 6.4e-7), and the
# queries with one or two keys (dq of token 1 at hd 128, S 129: 2.3e-6 against 6.9e-7).  Plain f32
# math handed the KERNEL's o and lse gives the kernel's figures: dk 3.86 x (3.69 x with the
# exponent formed in log2 units as the kernel does) against the kernel's 3.73 x at hd 32, S 200;
# dq 1.92 x (2.13 x) against 2.52 x at hd 128, S 129 and 1.57 x (1.82 x) against 2.11 x at hd 64,
# S 129 without the causal mask; handed the ideal's o with the kernel's lse it gives 1.35 x, 1.05 x
# and 1.40 x.  Measured on the MI355X over the 33 cases, against the plain-f32 ideal's worst row:
# dq 2.52 x, dk 3.73 x; the constants are those x 1.25, rounded up to one decimal.
MARGIN_ATTN_F32_DQ = 3.2
MARGIN_ATTN_F32_DK = 4.7
GELU_LIPSCHITZ = 1.13  # max |gelu'| (and > max |gelu''|)

# quiet-NaN patterns for the float types (a kernel that READS a guard poisons its output too),
# 0xA5.. bytes for the rest; compared through integer views, so NaN == NaN
_PATTERN = {1: 0xA5 - 256, 2: 0x7FC5, 4: 0x7FC5A5A5, 8: 0x7FF8A5A5A5A5A5A5}
_INT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _prod(xs):
    p = 1
    for x in xs:
        p *= int(x)
    return p


def guarded(shape, dtype, device="cpu", ld=None, guard=1024, offset=False, fill=None):
    """A ``shape`` view of ``dtype`` inside a larger sentinel-filled buffer.

    At least ``guard`` sentinel elements lie before and after the view; with ``ld`` larger than
    the last dimension the ``ld - cols`` elements after every row are sentinel too.  The view's
    base is 16-B aligned and ``ld`` must be a multiple of 8 (what the kernels require) unless
    ``offset``: then the base sits one element past a 16-B boundary (for the ops that take it).
    ``fill``: a tensor (or number) copied into the view; otherwise the view holds sentinel."""
    if isinstance(shape, int):
        shape = (shape,)
    shape = tuple(int(s) for s in shape)
    cols = shape[-1]
    rows = _prod(shape[:-1])
    ld = cols if ld is None else int(ld)
    if ld < cols:
        raise ValueError(f"guarded: ld {ld} < row length {cols}")
    if ld != cols and len(shape) != 2:
        raise ValueError("guarded: a leading dimension needs a 2-D shape")
    if ld != cols and ld % 8 and not offset:
        raise ValueError("guarded: ld must be a multiple of 8")
    es = torch.empty((), dtype=dtype).element_size()
    front = (int(guard) + 63) // 64 * 64 + (1 if offset else 0)  # 64 elements: a multiple of 16 B
    body = rows * ld
    total = front + body + int(guard)
    raw = torch.empty(total, dtype=_INT[es], device=device).fill_(_PATTERN[es])
    buf = raw.view(dtype)
    view = buf[front:front + body].view(rows, ld)[:, :cols]
    view = view.view(shape) if ld == cols else view
    if not offset:
        assert view.data_ptr() % 16 == 0
    if fill is not None:
        view.copy_(fill) if torch.is_tensor(fill) else view.fill_(fill)
    view._guard_info = (raw, front, rows, cols, ld)
    return view


def guarded_like(t, ld=None, guard=1024, offset=False):
    """A guarded copy of ``t`` (same shape, dtype, device and contents)."""
    return guarded(t.shape, t.dtype, t.device, ld=ld, guard=guard, offset=offset, fill=t)


def guard_touched(view):
    """Offsets (relative to the view's first element, ascending) of every changed guard element."""
    raw, front, rows, cols, ld = view._guard_info
    es = raw.element_size()
    bad = raw != _PATTERN[es]
    body = bad[front:front + rows * ld].view(rows, ld)
    body[:, :cols] = False  # (bad is a fresh tensor: this edits the mask, not the buffer)
    return bad.nonzero().flatten() - front


def assert_guards_intact(*views, what=""):
    for i, view in enumerate(views):
        idx = guard_touched(view)
        if idx.numel():
            _, _, rows, cols, ld = view._guard_info
            first, last = int(idx[0]), int(idx[-1])

            def where(o):
                if o < 0:
                    return f"{-o} before the view"
                if o >= (rows - 1) * ld + cols:
                    return f"{o - ((rows - 1) * ld + cols) + 1} past the last element"
                return f"row {o // ld} gap column {o % ld}"

            raise AssertionError(
                f"{what or 'output'} #{i}: {idx.numel()} guard elements written, offsets {first} ({where(first)}) "
                f".. {last} ({where(last)}) relative to a {rows} x {cols} view with ld {ld}")


# ---------------------------------------------------------------- localised error
def _as2d(t):
    t = t.detach().double()
    return t.reshape(1, -1) if t.dim() < 2 else t.reshape(-1, t.shape[-1])


def _worst(diff, ref, dim):
    num = diff.norm(dim=dim)
    den = ref.norm(dim=dim)
    zero = den == 0
    ratio = num / torch.where(zero, torch.ones_like(den), den)
    # a reference row / column of zeros: the output must be exactly zero there
    ratio = torch.where(zero, torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, math.inf)), ratio)
    ratio = torch.nan_to_num(ratio, nan=math.inf, posinf=math.inf)
    return ratio.max().item() if ratio.numel() else 0.0


def row_col_err(out, ref64):
    """(worst per-row, worst per-column) ratio |out - ref| / |ref|; leading dimensions are rows."""
    o, r = _as2d(out), _as2d(ref64)
    assert o.shape == r.shape, (o.shape, r.shape)
    d = torch.nan_to_num(o - r, nan=math.inf, posinf=math.inf, neginf=math.inf)
    return _worst(d, r, 1), _worst(d, r, 0)


# Reporting, beside the assertions: every check given ``family=`` records its error as a multiple
# of its tolerance's base (the ideal floor, or the bound) here, keeping the largest per family, so
# that a run can say how much of each margin the kernels use.  With the environment variable
# KERNEL_CHECKS_REPORT=<path> set, the dict is written there as JSON when the process exits;
# without it nothing is written.
observed: dict = {}


def _note(family, ratio):
    if family is not None and ratio == ratio:
        observed[family] = max(observed.get(family, 0.0), ratio)


def assert_local_close(out, ref64, ideal, margin, axes="both", what="", family=None):
    """Worst row (and column) error of ``out`` within ``margin`` x that of the ideal kernel's
    output ``ideal``, both against the f64 reference.  ``axes``: "both", "rows" or "cols"."""
    e = row_col_err(out, ref64)
    floor = row_col_err(ideal, ref64)
    for k, name in ((0, "row"), (1, "column")):
        if axes != "both" and axes != name[:3] + "s":
            continue
        tol = margin * floor[k]
        if floor[k] > 0 and math.isfinite(e[k]):
            _note(family, e[k] / floor[k])
        assert e[k] <= tol, (f"{what}: worst {name} error {e[k]:.3e} > {margin} x ideal floor {floor[k]:.3e}")
    return e, floor


def assert_elem_close(out, ref64, ideals, margin, what="", family=None, ulp_floor=False):
    """Every element of ``out`` within ``margin`` x the ideal kernel's LARGEST element error, both
    against the f64 reference -- for vectors of sums (bias / gain gradients, column sums, row
    statistics) whose elements share one scale: an error relative to each element would be decided
    by whichever sum happens to cancel to almost nothing, in the ideal and in the kernel alike.
    ``ideals``: one ideal output or several (the same plain f32 sum in several orders -- a kernel
    differs from them in summation order only, and one order over a handful of elements is one
    sample: measured on the MI355X, LayerNorm's gsum at T = 67, D = 4 is 2.16 x the floor of the
    first-to-last order alone, and 1.5 to 1.7 x the floor of three orders).
    ``ulp_floor``: the floor is at least half an ulp of the largest f32 reference element -- no f32
    output can be held below its own rounding, however lucky the ideal's few elements are."""
    ideals = [ideals] if torch.is_tensor(ideals) else list(ideals)
    floor = max((i.detach().double() - ref64.double()).abs().max() for i in ideals)
    if ulp_floor:
        floor = torch.maximum(floor, ref64.double().abs().max() * 2.0 ** -24)
    if family is not None and floor > 0:
        _note(family, ((out.detach().double() - ref64.double()).abs().max() / floor).item())
    assert_elem_bound(out, ref64, (margin * floor).expand_as(ref64), what=what)


def gemm_elem_bound(a, b, ref64, out_dtype, K, lipschitz=1.0):
    """Per-element error bound of an f32-accumulated product ``a @ b^T`` (a [M, K], b [N, K], the
    rounded operands) behind ``ref64`` (the f64 result after the epilogue):
    lipschitz x (u |ref| + 4 K 2^-24 (|a| |b|^T)), u = 2^-7 for a bf16 output (its half-ulp 2^-8
    and one intermediate rounding), 2^-22 for an f32 output."""
    u = {torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -22}[out_dtype]
    ab = a.detach().double().abs() @ b.detach().double().abs().t()
    return lipschitz * (u * ref64.double().abs() + 4.0 * K * 2.0 ** -24 * ab)


def assert_elem_bound(out, ref64, bound, what="", family=None):
    """|out - ref| <= bound for every element (NaN / inf in ``out`` fail)."""
    d = torch.nan_to_num((out.detach().double() - ref64.double()).abs(), nan=math.inf, posinf=math.inf)
    bad = d > bound
    if family is not None and d.numel():
        r = (d / bound.clamp_min(1e-300)).max().item()
        _note(family, r)
    if bad.any():
        idx = bad.nonzero()
        first = tuple(idx[0].tolist())
        last = tuple(idx[-1].tolist())
        worst = (d / bound.clamp_min(1e-300)).max().item()
        raise AssertionError(f"{what}: {int(bad.sum())} elements over the bound (worst {worst:.2f}x), "
                             f"first at {first}, last at {last}")


def _dump():  # KERNEL_CHECKS_REPORT=path: the observed error / floor ratios of this run as JSON
    path = os.environ.get("KERNEL_CHECKS_REPORT")
    if path and observed:
        with open(path, "w") as f:
            json.dump({k: round(v, 4) for k, v in sorted(observed.items())}, f, indent=1)


atexit.register(_dump)


# ---------------------------------------------------------------- plain references
def attention_plain(qkv, N, S, heads, head_dim, pad_mask=None, causal=True, dtype=torch.float64):
    """Softmax attention over the fused [T, 3 H hd] projection in ``dtype``, the O(S^2) way:
    (o [T, H hd], lse [N H, S]) in ``dtype``; a query with no allowed key gives o = 0, lse = inf."""
    E = heads * head_dim
    q, k, v = (qkv[:, i * E:(i + 1) * E].to(dtype).reshape(N, S, heads, head_dim).transpose(1, 2) for i in range(3))
    s = (q @ k.transpose(-1, -2)) / math.sqrt(head_dim)
    allowed = torch.ones(S, S, dtype=torch.bool, device=qkv.device)
    if causal:
        allowed = torch.tril(allowed)
    allowed = allowed.expand(N, 1, S, S)
    if pad_mask is not None:
        allowed = allowed & ~pad_mask.bool()[:, None, None, :]
    s = s.masked_fill(~allowed, -math.inf)
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p = torch.where(l > 0, e / l.clamp_min(1e-300), torch.zeros_like(e))
    o = (p @ v).transpose(1, 2).reshape(N * S, E)
    lse = torch.where(l > 0, m + torch.log(l.clamp_min(1e-300)), torch.full_like(l, math.inf))
    return o, lse.reshape(N * heads, S)


def attention_bwd_plain(qkv, dout, o, lse, N, S, heads, head_dim, pad_mask=None, causal=True, dtype=torch.float32):
    """The flash backward's math done the plain way in ``dtype`` from the operands the kernel is
    handed -- qkv, dout, the forward's (rounded) output ``o`` and ``lse``: P = exp(S - lse),
    dV = P^T dO, delta = rowsum(dO o), dS = P (dO V^T - delta), dQ = dS K, dK = dS^T Q."""
    E = heads * head_dim
    sc = 1.0 / math.sqrt(head_dim)

    def heads_of(t):
        return t.to(dtype).reshape(N, S, heads, head_dim).transpose(1, 2)

    q, k, v = (heads_of(qkv[:, i * E:(i + 1) * E]) for i in range(3))
    do, oo = heads_of(dout), heads_of(o)
    s = (q @ k.transpose(-1, -2)) * sc
    allowed = torch.ones(S, S, dtype=torch.bool, device=qkv.device)
    if causal:
        allowed = torch.tril(allowed)
    allowed = allowed.expand(N, 1, S, S)
    if pad_mask is not None:
        allowed = allowed & ~pad_mask.bool()[:, None, None, :]
    l = lse.to(dtype).reshape(N, heads, S, 1)
    p = torch.where(allowed & torch.isfinite(l), torch.exp(s - torch.where(torch.isfinite(l), l, torch.zeros_like(l))),
                    torch.zeros_like(s))
    dv = p.transpose(-1, -2) @ do
    delta = (do * oo).sum(-1, keepdim=True)
    ds = p * (do @ v.transpose(-1, -2) - delta)
    dq = (ds @ k) * sc
    dk = (ds.transpose(-1, -2) @ q) * sc
    return torch.cat([t.transpose(1, 2).reshape(N * S, E) for t in (dq, dk, dv)], dim=1)
