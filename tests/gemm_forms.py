"""Argument forms of the GEMMs (and of the f32 attention) that the training step passes on every
step, as cases for the CPU and the GPU tests: the device scalar ``alpha_t``, operands stored
smaller than the logical product, every epilogue of the f32 kernel, and the f32 attention at its
edge lengths.  Pure torch, no fixtures; every builder takes the device.

A ``Form`` names the epilogue arguments of one ``gemm()`` call.  ``run_form`` makes the call with
every output in guard bands (tests/kernel_checks.py), ``check_form`` holds each output to
``gemm_elem_bound`` against ``epilogue64``: the f64 epilogue in the order of ops/gemm.py's
docstring.  With a multiplier the bound is that of the operands ``|alpha| a`` and ``b`` at
``K + 1``: the one f32 rounding of ``alpha * acc`` is at most 2^-24 |alpha| (|a| |b|^T), one more
term of the 4 K 2^-24 sum.  The multipliers are exact in f32 (0.75, 1.3125, -0.40625, and their
products), so the reference has no rounding of its own to argue about.

test_gemm_forms_cpu.py runs the same forms through ``gemm()`` on CPU tensors (ops/gemm.py:
``_gemm_ref``) and asserts the same inequalities, so that a wrong reference or a bound no f32
implementation can meet shows before a GPU is involved."""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from kernel_checks import (GELU_LIPSCHITZ, MARGIN, assert_elem_bound, assert_guards_intact, assert_local_close,
                           attention_bwd_plain, attention_plain, gemm_elem_bound, guarded)

BF, F32 = torch.bfloat16, torch.float32

ALPHA = 0.75         # the host multiplier
ALPHA_T = 1.3125     # the device multiplier (0.75 x 1.3125 = 0.984375)
ALPHA_T2 = -0.40625  # its second value (the freshness tests)


def gelu64(z):
    return F.gelu(z.double(), approximate="tanh")


def dgelu64(z):
    z = z.double()
    k0, k1 = math.sqrt(2.0 / math.pi), 0.044715
    t = torch.tanh(k0 * (z + k1 * z ** 3))
    return 0.5 * (1 + t) + 0.5 * z * (1 - t * t) * k0 * (1 + 3 * k1 * z * z)


def dact64(z, act):
    return dgelu64(z) if act == 2 else (z.double() > 0).double()


def _store(x, kmaj):
    """Operand storage as the model lays it out: k-major rows (or mn-major columns) padded to a
    multiple of 8 elements."""
    r, c = x.shape
    if kmaj:
        buf = torch.zeros(r, (c + 7) // 8 * 8, device=x.device, dtype=x.dtype)
        buf[:, :c] = x
        return buf[:, :c]
    buf = torch.zeros(c, (r + 7) // 8 * 8, device=x.device, dtype=x.dtype)
    buf[:, :r] = x.t()
    return buf[:, :r]


LAYOUTS = [(True, True), (True, False), (False, False), (False, True)]
IMPLS = [1, 2, 3, 4, 10, 16, 17, 19, 20, 21, 22, 25, 26]
GEMM_SHAPES = [(1, 8, 8),          # the smallest legal product
               (300, 264, 136),    # one full tile + tails in M, N and K
               (513, 520, 200),    # several tiles, tails everywhere
               # K % 64 == 0: with a k-major operand the persistent 256 x 256 kernels (and the
               # LDS-DMA 128 x 128 ones) hand every K above to the register-staged kernel; this
               # one they run themselves, on ragged M and N
               (300, 264, 192)]
ALPHA_SHAPES = [(300, 264, 136), (300, 264, 192)]
SPLIT_K_SHAPE = (77, 264, 4160)
_gemm_cache = {}


def gemm_data(M, N, K, dtype=BF, device="cuda"):
    """Operands and the f64 results of every epilogue form, computed once per shape (shared by
    the implementations and layouts, never modified)."""
    key = (M, N, K, dtype, str(device))
    if key in _gemm_cache:
        return _gemm_cache[key]
    g = torch.Generator(device=device).manual_seed(M * 1000003 + N * 1009 + K)

    def rn(*s):
        return torch.randn(*s, device=device, generator=g)

    d = {}
    d["a"] = a = rn(M, K).to(dtype)
    d["b"] = b = (rn(N, K) / math.sqrt(K)).to(dtype)  # pre-activations of order 1: GELU's bend
    d["bias"] = bias = rn(N)
    d["res"] = res = rn(M, N)
    d["z"] = z = rn(M, N).bfloat16()
    d["acc0"] = acc0 = rn(M, N)
    P = a.double() @ b.double().t()
    z1 = P + bias.double()
    d["plain"] = P
    d["pre"] = z1
    d["gelu"] = gelu64(z1)
    d["dgelu"] = dgelu64(z1)
    d["relu_res"] = torch.relu(z1) + res.double()
    d["act_bwd"] = P * dgelu64(z)
    d["acc"] = acc0.double() + P
    d["z32"] = rn(M, N)  # an f32 aux_in (drawn last: the values above are those of every earlier run)
    _gemm_cache[key] = d
    return d


# ---------------------------------------------------------------- forms
@dataclass(frozen=True)
class Form:
    """The epilogue arguments of one gemm() call.  ``alpha`` None: not passed (the default 1.0);
    ``alpha_t``: the device scalar is passed; ``aux_out`` / ``aux_in``: the dtype, or None."""
    name: str
    out: torch.dtype = F32
    bias: bool = False
    act: int = 0
    aux_out: torch.dtype | None = None
    aux_deriv: bool = False
    residual: bool = False
    act_bwd: int = 0
    aux_in: torch.dtype | None = None
    colsum: bool = False
    accumulate: bool = False
    alpha: float | None = None
    alpha_t: bool = False

    def scale(self, t_value=ALPHA_T):
        return (1.0 if self.alpha is None else self.alpha) * (t_value if self.alpha_t else 1.0)

    def flags(self):
        """The epilogue arguments this form turns on, as names."""
        on = [n for n in ("bias", "aux_deriv", "residual", "colsum", "accumulate") if getattr(self, n)]
        on += [f"act{self.act}"] if self.act else []
        on += [f"act_bwd{self.act_bwd}"] if self.act_bwd else []
        on += ["aux_out"] if self.aux_out is not None else []
        on += ["aux_in"] if self.aux_in is not None else []
        on += ["out_bf16" if self.out == BF else "out_f32"]
        return on


_AT = dict(alpha=ALPHA, alpha_t=True)
# A: bf16 operands, every implementation; host and device multiplier together, and the device
# multiplier alone where the host one keeps its default
ALPHA_FORMS = [
    Form("plain_bf16", out=BF, **_AT),
    Form("plain_f32", **_AT),
    Form("bias_gelu_aux", out=BF, bias=True, act=2, aux_out=BF, **_AT),
    Form("bias_relu_res", bias=True, act=1, residual=True, **_AT),
    Form("act_bwd_colsum", out=BF, act_bwd=2, aux_in=BF, colsum=True, **_AT),
    Form("accumulate", accumulate=True, **_AT),
    Form("plain_f32_t_alone", alpha_t=True),
    Form("accumulate_t_alone", accumulate=True, alpha_t=True),
]
SPLIT_K_FORMS = [Form("fresh", **_AT), Form("accumulated", accumulate=True, **_AT)]
FRESH_FORMS = [Form("plain_f32", **_AT), Form("bias_gelu_aux", out=BF, bias=True, act=2, aux_out=BF, **_AT)]
# C: f32 operands (csrc/gemm_f32.hip)
F32_FORMS = [
    Form("bias_relu_res", bias=True, act=1, residual=True),
    Form("bias_gelu_aux_deriv", bias=True, act=2, aux_out=F32, aux_deriv=True),
    Form("bias_gelu_aux_bf16", bias=True, act=2, aux_out=BF),
    Form("act_bwd1_f32_colsum", act_bwd=1, aux_in=F32, colsum=True),
    Form("act_bwd1_bf16_colsum", act_bwd=1, aux_in=BF, colsum=True),
    Form("act_bwd2_f32_colsum", act_bwd=2, aux_in=F32, colsum=True),
    Form("act_bwd2_bf16_colsum", act_bwd=2, aux_in=BF, colsum=True),
    Form("accumulate", accumulate=True),
    Form("alpha", **_AT),
    Form("alpha_bias_gelu_aux", bias=True, act=2, aux_out=F32, **_AT),  # alpha goes in before the bias
    Form("alpha_accumulate", accumulate=True, **_AT),  # the old C enters unscaled
    Form("alpha_bias_gelu_aux_deriv", bias=True, act=2, aux_out=F32, aux_deriv=True, **_AT),
    Form("alpha_act_bwd1_colsum", act_bwd=1, aux_in=BF, colsum=True, **_AT),
    Form("accumulate_residual", accumulate=True, residual=True),
]
# C: the two forms run once per operand storage
F32_STORAGE_FORMS = [Form("plain"), Form("bias_gelu_aux", bias=True, act=2, aux_out=F32)]
F32_STORAGES = ["aligned", "ld_odd", "offset"]
# K = 203: the last group of four k-major elements is cut inside (k + j < K holds for three of
# them), in the float4 arm's tail and in the scalar arm; every K of GEMM_SHAPES is a multiple of 4,
# where only an mn-major operand (M = 513) meets a partly valid group
F32_STORAGE_SHAPES = GEMM_SHAPES + [(67, 72, 203)]


def epilogue64(P, form, d, scale):
    """(out, aux_out, column sums) of ``form`` on the f64 product ``P``, in f64, in the order of
    ops/gemm.py's docstring: v = P scale + bias; act'; column sums; aux_out; act; residual;
    accumulate (the old C enters unscaled).  ``d``: bias, res, z / z32, acc0."""
    v = P.double() * scale
    if form.bias:
        v = v + d["bias"].double()
    if form.act_bwd:
        v = v * dact64(d["z32"] if form.aux_in == F32 else d["z"], form.act_bwd)
    cs = v.sum(0)
    aux = dact64(v, form.act) if form.aux_deriv else v
    if form.act:
        v = gelu64(v) if form.act == 2 else torch.relu(v)
    if form.residual:
        v = v + d["res"].double()
    if form.accumulate:
        v = d["acc0"].double() + v
    return v, aux, cs


COLSUM_START = 0.25


def run_form(gemm, form, d, A, B, a_kmaj, b_kmaj, M, N, alpha_t=None, outputs=None):
    """One gemm() call of ``form`` on the stored operands A, B; every output in guard bands at
    ld = N + 8 (the column sums prefilled with COLSUM_START, an accumulated C with acc0).
    ``alpha_t``: the device scalar of a form that takes one.  ``outputs``: write into the
    buffers of an earlier run of the form (graph replays).  -> {"out", "aux", "colsum"}"""
    dev = A.device
    o = outputs or {}
    if not o:
        o["out"] = guarded((M, N), form.out, dev, ld=N + 8, fill=d["acc0"] if form.accumulate else None)
        if form.aux_out is not None:
            o["aux"] = guarded((M, N), form.aux_out, dev, ld=N + 8)
        if form.colsum:
            o["colsum"] = guarded(N, F32, dev, fill=COLSUM_START)
    kw = dict(a_kmaj=a_kmaj, b_kmaj=b_kmaj, out=o["out"])
    if form.bias:
        kw["bias"] = d["bias"]
    if form.act:
        kw["act"] = form.act
    if form.aux_out is not None:
        kw["aux_out"] = o["aux"]
    if form.aux_deriv:
        kw["aux_deriv"] = True
    if form.residual:
        kw["residual"] = d["res"]
    if form.act_bwd:
        kw["act_bwd"] = form.act_bwd
        kw["aux_in"] = d["z32"] if form.aux_in == F32 else d["z"]
    if form.colsum:
        kw["colsum"] = o["colsum"]
    if form.accumulate:
        kw["accumulate"] = True
    if form.alpha is not None:
        kw["alpha"] = form.alpha
    if form.alpha_t:
        assert alpha_t is not None and alpha_t.device == dev
        kw["alpha_t"] = alpha_t
    gemm(A, B, **kw)
    return o


def check_form(form, d, K, o, t_value=ALPHA_T, family=None, what=""):
    """Every output of ``run_form`` inside gemm_elem_bound of its epilogue64 value (operands
    |scale| a and b, K + 1 with a multiplier); the column sums inside that bound summed over the
    rows (f32: the kernels sum the f32 values); guards intact."""
    scale = form.scale(t_value)
    Kb = K + 1 if scale != 1.0 else K
    a_s = d["a"].double() * abs(scale)
    ref, aux, cs = epilogue64(d["plain"], form, d, scale)
    what = f"{what} {form.name}".strip()
    lip = GELU_LIPSCHITZ if (form.act == 2 or form.act_bwd == 2) else 1.0
    assert_elem_bound(o["out"], ref, gemm_elem_bound(a_s, d["b"], ref, o["out"].dtype, Kb, lip), what=what, family=family)
    if form.aux_out is not None:
        lip_aux = GELU_LIPSCHITZ if form.aux_deriv else 1.0
        assert_elem_bound(o["aux"], aux, gemm_elem_bound(a_s, d["b"], aux, o["aux"].dtype, Kb, lip_aux),
                          what=what + " aux_out", family=family)
    if form.colsum:
        # the sums of v before aux / act / residual: act_bwd forms only, whose v is the output
        assert not (form.act or form.residual or form.accumulate)
        assert_elem_bound(o["colsum"], COLSUM_START + cs, gemm_elem_bound(a_s, d["b"], ref, F32, Kb, lip).sum(0),
                          what=what + " colsum", family=family)
    assert_guards_intact(*o.values(), what=what)


def alpha_scalar(device, value=ALPHA_T):
    """The device scalar, written by device ops alone (a fill and an in-place multiply)."""
    return torch.full((1,), value / 2.0, device=device).mul_(2.0)


# ---------------------------------------------------------------- f32 operand storage
def store_f32(x, kmaj, storage):
    """An f32 operand as csrc/gemm_f32.hip's f32_load meets it.  "aligned": as the model stores it
    (_store): the float4 arm.  "ld_odd": a 16-B aligned base with a row stride that is no
    multiple of 4.  "offset": a row stride that is one, the base 4 bytes past a 16-B boundary.
    The last two take the scalar arm.  Everything around the operand is NaN."""
    if storage == "aligned":
        return _store(x, kmaj)
    s = x if kmaj else x.t()
    r, c = s.shape
    if storage == "ld_odd":
        ld = c + 1 if (c + 1) % 4 else c + 2
        buf = torch.full((r, ld), math.nan, device=x.device, dtype=x.dtype)
        buf[:, :c] = s
        return buf[:, :c]
    assert storage == "offset"
    return guarded((r, c), x.dtype, x.device, ld=(c + 7) // 8 * 8 + 8, offset=True, fill=s)


def scalar_arm(t):
    """Which condition of f32_load's ``vec`` an operand fails: "ld", "base", "both", or None."""
    ld, base = t.stride(0) % 4 != 0, t.data_ptr() % 16 != 0
    return "both" if ld and base else "ld" if ld else "base" if base else None


# ---------------------------------------------------------------- stored extents
# T rows, D features, V vocabulary rows stored of N = Npad = 256: 201 and 250 cut inside an
# 8-column chunk of the output (250 inside the last one), 200 on a chunk boundary
EXT_T, EXT_D, EXT_N = 77, 192, 256
EXT_V = [201, 250, 200]
# rows of A stored of M = 96: 77 cuts inside an 8-element chunk of an mn-major A, 72 between two
EXT_M = 96
EXT_ROWS = [77, 72]
EXTENT_CASES = ([("fwd_head", V) for V in EXT_V] + [("dgrad_head", V) for V in EXT_V]
                + [("short_a_k", R) for R in EXT_ROWS] + [("short_a_mn", R) for R in EXT_ROWS]
                + [("short_b_mn", R) for R in EXT_ROWS])
EXTENT_FORMS = {
    "fwd_head": [Form("plain_bf16", out=BF), Form("plain_f32")],
    # (production: the LM head's input gradient carries the loss scale as alpha_t)
    "dgrad_head": [Form("plain_bf16", out=BF), Form("plain_f32_t", alpha_t=True)],
    # rows past A are epilogue(0): exact zeros, or relu(bias) + residual -- one f32 rounding, which
    # the bound's output term allows (GELU of a bias alone is not held to 2^-22 by any f32 tanh)
    "short_a_k": [Form("plain_bf16", out=BF), Form("plain_f32"), Form("bias_relu_res", bias=True, act=1, residual=True)],
    "short_a_mn": [Form("plain_bf16", out=BF), Form("plain_f32"), Form("bias_relu_res", bias=True, act=1, residual=True)],
    # the same cut in an mn-major B: fewer stored columns than the output has (not a form of the
    # model; the dispatcher's rule for a short mn-major operand covers both operands)
    "short_b_mn": [Form("plain_bf16", out=BF), Form("plain_f32")],
}
_extent_cache = {}


def extent_forms(kind, dtype):
    """The forms of an extent case; the f32 kernel writes f32 outputs only."""
    return [f for f in EXTENT_FORMS[kind] if dtype == BF or f.out == F32]


def short_guard(missing_rows, ld):
    """Sentinel elements behind a short operand: the whole missing part and 1024 more, so that a
    kernel that ignores the extent reads NaN inside the allocation, never outside it."""
    return missing_rows * ld + 1024


def extent_case(kind, cut, dtype, device):
    """-> dict(A, B, a_kmaj, b_kmaj, M, N, K, d, zero_cols, zero_rows): stored operands (the short
    one in guard bands sized by short_guard), the logical zero-extended operands and product in
    ``d``, and the output columns / rows that are products with nothing stored."""
    key = (kind, cut, dtype, str(device))
    if key in _extent_cache:
        return _extent_cache[key]
    g = torch.Generator(device=device).manual_seed(7919 * cut + len(kind))
    T, D, N = EXT_T, EXT_D, EXT_N

    def rn(*s):
        return torch.randn(*s, device=device, generator=g)

    def zeros(*s):
        return torch.zeros(*s, device=device, dtype=dtype)

    c = dict(zero_cols=slice(0, 0), zero_rows=slice(0, 0))
    ld = D + 8
    if kind == "fwd_head":  # logits = h W^T over the padded vocabulary: B has V < N rows
        V = cut
        a, w = rn(T, D).to(dtype), (rn(V, D) / math.sqrt(D)).to(dtype)
        c.update(A=_store(a, True), B=guarded((V, D), dtype, device, ld=ld, guard=short_guard(N - V, ld), fill=w),
                 a_kmaj=True, b_kmaj=True, M=T, N=N, K=D, zero_cols=slice(V, N))
        b = torch.cat([w, zeros(N - V, D)])
    elif kind == "dgrad_head":  # dh = dlogits W: K = the padded vocabulary, W holds V k-rows
        V = cut
        a, w = rn(T, N).to(dtype), (rn(V, D) / math.sqrt(V)).to(dtype)
        assert (a[:, V:] != 0).all() and torch.isfinite(a).all()  # B's missing k-rows must read as zero
        c.update(A=_store(a, True), B=guarded((V, D), dtype, device, ld=ld, guard=short_guard(N - V, ld), fill=w),
                 a_kmaj=True, b_kmaj=False, M=T, N=D, K=N)
        b = torch.cat([w.t(), zeros(D, N - V)], dim=1)
    elif kind == "short_b_mn":  # B [K, R] mn-major under an output of EXT_M columns
        R, Nn = cut, EXT_M
        a, w = rn(T, D).to(dtype), (rn(R, D) / math.sqrt(D)).to(dtype)
        ldb = (Nn + 7) // 8 * 8 + 8
        c.update(A=_store(a, True), B=guarded((D, R), dtype, device, ld=ldb, guard=short_guard(1, ldb), fill=w.t()),
                 a_kmaj=True, b_kmaj=False, M=T, N=Nn, K=D, zero_cols=slice(R, Nn))
        b = torch.cat([w, zeros(Nn - R, D)])
    else:  # fewer rows of A than of the output
        R, M, Nb = cut, EXT_M, 264
        a_st, b = rn(R, D).to(dtype), (rn(Nb, D) / math.sqrt(D)).to(dtype)
        a = torch.cat([a_st, zeros(M - R, D)])
        if kind == "short_a_k":
            A = guarded((R, D), dtype, device, ld=ld, guard=short_guard(M - R, ld), fill=a_st)
        else:  # mn-major: the missing rows are the columns R .. M of every k-row, sentinel too
            lda = (M + 7) // 8 * 8 + 8
            A = guarded((D, R), dtype, device, ld=lda, guard=short_guard(1, lda), fill=a_st.t())
        c.update(A=A, B=_store(b, True), a_kmaj=kind == "short_a_k", b_kmaj=True, M=M, N=Nb, K=D,
                 zero_rows=slice(R, M))
    M, N = c["M"], c["N"]
    c["d"] = dict(a=a, b=b, plain=a.double() @ b.double().t(), bias=rn(N), res=rn(M, N), acc0=rn(M, N))
    _extent_cache[key] = c
    return c


def check_extent_form(form, c, o, family=None, what=""):
    """check_form, and the products with nothing stored: exactly zero where the form is plain."""
    check_form(form, c["d"], c["K"], o, family=family, what=what)
    if not (form.bias or form.residual or form.accumulate):
        assert torch.count_nonzero(o["out"][:, c["zero_cols"]]) == 0, f"{what} {form.name}: padded columns"
        assert torch.count_nonzero(o["out"][c["zero_rows"]]) == 0, f"{what} {form.name}: rows past A"


# ---------------------------------------------------------------- f32 attention at the edge lengths
ATTN_F32_N, ATTN_F32_H = 2, 2
ATTN_F32_CASES = ([(hd, S, True, wp) for hd in (32, 64, 128) for S in (1, 63, 65, 129, 200) for wp in (False, True)]
                  + [(hd, 129, False, False) for hd in (32, 64, 128)])


def attn_pad_mask(N, S, device):
    pad = torch.zeros(N, S, dtype=torch.bool, device=device)
    pad[0, S - S // 4:] = True  # right padding
    pad[1, 5:9] = True          # an interior gap
    return pad


def attention_f32_case(hd, S, causal, with_pad, device):
    """f32 inputs of one case and its reference pair: the f64 forward and autograd gradient, and
    the ideal -- the same math in plain f32, the backward from the ideal's own o and lse."""
    N, H = ATTN_F32_N, ATTN_F32_H
    T, E = N * S, H * hd
    g = torch.Generator(device=device).manual_seed(1000 * hd + S)
    qkv = torch.randn(T, 3 * E, device=device, generator=g)
    do = torch.randn(T, E + 8, device=device, generator=g)[:, :E]
    pad = attn_pad_mask(N, S, device) if with_pad else None
    x = qkv.double().requires_grad_(True)
    o64, lse64 = attention_plain(x, N, S, H, hd, pad, causal)
    (g64,) = torch.autograd.grad(o64, x, do.double())
    o32, lse32 = attention_plain(qkv, N, S, H, hd, pad, causal, dtype=F32)
    g32 = attention_bwd_plain(qkv, do, o32, lse32, N, S, H, hd, pad, causal, dtype=F32)
    return dict(qkv=qkv, do=do, pad=pad, o64=o64.detach(), lse64=lse64.detach(), g64=g64, o32=o32, g32=g32)


def check_attention_f32(c, hd, S, causal, o, lse, dqkv, margins=None):
    """o, dq, dk, dv per row within the margin of the ideal's floor; lse at 1e-5 where the
    reference is finite; the rows a causal query 0 makes by cancellation alone held to the
    product bound of test_attention_edges with the f32 output term.  ``margins``: per family
    ("fwd", "dq", "dk", "dv"), MARGIN where not named.

    S = 1: dv = P do with P = exp(s - lse) = 1.  The ideal takes s and lse from one and the same
    f32 product, so its P is 1 and its dv is do bit for bit -- a floor of zero, which no backward
    that is handed lse as an f32 number and forms s again can be held to (csrc/attention_f32.hip:
    |dv - do| / |do| measured 6.8e-8 at hd 32, 3.4e-7 at hd 128).  Those rows are held to the
    product bound instead, as dq and dk are: the two s differ by at most 4 hd 2^-24 |q|.|k| /
    sqrt(hd), lse is rounded to f32 and once more on its way to the exponent (2 x 2^-24 |lse|),
    and the output's 2^-22."""
    N, H = ATTN_F32_N, ATTN_F32_H
    T, E = N * S, H * hd
    dev = o.device
    qkv, do, g64 = c["qkv"], c["do"], c["g64"]
    margins = margins or {}
    assert_local_close(o, c["o64"], c["o32"], margins.get("fwd", MARGIN), axes="rows", what="o",
                       family="attention f32 fwd")
    fin = torch.isfinite(c["lse64"])
    assert torch.isfinite(lse[fin]).all()
    assert torch.allclose(lse[fin].double(), c["lse64"][fin], atol=1e-5, rtol=1e-5)
    # A causal query 0 sees one key: P = 1 and dS = do.v - do.o is zero only by cancellation of two
    # f32 sums over hd, so the dq rows it makes (and dk, when S = 1 leaves nothing else) are no
    # structural zeros: |dS| <= 4 hd 2^-24 |do|.|v|, times |k| (or |q|) / sqrt(hd), and the f32
    # output's rounding.  Every other row is checked against the ideal's floor, where a reference
    # row of zeros (a padded key's dk and dv) must be zero exactly.
    first = torch.zeros(T, dtype=torch.bool, device=dev)
    if causal:
        first[torch.arange(N, device=dev) * S] = True

        def per_head(t):
            return t[first].double().abs().reshape(N, H, hd)

        ds = 4 * hd * 2.0 ** -24 * (per_head(do) * per_head(qkv[:, 2 * E:])).sum(-1, keepdim=True)
        for name, sl, other in (("dq", slice(0, E), slice(E, 2 * E)), ("dk", slice(E, 2 * E), slice(0, E))):
            if name == "dq" or S == 1:
                bound = (1 + 2.0 ** -22) * ds * per_head(qkv[:, other]) / math.sqrt(hd)
                assert_elem_bound(dqkv[first][:, sl], g64[first][:, sl], bound.reshape(N, E), what=name + " of query 0")
        if S == 1:
            dp = (4 * hd * 2.0 ** -24 * (per_head(qkv[:, :E]) * per_head(qkv[:, E:2 * E])).sum(-1, keepdim=True) / math.sqrt(hd)
                  + 2 * 2.0 ** -24 * c["lse64"].abs().reshape(N, H, 1) + 2.0 ** -22)
            assert_elem_bound(dqkv[:, 2 * E:], g64[:, 2 * E:], (dp * per_head(do)).reshape(N, E), what="dv of one key")
    for i, name in enumerate(("dq", "dk", "dv")):
        sl = slice(i * E, (i + 1) * E)
        rows = ~first if (name == "dq" or S == 1) else torch.ones_like(first)
        if rows.any():
            assert_local_close(dqkv[rows][:, sl], g64[rows][:, sl], c["g32"][rows][:, sl], margins.get(name, MARGIN),
                               axes="rows", what=name, family=f"attention f32 {name}")
