"""Edges of every HIP kernel: small shapes with tails in every dimension, every output the kernel
is handed inside guard bands (tests/kernel_checks.py), and errors measured per row, per column or
per element against an f64 reference -- never as one norm over the whole output.

Tolerances: ``gemm_elem_bound`` per element for the products; elsewhere a margin times the error
an ideal kernel (the same math in plain f32 PyTorch on the same rounded inputs, rounded to the
output dtype) makes against the same f64 reference."""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

from kernel_checks import (GELU_LIPSCHITZ, MARGIN, MARGIN_ATTN, assert_elem_bound, assert_guards_intact,
                           assert_elem_close, assert_local_close, attention_bwd_plain, attention_plain, gemm_elem_bound, guarded)
from gemm_forms import GEMM_SHAPES, IMPLS, LAYOUTS, _store, dact64, dgelu64, gelu64, gemm_data
from mem_cases import check_cross_entropy, first_argmax

from distributed_pytorch_cookbook_amd.ops import _lib
from distributed_pytorch_cookbook_amd.ops.attention import attention_bwd, attention_fwd, decode_attention
from distributed_pytorch_cookbook_amd.ops.dropout import DropSpec, dropout_residual, keep_mask
from distributed_pytorch_cookbook_amd.ops.elementwise import bias_act_bwd, cast_f32_bf16
from distributed_pytorch_cookbook_amd.ops.embedding import embedding_bwd, embedding_fwd
from distributed_pytorch_cookbook_amd.ops.gemm import gemm, linear_fwd
from distributed_pytorch_cookbook_amd.ops.loss import cross_entropy_rows
from distributed_pytorch_cookbook_amd.ops.norm import layernorm_bwd, layernorm_fwd
from distributed_pytorch_cookbook_amd.ops.optim import FlatAdamW

pytestmark = pytest.mark.gpu
dev = "cuda"
BF, F32 = torch.bfloat16, torch.float32


def _ld(n):
    """A leading dimension past the row: the next multiple of 8, and 8 more."""
    return (n + 7) // 8 * 8 + 8


# ---------------------------------------------------------------- GEMM
def _g(M, N, dtype, fill=None):
    return guarded((M, N), dtype, dev, ld=N + 8, fill=fill)


def _check_gemm(d, K, out, ref, lipschitz=1.0, what=""):
    assert_elem_bound(out, d[ref], gemm_elem_bound(d["a"], d["b"], d[ref], out.dtype, K, lipschitz),
                      what=what or ref, family=f"gemm {str(out.dtype)[6:]} (fraction of the element bound)")


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("a_kmaj,b_kmaj", LAYOUTS)
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_edges(impl, a_kmaj, b_kmaj, M, N, K):
    """Every forced implementation (one that cannot take a shape hands it to the 128 x 128
    kernels inside the dispatcher, as in test_kernels_gpu.py) x layout x epilogue form, outputs
    written at ldc = N + 8 into guard bands, every element inside gemm_elem_bound."""
    d = gemm_data(M, N, K)
    A, B = _store(d["a"], a_kmaj), _store(d["b"], b_kmaj)
    kw = dict(a_kmaj=a_kmaj, b_kmaj=b_kmaj)
    ob, of = _g(M, N, BF), _g(M, N, F32)
    og, aux = _g(M, N, BF), _g(M, N, BF)
    og2, auxd = _g(M, N, BF), _g(M, N, BF)
    orr = _g(M, N, F32)
    od, cs = _g(M, N, BF), guarded(N, F32, dev, fill=0.25)
    acc = _g(M, N, F32, fill=d["acc0"])
    _lib.set_gemm_impl(impl)
    try:
        gemm(A, B, out=ob, **kw)
        gemm(A, B, out=of, **kw)
        gemm(A, B, out=og, bias=d["bias"], act=2, aux_out=aux, **kw)
        gemm(A, B, out=og2, bias=d["bias"], act=2, aux_out=auxd, aux_deriv=True, **kw)
        gemm(A, B, out=orr, bias=d["bias"], act=1, residual=d["res"], **kw)
        gemm(A, B, out=od, act_bwd=2, aux_in=d["z"], colsum=cs, **kw)
        gemm(A, B, out=acc, accumulate=True, **kw)
    finally:
        _lib.set_gemm_impl(-1)
    _check_gemm(d, K, ob, "plain")
    _check_gemm(d, K, of, "plain")
    _check_gemm(d, K, og, "gelu", GELU_LIPSCHITZ)
    _check_gemm(d, K, aux, "pre", what="aux_out")
    _check_gemm(d, K, og2, "gelu", GELU_LIPSCHITZ, what="gelu beside aux_deriv")
    _check_gemm(d, K, auxd, "dgelu", GELU_LIPSCHITZ, what="aux_deriv")
    _check_gemm(d, K, orr, "relu_res")
    _check_gemm(d, K, od, "act_bwd", GELU_LIPSCHITZ)
    _check_gemm(d, K, acc, "acc")
    # column sums of the f32 values: per element, the f32 element bound summed over the rows
    cs_bound = gemm_elem_bound(d["a"], d["b"], d["act_bwd"], F32, K, GELU_LIPSCHITZ).sum(0)
    assert_elem_bound(cs, 0.25 + d["act_bwd"].sum(0), cs_bound, what="colsum")
    assert_guards_intact(ob, of, og, aux, og2, auxd, orr, od, cs, acc)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("splits", [2, 3])
@pytest.mark.parametrize("a_kmaj,b_kmaj", LAYOUTS)
def test_gemm_split_k_edges(impl, splits, a_kmaj, b_kmaj):
    M, N, K = 77, 264, 4160
    d = gemm_data(M, N, K)
    A, B = _store(d["a"], a_kmaj), _store(d["b"], b_kmaj)
    fresh = _g(M, N, F32)
    acc = _g(M, N, F32, fill=d["acc0"])
    _lib.set_gemm_impl(impl)
    _lib.set_gemm_splits(splits)
    try:
        gemm(A, B, a_kmaj=a_kmaj, b_kmaj=b_kmaj, out=fresh)
        gemm(A, B, a_kmaj=a_kmaj, b_kmaj=b_kmaj, out=acc, accumulate=True)
    finally:
        _lib.set_gemm_impl(-1)
        _lib.set_gemm_splits(0)
    _check_gemm(d, K, fresh, "plain")
    _check_gemm(d, K, acc, "acc")
    assert_guards_intact(fresh, acc)


@pytest.mark.parametrize("a_kmaj,b_kmaj", LAYOUTS)
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_f32_operand_edges(a_kmaj, b_kmaj, M, N, K):
    """csrc/gemm_f32.hip (f32 operands on the f32 matrix cores): plain and bias + GELU + aux."""
    d = gemm_data(M, N, K, F32)
    A, B = _store(d["a"], a_kmaj), _store(d["b"], b_kmaj)
    of, og, aux = _g(M, N, F32), _g(M, N, F32), _g(M, N, F32)
    gemm(A, B, a_kmaj=a_kmaj, b_kmaj=b_kmaj, out=of)
    gemm(A, B, a_kmaj=a_kmaj, b_kmaj=b_kmaj, out=og, bias=d["bias"], act=2, aux_out=aux)
    fam = "gemm f32 operands (fraction of the element bound)"
    for out, ref, lip in ((of, "plain", 1.0), (og, "gelu", GELU_LIPSCHITZ), (aux, "pre", 1.0)):
        assert_elem_bound(out, d[ref], gemm_elem_bound(d["a"], d["b"], d[ref], F32, K, lip), what=ref, family=fam)
    assert_guards_intact(of, og, aux)


# ---------------------------------------------------------------- attention
def _pad_mask(N, S):
    pad = torch.zeros(N, S, dtype=torch.bool, device=dev)
    pad[0, S - S // 4:] = True  # right padding
    pad[1, 5:9] = True          # an interior gap
    return pad


ATTN_CASES = ([(hd, S, True, wp) for hd in (32, 64, 128, 96) for S in (1, 63, 65, 129, 200) for wp in (False, True)]
              + [(hd, 129, False, False) for hd in (32, 64, 128, 96)]
              # the hd 32 forward changes kernel at S = 512; 513 is 5 query blocks, so the middle
              # block pairs with itself
              + [(32, S, True, wp) for S in (511, 513) for wp in (False, True)])


@pytest.mark.parametrize("hd,S,causal,with_pad", ATTN_CASES)
def test_attention_edges(hd, S, causal, with_pad):
    """Forward and backward per query / token row; o and dqkv in guard bands.  The ideal backward
    is the plain f32 math on what the kernel is handed: the bf16 output of the (ideal) forward."""
    N, H = 2, 2
    T, E = N * S, H * hd
    torch.manual_seed(1000 * hd + S)
    qkv = torch.randn(T, 3 * E, device=dev).bfloat16()
    do_buf = torch.randn(T, E + 8, device=dev).bfloat16()
    do = do_buf[:, :E]
    pad = _pad_mask(N, S) if with_pad else None
    o = guarded((T, E), BF, dev, ld=E + 8)
    o_ret, lse = attention_fwd(qkv, N, S, H, hd, pad, causal=causal, out=o)
    assert o_ret.data_ptr() == o.data_ptr()
    dqkv = guarded((T, 3 * E), BF, dev, ld=3 * E + 8)
    attention_bwd(do, qkv, o, lse, N, S, H, hd, pad, causal=causal, dqkv=dqkv)

    x = qkv.double().requires_grad_(True)
    o64, lse64 = attention_plain(x, N, S, H, hd, pad, causal)
    (g64,) = torch.autograd.grad(o64, x, do.double())
    o64, lse64 = o64.detach(), lse64.detach()
    o32, lse32 = attention_plain(qkv, N, S, H, hd, pad, causal, dtype=F32)
    o_ideal = o32.bfloat16()
    g_ideal = attention_bwd_plain(qkv, do, o_ideal, lse32, N, S, H, hd, pad, causal, dtype=F32).bfloat16()

    assert_local_close(o, o64, o_ideal, MARGIN_ATTN, axes="rows", what="o", family="attention fwd")
    fin = torch.isfinite(lse64)
    assert torch.isfinite(lse[fin]).all()
    assert torch.allclose(lse[fin].double(), lse64[fin], atol=2e-2, rtol=1e-3)
    # A causal query 0 sees one key: P = 1 and dS = dP - delta = do.v - do.o is zero only by
    # cancellation of two f32 sums over hd, so the dq rows it makes (and dk, when S = 1 leaves
    # nothing else) are no structural zeros.  They are held to the product bound of
    # gemm_elem_bound with K = hd: |dS| <= 4 hd 2^-24 |do|.|v|, times |k| (or |q|) / sqrt(hd),
    # and the output's bf16 rounding; every other row is checked against the ideal's floor.
    first = torch.zeros(T, dtype=torch.bool, device=dev)
    if causal:
        first[torch.arange(N, device=dev) * S] = True

        def per_head(t):
            return t[first].double().abs().reshape(N, H, hd)

        ds = 4 * hd * 2.0 ** -24 * (per_head(do) * per_head(qkv[:, 2 * E:])).sum(-1, keepdim=True)
        for name, sl, other in (("dq", slice(0, E), slice(E, 2 * E)), ("dk", slice(E, 2 * E), slice(0, E))):
            if name == "dq" or S == 1:
                bound = (1 + 2.0 ** -7) * ds * per_head(qkv[:, other]) / math.sqrt(hd)
                assert_elem_bound(dqkv[first][:, sl], g64[first][:, sl], bound.reshape(N, E), what=name + " of query 0")
    for i, name in enumerate(("dq", "dk", "dv")):
        sl = slice(i * E, (i + 1) * E)
        rows = ~first if (name == "dq" or (name == "dk" and S == 1)) else torch.ones_like(first)
        if rows.any():
            assert_local_close(dqkv[rows][:, sl], g64[rows][:, sl], g_ideal[rows][:, sl], MARGIN_ATTN, axes="rows",
                               what=name, family=f"attention {name}")
    if causal and not with_pad:
        # softmax over one key is 1: the first row of every sequence and head is v[0], bit for bit
        rows = torch.arange(N, device=dev) * S
        assert torch.equal(o[rows], qkv[rows, 2 * E:])
    assert_guards_intact(o, dqkv)


# ---------------------------------------------------------------- LayerNorm
def _ln64(x, g, b, eps=1e-5):
    x = x.double()
    mean = x.mean(-1)
    rstd = torch.rsqrt(x.var(-1, unbiased=False) + eps)
    return (x - mean[:, None]) * rstd[:, None] * g.double() + b.double(), mean, rstd


def _ln32(x, g, b, eps=1e-5):
    mean = x.mean(-1)
    rstd = torch.rsqrt(x.var(-1, unbiased=False) + eps)
    return (x - mean[:, None]) * rstd[:, None] * g + b, mean, rstd


def _ln_bwd(dy, x, mean, rstd, g, dres):
    """(dx, dgamma, dbeta) of LN + the residual gradient, in the dtype of the operands."""
    xh = (x - mean[:, None]) * rstd[:, None]
    dg = dy * g
    s1 = dg.mean(-1, keepdim=True)
    s2 = (dg * xh).mean(-1, keepdim=True)
    return dres + rstd[:, None] * (dg - s1 - xh * s2), (dy * xh).sum(0), dy.sum(0)


def _seq_sum(v, start):
    """Column sums the plainest way: one f32 accumulator per column, rows added in order."""
    acc = torch.full_like(v[0], start) if not torch.is_tensor(start) else start.clone()
    for t in range(v.shape[0]):
        acc = acc + v[t]
    return acc


def _sum_orders(v, start):
    """The column sums of v (+ start) as plain f32 PyTorch makes them in four orders: rows first
    to last, last to first, torch's own reduction, and four rows at a time (a workgroup's rows
    in one sweep of the row kernels) with the groups' sums added first to last.  The kernels add
    their workgroups' sums with atomics, in an order that changes from launch to launch, and any
    fixed order is one sample of that.  The fourth came with the cases of more than one sweep:
    LayerNorm's gsum at T = 1026, D = 100 measured at most 1.48 x the floor of the first three in
    60 launches and 2.00 x in one more (test_kernel_trips_gpu.py)."""
    T = v.shape[0]
    pad = torch.cat([v, torch.zeros((-T) % 4, *v.shape[1:], device=v.device, dtype=v.dtype)])
    groups = pad.reshape(-1, 4, *v.shape[1:])
    by_group = _seq_sum(((groups[:, 0] + groups[:, 1]) + groups[:, 2]) + groups[:, 3], start)
    return [_seq_sum(v, start), _seq_sum(v.flip(0), start), start + v.sum(0), by_group]


def _row_sum(v, order):
    """The row sums of v in plain f32 PyTorch: columns first to last (0), last to first (1), or
    torch's own reduction (2)."""
    if order == 2:
        return v.sum(-1)
    acc = torch.zeros_like(v[:, 0])
    D = v.shape[1]
    for j in range(D):
        acc = acc + v[:, j if order == 0 else D - 1 - j]
    return acc


def _check_stats(x32, x64, mean, rstd, what):
    """Row statistics per element against f64, within MARGIN x the largest element error of the
    ideal: the two-pass mean and variance in plain f32, summed in three orders."""
    D = x32.shape[1]
    x64 = x64.double()
    mean64 = x64.mean(-1)
    rstd64 = torch.rsqrt(x64.var(-1, unbiased=False) + 1e-5)
    means = [_row_sum(x32, k) / D for k in range(3)]
    rstds = [torch.rsqrt(_row_sum((x32 - means[k][:, None]) ** 2, k) / D + 1e-5) for k in range(3)]
    assert_elem_close(mean, mean64, means, MARGIN, what=what + " mean", family="layernorm mean", ulp_floor=True)
    assert_elem_close(rstd, rstd64, rstds, MARGIN, what=what + " rstd", family="layernorm rstd", ulp_floor=True)


# Every case of the dispatchers' switch ((D + 255) / 256, 64 lanes x 4 columns per vector, NV
# vectors per lane).  4: the smallest the kernel takes (D % 4 == 0, ops/norm.py), NV 1; 100: NV 1
# ragged; 260: NV 2 with one live lane in the second vector; 768: NV 3; 1024 / 1280: NV 4 / 5 full
# (GPT-2 medium / large); 1300: NV 6 ragged; 1600: NV 7; 1796: NV 8 with one live lane in the
# last vector; 2048: NV 8 full, the widest
LN_DIMS = [4, 100, 260, 768, 1024, 1280, 1300, 1600, 1796, 2048]
LN_DIMS_BF16_DY = [100, 1024, 2048]  # the bf16-dy instantiations: NV 1 ragged, 4 and 8 full


@pytest.mark.parametrize("D", LN_DIMS)
@pytest.mark.parametrize("T", [1, 67])
def test_layernorm_fwd_edges(T, D):
    """Plain forward and the fused residual input xs = x + keep * relu(y + bias) with x_out.
    (ReLU: x_out is an f32 output whose ideal floor is one f32 rounding, and only ReLU is exact
    enough on the device to be held to it; GELU's tanh is covered at 1e-5 in
    test_layernorm_fwd_fused_residual_add.)  x is centred on 3 so that no row mean cancels."""
    torch.manual_seed(31 * D + T)
    x = torch.randn(T, D, device=dev) + 3
    g, b = torch.randn(D, device=dev), torch.randn(D, device=dev)
    y = guarded((T, D), BF, dev, ld=_ld(D))
    _, mean, rstd = layernorm_fwd(x, g, b, out=y)
    y64, mean64, rstd64 = _ln64(x, g, b)
    y32 = _ln32(x, g, b)[0]
    assert_local_close(y, y64, y32.bfloat16(), MARGIN, axes="rows", what="y", family="layernorm y")
    _check_stats(x, x, mean, rstd, "plain")
    # fused input
    ya = torch.randn(T, D, device=dev).bfloat16()
    ba = torch.randn(D, device=dev)
    drop = DropSpec.make(0.2, seed=5, site=3)
    keep = keep_mask(drop, T, D, dev)
    xs = guarded((T, D), F32, dev, ld=_ld(D))
    h = guarded((T, D), BF, dev, ld=_ld(D))
    _, mu, rs = layernorm_fwd(x, g, b, 1e-5, BF, out=h, add=(ya, ba, drop, 1), x_out=xs)
    xs64 = x.double() + keep.double() * torch.relu(ya.double() + ba.double())
    xs32 = x + keep * torch.relu(ya.float() + ba)
    assert_local_close(xs, xs64, xs32, MARGIN, axes="rows", what="x_out", family="layernorm x_out")
    h64, mu64, rs64 = _ln64(xs64, g, b)
    h32 = _ln32(xs32, g, b)[0]
    assert_local_close(h, h64, h32.bfloat16(), MARGIN, axes="rows", what="fused y", family="layernorm y")
    _check_stats(xs32, xs64, mu, rs, "fused")
    # the same with GELU: its bf16 output against the bf16 floor (x_out's f32 floor: see above)
    xs_g = guarded((T, D), F32, dev, ld=_ld(D))
    h_g = guarded((T, D), BF, dev, ld=_ld(D))
    layernorm_fwd(x, g, b, 1e-5, BF, out=h_g, add=(ya, ba, drop, 2), x_out=xs_g)
    xg64 = x.double() + keep.double() * gelu64(ya.double() + ba.double())
    xg32 = x + keep * F.gelu(ya.float() + ba, approximate="tanh")
    assert_local_close(h_g, _ln64(xg64, g, b)[0], _ln32(xg32, g, b)[0].bfloat16(), MARGIN, axes="rows",
                       what="fused GELU y", family="layernorm y")
    assert_guards_intact(y, xs, h, xs_g, h_g)


@contextlib.contextmanager
def _ln_bwd_mode(pf, blocks=0):
    """The LayerNorm backward with the row-prefetch kernel (1) or the one-row kernel (0), and
    with ``blocks`` > 0 its persistent grid pinned to that many workgroups."""
    lib = _lib.lib()
    lib.dpc_layernorm_set_bwd_prefetch(pf)
    lib.dpc_layernorm_set_bwd_blocks(blocks)
    try:
        yield
    finally:
        lib.dpc_layernorm_set_bwd_prefetch(-1)
        lib.dpc_layernorm_set_bwd_blocks(0)


def check_layernorm_bwd(T, D, pf, dy_bf16=False, blocks=0):
    """dx (accumulated and dx_set), dgamma, dbeta, and the fused consumer gout = bf16(dx * keep *
    relu'(gz)) with gsum; mean / rstd are the exact f64 statistics rounded to f32, as handed to
    every implementation.  ``dy_bf16``: the kernel is handed dy rounded to bf16 (the DYB
    instantiations), and the reference and the ideal use the rounded values."""
    torch.manual_seed(17 * D + T)
    x = torch.randn(T, D, device=dev) + 3
    g = torch.randn(D, device=dev)
    dy = torch.randn(T, D, device=dev)
    dy_k = dy.bfloat16() if dy_bf16 else dy  # what the kernel reads
    dy = dy_k.float()
    dres = torch.randn(T, D, device=dev)
    _, mean64, rstd64 = _ln64(x, g, torch.zeros(D, device=dev))
    mean, rstd = mean64.float(), rstd64.float()
    gz = torch.randn(T, D, device=dev).bfloat16()
    drop = DropSpec.make(0.2, seed=7, site=1)
    keep = keep_mask(drop, T, D, dev)
    dx = guarded((T, D), F32, dev, ld=_ld(D), fill=dres)
    dx_only = guarded((T, D), F32, dev, ld=_ld(D))  # dx_set: the NaN sentinel inside is never read
    dx2 = guarded((T, D), F32, dev, ld=_ld(D), fill=dres)
    dgam, dbet = guarded(D, F32, dev, fill=0.5), guarded(D, F32, dev, fill=-0.5)
    scratch = [guarded(D, F32, dev, fill=0.0) for _ in range(4)]
    gout = guarded((T, D), BF, dev, ld=_ld(D))
    gsum = guarded(D, F32, dev, fill=1.0)
    with _ln_bwd_mode(pf, blocks):
        layernorm_bwd(dy_k, x, mean, rstd, g, dx, dgam, dbet)
        layernorm_bwd(dy_k, x, mean, rstd, g, dx_only, scratch[0], scratch[1], dx_set=True)
        layernorm_bwd(dy_k, x, mean, rstd, g, dx2, scratch[2], scratch[3], gout=gout, gsum=gsum, drop=drop,
                      gz=gz, gact=1)
    m64, r64 = mean.double(), rstd.double()
    dx64, dg64, db64 = _ln_bwd(dy.double(), x.double(), m64, r64, g.double(), dres.double())
    dx32 = _ln_bwd(dy, x, mean, rstd, g, dres)[0]
    xh32 = (x - mean[:, None]) * rstd[:, None]
    fam = "layernorm bwd"
    assert_local_close(dx, dx64, dx32, MARGIN, axes="rows", what="dx", family=fam + " dx")
    assert_local_close(dx2, dx64, dx32, MARGIN, axes="rows", what="dx beside gout", family=fam + " dx")
    zero = torch.zeros_like(dres)
    assert_local_close(dx_only, _ln_bwd(dy.double(), x.double(), m64, r64, g.double(), zero.double())[0],
                       _ln_bwd(dy, x, mean, rstd, g, zero)[0], MARGIN, axes="rows", what="dx_set", family=fam + " dx")
    assert_elem_close(dgam, 0.5 + dg64, _sum_orders(dy * xh32, 0.5), MARGIN, what="dgamma", family=fam + " dgamma")
    assert_elem_close(dbet, -0.5 + db64, _sum_orders(dy, -0.5), MARGIN, what="dbeta", family=fam + " dbeta")
    dg_orders, db_orders = _sum_orders(dy * xh32, 0.0), _sum_orders(dy, 0.0)
    for k in (0, 2):
        assert_elem_close(scratch[k], dg64, dg_orders, MARGIN, what="dgamma", family=fam + " dgamma")
        assert_elem_close(scratch[k + 1], db64, db_orders, MARGIN, what="dbeta", family=fam + " dbeta")
    mask64 = keep.double() * dact64(gz, 1)
    go64 = dx64 * mask64
    go32 = dx32 * keep * (gz.float() > 0).float()
    assert_local_close(gout, go64, go32.bfloat16(), MARGIN, axes="rows", what="gout", family=fam + " gout")
    assert_elem_close(gsum, 1.0 + go64.sum(0), _sum_orders(go32, 1.0), MARGIN, what="gsum", family=fam + " gsum")
    # the same consumer with GELU': its bf16 gout against the bf16 floor (gsum's f32 floor holds
    # for the exact ReLU' only; GELU' on the device is an approximation)
    dx3 = guarded((T, D), F32, dev, ld=_ld(D), fill=dres)
    gout_g, gsum_g = guarded((T, D), BF, dev, ld=_ld(D)), guarded(D, F32, dev, fill=1.0)
    extra = [guarded(D, F32, dev, fill=0.0) for _ in range(2)]
    with _ln_bwd_mode(pf, blocks):
        layernorm_bwd(dy_k, x, mean, rstd, g, dx3, extra[0], extra[1], gout=gout_g, gsum=gsum_g, drop=drop,
                      gz=gz, gact=2)
    gg64 = dx64 * keep.double() * dgelu64(gz)
    gg32 = (dx32.double() * keep.double() * dgelu64(gz)).float()  # (f32 dx, GELU' exact, one rounding)
    assert_local_close(gout_g, gg64, gg32.bfloat16(), MARGIN, axes="rows", what="gout GELU'", family=fam + " gout")
    assert_guards_intact(dx, dx_only, dx2, dgam, dbet, *scratch, gout, gsum, dx3, gout_g, gsum_g, *extra)


# (ids: the f32-dy cases keep the names they had before dy_bf16 was a parameter)
LN_BWD_CASES = ([pytest.param(T, D, pf, False, id=f"{T}-{D}-{pf}") for pf in (1, 0) for D in LN_DIMS for T in (1, 67)]
                + [pytest.param(T, D, pf, True, id=f"{T}-{D}-{pf}-dy_bf16")
                   for pf in (1, 0) for D in LN_DIMS_BF16_DY for T in (1, 67)])


@pytest.mark.parametrize("T,D,pf,dy_bf16", LN_BWD_CASES)
def test_layernorm_bwd_edges(T, D, pf, dy_bf16):
    """check_layernorm_bwd at one row and at 67 (a ragged last workgroup), both kernels, f32 dy
    at every width class and bf16 dy at three of them."""
    check_layernorm_bwd(T, D, pf, dy_bf16)


def test_layernorm_refuses_wide_rows():
    """D = 2052 is past the widest instantiation (8 vectors per lane): both directions raise."""
    T, D = 3, 2052
    x = torch.randn(T, D, device=dev)
    g, b = torch.randn(D, device=dev), torch.randn(D, device=dev)
    with pytest.raises(ValueError, match="D <= 2048"):
        layernorm_fwd(x, g, b)
    dx = guarded((T, D), F32, dev, fill=0.0)
    dgam, dbet = guarded(D, F32, dev, fill=0.0), guarded(D, F32, dev, fill=0.0)
    stat = torch.ones(T, device=dev)
    with pytest.raises(ValueError, match="D <= 2048"):
        layernorm_bwd(x, x, stat, stat, g, dx, dgam, dbet)
    assert torch.count_nonzero(dx) == 0 and torch.count_nonzero(dgam) == 0 and torch.count_nonzero(dbet) == 0
    assert_guards_intact(dx, dgam, dbet)


# ---------------------------------------------------------------- cross-entropy
# V -> ld = ceil64(V) -> 16-B chunks per thread of 512 (misc.hip: dpc_cross_entropy).  Mode 0:
# 1000 ce_kernel2<1>; 4104 <2> nearly empty (ld 4160, one chunk past 4096); 8192 <2> full; 8200 <4>
# just past <2>; 32768 <8> full; 50257 <13> (GPT-2); 53250 <16> ragged (ld 53312 > 13 x 4096);
# 65536 <16> full, the last register-resident width; 65537 and 70001 the streaming kernel.
CE_CASES = ([(1000, 0), (50257, 0), (50257, 1), (50257, 2), (50257, 3), (70001, 0)]
            + [(V, 0) for V in (4104, 8192, 8200, 32768, 53250, 65536, 65537)])


def _ce_targets(T, V):
    """Random targets with every 7th row ignored; at T = 37 also the targets a kernel can get
    wrong by position -- 0, V - 1, the first index of the tail chunk (V & 7) or of the last
    chunk, one inside the last full chunk, and 8 * 512 * k (the first chunk of a thread's k-th
    register) -- and rows 8 / 9 for the planted ties (their targets are set with the ties)."""
    tg = torch.randint(0, V, (T,), device=dev)
    if T > 1:
        tg[::7] = -100
    if T >= 37:
        last_full = V // 8 * 8 - (8 if V % 8 == 0 else 0)  # start of the last chunk / the tail chunk
        k = (V - 1) // 4096
        fixed = [0, V - 1, last_full, last_full - 3, 4096 * k, 4096 * max(k // 2, 0)]
        for row, t in zip((1, 2, 3, 4, 5, 6), fixed):
            tg[row] = t
    return tg


@pytest.mark.parametrize("V,mode", CE_CASES)
@pytest.mark.parametrize("T", [1, 37])
def test_cross_entropy_edges(T, V, mode):
    """Per-row loss and gradient rows (the default dispatch at every register-resident width and
    at the first streamed one, the three forced modes at V = 50257 -- 3 is the older
    register-resident ce_kernel<13> -- and the streaming fallback at V = 70001), in place in a
    guarded [T, ld] buffer.  At T = 37 rows 8 and 9 hold the row maximum twice, in different
    chunks (the maximum copied to a column half a row away): the target on the first is a hit,
    the target on the last is not.

    [37-53250-0]: row 9's target is the row maximum, so its loss is log(s) = 5.012 alone.  With an
    f32 log the kernel returned the float below the correctly rounded one there, 1.33 ulp from
    the f64 value and 2.08 x the floor, although its s is within 4e-8; the kernels now take the
    log in f64 (misc.hip: ce_kernel2)."""
    torch.manual_seed(V + T)
    ld = (V + 63) // 64 * 64
    vals = (torch.randn(T, V, device=dev) * 2).bfloat16()
    tg = _ce_targets(T, V)
    if T >= 37:
        for r in (8, 9):  # the row's maximum a second time, half a row away from the first
            top = vals[r].max()
            vals[r, (int(first_argmax(vals[r:r + 1])) + V // 2 + 5) % V] = top
            at = (vals[r] == top).nonzero().flatten()
            tg[r] = at[0] if r == 8 else at[-1]
    buf = guarded((T, ld), BF, dev, fill=0.0)
    buf[:, :V] = vals
    valid = tg != -100
    inv = (1.0 / valid.sum().clamp_min(1).float()).reshape(1)
    row_loss = guarded(T, F32, dev)
    row_correct = guarded(T, F32, dev)
    _lib.lib().dpc_ce_set_mode(mode)
    try:
        cross_entropy_rows(buf, tg, V, inv, row_loss, row_correct)
    finally:
        _lib.lib().dpc_ce_set_mode(-1)
    check_cross_entropy(row_loss, buf[:, :V], buf[:, V:], row_correct, vals, tg, inv)
    if T >= 37:
        assert row_correct[8] == 1.0 and row_correct[9] == 0.0
    assert_guards_intact(buf, row_loss, row_correct)


# ---------------------------------------------------------------- AdamW
def _adam64(p, m, v, g, t, lr, b1, b2, eps, wd):
    p = p * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1 - b2 ** t) + eps
    return p - (lr / (1 - b1 ** t)) * m / denom, m, v


@pytest.mark.parametrize("variant", ["plain", "grad_scale_t", "skip_all", "device_step"])
@pytest.mark.parametrize("n", [4, 2052, 4096 + 12])
def test_adamw_subrange_edges(n, variant):
    """FlatAdamW.update on sub-ranges, three steps with new gradients, against f64 AdamW.  Inside
    [lo, hi): param within 4 ulp (relative, f32) of the f64 result and shadow == bf16(param) bit
    for bit; outside, param / exp_avg / exp_avg_sq / shadow and every guard bit-unchanged.
    |param| >= 0.5 so that a 1e-3 update cannot cancel the parameter it is measured against.
    device_step: the second of the three steps is skipped on the device (skip_t = 1), so the
    third runs with the device count 2 while the host count says 3."""
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.999, 1e-8, 1e-2
    ranges = [r for r in ((0, n), (4, n - 4), (1028, 1032)) if 0 <= r[0] < r[1] <= n]
    for lo, hi in ranges:
        torch.manual_seed(n + lo)
        p0 = torch.randn(n, device=dev)
        p0 = torch.where(p0 >= 0, p0 + 0.5, p0 - 0.5)
        p = guarded(n, F32, dev, fill=p0)
        g = guarded(n, F32, dev, fill=0.0)
        sh = guarded(n, BF, dev, fill=7.0)
        opt = FlatAdamW(p, g, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, shadow=sh)
        opt.exp_avg = guarded(n, F32, dev, fill=0.0)
        opt.exp_avg_sq = guarded(n, F32, dev, fill=0.0)
        p64, m64, v64 = p0.double(), torch.zeros(n, device=dev, dtype=torch.float64), torch.zeros(
            n, device=dev, dtype=torch.float64)
        scale_t = torch.full((1,), 0.5, device=dev) if variant == "grad_scale_t" else None
        t_dev = 0
        for step in range(3):
            g.normal_()
            skip = {"plain": None, "grad_scale_t": None, "skip_all": 1.0,
                    "device_step": 1.0 if step == 1 else 0.0}[variant]
            skip_t = None if skip is None else torch.full((), skip, device=dev)
            before = [t.clone() for t in (p, opt.exp_avg, opt.exp_avg_sq, sh)]
            opt.begin_step(skip_t)
            opt.update(lo, hi, grad_scale_t=scale_t, skip_t=skip_t)
            if skip:
                for t, b in zip((p, opt.exp_avg, opt.exp_avg_sq, sh), before):
                    assert torch.equal(t.view(torch.int16 if t.dtype == BF else torch.int32),
                                       b.view(torch.int16 if t.dtype == BF else torch.int32))
            else:
                t_dev += 1
                gs = g.double() * (0.5 if scale_t is not None else 1.0)
                pn, mn, vn = _adam64(p64, m64, v64, gs, t_dev, lr, b1, b2, eps, wd)
                p64[lo:hi], m64[lo:hi], v64[lo:hi] = pn[lo:hi], mn[lo:hi], vn[lo:hi]
            if variant in ("skip_all", "device_step"):
                assert float(opt.step_t) == t_dev  # the device count leaves the skipped steps out
        inside = torch.zeros(n, dtype=torch.bool, device=dev)
        inside[lo:hi] = True
        assert_elem_bound(p[inside], p64[inside], 4 * 2.0 ** -23 * p64[inside].abs(), what=f"param [{lo},{hi})",
                          family="adamw (fraction of 4 ulp)")
        if variant != "skip_all":
            assert torch.equal(sh[inside].view(torch.int16), p[inside].bfloat16().view(torch.int16))
            assert (opt.exp_avg[inside] != 0).all() and (opt.exp_avg_sq[inside] != 0).all()
        out = ~inside
        assert torch.equal(p[out], p0[out])
        assert torch.count_nonzero(opt.exp_avg[out]) == 0 and torch.count_nonzero(opt.exp_avg_sq[out]) == 0
        assert torch.equal(sh[out].float(), torch.full_like(sh[out], 7.0).float())
        assert_guards_intact(p, g, sh, opt.exp_avg, opt.exp_avg_sq)


# ---------------------------------------------------------------- the remaining kernels
@pytest.mark.parametrize("tdt", [F32, BF])
def test_embedding_edges(tdt):
    torch.manual_seed(5)
    V, P, D, T = 37, 9, 100, 3 * 7
    tok = torch.randn(V, D, device=dev).to(tdt)
    pt = torch.randn(P, D, device=dev).to(tdt)
    ids = torch.randint(0, V, (T,), device=dev)
    ids[-1] = V - 1
    pos = torch.arange(7, device=dev).repeat(3)
    x = guarded((T, D), F32, dev)
    embedding_fwd(ids, pos, tok, pt, out=x)
    ref64 = tok[ids].double() + pt[pos].double()
    assert_local_close(x, ref64, tok[ids].float() + pt[pos].float(), MARGIN, axes="rows", what="embedding",
                       family="embedding fwd")
    # backward into guarded tables, one id out of range (ignored)
    dx = torch.randn(T, D, device=dev)
    bt, bp = torch.randn(V, D, device=dev), torch.randn(P, D, device=dev)
    dt, dp = guarded((V, D), F32, dev, fill=bt), guarded((P, D), F32, dev, fill=bp)
    ids2 = ids.clone()
    ids2[3] = V + 5
    embedding_bwd(dx, ids2, pos, dt, dp)
    ok = ids2 < V
    rt64 = bt.double().index_add_(0, ids2[ok], dx[ok].double())
    rp64 = bp.double().index_add_(0, pos, dx.double())
    rt32 = bt.clone().index_add_(0, ids2[ok], dx[ok])
    rp32 = bp.clone().index_add_(0, pos, dx)
    # rows no token names are bit-unchanged; the others within the ideal's own f32 summation error
    untouched = torch.ones(V, dtype=torch.bool, device=dev)
    untouched[ids2[ok]] = False
    assert torch.equal(dt[untouched], bt[untouched])
    assert_local_close(dt, rt64, rt32, MARGIN, axes="rows", what="dtok", family="embedding bwd")
    assert_local_close(dp, rp64, rp32, MARGIN, axes="rows", what="dpos", family="embedding bwd")
    assert_guards_intact(x, dt, dp)


def test_dropout_residual_edges():
    torch.manual_seed(13)
    T, N = 67, 100
    spec = DropSpec.make(0.1, seed=(5 << 32) | 17, site=9)
    y, r = torch.randn(T, N, device=dev), torch.randn(T, N, device=dev)
    out = guarded((T, N), F32, dev, ld=_ld(N))
    dropout_residual(y, r, spec, out=out)
    keep = keep_mask(spec, T, N, dev)
    assert_local_close(out, r.double() + y.double() * keep.double(), r + y * keep, MARGIN, axes="rows",
                       what="dropout_residual", family="elementwise")
    assert torch.equal(out == r, (keep == 0) | (y == 0))
    assert_guards_intact(out)


@pytest.mark.parametrize("act", [0, 1, 2])
def test_bias_act_bwd_edges(act):
    torch.manual_seed(8)
    T, N = 67, 100
    dy = torch.randn(T, N, device=dev)
    z = torch.randn(T, N, device=dev).bfloat16()
    db = guarded(N, F32, dev, fill=0.25)
    dz = guarded((T, N), BF, dev, ld=_ld(N))
    bias_act_bwd(dy, z, act, db, out=dz)
    d64 = dact64(z, act) if act else torch.ones(T, N, device=dev, dtype=torch.float64)
    ref64 = dy.double() * d64
    ideal32 = dy * d64.float()
    assert_local_close(dz, ref64, ideal32.bfloat16(), MARGIN, axes="both", what="dz", family="elementwise")
    if act != 2:  # (GELU' on the device is an approximation: db's f32 floor holds for the exact forms)
        assert_elem_close(db, 0.25 + ref64.sum(0), _sum_orders(ideal32, 0.25), MARGIN, what="db",
                          family="bias_act_bwd db")
    assert_guards_intact(db, dz)


@pytest.mark.parametrize("n", [4, 1028])
def test_cast_edges(n):
    torch.manual_seed(n)
    src = torch.randn(n, device=dev)
    dst = guarded(n, BF, dev)
    cast_f32_bf16(src, dst)
    assert torch.equal(dst.view(torch.int16), src.bfloat16().view(torch.int16))
    assert_guards_intact(dst)


# M = 1, 2, 9, 16 launch gemv_kernel<1>, <2>, <16> with 7 masked rows, <16> full (<4> and <8>:
# test_kernels_gpu.py).  K = 64: one trip of the K loop that lanes 0..7 enter; K = 520: a second
# trip (k = 512) that only lane 0 enters.  (ids: the K = 64 cases keep the names they had.)
FEW_ROWS_CASES = ([pytest.param(epi, M, 64, id=f"{epi}-{M}") for M in (1, 16, 2, 9)
                   for epi in ("plain", "bias_gelu", "bias_relu_res")]
                  + [pytest.param(epi, M, 520, id=f"{epi}-{M}-K520") for M in (1, 16, 2, 9)
                     for epi in ("plain", "bias_gelu", "bias_relu_res")])


@pytest.mark.parametrize("epi,M,K", FEW_ROWS_CASES)
def test_linear_few_rows_edges(epi, M, K):
    """csrc/decode.hip dpc_gemv through linear_fwd(out=): Nw = 100 weight rows into N = 104 output
    columns (the padding written as 0), K = 64 or 520."""
    Nw, N = 100, 104
    torch.manual_seed(7 + M)
    x = torch.randn(M, K, device=dev).bfloat16()
    w = (torch.randn(Nw, K, device=dev) / K ** 0.5).bfloat16()
    bias = torch.randn(Nw, device=dev) if epi != "plain" else None
    act = {"plain": 0, "bias_gelu": 2, "bias_relu_res": 1}[epi]
    res = torch.randn(M, N, device=dev) if epi == "bias_relu_res" else None
    odt = F32 if res is not None else BF
    out = guarded((M, N), odt, dev, ld=N + 8)
    y = linear_fwd(x, w, bias=bias, act=act, residual=res, out=out, out_dtype=odt)
    assert y.data_ptr() == out.data_ptr()
    ref = x.double() @ w.double().t()
    if bias is not None:
        ref = ref + bias.double()
    ref = gelu64(ref) if act == 2 else (torch.relu(ref) if act == 1 else ref)
    if res is not None:
        ref = ref + res[:, :Nw].double()
    assert_elem_bound(out[:, :Nw], ref, gemm_elem_bound(x, w, ref, odt, K, GELU_LIPSCHITZ if act == 2 else 1.0),
                      what=epi, family="gemv (fraction of the element bound)")
    assert torch.count_nonzero(out[:, Nw:]) == 0
    assert_guards_intact(out)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("pos", [0, 37])
def test_decode_attention_edges(hd, pos):
    """The KV caches are guarded: row ``pos`` receives the new key / value and nothing after it
    (or anywhere else) changes."""
    torch.manual_seed(7)
    N, H, Smax = 2, 3, 40
    E = H * hd
    k0 = torch.randn(N, Smax, E, device=dev).bfloat16()
    v0 = torch.randn(N, Smax, E, device=dev).bfloat16()
    kc, vc = guarded((N, Smax, E), BF, dev, fill=k0), guarded((N, Smax, E), BF, dev, fill=v0)
    qkv = torch.randn(N, 3 * E, device=dev).bfloat16()
    length = torch.full((1,), pos, device=dev, dtype=torch.int64)
    o = decode_attention(qkv, kc, vc, length, H, hd)
    k0[:, pos], v0[:, pos] = qkv[:, E:2 * E], qkv[:, 2 * E:]
    assert torch.equal(kc, k0) and torch.equal(vc, v0)
    L = pos + 1

    def run(dt):
        q = qkv[:, :E].to(dt).reshape(N, H, 1, hd)
        k = k0[:, :L].to(dt).reshape(N, L, H, hd).transpose(1, 2)
        v = v0[:, :L].to(dt).reshape(N, L, H, hd).transpose(1, 2)
        return (torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), -1) @ v).reshape(N * H, hd)

    assert_local_close(o.reshape(N * H, hd), run(torch.float64), run(F32).bfloat16(), MARGIN_ATTN, axes="rows",
                       what="decode o", family="decode attention")
    assert_guards_intact(kc, vc)
