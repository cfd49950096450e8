"""The edge checks of tests/kernel_checks.py, checked themselves on the CPU: an ideal kernel
(f32 product rounded to the output dtype) passes them, four small edge mutations that the global
Frobenius thresholds of test_kernels_gpu.py let through fail them, and a guard band notices a
write one element outside its view."""
import math

import pytest
import torch

import kernel_checks as kc
from kernel_checks import (MARGIN, MARGIN_ATTN, assert_elem_bound, assert_guards_intact, assert_local_close,
                           attention_plain, gemm_elem_bound, guarded, row_col_err)

SHAPES = [(1023, 768, 768), (200, 300, 136), (77, 1000, 1023), (300, 264, 96)]


def rel_err(a, b):  # the global metric of test_kernels_gpu.py
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _gemm_case(M, N, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).bfloat16()
    b = torch.randn(N, K, generator=g).bfloat16()
    bias = torch.randn(N, generator=g)
    ref64 = a.double() @ b.double().t() + bias.double()
    prod32 = a.float() @ b.float().t()
    return a, b, bias, ref64, prod32


_cache = {}


def gemm_case(M, N, K):
    if (M, N, K) not in _cache:
        _cache[(M, N, K)] = _gemm_case(M, N, K)
    return _cache[(M, N, K)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_ideal_gemm_passes(M, N, K):
    a, b, bias, ref64, prod32 = gemm_case(M, N, K)
    ideal = (prod32 + bias).bfloat16()
    # a second correct kernel: another summation order (two K halves), rounded the same way
    h = K // 2
    other = ((a[:, :h].float() @ b[:, :h].float().t()) + (a[:, h:].float() @ b[:, h:].float().t()) + bias).bfloat16()
    assert_local_close(other, ref64, ideal, MARGIN, what="bf16")
    assert_elem_bound(other, ref64, gemm_elem_bound(a, b, ref64, torch.bfloat16, K), what="bf16")
    assert_elem_bound(ideal, ref64, gemm_elem_bound(a, b, ref64, torch.bfloat16, K), what="bf16 ideal")
    other32 = (a[:, :h].float() @ b[:, :h].float().t()) + (a[:, h:].float() @ b[:, h:].float().t()) + bias
    assert_elem_bound(other32, ref64, gemm_elem_bound(a, b, ref64, torch.float32, K), what="f32")
    assert_elem_bound(prod32 + bias, ref64, gemm_elem_bound(a, b, ref64, torch.float32, K), what="f32 ideal")
    fr, fc = row_col_err(ideal, ref64)
    assert 1e-3 < fr < 3e-3 and 1e-3 < fc < 3e-3, (fr, fc)  # the bf16 floor, ~2^-9


def _mutants(M, N, K):
    a, b, bias, ref64, prod32 = gemm_case(M, N, K)
    ideal = (prod32 + bias).bfloat16()
    m1 = ideal.clone()  # the last row misses its final 32 of K (one MFMA K-step)
    m1[-1] = (a[-1:, :K - 32].float() @ b[:, :K - 32].float().t() + bias).bfloat16()
    m2 = ideal.clone()  # the last column gets no bias
    m2[:, -1] = prod32[:, -1].bfloat16()
    m3 = ideal.clone()  # one element never stored
    m3[-1, -1] = 0
    return a, b, ref64, ideal, {"tail_k": m1, "no_bias_col": m2, "zero_elem": m3}


@pytest.mark.parametrize("which", ["tail_k", "no_bias_col", "zero_elem"])
def test_gemm_edge_mutations_are_caught(which):
    M, N, K = 1023, 768, 768
    a, b, ref64, ideal, ms = _mutants(M, N, K)
    out = ms[which]
    assert rel_err(out, ref64) < 1e-2  # the old global threshold lets it through
    with pytest.raises(AssertionError):
        assert_local_close(out, ref64, ideal, MARGIN)
    with pytest.raises(AssertionError):
        assert_elem_bound(out, ref64, gemm_elem_bound(a, b, ref64, torch.bfloat16, K))


def _attn_case(S):
    N, H, hd = 1, 2, 64
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(N * S, 3 * H * hd, generator=g).bfloat16()
    ref64, _ = attention_plain(qkv, N, S, H, hd)
    ideal = attention_plain(qkv, N, S, H, hd, dtype=torch.float32)[0].bfloat16()
    return ref64, ideal, S


@pytest.mark.parametrize("row", [0, -1])
def test_attention_row_mutation_is_caught(row):
    """One query row scaled by 0.9 (an element bound does not apply to attention: the local check
    alone).  The global 1e-2 threshold happens to see row 0 (2.6e-2: a causal row 0 is v[0]
    itself, the longest row of the output at any S) but not the same error in the last row."""
    ref64, ideal, S = _attn_case(200)
    out = ideal.clone()
    out[row] = (out[row].float() * 0.9).bfloat16()
    assert_local_close(ideal, ref64, ideal, MARGIN_ATTN, axes="rows")
    fr, _ = row_col_err(ideal, ref64)
    assert 1e-3 < fr < 4e-3, fr
    if row == -1:
        assert rel_err(out, ref64) < 1e-2
    with pytest.raises(AssertionError):
        assert_local_close(out, ref64, ideal, MARGIN_ATTN, axes="rows")


def test_row_col_err_zero_reference_and_nan():
    ref = torch.zeros(3, 4, dtype=torch.float64)
    ref[0] = 1.0
    out = ref.clone().float()
    assert row_col_err(out, ref) == (0.0, 0.0)
    out[2, 1] = 1e-30  # a reference row of zeros must be exactly zero
    assert row_col_err(out, ref)[0] == math.inf
    out[2, 1] = float("nan")
    assert row_col_err(out, ref) == (math.inf, math.inf)
    with pytest.raises(AssertionError):
        assert_elem_bound(out, ref, torch.ones_like(ref))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.int64])
@pytest.mark.parametrize("offset", [False, True])
def test_guard_bands(dtype, offset):
    v = guarded((5, 13), dtype, ld=16, offset=offset, fill=0)
    raw, front, rows, cols, ld = v._guard_info
    assert v.shape == (5, 13) and v.stride() == (16, 1) and front >= 1024
    es = v.element_size()
    assert (v.data_ptr() % 16 == 0) != offset and (not offset or v.data_ptr() % 16 == es)
    v.fill_(3)  # every element of the view itself may be written
    assert_guards_intact(v)
    buf = raw.view(dtype)
    for pos, text in ((front - 1, "1 before the view"), (front + 4 * ld + cols, "1 past the last element"),
                      (front + 2 * ld + cols, "row 2 gap column 13"), (0, "before"), (raw.numel() - 1, "past")):
        old = raw[pos].clone()
        buf[pos] = 0
        with pytest.raises(AssertionError, match=text):
            assert_guards_intact(v)
        raw[pos] = old
        assert_guards_intact(v)


def test_guard_flat_and_nan_sentinel():
    v = guarded(1000, torch.float32)
    assert v.shape == (1000,) and torch.isnan(v).all()  # reading a guard poisons the result
    v.zero_()
    assert_guards_intact(v)
    assert kc.guard_touched(v).numel() == 0
    v._guard_info[0][v._guard_info[1] + 1000 + 23] = 0  # 24 past the end, as round64(1000) would
    with pytest.raises(AssertionError, match="24 past the last element"):
        assert_guards_intact(v)
    k = guarded((2, 3, 8), torch.bfloat16, fill=0)
    assert k.shape == (2, 3, 8) and k.is_contiguous()
    assert_guards_intact(k)


@pytest.mark.parametrize("causal,with_pad", [(True, False), (True, True), (False, False)])
def test_attention_bwd_plain_is_the_gradient(causal, with_pad):
    """The explicit backward that stands for the ideal kernel equals autograd of the forward."""
    N, S, H, hd = 2, 37, 2, 16
    g = torch.Generator().manual_seed(4)
    qkv = torch.randn(N * S, 3 * H * hd, generator=g, dtype=torch.float64)
    do = torch.randn(N * S, H * hd, generator=g, dtype=torch.float64)
    pad = None
    if with_pad:
        pad = torch.zeros(N, S, dtype=torch.bool)
        pad[0, S - S // 4:] = True
        pad[1, 5:9] = True
    x = qkv.clone().requires_grad_(True)
    o, lse = attention_plain(x, N, S, H, hd, pad, causal)
    (gr,) = torch.autograd.grad(o, x, do)
    mine = kc.attention_bwd_plain(qkv, do, o.detach(), lse.detach(), N, S, H, hd, pad, causal, dtype=torch.float64)
    assert torch.allclose(mine, gr, rtol=1e-10, atol=1e-12)


def test_elem_close_uses_the_ideals_largest_error():
    ref = torch.tensor([10.0, -3.0, 1e-4, 7.0], dtype=torch.float64)  # one sum cancels to almost nothing
    ideal = (ref + torch.tensor([2e-7, -1e-6, 5e-7, 0.0], dtype=torch.float64))
    out = ref + torch.tensor([-1.5e-6, 1e-6, -1.9e-6, 2e-6], dtype=torch.float64)
    kc.assert_elem_close(out, ref, [ideal, ref.clone()], MARGIN)  # every element within 2 x 1e-6
    with pytest.raises(AssertionError):  # ...which a relative view of the third element would refuse
        assert_local_close(out, ref, ideal, MARGIN, axes="cols")
    out[3] += 1e-6
    with pytest.raises(AssertionError):
        kc.assert_elem_close(out, ref, ideal, MARGIN)


def test_elem_close_ulp_floor():
    ref = torch.tensor([3.00000002], dtype=torch.float64)
    ideal = ref.float()  # one element, and the ideal happens to be the correctly rounded one
    out = torch.tensor([3.0 + 2.0 ** -22], dtype=torch.float64)  # the next f32: one ulp from the ideal
    with pytest.raises(AssertionError):
        kc.assert_elem_close(out, ref, ideal, MARGIN)
    kc.assert_elem_close(out.float(), ref, ideal, MARGIN, ulp_floor=True)  # 2 x half an ulp of 3.0..4.0
    with pytest.raises(AssertionError):
        kc.assert_elem_close(out + 4e-7, ref, ideal, MARGIN, ulp_floor=True)
