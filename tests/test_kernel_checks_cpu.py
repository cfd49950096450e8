"""The edge checks of tests/kernel_checks.py, checked themselves on the CPU: an ideal kernel
(f32 product rounded to the output dtype) passes them, four small edge mutations that the global
Frobenius thresholds of test_kernels_gpu.py let through fail them, and a guard band notices a
write one element outside its view."""
import math

import pytest
import torch

import attn_cases as ac
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


def test_attention_bwd_plain_with_dead_rows():
    """Left padding under the causal mask (query rows with no allowed key) and an all-padding
    sequence: the explicit backward equals autograd wherever a row lives, and is exactly zero in
    dq of the dead rows, in dk / dv of the padded keys and in all of the dead sequence."""
    N, S, H, hd = 3, 37, 2, 16
    E = H * hd
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(N * S, 3 * E, generator=g, dtype=torch.float64)
    do = torch.randn(N * S, E, generator=g, dtype=torch.float64)
    pad = torch.zeros(N, S, dtype=torch.bool)
    pad[0, :9] = True
    pad[1, 11:20] = True
    pad[2, :] = True
    x = qkv.clone().requires_grad_(True)
    o, lse = attention_plain(x, N, S, H, hd, pad, True)
    assert torch.equal(o[:9], torch.zeros(9, E, dtype=torch.float64)) and torch.isinf(lse[:H, :9]).all()
    assert torch.equal(o[2 * S:], torch.zeros(S, E, dtype=torch.float64)) and torch.isinf(lse[2 * H:]).all()
    (gr,) = torch.autograd.grad(o, x, do)
    mine = kc.attention_bwd_plain(qkv, do, o.detach(), lse.detach(), N, S, H, hd, pad, True, dtype=torch.float64)
    assert torch.isfinite(mine).all()
    assert torch.allclose(mine[:2 * S], gr[:2 * S], rtol=1e-10, atol=1e-12)
    zeros = torch.zeros(S, E, dtype=torch.float64)
    assert torch.equal(mine[:9, :E], zeros[:9])                    # dq of the dead query rows
    assert torch.equal(mine[:9, E:], torch.cat([zeros[:9]] * 2, 1))  # dk, dv of the padded keys
    assert torch.equal(mine[S + 11:S + 20, E:], torch.cat([zeros[:9]] * 2, 1))
    assert torch.equal(mine[2 * S:], torch.cat([zeros] * 3, 1))


# ---- the score cases of tests/attn_cases.py reach what they are for (else the GPU tests of
# test_attention_scores_gpu.py would pass without running the arms they were written for)
@pytest.mark.parametrize("hd,S", ac.SHAPES)
@pytest.mark.parametrize("profile,G", ac.PROFILES)
def test_attention_score_cases_reach_their_arms(profile, G, hd, S):
    N, H = ac.N_SEQ, ac.HEADS
    E = H * hd
    qkv = ac.attention_score_case(profile, G, hd, S)
    do = ac.attention_score_dout(profile, G, hd, S)
    assert qkv.dtype == torch.bfloat16 and qkv.shape == (N * S, 3 * E) and do.shape == (N * S, E)
    assert torch.equal(qkv, ac.attention_score_case(profile, G, hd, S))  # a function of its arguments
    assert (qkv[:, :E].reshape(-1, H, hd)[:, :, 0] == ac.A_Q).all()
    for causal in (True, False):
        for with_pad in (False, True):
            what = f"{profile} {G} hd {hd} S {S} causal {causal} pad {with_pad}"
            pad = ac.attention_score_mask(N, S) if with_pad else None
            ev = ac.rescale_event_rows(qkv, N, S, H, hd, pad, causal)
            if profile == "falling":
                assert ev == 0.0, (what, ev)
            elif G != 70:
                assert ev >= (0.05 if with_pad else 0.30), (what, ev)
            if G == 70 and ((profile == "rising" and causal) or (profile == "falling" and with_pad)):
                ex = ac.masked_excess(qkv, N, S, H, hd, pad, causal)
                assert ex >= 128.0, (what, ex)
            o64, lse64, g64, o_ideal, lse32, g_ideal = ac.score_references(qkv, do, N, S, H, hd, pad, causal)
            fr, _ = row_col_err(o_ideal, o64)
            assert 1e-3 < fr < 4e-3, (what, fr)
            assert torch.isfinite(g64).all() and torch.isfinite(g_ideal.float()).all(), what
            dead = ~torch.isfinite(lse64)  # [N H, S]
            assert bool(dead.any()) == with_pad
            if with_pad:
                assert dead[2 * H:].all() and (dead[:H, :140].all() if causal else not dead[:2 * H].any())
            if (profile, G) in ac.MODERATE:
                # what the GPU test requires of the inputs before it holds dk / dv to a row bound
                fk, _ = row_col_err(g_ideal[:, E:2 * E], g64[:, E:2 * E])
                fv, _ = row_col_err(g_ideal[:, 2 * E:], g64[:, 2 * E:])
                assert fk <= 0.1 and fv <= 5e-3, (what, fk, fv)


def test_attention_score_helpers_see_a_plain_randn_case_as_plain():
    """With randn inputs (what every other attention test uses) no row rescales with live
    accumulators and no masked score comes near an exp2 overflow."""
    N, S, H, hd = 3, 320, 2, 64
    qkv = torch.randn(N * S, 3 * H * hd, generator=torch.Generator().manual_seed(3)).bfloat16()
    pad = ac.attention_score_mask(N, S)
    for causal in (True, False):
        assert ac.rescale_event_rows(qkv, N, S, H, hd, None, causal) == 0.0
        assert ac.masked_excess(qkv, N, S, H, hd, pad, causal) < 16.0
    assert ac.masked_excess(qkv, N, S, H, hd, None, False) == -math.inf


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
