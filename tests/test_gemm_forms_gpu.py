"""The argument forms of tests/gemm_forms.py on the HIP kernels: the device scalar ``alpha_t`` on
every GEMM implementation (and that it is read afresh by every launch and every graph replay),
operands stored smaller than the logical product, every epilogue of the f32 GEMM in both arms of
its operand loads, and the f32 attention at the edge lengths.  Every output sits in guard bands
and is held per element (attention: per row) to the bounds the CPU tests hold the torch paths to."""
import pytest
import torch

import gemm_forms as gf
from gemm_forms import BF, F32, IMPLS, LAYOUTS
from kernel_checks import MARGIN_ATTN_F32_DK, MARGIN_ATTN_F32_DQ, assert_guards_intact, guarded

from distributed_pytorch_cookbook_amd.ops import _lib
from distributed_pytorch_cookbook_amd.ops.attention import attention_bwd, attention_fwd
from distributed_pytorch_cookbook_amd.ops.gemm import gemm

pytestmark = pytest.mark.gpu
dev = "cuda"
FAM_ALPHA = "gemm alpha (fraction of the element bound)"
FAM_EXT = "gemm extents (fraction of the element bound)"
FAM_F32 = "gemm f32 forms (fraction of the element bound)"


class forced:
    """A forced implementation (-1: the dispatcher's choice) and split-K count, restored on exit."""

    def __init__(self, impl, splits=0):
        self.impl, self.splits = impl, splits

    def __enter__(self):
        _lib.set_gemm_impl(self.impl)
        _lib.set_gemm_splits(self.splits)

    def __exit__(self, *exc):
        _lib.set_gemm_impl(-1)
        _lib.set_gemm_splits(0)


# ---------------------------------------------------------------- A: alpha and alpha_t
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("a_kmaj,b_kmaj", LAYOUTS)
@pytest.mark.parametrize("M,N,K", gf.ALPHA_SHAPES)
def test_gemm_alpha_forms(impl, a_kmaj, b_kmaj, M, N, K):
    """alpha = 0.75 with the device scalar 1.3125 (and the device scalar alone) through every
    epilogue family of every forced implementation; the old C of an accumulated output enters
    unscaled."""
    d = gf.gemm_data(M, N, K, BF, dev)
    A, B = gf._store(d["a"], a_kmaj), gf._store(d["b"], b_kmaj)
    t = gf.alpha_scalar(dev)
    with forced(impl):
        runs = [(f, gf.run_form(gemm, f, d, A, B, a_kmaj, b_kmaj, M, N, alpha_t=t)) for f in gf.ALPHA_FORMS]
    for f, o in runs:
        gf.check_form(f, d, K, o, family=FAM_ALPHA)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("splits", [2, 3])
@pytest.mark.parametrize("a_kmaj,b_kmaj", LAYOUTS)
def test_gemm_alpha_split_k(impl, splits, a_kmaj, b_kmaj):
    """Split-K, fresh (the slab arm: gemm() hands a plain f32 product the workspace) and
    accumulated: the multiplier is applied once to the product, never to the old C."""
    M, N, K = gf.SPLIT_K_SHAPE
    d = gf.gemm_data(M, N, K, BF, dev)
    A, B = gf._store(d["a"], a_kmaj), gf._store(d["b"], b_kmaj)
    t = gf.alpha_scalar(dev)
    with forced(impl, splits):
        runs = [(f, gf.run_form(gemm, f, d, A, B, a_kmaj, b_kmaj, M, N, alpha_t=t)) for f in gf.SPLIT_K_FORMS]
    for f, o in runs:
        gf.check_form(f, d, K, o, family=FAM_ALPHA, what=f"splits {splits}")


def test_gemm_alpha_split_k_atomic_arm(monkeypatch):
    """The same without a workspace: the k-ranges meet in C through f32 atomics."""
    from distributed_pytorch_cookbook_amd.ops import gemm as gemm_mod

    monkeypatch.setattr(gemm_mod, "_workspace", lambda device: None)
    M, N, K = gf.SPLIT_K_SHAPE
    d = gf.gemm_data(M, N, K, BF, dev)
    t = gf.alpha_scalar(dev)
    for impl in (2, 20, 26):
        for a_kmaj, b_kmaj in LAYOUTS:
            A, B = gf._store(d["a"], a_kmaj), gf._store(d["b"], b_kmaj)
            with forced(impl, 3):
                runs = [(f, gf.run_form(gemm, f, d, A, B, a_kmaj, b_kmaj, M, N, alpha_t=t)) for f in gf.SPLIT_K_FORMS]
            for f, o in runs:
                gf.check_form(f, d, K, o, family=FAM_ALPHA, what=f"atomic impl {impl}")


FRESH_IMPLS = [26, 20, -1]  # the v9 and a v7 persistent kernel (scalar-cache load), the default dispatch
FRESH_SHAPE = (300, 264, 192)


@pytest.mark.parametrize("impl", FRESH_IMPLS)
def test_gemm_alpha_t_is_read_by_every_launch(impl):
    """The device scalar is written and changed by device ops with no host synchronisation in
    between; each launch's output meets the bound for the value it was launched behind."""
    M, N, K = FRESH_SHAPE
    d = gf.gemm_data(M, N, K, BF, dev)
    A, B = gf._store(d["a"], True), gf._store(d["b"], True)
    with forced(impl):
        t = gf.alpha_scalar(dev, gf.ALPHA_T)
        first = [(f, gf.run_form(gemm, f, d, A, B, True, True, M, N, alpha_t=t)) for f in gf.FRESH_FORMS]
        t.fill_(gf.ALPHA_T2)
        second = [(f, gf.run_form(gemm, f, d, A, B, True, True, M, N, alpha_t=t)) for f in gf.FRESH_FORMS]
    for runs, value in ((first, gf.ALPHA_T), (second, gf.ALPHA_T2)):
        for f, o in runs:
            gf.check_form(f, d, K, o, t_value=value, family=FAM_ALPHA, what=f"alpha_t {value}")


@pytest.mark.parametrize("impl", FRESH_IMPLS)
def test_gemm_alpha_t_is_read_by_every_replay(impl):
    """The same calls captured once (one stream, after an eager warm-up) and replayed twice with
    the device scalar changed between the replays."""
    M, N, K = FRESH_SHAPE
    d = gf.gemm_data(M, N, K, BF, dev)
    A, B = gf._store(d["a"], True), gf._store(d["b"], True)
    t = gf.alpha_scalar(dev, gf.ALPHA_T)
    with forced(impl):
        outs = [gf.run_form(gemm, f, d, A, B, True, True, M, N, alpha_t=t) for f in gf.FRESH_FORMS]  # warm-up
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for f, o in zip(gf.FRESH_FORMS, outs):
                gf.run_form(gemm, f, d, A, B, True, True, M, N, alpha_t=t, outputs=o)
    for value in (gf.ALPHA_T, gf.ALPHA_T2):
        t.fill_(value)
        for o in outs:  # nothing of an earlier run may pass for this one's
            for buf in o.values():
                buf.fill_(float("nan"))
        graph.replay()
        for f, o in zip(gf.FRESH_FORMS, outs):
            gf.check_form(f, d, K, o, t_value=value, family=FAM_ALPHA, what=f"replay alpha_t {value}")


# ---------------------------------------------------------------- B: stored extents
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("kind,cut", gf.EXTENT_CASES)
def test_gemm_stored_extents(impl, kind, cut):
    """bf16 operands stored smaller than the product: what is not stored reads as zero, not as
    whatever lies behind the operand (NaN here).  The persistent kernels refuse an mn-major
    operand with short k-rows; forcing them exercises the hand-down.

    Caught: an mn-major A stored with 77 (or 72) columns under an output of 96 rows gave NaN in
    the rows past the stored ones -- 77 .. 79 from the register-staged kernel, which read the whole
    last 16-B chunk of a k-row, and 77 (72) .. 95 from every descriptor-bounded kernel, which end
    an operand at its last byte and not at the end of a stored row.  The register-staged kernel
    now zeroes the rest of such a chunk (gemm.hip: g_load) and the dispatcher hands it every
    product whose mn-major operand holds fewer columns than the product needs (gemm_plan.h:
    mn_cols_ok; short_b_mn is the same cut in B)."""
    c = gf.extent_case(kind, cut, BF, dev)
    t = gf.alpha_scalar(dev)
    forms = gf.extent_forms(kind, BF)
    with forced(impl):
        runs = [(f, gf.run_form(gemm, f, c["d"], c["A"], c["B"], c["a_kmaj"], c["b_kmaj"], c["M"], c["N"], alpha_t=t))
                for f in forms]
    for f, o in runs:
        gf.check_extent_form(f, c, o, family=FAM_EXT, what=f"{kind} {cut}")
    assert_guards_intact(*(x for x in (c["A"], c["B"]) if hasattr(x, "_guard_info")), what="operand")


@pytest.mark.parametrize("kind,cut", gf.EXTENT_CASES)
def test_gemm_f32_stored_extents(kind, cut):
    """The same with f32 operands: csrc/gemm_f32.hip's own extent logic (f32_load)."""
    c = gf.extent_case(kind, cut, F32, dev)
    t = gf.alpha_scalar(dev)
    for f in gf.extent_forms(kind, F32):
        o = gf.run_form(gemm, f, c["d"], c["A"], c["B"], c["a_kmaj"], c["b_kmaj"], c["M"], c["N"], alpha_t=t)
        gf.check_extent_form(f, c, o, family=FAM_EXT, what=f"f32 {kind} {cut}")


# ---------------------------------------------------------------- C: the f32 GEMM
@pytest.mark.parametrize("a_kmaj,b_kmaj", LAYOUTS)
@pytest.mark.parametrize("M,N,K", gf.GEMM_SHAPES)
def test_gemm_f32_forms(a_kmaj, b_kmaj, M, N, K):
    """Every epilogue of csrc/gemm_f32.hip beyond plain and bias + GELU + aux_out."""
    d = gf.gemm_data(M, N, K, F32, dev)
    A, B = gf._store(d["a"], a_kmaj), gf._store(d["b"], b_kmaj)
    t = gf.alpha_scalar(dev)
    for f in gf.F32_FORMS:
        o = gf.run_form(gemm, f, d, A, B, a_kmaj, b_kmaj, M, N, alpha_t=t)
        gf.check_form(f, d, K, o, family=FAM_F32)


@pytest.mark.parametrize("storage", gf.F32_STORAGES)
@pytest.mark.parametrize("a_kmaj,b_kmaj", LAYOUTS)
@pytest.mark.parametrize("M,N,K", gf.F32_STORAGE_SHAPES)
def test_gemm_f32_operand_storage(storage, a_kmaj, b_kmaj, M, N, K):
    """Both arms of f32_load: float4 loads, and the scalar loads an operand takes whose row
    stride is no multiple of 4 or whose base is not 16-B aligned.  K = 136 and 200 end whole groups
    of four k-major elements short of the 16-wide slice; K = 203 cuts the last group inside."""
    d = gf.gemm_data(M, N, K, F32, dev)
    A, B = gf.store_f32(d["a"], a_kmaj, storage), gf.store_f32(d["b"], b_kmaj, storage)
    want = {"aligned": None, "ld_odd": "ld", "offset": "base"}[storage]
    assert gf.scalar_arm(A) == want and gf.scalar_arm(B) == want
    for f in gf.F32_STORAGE_FORMS:
        o = gf.run_form(gemm, f, d, A, B, a_kmaj, b_kmaj, M, N)
        gf.check_form(f, d, K, o, family=FAM_F32, what=storage)


# ---------------------------------------------------------------- D: the f32 attention
@pytest.mark.parametrize("hd,S,causal,with_pad", gf.ATTN_F32_CASES)
def test_attention_f32_edges(hd, S, causal, with_pad):
    """csrc/attention_f32.hip at the edge lengths of the bf16 kernels, o and dqkv in guard bands,
    per row within a margin of the plain f32 ideal: MARGIN for o and dv (the kernels round nothing
    the ideal keeps).

    dq and dk exceeded MARGIN in 4 of the 33 cases on the MI355X (dq 2.52 x at hd 128, S 129 causal
    and 2.11 x at hd 64, S 129 without the mask; dk 3.73 x at hd 32, S 200 causal): the backward's
    f32 scores against the o and lse of the forward's f64-summed ones, in rows that are
    near-cancellations over one or two keys.  They carry the named margins of kernel_checks.py,
    where the cause and the measurements are written down.
    S = 1: dv's floor is exactly zero (the ideal's P is exp(0)); gemm_forms.check_attention_f32
    holds those rows to a product bound instead."""
    N, H = gf.ATTN_F32_N, gf.ATTN_F32_H
    T, E = N * S, H * hd
    c = gf.attention_f32_case(hd, S, causal, with_pad, dev)
    o = guarded((T, E), F32, dev, ld=E + 8)
    o_ret, lse = attention_fwd(c["qkv"], N, S, H, hd, c["pad"], causal=causal, out=o)
    assert o_ret.data_ptr() == o.data_ptr()
    dqkv = guarded((T, 3 * E), F32, dev, ld=3 * E + 8)
    attention_bwd(c["do"], c["qkv"], o, lse, N, S, H, hd, c["pad"], causal=causal, dqkv=dqkv)
    gf.check_attention_f32(c, hd, S, causal, o, lse, dqkv, margins=dict(dq=MARGIN_ATTN_F32_DQ, dk=MARGIN_ATTN_F32_DK))
    assert_guards_intact(o, dqkv)
