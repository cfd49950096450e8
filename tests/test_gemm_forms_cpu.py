"""The cases of tests/gemm_forms.py cover what they claim, its f64 references and bounds can be
met, and its assertions bite -- on the CPU: every form of the GPU tests runs through ``gemm()`` on
CPU tensors (ops/gemm.py: ``_gemm_ref``, plain f32 torch) and is held to the same inequalities,
and small arithmetic mutations of that path fail them."""
import pytest
import torch

import gemm_forms as gf
from gemm_forms import BF, F32, LAYOUTS
from kernel_checks import assert_guards_intact

from distributed_pytorch_cookbook_amd.ops.attention import attention_bwd, attention_fwd
from distributed_pytorch_cookbook_amd.ops.gemm import gemm

cpu = "cpu"


def _run_check(forms, d, A, B, a_kmaj, b_kmaj, M, N, K, fn=gemm, t_value=gf.ALPHA_T, what=""):
    t = gf.alpha_scalar(cpu, t_value)
    for f in forms:
        o = gf.run_form(fn, f, d, A, B, a_kmaj, b_kmaj, M, N, alpha_t=t)
        gf.check_form(f, d, K, o, t_value=t_value, what=what)


# ---------------------------------------------------------------- coverage of the case lists
def test_multipliers_are_exact_in_f32():
    for v in (gf.ALPHA, gf.ALPHA_T, gf.ALPHA_T2, gf.ALPHA * gf.ALPHA_T, gf.ALPHA * gf.ALPHA_T2):
        assert float(torch.tensor(v, dtype=F32)) == v
        assert float(torch.tensor(v, dtype=F32) * torch.tensor(3.0, dtype=F32)) == 3.0 * v  # with bits to spare
    assert gf.ALPHA * gf.ALPHA_T == 0.984375
    assert float(gf.alpha_scalar(cpu)) == gf.ALPHA_T and float(gf.alpha_scalar(cpu, gf.ALPHA_T2)) == gf.ALPHA_T2


def test_every_flag_appears_with_and_without_alpha_t():
    forms = gf.ALPHA_FORMS + gf.SPLIT_K_FORMS + gf.F32_FORMS + gf.F32_STORAGE_FORMS + [
        f for fs in gf.EXTENT_FORMS.values() for f in fs]
    with_t = {flag for f in forms if f.alpha_t for flag in f.flags()}
    without = {flag for f in forms if not f.alpha_t for flag in f.flags()}
    every = {"bias", "aux_deriv", "residual", "colsum", "accumulate", "act1", "act2", "act_bwd1", "act_bwd2", "aux_out",
             "aux_in", "out_bf16", "out_f32"}
    assert without == every and with_t == every
    # host and device multiplier together, and the device one alone
    assert any(f.alpha_t and f.alpha is not None for f in gf.ALPHA_FORMS)
    assert {f.name for f in gf.ALPHA_FORMS if f.alpha_t and f.alpha is None} == {"plain_f32_t_alone", "accumulate_t_alone"}
    assert all(f.alpha_t for f in gf.ALPHA_FORMS + gf.SPLIT_K_FORMS + gf.FRESH_FORMS)
    # the f32 kernel: both aux dtypes, read and written; alpha next to a bias
    assert {f.aux_in for f in gf.F32_FORMS if f.act_bwd} == {F32, BF}
    assert {f.aux_out for f in gf.F32_FORMS if f.aux_out is not None} == {F32, BF}
    assert {(f.act_bwd, f.aux_in) for f in gf.F32_FORMS if f.act_bwd} == {(1, F32), (1, BF), (2, F32), (2, BF)}
    assert all(f.colsum for f in gf.F32_FORMS if f.act_bwd)
    assert any(f.alpha_t and f.bias for f in gf.F32_FORMS) and any(f.accumulate and f.residual for f in gf.F32_FORMS)
    assert all(f.out == F32 for f in gf.F32_FORMS + gf.F32_STORAGE_FORMS)


def test_shapes_are_the_ones_the_kernels_split_on():
    assert set(gf.ALPHA_SHAPES) <= set(gf.GEMM_SHAPES)
    assert {K % 64 == 0 for _, _, K in gf.ALPHA_SHAPES} == {True, False}  # persistent kernels: own / handed down
    assert {K % 16 for _, _, K in gf.GEMM_SHAPES} == {0, 8}  # f32 k-slices of 16: whole, and a tail
    assert gf.SPLIT_K_SHAPE[2] % 64 == 0


@pytest.mark.parametrize("a_kmaj,b_kmaj", LAYOUTS)
def test_both_scalar_load_conditions_appear(a_kmaj, b_kmaj):
    M, N, K = gf.GEMM_SHAPES[1]
    d = gf.gemm_data(M, N, K, F32, cpu)
    seen = set()
    for storage in gf.F32_STORAGES:
        A, B = gf.store_f32(d["a"], a_kmaj, storage), gf.store_f32(d["b"], b_kmaj, storage)
        assert gf.scalar_arm(A) == gf.scalar_arm(B)
        assert torch.equal(A, d["a"] if a_kmaj else d["a"].t()) and torch.equal(B, d["b"] if b_kmaj else d["b"].t())
        seen.add(gf.scalar_arm(A))
    assert seen == {None, "ld", "base"}
    # k tails: whole groups of four past K inside a 16-wide slice, and a group cut inside
    assert any(K % 16 and K % 4 == 0 for _, _, K in gf.F32_STORAGE_SHAPES)
    assert any(K % 4 for _, _, K in gf.F32_STORAGE_SHAPES) and set(gf.GEMM_SHAPES) <= set(gf.F32_STORAGE_SHAPES)


def test_extent_cuts_inside_and_between_chunks():
    assert {V % 8 == 0 for V in gf.EXT_V} == {True, False}
    assert any(gf.EXT_N - V < 8 for V in gf.EXT_V)  # inside the last chunk
    assert {R % 8 == 0 for R in gf.EXT_ROWS} == {True, False}
    assert all(V < gf.EXT_N for V in gf.EXT_V) and all(R < gf.EXT_M for R in gf.EXT_ROWS)
    assert {k for k, _ in gf.EXTENT_CASES} == set(gf.EXTENT_FORMS)
    for kind, cut in gf.EXTENT_CASES:
        for dtype in (BF, F32):
            c = gf.extent_case(kind, cut, dtype, cpu)
            short = c["A"] if kind.startswith("short_a") else c["B"]
            if kind == "short_b_mn":  # the columns past the stored ones, in every k-row
                raw, front, rows, cols, ld = short._guard_info
                assert torch.isnan(raw.view(dtype)[front:front + rows * ld].view(rows, ld)[:, cols:c["N"]]).all()
                continue
            raw, front, rows, cols, ld = short._guard_info
            # what a kernel that ignored the extent would read lies inside the allocation, and is NaN
            logical_rows = {"fwd_head": c["N"], "dgrad_head": c["K"], "short_a_k": c["M"], "short_a_mn": rows}[kind]
            logical_cols = c["M"] if kind == "short_a_mn" else cols
            last = (logical_rows - 1) * ld + (logical_cols + 7) // 8 * 8
            assert front + last <= raw.numel()
            flat = raw.view(dtype)
            if kind == "short_a_mn":  # the columns past the stored ones, in every k-row
                assert torch.isnan(flat[front:front + rows * ld].view(rows, ld)[:, cols:c["M"]]).all()
            else:  # the rows past the stored ones
                assert last > rows * ld and torch.isnan(flat[front + rows * ld:front + last]).all()
            # the logical operands are the stored ones, extended with zeros
            a, b = c["d"]["a"], c["d"]["b"]
            assert a.shape == (c["M"], c["K"]) and b.shape == (c["N"], c["K"])
            if kind == "dgrad_head":
                assert (a[:, cut:] != 0).all() and torch.count_nonzero(b[:, cut:]) == 0
                assert torch.equal(b[:, :cut], c["B"].t())


# ---------------------------------------------------------------- the forms on the torch path
@pytest.mark.parametrize("a_kmaj,b_kmaj", LAYOUTS)
@pytest.mark.parametrize("M,N,K", gf.ALPHA_SHAPES + [gf.SPLIT_K_SHAPE])
def test_alpha_forms_cpu(a_kmaj, b_kmaj, M, N, K):
    d = gf.gemm_data(M, N, K, BF, cpu)
    A, B = gf._store(d["a"], a_kmaj), gf._store(d["b"], b_kmaj)
    forms = gf.SPLIT_K_FORMS if (M, N, K) == gf.SPLIT_K_SHAPE else gf.ALPHA_FORMS + gf.FRESH_FORMS
    _run_check(forms, d, A, B, a_kmaj, b_kmaj, M, N, K)
    _run_check(forms, d, A, B, a_kmaj, b_kmaj, M, N, K, t_value=gf.ALPHA_T2)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("kind,cut", gf.EXTENT_CASES)
def test_stored_extents_cpu(kind, cut, dtype):
    c = gf.extent_case(kind, cut, dtype, cpu)
    t = gf.alpha_scalar(cpu)
    for f in gf.extent_forms(kind, dtype):
        o = gf.run_form(gemm, f, c["d"], c["A"], c["B"], c["a_kmaj"], c["b_kmaj"], c["M"], c["N"], alpha_t=t)
        gf.check_extent_form(f, c, o, what=f"{kind} {cut}")
    assert_guards_intact(*(x for x in (c["A"], c["B"]) if hasattr(x, "_guard_info")), what="operand")


@pytest.mark.parametrize("a_kmaj,b_kmaj", LAYOUTS)
@pytest.mark.parametrize("M,N,K", gf.F32_STORAGE_SHAPES)
def test_f32_forms_cpu(a_kmaj, b_kmaj, M, N, K):
    d = gf.gemm_data(M, N, K, F32, cpu)
    if (M, N, K) in gf.GEMM_SHAPES:
        _run_check(gf.F32_FORMS, d, gf._store(d["a"], a_kmaj), gf._store(d["b"], b_kmaj), a_kmaj, b_kmaj, M, N, K)
    for storage in gf.F32_STORAGES:
        A, B = gf.store_f32(d["a"], a_kmaj, storage), gf.store_f32(d["b"], b_kmaj, storage)
        _run_check(gf.F32_STORAGE_FORMS, d, A, B, a_kmaj, b_kmaj, M, N, K, what=storage)


# ---------------------------------------------------------------- the assertions bite
def _without_alpha_t(a, b, **kw):
    kw.pop("alpha_t", None)
    return gemm(a, b, **kw)


def _old_c_scaled(a, b, **kw):
    if kw.get("accumulate"):
        kw["out"].mul_(kw.get("alpha", 1.0) * float(kw["alpha_t"]))
    return gemm(a, b, **kw)


def _alpha_after_bias(a, b, **kw):
    if kw.get("bias") is not None:
        kw["bias"] = kw["bias"] * (kw.get("alpha", 1.0) * float(kw["alpha_t"]))
    return gemm(a, b, **kw)


@pytest.mark.parametrize("dtype,forms", [(BF, gf.ALPHA_FORMS), (F32, gf.F32_FORMS)], ids=["bf16", "f32"])
def test_multiplier_mutations_fail(dtype, forms):
    M, N, K = gf.ALPHA_SHAPES[1]
    d = gf.gemm_data(M, N, K, dtype, cpu)
    A, B = gf._store(d["a"], True), gf._store(d["b"], True)
    t = gf.alpha_scalar(cpu)
    for wrong, hit in ((_without_alpha_t, lambda f: f.alpha_t),
                       (_old_c_scaled, lambda f: f.alpha_t and f.accumulate),
                       (_alpha_after_bias, lambda f: f.alpha_t and f.bias)):
        hits = [f for f in forms if hit(f)]
        assert hits
        for f in hits:
            o = gf.run_form(wrong, f, d, A, B, True, True, M, N, alpha_t=t)
            with pytest.raises(AssertionError, match="over the bound"):
                gf.check_form(f, d, K, o)
    # a stale scalar: the output behind the first value does not pass for the second
    f = gf.FRESH_FORMS[0] if dtype == BF else [x for x in forms if x.alpha_t][0]
    o = gf.run_form(gemm, f, d, A, B, True, True, M, N, alpha_t=t)
    gf.check_form(f, d, K, o, t_value=gf.ALPHA_T)
    with pytest.raises(AssertionError, match="over the bound"):
        gf.check_form(f, d, K, o, t_value=gf.ALPHA_T2)


# (an mn-major operand cut between two chunks has no in-chunk tail to misread)
@pytest.mark.parametrize("kind,cut", [c for c in gf.EXTENT_CASES if not (c[0].endswith("_mn") and c[1] % 8 == 0)])
def test_ignored_extent_fails(kind, cut):
    """A product that reads the logical extent from the short operand's storage meets the NaN
    behind it (inside the allocation) and fails; one that reads zeros for everything missing but
    the in-chunk tail of an mn-major A fails too."""
    c = gf.extent_case(kind, cut, BF, cpu)
    short = "A" if kind.startswith("short_a") else "B"
    s = c[short]
    if kind in ("short_a_mn", "short_b_mn"):
        full = s.as_strided((s.shape[0], (cut + 7) // 8 * 8), s.stride(), s.storage_offset())
    else:
        rows = {"fwd_head": c["N"], "dgrad_head": c["K"], "short_a_k": c["M"]}[kind]
        full = s.as_strided((rows, s.shape[1]), s.stride(), s.storage_offset())
    assert full.shape != s.shape
    f = gf.extent_forms(kind, BF)[0]
    ops = dict(A=c["A"], B=c["B"])
    ops[short] = full
    o = gf.run_form(gemm, f, c["d"], ops["A"], ops["B"], c["a_kmaj"], c["b_kmaj"], c["M"], c["N"])
    with pytest.raises(AssertionError, match="over the bound"):
        gf.check_extent_form(f, c, o)


# ---------------------------------------------------------------- the f32 attention reference pair
@pytest.mark.parametrize("hd,S,causal,with_pad", [(32, 65, True, True), (32, 1, True, False), (64, 63, False, False)])
def test_attention_f32_reference_pair_cpu(hd, S, causal, with_pad):
    """ops/attention.py's torch path (plain f32) through the checks of the GPU test: the ideal and
    the f64 reference agree, and MARGIN can be met by an f32 implementation."""
    assert {c[1] for c in gf.ATTN_F32_CASES} == {1, 63, 65, 129, 200}
    assert {c[0] for c in gf.ATTN_F32_CASES} == {32, 64, 128} and (128, 129, False, False) in gf.ATTN_F32_CASES
    N, H = gf.ATTN_F32_N, gf.ATTN_F32_H
    c = gf.attention_f32_case(hd, S, causal, with_pad, cpu)
    o, lse = attention_fwd(c["qkv"], N, S, H, hd, c["pad"], causal=causal)
    dqkv = attention_bwd(c["do"], c["qkv"], o, lse, N, S, H, hd, c["pad"], causal=causal)
    assert o.dtype == F32 and dqkv.dtype == F32
    gf.check_attention_f32(c, hd, S, causal, o, lse, dqkv)
    if with_pad:  # a padded key's dk and dv are structural zeros; one wrong bit there fails
        E = H * hd
        dead = int(c["pad"].reshape(-1).nonzero()[0])
        assert torch.count_nonzero(c["g64"][dead, E:]) == 0
        dqkv[dead, 2 * E] = 1e-30
        with pytest.raises(AssertionError, match="dv"):
            gf.check_attention_f32(c, hd, S, causal, o, lse, dqkv)
