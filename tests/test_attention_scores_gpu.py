"""The attention kernels on scores that move the running max, with masked tiles and masked rows.

Every other attention test draws qkv from randn: scaled scores of N(0, 1), under which the flash
forwards' lazy rescale runs once per block on zero accumulators, P never exceeds ~4, no tile and
no row is wholly masked, and no masked score overflows exp2.  The inputs of tests/attn_cases.py
(score = small noise + a profile over the key index; the CPU tests of test_kernel_checks_cpu.py
assert what each case reaches) run those arms in all three bf16 forwards (hd 64 and hd 32 at
S >= 512: attn_fwd3_kernel; hd 128: attn_fwd_kernel; hd 32 below 512: attn_fwd2_kernel), the two
backward kernels, the f32 kernels and the decode kernel.

o and dqkv sit in guard bands.  Tolerances are a margin times the error of the ideal kernel (plain
f32 math on the same rounded inputs, rounded to the output type) against the f64 reference; rows
with no allowed key must be o = 0 and lse = +inf bit for bit, and their gradients exact zeros."""
import math

import pytest
import torch

import attn_cases as ac
from kernel_checks import (MARGIN_ATTN, MARGIN_ATTN_DK_ELEM, MARGIN_ATTN_DK_ROWS, assert_elem_close, assert_guards_intact, assert_local_close,
                           attention_bwd_plain, attention_plain, guarded, row_col_err)

from distributed_pytorch_cookbook_amd.ops.attention import attention_bwd, attention_fwd, decode_attention

pytestmark = pytest.mark.gpu
dev = "cuda"
BF, F32 = torch.bfloat16, torch.float32
N, H = ac.N_SEQ, ac.HEADS

CASES = [(profile, G, hd, S, causal, with_pad) for profile, G in ac.PROFILES for hd, S in ac.SHAPES
         for causal in (True, False) for with_pad in (False, True)]
F32_CASES = [c for c in CASES if (c[0], c[1]) in (("rising", 12), ("spike", 12), ("falling", 70))]


class Checks:
    """Runs every check of a case and fails once, with all the messages (a case that misses one
    bound still reports the others)."""

    def __init__(self, what):
        self.what, self.failed = what, []

    def run(self, fn, *args, **kw):
        try:
            fn(*args, **kw)
        except AssertionError as e:
            self.failed.append(str(e))

    def true(self, cond, text):
        if not bool(cond):
            self.failed.append(text)

    def done(self):
        if self.failed:
            raise AssertionError(self.what + ":\n  " + "\n  ".join(self.failed))


_inputs, _runs = {}, {}


def _case_inputs(profile, G, hd, S):
    key = (profile, G, hd, S)
    if key not in _inputs:
        _inputs[key] = (ac.attention_score_case(profile, G, hd, S, device=dev),
                        ac.attention_score_dout(profile, G, hd, S, device=dev))
    return _inputs[key]


def _dead_tokens(lse64, S):
    """[T] bool: the query rows with no allowed key (the mask is the same for every head)."""
    return (~torch.isfinite(lse64)).reshape(N, H, S)[:, 0].reshape(N * S)


def _run_bf16(case):
    """The kernels (forward, then the backward from the kernel's own o and lse) and the references
    of a case, once for the forward and the backward test."""
    if case not in _runs:
        profile, G, hd, S, causal, with_pad = case
        T, E = N * S, H * hd
        qkv, do = _case_inputs(profile, G, hd, S)
        pad = ac.attention_score_mask(N, S, dev) if with_pad else None
        o = guarded((T, E), BF, dev, ld=E + 8)
        o_ret, lse = attention_fwd(qkv, N, S, H, hd, pad, causal=causal, out=o)
        assert o_ret.data_ptr() == o.data_ptr()
        dqkv = guarded((T, 3 * E), BF, dev, ld=3 * E + 8)
        attention_bwd(do, qkv, o, lse, N, S, H, hd, pad, causal=causal, dqkv=dqkv)
        _runs[case] = (o, lse, dqkv, pad, ac.score_references(qkv, do, N, S, H, hd, pad, causal))
    return _runs[case]


def _ids(c):
    return f"{c[0]}{c[1]}-hd{c[2]}-S{c[3]}-{'causal' if c[4] else 'full'}-{'pad' if c[5] else 'nopad'}"


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_attention_scores_fwd(case):
    """o per query row within MARGIN_ATTN x the ideal's worst row; lse at the project's tolerance
    on the live rows; dead rows o = 0 (all bits) and lse = +inf."""
    profile, G, hd, S, causal, with_pad = case
    o, lse, dqkv, pad, (o64, lse64, g64, o_ideal, lse32, g_ideal) = _run_bf16(case)
    ck = Checks(_ids(case))
    ck.run(assert_local_close, o, o64, o_ideal, MARGIN_ATTN, axes="rows", what="o", family="attention scores fwd")
    fin = torch.isfinite(lse64)
    ck.true(torch.isfinite(lse[fin]).all(), "lse of a live row is not finite")
    d = (lse[fin].double() - lse64[fin]).abs()
    ck.true((d <= 2e-2 + 1e-3 * lse64[fin].abs()).all(), f"lse off by up to {d.max().item() if d.numel() else 0:.3e}")
    dead = _dead_tokens(lse64, S)
    ck.true(bool(dead.any()) == with_pad, "the case's dead rows")
    ck.true((lse[~fin] == math.inf).all(), "lse of a row with no allowed key is not +inf")
    ck.true((o[dead].contiguous().view(torch.int16) == 0).all(), "o of a row with no allowed key is not +0")
    ck.run(assert_guards_intact, o, what="o")
    ck.done()


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_attention_scores_bwd(case):
    """dq, dk, dv from the kernel's own o and lse: every element within MARGIN_ATTN x the ideal's
    largest element error of that block (NaN / inf fail).  A per-row bound does not apply to dq
    here -- rows that see one or two keys make dS a cancellation, and the ideal's own worst dq row
    is off by 1 to 5 with the mask -- and for the 70-profiles, where the ideal's largest dq error is
    up to a third of the block's largest element, the dq check is mainly finite-and-bounded: what
    those cases are for is the exp2 of a masked score far above the lse (the padding arm; under
    the causal mask alone both backward kernels skip every sub-block wholly above the diagonal,
    so a computed future score is at most 62 keys ahead).  dk and dv of the four moderate profiles
    are also held per key row, once the ideal's own floor shows that the inputs allow it (a
    condition on the inputs, not a tolerance on the kernel).  dk has margins of its own, measured
    and explained in kernel_checks.py.  Structural zeros are exact."""
    profile, G, hd, S, causal, with_pad = case
    T, E = N * S, H * hd
    o, lse, dqkv, pad, (o64, lse64, g64, o_ideal, lse32, g_ideal) = _run_bf16(case)
    ck = Checks(_ids(case))
    for i, name in enumerate(("dq", "dk", "dv")):
        sl = slice(i * E, (i + 1) * E)
        # (dk: the cases' constant q coordinate weighs the kernel's bf16 dS operand 32-fold in one
        # column -- kernel_checks.py has the measurement behind its two margins)
        ck.run(assert_elem_close, dqkv[:, sl], g64[:, sl], g_ideal[:, sl],
               MARGIN_ATTN_DK_ELEM if name == "dk" else MARGIN_ATTN, what=name, family=f"attention scores {name} elem")
        if name != "dq" and (profile, G) in ac.MODERATE:
            floor, _ = row_col_err(g_ideal[:, sl], g64[:, sl])
            assert floor <= (0.1 if name == "dk" else 5e-3), (name, floor)
            ck.run(assert_local_close, dqkv[:, sl], g64[:, sl], g_ideal[:, sl],
                   MARGIN_ATTN_DK_ROWS if name == "dk" else MARGIN_ATTN, axes="rows",
                   what=name + " rows", family=f"attention scores {name} rows")
    if with_pad:
        dead = _dead_tokens(lse64, S)
        padded = pad.reshape(T)
        z = torch.zeros(T, E, dtype=BF, device=dev)
        ck.true(torch.equal(dqkv[dead][:, :E], z[dead]), "dq of a row with no allowed key is not zero")
        ck.true(torch.equal(dqkv[padded][:, E:2 * E], z[padded]), "dk of a padded key is not zero")
        ck.true(torch.equal(dqkv[padded][:, 2 * E:], z[padded]), "dv of a padded key is not zero")
        ck.true(torch.equal(dqkv[2 * S:], torch.zeros(S, 3 * E, dtype=BF, device=dev)), "dqkv of the all-padding sequence")
        ck.true((o[2 * S:].contiguous().view(torch.int16) == 0).all(), "o of the all-padding sequence")
    ck.run(assert_guards_intact, o, dqkv, what="o / dqkv")
    ck.done()


def _rel(x, ref):  # the whole-tensor measure of test_fp32_gpu.py, against f64
    return float((x.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


_runs_f32 = {}


def _run_f32(case):
    if case not in _runs_f32:
        profile, G, hd, S, causal, with_pad = case
        T, E = N * S, H * hd
        qkv_b, do_b = _case_inputs(profile, G, hd, S)
        qkv, do = qkv_b.float(), do_b.float()
        pad = ac.attention_score_mask(N, S, dev) if with_pad else None
        o = guarded((T, E), F32, dev, ld=E + 8)
        _, lse = attention_fwd(qkv, N, S, H, hd, pad, causal=causal, out=o)
        dqkv = guarded((T, 3 * E), F32, dev, ld=3 * E + 8)
        attention_bwd(do, qkv, o, lse, N, S, H, hd, pad, causal=causal, dqkv=dqkv)
        o64, lse64 = attention_plain(qkv, N, S, H, hd, pad, causal)
        g64 = attention_bwd_plain(qkv, do, o64, lse64, N, S, H, hd, pad, causal, dtype=torch.float64)
        _runs_f32[case] = (o, lse, dqkv, pad, o64, lse64, g64)
    return _runs_f32[case]


@pytest.mark.parametrize("case", F32_CASES, ids=_ids)
def test_attention_scores_f32_fwd(case):
    """The f32 forward (exact online softmax, alpha = 0 at m = -inf) on the same values cast to f32,
    at the tolerances of test_attention_f32 (whole-tensor rel < 1e-5, lse 1e-5) against f64; dead
    rows o = +0 and lse = +inf.

    This bound is what made the forward sum its scores in f64 (attention_f32.hip: fwd_kernel).
    With one f32 accumulator per score the kernel missed it in 14 of the 48 cases -- rising 12
    without the causal mask at (hd 64, S 320), (hd 128, S 320), (hd 32, S 576), rel 1.15e-5 ..
    1.90e-5, and falling 70 with the padding mask at all four shapes, 1.60e-5 .. 4.03e-5 -- as
    plain f32 PyTorch math does on the same values (1.15e-5 .. 4.63e-5 from f64 in exactly those
    cases): the raw score q . k reaches 300 to 850, where an f32 step is 3e-5 to 6e-5, and the
    accumulation over head_dim rounds there at every step.  Measured on the MI355X with the f64
    sums: at most 2.2e-6 (rising 12), 1.2e-6 (spike 12), 3.8e-6 (falling 70)."""
    profile, G, hd, S, causal, with_pad = case
    o, lse, dqkv, pad, o64, lse64, g64 = _run_f32(case)
    ck = Checks(_ids(case))
    ck.true(torch.isfinite(o).all(), "NaN / inf in o")
    r = _rel(o, o64)
    ck.true(r < 1e-5, f"o rel {r:.3e}")
    fin = torch.isfinite(lse64)
    d = (lse[fin].double() - lse64[fin]).abs()
    ck.true((d <= 1e-5 + 1e-5 * lse64[fin].abs()).all(), f"lse off by up to {d.max().item() if d.numel() else 0:.3e}")
    dead = _dead_tokens(lse64, S)
    ck.true(bool(dead.any()) == with_pad, "the case's dead rows")
    ck.true((lse[~fin] == math.inf).all(), "lse of a row with no allowed key is not +inf")
    ck.true((o[dead].contiguous().view(torch.int32) == 0).all(), "o of a row with no allowed key is not +0")
    ck.run(assert_guards_intact, o, what="o")
    ck.done()


@pytest.mark.parametrize("case", F32_CASES, ids=_ids)
def test_attention_scores_f32_bwd(case):
    """The f32 backward from the kernel's own o and lse: whole-tensor rel < 1e-4 against f64 (the
    tolerance of test_attention_f32), structural zeros exact."""
    profile, G, hd, S, causal, with_pad = case
    T, E = N * S, H * hd
    o, lse, dqkv, pad, o64, lse64, g64 = _run_f32(case)
    ck = Checks(_ids(case))
    ck.true(torch.isfinite(dqkv).all(), "NaN / inf in dqkv")
    r = _rel(dqkv, g64)
    ck.true(r < 1e-4, f"dqkv rel {r:.3e}")
    if with_pad:
        dead = _dead_tokens(lse64, S)
        padded = pad.reshape(T)
        z = torch.zeros(T, E, device=dev)
        ck.true(torch.equal(dqkv[dead][:, :E], z[dead]), "dq of a row with no allowed key is not zero")
        ck.true(torch.equal(dqkv[padded][:, E:2 * E], z[padded]), "dk of a padded key is not zero")
        ck.true(torch.equal(dqkv[padded][:, 2 * E:], z[padded]), "dv of a padded key is not zero")
        ck.true(torch.equal(dqkv[2 * S:], torch.zeros(S, 3 * E, device=dev)), "dqkv of the all-padding sequence")
    ck.run(assert_guards_intact, o, dqkv, what="o / dqkv")
    ck.done()


@pytest.mark.parametrize("profile,G", [("rising", 12), ("spike", 12)])
@pytest.mark.parametrize("hd", [64, 128])
def test_decode_attention_scores(hd, profile, G):
    """The decode kernel at position 299 of a cache filled from a score case (the new token is the
    case's own row 299), in the form of test_decode_attention_edges."""
    S, pos = 320, 299
    E = H * hd
    qkv_all, _ = _case_inputs(profile, G, hd, S)
    k0 = qkv_all[:, E:2 * E].reshape(N, S, E).clone()
    v0 = qkv_all[:, 2 * E:].reshape(N, S, E).clone()
    qkv = qkv_all.reshape(N, S, 3 * E)[:, pos].contiguous()
    kc, vc = guarded((N, S, E), BF, dev, fill=k0), guarded((N, S, E), BF, dev, fill=v0)
    kc[:, pos], vc[:, pos] = 0, 0  # the kernel appends the new token's key / value there
    length = torch.full((1,), pos, device=dev, dtype=torch.int64)
    o = decode_attention(qkv, kc, vc, length, H, hd)
    assert torch.equal(kc, k0) and torch.equal(vc, v0)
    L = pos + 1

    def run(dt):
        q = qkv[:, :E].to(dt).reshape(N, H, 1, hd)
        k = k0[:, :L].to(dt).reshape(N, L, H, hd).transpose(1, 2)
        v = v0[:, :L].to(dt).reshape(N, L, H, hd).transpose(1, 2)
        return (torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), -1) @ v).reshape(N * H, hd)

    assert_local_close(o.reshape(N * H, hd), run(torch.float64), run(F32).bfloat16(), MARGIN_ATTN, axes="rows",
                       what="decode o", family="decode attention scores")
    assert_guards_intact(kc, vc)
