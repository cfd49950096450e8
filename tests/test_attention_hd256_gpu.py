"""The head_dim-256 flash kernels (csrc/attention.hip, namespace hd256): natively at 256 and through
the zero-pad path at 160, with the reference math patched out so that a fall-back fails.

test_hd256_fwd_bwd holds them to test_attention_fwd_bwd's tolerances against the f32 O(S^2)
reference at one tile (S 64), a ragged second query block (200) and many ring wraps (1023).
test_hd256_scores runs the checks of test_attention_scores_gpu.py at (hd 256, S 320): five tiles
(the 2-slot ring wraps twice), two plain tiles ahead of the last query block.  Its input
conditions -- rows that rescale live accumulators, the ideal kernel's own dk / dv row floor --
hold for the reference alone at hd 256 (computed on the CPU: rescale rows 0.40 .. 1.00 without and
0.07 .. 0.67 with the padding mask; floors dk <= 0.029, dv <= 1.9e-3)."""
import pytest
import torch

import attn_cases as ac
import distributed_pytorch_cookbook_amd.ops.attention as attn_mod
import test_attention_scores_gpu as scores
from kernel_checks import attention_bwd_plain, attention_plain

pytestmark = pytest.mark.gpu
dev = "cuda"
HD, S_SCORES = 256, 320
SCORE_CASES = [(profile, G, HD, S_SCORES, causal, with_pad) for profile, G in ac.PROFILES
               for causal in (True, False) for with_pad in (False, True)]


def rel_err(a, b):  # the global metric of test_kernels_gpu.py
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


@pytest.fixture
def hip_only(monkeypatch):
    """attention_fwd / attention_bwd may not reach the reference math."""
    def _no_ref(*a, **k):
        raise AssertionError("head_dim 129..256 in bf16 must run the HIP kernels")

    monkeypatch.setattr(attn_mod, "attention_ref", _no_ref)


@pytest.mark.parametrize("hd", [256, 160])
@pytest.mark.parametrize("S", [64, 200, 1023])
@pytest.mark.parametrize("with_pad", [False, True])
def test_hd256_fwd_bwd(S, with_pad, hd, hip_only, monkeypatch):
    if hd == HD:
        def _no_pad(*a, **k):
            raise AssertionError("native head_dim must not take the zero-pad path")

        monkeypatch.setattr(attn_mod, "_pad_heads", _no_pad)
    torch.manual_seed(2)
    N, H = 2, 2
    T, E = N * S, H * hd
    qkv = torch.randn(T, 3 * E, device=dev).bfloat16()
    do = torch.randn(T, E, device=dev).bfloat16()
    pad = None
    if with_pad:
        pad = torch.zeros(N, S, dtype=torch.bool, device=dev)
        pad[0, S - S // 4:] = True  # right padding
        pad[1, 5:9] = True
    o, lse = attn_mod.attention_fwd(qkv, N, S, H, hd, pad, causal=True)
    dqkv = attn_mod.attention_bwd(do, qkv, o, lse, N, S, H, hd, pad, causal=True)
    o_r, lse_r = attention_plain(qkv, N, S, H, hd, pad, True, dtype=torch.float32)
    g = attention_bwd_plain(qkv, do, o_r, lse_r, N, S, H, hd, pad, True, dtype=torch.float32)
    assert rel_err(o, o_r) < 1e-2
    fin = torch.isfinite(lse_r)
    assert torch.allclose(lse[fin], lse_r[fin].float(), atol=2e-2, rtol=1e-3)
    for i, name in enumerate(("dq", "dk", "dv")):
        assert rel_err(dqkv[:, i * E:(i + 1) * E], g[:, i * E:(i + 1) * E]) < 2e-2, name


@pytest.mark.parametrize("case", SCORE_CASES, ids=scores._ids)
def test_hd256_scores(case, hip_only):
    profile, G, hd, S, causal, with_pad = case
    if (profile, G) in ac.MODERATE and profile != "falling":
        qkv, _ = scores._case_inputs(profile, G, hd, S)
        pad = ac.attention_score_mask(scores.N, S, dev) if with_pad else None
        ev = ac.rescale_event_rows(qkv, scores.N, S, scores.H, hd, pad, causal)
        assert ev >= (0.05 if with_pad else 0.30), ev  # the bound of the CPU test of these cases
    scores.test_attention_scores_fwd(case)
    scores.test_attention_scores_bwd(case)  # (asserts the ideal's dk / dv row floor itself)
