"""Split-KV decode attention against the f64 softmax of q.K^T / sqrt(hd) over the bf16 inputs; bound:
MARGIN_ATTN x the error of the same math in f32 rounded to bf16.  Guarded caches change in row pos only."""
import math

import pytest
import torch

import attn_cases as ac
from kernel_checks import MARGIN_ATTN, assert_guards_intact, assert_local_close, guarded

from distributed_pytorch_cookbook_amd.models.gpt import TransformerDecoderLM
from distributed_pytorch_cookbook_amd.ops.attention import decode_attention, decode_split_keys_per_pass

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16


def _ref(qkv, k, v, L, H, hd, dt):
    """softmax(q K^T / sqrt(hd)) V over the first L cache rows in ``dt``: [N*H, hd]."""
    N, E = qkv.shape[0], H * hd
    q = qkv[:, :E].to(dt).reshape(N, H, 1, hd)
    k = k[:, :L].to(dt).reshape(N, L, H, hd).transpose(1, 2)
    v = v[:, :L].to(dt).reshape(N, L, H, hd).transpose(1, 2)
    return (torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), -1) @ v).reshape(N * H, hd)


def _check(o, qkv, k0, v0, L, H, hd, what):
    assert_local_close(o.reshape(-1, hd), _ref(qkv, k0, v0, L, H, hd, torch.float64),
                       _ref(qkv, k0, v0, L, H, hd, torch.float32).bfloat16(), MARGIN_ATTN, axes="rows", what=what)


@pytest.mark.parametrize("splits", [1, 3, 8])
@pytest.mark.parametrize("hd", [8, 32, 64, 96, 128, 256])
def test_decode_split_edges(hd, splits):
    """Position 0 (every split but one empty), L = splits, around the first chunk boundary (a
    multiple of the kernel's keys per pass) and the last row."""
    torch.manual_seed(7)
    N, H, Smax = 2, 3, 300
    E = H * hd
    kpp = decode_split_keys_per_pass(hd)
    before_k = torch.randn(N, Smax, E, device=dev).bfloat16()
    before_v = torch.randn(N, Smax, E, device=dev).bfloat16()
    kc, vc = guarded((N, Smax, E), BF, dev, fill=before_k), guarded((N, Smax, E), BF, dev, fill=before_v)
    qkv = torch.randn(N, 3 * E, device=dev).bfloat16()
    for pos in sorted({0, splits - 1, kpp - 2, kpp - 1, kpp, 299}):
        kc.copy_(before_k), vc.copy_(before_v)
        length = torch.full((1,), pos, device=dev, dtype=torch.int64)
        o = decode_attention(qkv, kc, vc, length, H, hd, splits=splits)
        k0, v0 = before_k.clone(), before_v.clone()
        k0[:, pos], v0[:, pos] = qkv[:, E:2 * E], qkv[:, 2 * E:]
        assert torch.equal(kc, k0) and torch.equal(vc, v0), pos
        _check(o, qkv, k0, v0, pos + 1, H, hd, f"o at pos {pos}")
        assert torch.equal(decode_attention(qkv, kc, vc, length, H, hd, splits=splits), o), pos
    assert_guards_intact(kc, vc)


@pytest.mark.parametrize("splits", [1, 3])
def test_decode_split_ragged(splits):
    """One launch over an empty, a short, an almost full and a full sequence."""
    torch.manual_seed(8)
    N, H, hd, Smax, lens = 4, 3, 64, 300, [0, 17, 299, 300]
    E = H * hd
    k0 = torch.randn(N, Smax, E, device=dev).bfloat16()
    v0 = torch.randn(N, Smax, E, device=dev).bfloat16()
    kc, vc = guarded((N, Smax, E), BF, dev, fill=k0), guarded((N, Smax, E), BF, dev, fill=v0)
    qkv = torch.randn(N, 3 * E, device=dev).bfloat16()
    o = decode_attention(qkv, kc, vc, torch.tensor(lens, device=dev), H, hd, per_seq=True, splits=splits)
    for n, pos in enumerate(lens[:3]):
        k0[n, pos], v0[n, pos] = qkv[n, E:2 * E], qkv[n, 2 * E:]
        _check(o[n], qkv[n:n + 1], k0[n:n + 1], v0[n:n + 1], pos + 1, H, hd, f"o of sequence {n}")
    assert torch.equal(kc, k0) and torch.equal(vc, v0)
    assert not o[3].any()
    assert_guards_intact(kc, vc)


@pytest.mark.parametrize("splits", [1, 4])
@pytest.mark.parametrize("profile,G", [("rising", 12), ("spike", 12)])
@pytest.mark.parametrize("hd", [64, 128])
def test_decode_split_moving_max(hd, profile, G, splits):
    """Position 299 of a cache filled from a score case: the running maximum moves inside a
    stream, between lane groups, between waves and between splits."""
    N, H, S, pos = ac.N_SEQ, ac.HEADS, 320, 299
    E = H * hd
    qkv_all = ac.attention_score_case(profile, G, hd, S, device=dev)
    k0 = qkv_all[:, E:2 * E].reshape(N, S, E).clone()
    v0 = qkv_all[:, 2 * E:].reshape(N, S, E).clone()
    qkv = qkv_all.reshape(N, S, 3 * E)[:, pos].contiguous()
    kc, vc = guarded((N, S, E), BF, dev, fill=k0), guarded((N, S, E), BF, dev, fill=v0)
    kc[:, pos], vc[:, pos] = 0, 0
    o = decode_attention(qkv, kc, vc, torch.full((1,), pos, device=dev), H, hd, splits=splits)
    assert torch.equal(kc, k0) and torch.equal(vc, v0)
    _check(o, qkv, k0, v0, pos + 1, H, hd, "o")
    assert_guards_intact(kc, vc)


def test_decode_past_one_workgroup_limit():
    """A cache longer than the one-workgroup kernel's 16384 rows, planned splits."""
    torch.manual_seed(9)
    N, H, hd, Smax, pos = 1, 2, 64, 16392, 16391
    E = H * hd
    k0 = torch.randn(N, Smax, E, device=dev).bfloat16()
    v0 = torch.randn(N, Smax, E, device=dev).bfloat16()
    kc, vc = guarded((N, Smax, E), BF, dev, fill=k0), guarded((N, Smax, E), BF, dev, fill=v0)
    qkv = torch.randn(N, 3 * E, device=dev).bfloat16()
    o = decode_attention(qkv, kc, vc, torch.full((1,), pos, device=dev), H, hd)
    k0[:, pos], v0[:, pos] = qkv[:, E:2 * E], qkv[:, 2 * E:]
    assert torch.equal(kc, k0) and torch.equal(vc, v0)
    _check(o, qkv, k0, v0, pos + 1, H, hd, "o")
    assert_guards_intact(kc, vc)


def test_graph_decoder_long_cache():
    """The graphed step over a 16400-row cache against the full forward's last row."""
    torch.manual_seed(0)
    with torch.device(dev):
        m = TransformerDecoderLM(64, 32, 2, 2, 512, 16448)
    m.eval()
    S0 = 16386
    ids = torch.randint(0, 512, (1, S0 + 3), device=dev)
    with torch.no_grad():
        cache = m.new_kv_cache(1, 16400)
        m.decode(ids[:, :S0], torch.arange(S0, device=dev)[None], cache)
        dec = m.graph_decoder(cache)
        assert dec is not None
        for t in range(S0, S0 + 3):
            lg = dec.step(ids[:, t:t + 1]).clone()
            ref = m(ids[:, :t + 1], torch.arange(t + 1, device=dev)[None])[:, -1:]
            err = ((lg.float() - ref.float()).norm() / ref.float().norm()).item()
            assert err < 2e-2, (t, err)
