"""The split-KV decode planner (host only) and the ``splits`` argument on the torch path."""
import pytest
import torch

from distributed_pytorch_cookbook_amd.ops.attention import (DECODE_MAX_SPLITS, DECODE_SPLIT_MIN_KEYS, decode_attention,
                                                            decode_splits)


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_decode_splits_plan(cus):
    for N, H, Smax in [(2, 3, 40), (1, 4, 40), (1, 2, 40), (3, 2, 320), (2, 3, 300), (8, 12, 320)]:
        assert decode_splits(N, H, Smax, cus) == 1  # the earlier decode tests keep the one-workgroup kernel
    assert DECODE_SPLIT_MIN_KEYS >= 160
    for Smax in (1, 255, 256, 1064, 4096, 16392, 1 << 20):
        last = None
        for NH in (1, 2, 12, 96, 255, 256, 257, 4096):
            s = decode_splits(1, NH, Smax, cus)
            assert 1 <= s <= max(1, min(DECODE_MAX_SPLITS, Smax // DECODE_SPLIT_MIN_KEYS))
            assert last is None or s <= last
            last = s
    assert decode_splits(1, 1, 1 << 20, 256) == DECODE_MAX_SPLITS


def test_decode_attention_cpu_ignores_splits():
    torch.manual_seed(0)
    N, H, hd, Smax = 2, 2, 16, 12
    E = H * hd
    qkv = torch.randn(N, 3 * E)
    k0, v0 = torch.randn(N, Smax, E), torch.randn(N, Smax, E)
    length = torch.tensor([5, 12])  # the second sequence's cache is full
    outs = []
    for splits in (None, 3):
        kc, vc = k0.clone(), v0.clone()
        outs.append((decode_attention(qkv, kc, vc, length, H, hd, per_seq=True, splits=splits), kc, vc))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
