"""The fp8 KV cache is read by HIP kernels only: a CPU model refuses it and keeps its usual cache."""
import pytest
import torch

from distributed_pytorch_cookbook_amd.models.gpt import TransformerDecoderLM


def test_fp8_cache_refused_on_cpu():
    torch.manual_seed(0)
    m = TransformerDecoderLM(32, 16, 2, 1, 64, 16)
    with pytest.raises(ValueError, match="fp8 KV cache"):
        m.new_kv_cache(1, 8, kv_dtype="fp8")
    cache = m.new_kv_cache(1, 8)
    assert cache.k[0].dtype in (torch.bfloat16, torch.float32) and cache.k[0].shape == (1, 8, 32)
