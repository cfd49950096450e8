"""ops/gemm.py: ln_linear_ok (what shapes linear_fwd(norm=) takes) and the refusal off the GPU."""
import pytest
import torch

from distributed_pytorch_cookbook_amd.ops.gemm import FP8, QWeight, linear_fwd, ln_linear_ok

BF = torch.bfloat16


def _w(K, fp8=False, dtype=BF):
    if fp8:
        return QWeight(torch.empty(24, K, dtype=FP8), torch.ones(24))
    return torch.empty(24, K, dtype=dtype)


# 160 KiB of LDS hold the image [M][K + pad] (bf16) and 8 KiB of partials per row block: 32 rows
# up to K = 2288, 16 rows up to K = 4848 (pad 8), not K = 4856 (pad 16)
@pytest.mark.parametrize("M,K,fp8,ok", [
    (1, 768, False, True), (16, 1600, True, True), (32, 1600, False, True), (33, 1600, False, False),
    (0, 768, False, False), (32, 2288, False, True), (32, 2304, False, False), (16, 4848, True, True),
    (16, 4856, False, False), (4, 24, False, True), (4, 24, True, False), (4, 20, False, False)])
def test_ln_linear_ok(M, K, fp8, ok):
    assert ln_linear_ok(M, K, _w(K, fp8)) == ok


def test_ln_linear_ok_weight():
    assert not ln_linear_ok(4, 64, _w(64, dtype=torch.float32))
    assert not ln_linear_ok(4, 64, _w(128))


def test_ln_linear_needs_the_gpu():
    with pytest.raises(ValueError, match="CUDA"):
        linear_fwd(torch.randn(2, 64), _w(64), norm=(torch.ones(64), torch.zeros(64), 1e-5))
