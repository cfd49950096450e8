"""The fp8 weight format on CPU: the torch twin of dpc_wq_quantize (ops/gemm.py:weight_quantize_ref
with weight_scales) and the recipes' flag."""
import torch

from distributed_pytorch_cookbook_amd.config import build_parser
from distributed_pytorch_cookbook_amd.ops.gemm import weight_quantize_ref, weight_scales


def test_weight_quantize_twin():
    torch.manual_seed(0)
    w = torch.randn(37, 272).bfloat16()
    w[5] = 0
    w[9] *= 1e-3
    w[9, 100] = 3.0e38
    scale, inv = weight_scales(w)
    amax = w.float().abs().amax(1)
    assert torch.equal(scale[amax > 0], (amax / 448.0)[amax > 0]) and scale[5] == 1.0
    q = weight_quantize_ref(w, inv)
    assert torch.count_nonzero(q[5].view(torch.uint8)) == 0
    assert not ((q.view(torch.uint8) & 0x7F) == 0x7F).any()
    # e4m3: half an ulp of a normal is 2^-4 of it, the subnormal step's half 2^-10 of the scaled unit
    err = (q.double() * scale.double()[:, None] - w.double()).abs()
    assert (err <= 2.0 ** -4 * w.double().abs() + 2.0 ** -10 * amax.double()[:, None]).all()


def test_decode_weight_dtype_flag():
    p = build_parser("single")
    assert p.parse_args([]).decode_weight_dtype == "bf16"
    assert p.parse_args(["--decode_weight_dtype", "fp8"]).decode_weight_dtype == "fp8"
