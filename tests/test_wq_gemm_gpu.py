"""csrc/wq_gemm.hip (dpc_gemm_wq8: the fp8-weight Linear of 1..64 rows, and dpc_wq_quantize): the
kernel against an f64 reference inside guard bands at the project's element bound, the quantiser
against its torch twin byte for byte, the dispatch from linear_fwd, and a graphed decode step on
fp8 weights."""
import pytest
import torch

from kernel_checks import GELU_LIPSCHITZ, assert_elem_bound, assert_guards_intact, gemm_elem_bound, guarded
from gemm_forms import gelu64

from distributed_pytorch_cookbook_amd.models.decode import GraphDecoder, decode_step, quantize_decode_weights
from distributed_pytorch_cookbook_amd.models.gpt import TransformerDecoderLM
from distributed_pytorch_cookbook_amd.ops.gemm import (QWeight, _linear_fwd_wq8, linear_fwd, quantize_weight,
                                                       weight_quantize_ref, weight_scales)

pytestmark = pytest.mark.gpu
dev = "cuda"
BF, F32 = torch.bfloat16, torch.float32
EPIS = {"plain": (False, 0, False), "bias_gelu": (True, 2, False), "bias_relu_res": (True, 1, True)}


def _operands(epi, M, Nw, N, K, seed=11):
    """x, the twin-quantised weight, the epilogue's operands and the f64 reference over q * scale."""
    torch.manual_seed(seed + M)
    has_bias, act, has_res = EPIS[epi]
    x = torch.randn(M, K, device=dev).bfloat16()
    w = (torch.randn(Nw, K, device=dev) / K ** 0.5).bfloat16()
    scale, inv = weight_scales(w)
    qw = QWeight(weight_quantize_ref(w, inv), scale)
    bias = torch.randn(Nw, device=dev) if has_bias else None
    res = torch.randn(M, N, device=dev) if has_res else None
    ref = x.double() @ (qw.q.float().double() * scale.double()[:, None]).t()
    if bias is not None:
        ref = ref + bias.double()
    ref = gelu64(ref) if act == 2 else (torch.relu(ref) if act == 1 else ref)
    if res is not None:
        ref = ref + res[:, :Nw].double()
    return x, qw, bias, act, res, F32 if has_res else BF, ref


# M: 1, 16 (one row block), 17, 33, 49, 64 (two to four).  K = 16: one cut step of a single chunk;
# 128: one whole step, the other waves add zeros; 448: three steps and a half; 1040: wave 0 gets a
# whole step and the one-chunk tail, with 8 waves and with 4.  Nw, N = 100, 104: a partial strip and
# zero padding; 202, 202: a partial last strip and a cut last quad.  The epilogues rotate over the
# cases; every (row blocks, plan) instantiation has a case.
_E = list(EPIS)
_SHAPES = ([(M, 100, 104, K, plan) for plan in ((16, 8), (32, 4))
            for M, K in ((1, 448), (16, 1040), (17, 128), (33, 1040), (49, 448), (64, 16))]
           + [(1, 202, 202, 16, (16, 8)), (17, 202, 202, 1040, (32, 4)), (33, 202, 202, 448, (16, 8)),
              (49, 202, 202, 128, (32, 4)), (64, 202, 202, 1040, (16, 8)), (64, 202, 202, 448, (32, 4)),
              (16, 202, 202, 128, None)])
CASES = [(_E[i % 3],) + s for i, s in enumerate(_SHAPES)]


@pytest.mark.parametrize("epi,M,Nw,N,K,plan", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_wq_kernel(epi, M, Nw, N, K, plan):
    x, qw, bias, act, res, odt, ref = _operands(epi, M, Nw, N, K)
    ld = (N + 7) // 8 * 8 + 8
    outs = []
    for _ in range(2):
        out = guarded((M, N), odt, dev, ld=ld)
        y = _linear_fwd_wq8(x, qw, bias, act, res, out, odt, plan=plan)
        assert y.data_ptr() == out.data_ptr()
        assert_guards_intact(out)
        outs.append(out)
    bound = gemm_elem_bound(x, qw.q.float() * qw.scale[:, None], ref, odt, K, GELU_LIPSCHITZ if act == 2 else 1.0)
    assert_elem_bound(outs[0][:, :Nw], ref, bound, what=epi, family="fp8-weight gemm (fraction of the element bound)")
    assert torch.count_nonzero(outs[0][:, Nw:]) == 0
    assert torch.equal(outs[0], outs[1])


def test_wq_quantize_matches_twin():
    torch.manual_seed(3)
    N, K, ldw = 37, 272, 288
    w = guarded((N, K), BF, dev, ld=ldw, fill=torch.randn(N, K, device=dev).bfloat16())
    w[5] = 0
    w[9] *= 1e-3
    w[9, 100] = 3.0e38
    w[20, 7] = w[20].abs().amax()  # (a second element exactly at the row's amax)
    qw = quantize_weight(w)
    scale, inv = weight_scales(w)
    assert torch.isfinite(scale).all() and torch.equal(qw.scale, scale) and scale[5] == 1.0
    got, want = qw.q.view(torch.uint8), weight_quantize_ref(w, inv).view(torch.uint8)
    assert torch.equal(got, want)
    assert not ((got & 0x7F) == 0x7F).any()
    assert torch.count_nonzero(got[5]) == 0 and got[9, 100] == 0x7E


def test_wq_dispatch():
    for M in (1, 40):
        x, qw, bias, act, _, odt, _ = _operands("bias_gelu", M, 100, 104, 448)
        a, b = (guarded((M, 104), odt, dev, ld=112) for _ in range(2))
        linear_fwd(x, qw, bias=bias, act=act, out=a)
        _linear_fwd_wq8(x, qw, bias, act, None, b, odt)
        assert torch.equal(a, b), M
    x, qw, *_ = _operands("plain", 65, 100, 100, 448)
    with pytest.raises(ValueError, match="at most 64 rows"):
        linear_fwd(x, qw)
    with pytest.raises(ValueError, match="aux_out"):
        linear_fwd(x[:8], qw, aux_out=torch.empty(8, 100, device=dev, dtype=BF))
    x, qw, *_ = _operands("plain", 8, 100, 100, 24)
    with pytest.raises(ValueError, match="does not take"):
        linear_fwd(x, qw)


def test_model_graph_step_fp8_weights(capsys):
    """One graphed decode step of five sequences at their own lengths on fp8 weights against the f32
    full forward of a copy of the model holding the dequantised weights (the step then differs by
    its bf16 activations alone: the bound of test_model_graph_step_batch20); the graphed step equals
    the eager one bit for bit; with an fp8 KV cache too the step captures and gives finite logits.

    Against the unquantised model (printed, not asserted; MI355X): relative norm of the logits'
    error 2.8e-2 worst sequence with fp8 weights, 3.7e-3 with the bf16 step; against the
    dequantised reference 3.8e-3."""
    torch.manual_seed(0)
    with torch.device(dev):
        m = TransformerDecoderLM(64, 32, 2, 2, 512, 256)
    m.eval()
    N = 5
    lens = [30 + 3 * s for s in range(N)]
    S = max(lens)
    ids = torch.randint(0, 512, (N, S + 1), device=dev)
    pos = torch.arange(S + 1, device=dev).expand(N, S + 1)
    tok = torch.stack([ids[s, lens[s]] for s in range(N)])[:, None]
    with torch.no_grad():
        wq = quantize_decode_weights(m)
        with torch.device(dev):
            deq = TransformerDecoderLM(64, 32, 2, 2, 512, 256)
        deq.load_state_dict(m.state_dict())
        deq.eval()
        for la, lb in zip(m.decoder.layers, deq.decoder.layers):
            qkv = wq.qkv_weight(la.attn)
            for lin, part in zip((lb.attn.to_q, lb.attn.to_k, lb.attn.to_v), (qkv.q.float() * qkv.scale[:, None]).chunk(3)):
                lin.weight.copy_(part)
            for a, b in ((la.attn.to_out, lb.attn.to_out), (la.fc.up_proj, lb.fc.up_proj), (la.fc.down_proj, lb.fc.down_proj)):
                b.weight.copy_(wq.weight(a.weight).q.float() * wq.weight(a.weight).scale[:, None])
        deq.lm_head.weight.copy_(wq.weight(m.lm_head.weight).q.float() * wq.weight(m.lm_head.weight).scale[:, None])
        ref = deq.reference_forward(ids, pos).float()
        full = m.reference_forward(ids, pos).float()
        steps = {}
        for name, kv, weights, graphed in (("graph", None, wq, True), ("eager", None, wq, False),
                                           ("bf16", None, None, True), ("fp8kv", "fp8", wq, True)):
            cache = m.new_kv_cache(N, S + 2, ragged=True, kv_dtype=kv)
            m.decode(ids[:, :S], None, cache, lens=lens)
            if graphed:
                steps[name] = GraphDecoder(m, cache, weights=weights).step(tok).float().clone()
            else:
                steps[name] = decode_step(m, weights, cache, tok).float().clone()

    def rel(a, b):
        return max(((a[s, 0] - b[s, lens[s]]).norm() / b[s, lens[s]].norm()).item() for s in range(N))

    with capsys.disabled():
        print(f"\nlogits vs the unquantised f32 model: fp8 weights {rel(steps['graph'], full):.3e}, "
              f"bf16 step {rel(steps['bf16'], full):.3e}; fp8 weights vs the dequantised f32 model "
              f"{rel(steps['graph'], ref):.3e}")
    assert rel(steps["graph"], ref) < 2e-2
    assert torch.equal(steps["graph"], steps["eager"])
    assert torch.isfinite(steps["fp8kv"]).all()
