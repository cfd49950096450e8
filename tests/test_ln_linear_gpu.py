"""csrc/ln_linear.hip (dpc_ln_linear: LayerNorm inside the few-row Linear that consumes it): the
kernel against an f64 reference inside guard bands at the project's element bound, rows that break a
single-pass variance, what linear_fwd(norm=) refuses, and the graphed one-token step that uses it."""
import pytest
import torch

from kernel_checks import GELU_LIPSCHITZ, assert_elem_bound, assert_guards_intact, gemm_elem_bound, guarded
from gemm_forms import gelu64

from distributed_pytorch_cookbook_amd.models import fused
from distributed_pytorch_cookbook_amd.models.decode import GraphDecoder, decode_step, quantize_decode_weights
from distributed_pytorch_cookbook_amd.models.gpt import TransformerDecoderLM
from distributed_pytorch_cookbook_amd.ops import gemm
from distributed_pytorch_cookbook_amd.ops.gemm import (_LN_LINEAR_MAX_ROWS, QWeight, _linear_fwd_ln, linear_fwd,
                                                       weight_quantize_ref, weight_scales)

pytestmark = pytest.mark.gpu
dev = "cuda"
BF, F32 = torch.bfloat16, torch.float32
EPS = 1e-5
EPIS = {"plain": (False, 0, False), "bias_gelu": (True, 2, False), "bias_res": (True, 0, True)}


def _check(x, fp8, epi, Nw, N, plan, seed=0):
    """One launch on x [M, K] (f32, any row stride) against
    act(bf16(LN(x)) @ W^T * scale + bias) + residual in f64, twice for the bits."""
    M, K = x.shape
    torch.manual_seed(seed)
    has_bias, act, has_res = EPIS[epi]
    gamma, beta = 1 + 0.1 * torch.randn(K, device=dev), 0.1 * torch.randn(K, device=dev)
    w = (torch.randn(Nw, K, device=dev) / K ** 0.5).bfloat16()
    if fp8:
        scale, inv = weight_scales(w)
        w = QWeight(weight_quantize_ref(w, inv), scale)
        w64 = w.q.float().double() * scale.double()[:, None]
    else:
        w64 = w.double()
    bias = torch.randn(Nw, device=dev) if has_bias else None
    res = torch.randn(M, N, device=dev) if has_res else None
    odt = F32 if has_res else BF
    x64 = x.double()
    mu, var = x64.mean(1, keepdim=True), x64.var(1, unbiased=False, keepdim=True)
    h = ((x64 - mu) / torch.sqrt(var + EPS) * gamma.double() + beta.double()).float().bfloat16()  # as the kernel rounds it
    ref = h.double() @ w64.t() + (bias.double() if has_bias else 0)
    ref = gelu64(ref) if act == 2 else ref
    if has_res:
        ref = ref + res[:, :Nw].double()
    outs = []
    for _ in range(2):
        out = guarded((M, N), odt, dev, ld=(N + 7) // 8 * 8 + 8)
        y = _linear_fwd_ln(x, w, (gamma, beta, EPS), bias, act, res, out, odt, plan=plan)
        assert y.data_ptr() == out.data_ptr()
        assert_guards_intact(out)
        outs.append(out)
    # the product's bound, plus one bf16 ulp of difference in any rounded LN(x) element (the kernel's
    # f32 statistics against the f64 ones): 2^-8 sum_k |h_k w_nk|
    lip = GELU_LIPSCHITZ if act == 2 else 1.0
    bound = gemm_elem_bound(h, w64, ref, odt, K, lip) + lip * 2.0 ** -8 * (h.double().abs() @ w64.abs().t())
    assert_elem_bound(outs[0][:, :Nw], ref, bound, what=epi, family="ln-linear (fraction of the element bound)")
    assert torch.count_nonzero(outs[0][:, Nw:]) == 0
    assert torch.equal(outs[0], outs[1])


# (Nw, N, K): one step for one wave only; a short last step (208 = 3 * 64 + 16); a second trip for the
# first wave of the 8-wave plan with a short step (592 = 9 * 64 + 16, 4 * 128 + 80 for e4m3); strips
# cut by Nw and padded columns.  M: one row, a few, a full row block, two row blocks.
@pytest.mark.parametrize("epi", list(EPIS))
@pytest.mark.parametrize("Nw,N,K", [(40, 48, 64), (100, 104, 208), (33, 40, 592)])
@pytest.mark.parametrize("M", [1, 5, 16, _LN_LINEAR_MAX_ROWS])
@pytest.mark.parametrize("plan", [(16, 8), (32, 4)], ids=["16x8", "32x4"])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_ln_linear_kernel(fp8, plan, M, Nw, N, K, epi):
    torch.manual_seed(M + K)
    x = guarded((M, K), F32, dev, ld=K + 8, fill=2 * torch.randn(M, K, device=dev) + 0.5)
    _check(x, fp8, epi, Nw, N, plan, seed=K)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_ln_linear_statistics(fp8):
    """Rows of mean 50 and standard deviation 0.1 (E[x^2] - E[x]^2 in f32 loses the variance) and a
    constant row (variance 0: LN(x) = beta), at the bound of the other cases."""
    torch.manual_seed(5)
    x = 50 + 0.1 * torch.randn(6, 592, device=dev)
    x[3] = 3.0
    _check(x, fp8, "bias_res", 33, 40, None)


def test_ln_linear_refusals():
    K = 64
    x = torch.randn(4, K, device=dev)
    w = torch.randn(48, K, device=dev).bfloat16()
    norm = (torch.ones(K, device=dev), torch.zeros(K, device=dev), EPS)
    assert linear_fwd(x, w, norm=norm).shape == (4, 48)
    with pytest.raises(ValueError, match="f32"):
        linear_fwd(x.bfloat16(), w, norm=norm)
    with pytest.raises(ValueError, match="aux_out"):
        linear_fwd(x, w, norm=norm, aux_out=torch.empty(4, 48, device=dev, dtype=BF))
    with pytest.raises(ValueError, match="rows"):
        linear_fwd(torch.randn(_LN_LINEAR_MAX_ROWS + 1, K, device=dev), w, norm=norm)
    big = 8192  # 16 rows of it are 256 KiB of image
    with pytest.raises(ValueError, match="LDS"):
        linear_fwd(torch.randn(16, big, device=dev), torch.empty(48, big, device=dev, dtype=BF),
                   norm=(torch.ones(big, device=dev), torch.zeros(big, device=dev), EPS))
    with pytest.raises(ValueError, match="K %"):
        linear_fwd(x[:, :60].contiguous(), w[:, :60].contiguous(), norm=tuple(t[:60] if torch.is_tensor(t) else t for t in norm))


def _dequantised(m, wq):
    """A copy of the model holding q * scale in place of every weight the fp8 step streams."""
    with torch.device(dev):
        deq = TransformerDecoderLM(64, 32, 2, 2, 512, 256)
    deq.load_state_dict(m.state_dict())
    deq.eval()

    def full(qw):
        return qw.q.float() * qw.scale[:, None]

    for la, lb in zip(m.decoder.layers, deq.decoder.layers):
        for lin, part in zip((lb.attn.to_q, lb.attn.to_k, lb.attn.to_v), full(wq.qkv_weight(la.attn)).chunk(3)):
            lin.weight.copy_(part)
        for a, b in ((la.attn.to_out, lb.attn.to_out), (la.fc.up_proj, lb.fc.up_proj), (la.fc.down_proj, lb.fc.down_proj)):
            b.weight.copy_(full(wq.weight(a.weight)))
    deq.lm_head.weight.copy_(full(wq.weight(m.lm_head.weight)))
    return deq


# the fused step's error against the f32 forward may exceed the separate-LayerNorm step's by this
# factor.  Both errors are the bf16 roundings of the activations; the two steps differ in the order
# of the Linears' sums and in the out-projection, which the fused step stores in f32.  Measured on
# the MI355X (docs/GENERATION.md): 3.726e-3 against 3.707e-3 with bf16 weights (1.005 x), 3.824e-3
# against 3.841e-3 with e4m3 weights (0.996 x).
STEP_MARGIN = 1.25


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_model_graph_step_ln_linear(fp8, monkeypatch, capsys):
    """One graphed decode step of five sequences at their own lengths with the LayerNorms inside the
    Linears, against the f32 full forward (of the dequantised weights under fp8) and against the
    same step with the switch off; the graphed step equals the eager one bit for bit.  The step takes
    the fused form up to gemm.LN_LINEAR_ROWS rows, which ships as 0 (docs/GENERATION.md): 16 here."""
    monkeypatch.setattr(gemm, "LN_LINEAR_ROWS", 16)
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
        wq = quantize_decode_weights(m) if fp8 else None
        ref = (_dequantised(m, wq) if fp8 else m).reference_forward(ids, pos).float()
        steps = {}
        for name, on, graphed in (("fused", True, True), ("eager", True, False), ("separate", False, True)):
            monkeypatch.setattr(fused, "_LN_LINEAR", on)
            store = fused.ensure_store(m) if wq is None else wq
            assert fused.ln_linear_step(store, torch.empty(N, 64, device=dev), store.weight(m.lm_head.weight)) == on
            cache = m.new_kv_cache(N, S + 2, ragged=True)
            m.decode(ids[:, :S], None, cache, lens=lens)
            if graphed:
                steps[name] = GraphDecoder(m, cache, weights=wq).step(tok).float().clone()
            else:
                steps[name] = decode_step(m, store, cache, tok).float().clone()

    def rel(a):
        return max(((a[s, 0] - ref[s, lens[s]]).norm() / ref[s, lens[s]].norm()).item() for s in range(N))

    with capsys.disabled():
        print(f"\nlogits vs the f32 forward ({'e4m3' if fp8 else 'bf16'} weights): LayerNorm in the Linears "
              f"{rel(steps['fused']):.3e}, separate LayerNorms {rel(steps['separate']):.3e}")
    assert rel(steps["fused"]) <= STEP_MARGIN * rel(steps["separate"])
    assert torch.equal(steps["fused"], steps["eager"])
