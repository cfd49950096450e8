"""The fp8 (e4m3) KV cache: quantising store, decode and append attention, and the model path.

Reference: the torch twin Qz(x, s) = (x.float() * float32(1 / s)).clamp(-448, 448).to(float8_e4m3fn)
gives the bytes the kernels must store, bit for bit; the output is held to the f64 softmax over
the DEQUANTISED cache (Qz(...).double() * s, bf16 q) -- the quantisation error is in the reference,
not in the tolerance -- within MARGIN_ATTN x the error of the same math in f32 rounded to bf16.
Caches are guarded byte buffers viewed as fp8: every row but the written ones, and the guards,
stay as they were."""
import math

import pytest
import torch

import attn_cases as ac
from kernel_checks import MARGIN_ATTN, assert_guards_intact, assert_local_close, guarded

from distributed_pytorch_cookbook_amd.models.gpt import TransformerDecoderLM
from distributed_pytorch_cookbook_amd.ops.attention import append_attention, decode_attention, decode_fp8_keys_per_pass
from distributed_pytorch_cookbook_amd.utils.batch import generate_batch
from distributed_pytorch_cookbook_amd.utils.tokenizer import ByteTokenizer

pytestmark = pytest.mark.gpu
dev = "cuda"
FP8, U8 = torch.float8_e4m3fn, torch.uint8


def Qz(x, s=1.0):
    """The bytes (uint8) of x quantised at scale s."""
    inv = torch.tensor(1.0 / s, dtype=torch.float32, device=x.device)
    return (x.float() * inv).clamp(-448, 448).to(FP8).view(U8)


def _caches(k8, v8):
    """Guarded byte buffers holding k8 / v8 (uint8 [N, Smax, E]) and their fp8 views."""
    gk, gv = guarded(k8.shape, U8, dev, fill=k8), guarded(v8.shape, U8, dev, fill=v8)
    return gk, gv, gk.view(FP8), gv.view(FP8)


def _ref(qkv, k8, v8, ks, vs, start, n, H, hd, dt):
    """Query i of each sequence over rows 0..start + i of the dequantised cache in ``dt``: [N*n*H, hd]."""
    N, E, L = k8.shape[0], H * hd, start + n
    q = qkv[:, :E].to(dt).reshape(N, n, H, hd).transpose(1, 2)
    k = (k8[:, :L].view(FP8).float().double() * ks).to(dt).reshape(N, L, H, hd).transpose(1, 2)
    v = (v8[:, :L].view(FP8).float().double() * vs).to(dt).reshape(N, L, H, hd).transpose(1, 2)
    s = q @ k.transpose(-1, -2) / math.sqrt(hd)
    s = s.masked_fill(torch.arange(L, device=dev)[None, :] > torch.arange(n, device=dev)[:, None] + start, -math.inf)
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(N * n * H, hd)


def _check(o, qkv, k8, v8, start, n, H, hd, what, ks=1.0, vs=1.0):
    assert_local_close(o.reshape(-1, hd), _ref(qkv, k8, v8, ks, vs, start, n, H, hd, torch.float64),
                       _ref(qkv, k8, v8, ks, vs, start, n, H, hd, torch.float32).bfloat16(), MARGIN_ATTN,
                       axes="rows", what=what)


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("hd", [32, 64, 128])
def test_decode_fp8_edges(hd, splits):
    """Position 0, L = splits, around the first pass boundary and the last row: the appended bytes,
    the output, and a second call's bits."""
    torch.manual_seed(7)
    N, H, Smax = 2, 3, 300
    E = H * hd
    kpp = decode_fp8_keys_per_pass(hd)
    bk, bv = Qz(torch.randn(N, Smax, E, device=dev)), Qz(torch.randn(N, Smax, E, device=dev))
    gk, gv, kc, vc = _caches(bk, bv)
    qkv = torch.randn(N, 3 * E, device=dev).bfloat16()
    for pos in sorted({0, splits - 1, kpp - 1, kpp, 299}):
        gk.copy_(bk), gv.copy_(bv)
        length = torch.full((1,), pos, device=dev, dtype=torch.int64)
        o = decode_attention(qkv, kc, vc, length, H, hd, splits=splits)
        k0, v0 = bk.clone(), bv.clone()
        k0[:, pos], v0[:, pos] = Qz(qkv[:, E:2 * E]), Qz(qkv[:, 2 * E:])
        assert torch.equal(gk, k0) and torch.equal(gv, v0), pos
        _check(o, qkv, k0, v0, pos, 1, H, hd, f"o at pos {pos}")
        assert torch.equal(decode_attention(qkv, kc, vc, length, H, hd, splits=splits), o), pos
    assert_guards_intact(gk, gv)


@pytest.mark.parametrize("splits", [1, 3])
def test_decode_fp8_ragged_scales_clamp(splits):
    """One launch over an empty, a short, an almost full and a full sequence at non-unit scales; a
    new k and a new v element far past the range are stored as 448 (0x7E), not NaN (0x7F)."""
    torch.manual_seed(8)
    N, H, hd, Smax, lens, ks, vs = 4, 3, 64, 300, [0, 17, 299, 300], 0.37, 1.9
    E = H * hd
    k0, v0 = Qz(torch.randn(N, Smax, E, device=dev), ks), Qz(torch.randn(N, Smax, E, device=dev), vs)
    gk, gv, kc, vc = _caches(k0, v0)
    qkv = torch.randn(N, 3 * E, device=dev).bfloat16()
    qkv[1, E + 5], qkv[2, 2 * E + 7] = 1000 * ks, 1000 * vs
    o = decode_attention(qkv, kc, vc, torch.tensor(lens, device=dev), H, hd, per_seq=True, splits=splits,
                         k_scale=ks, v_scale=vs)
    for n, pos in enumerate(lens[:3]):
        k0[n, pos], v0[n, pos] = Qz(qkv[n, E:2 * E], ks), Qz(qkv[n, 2 * E:], vs)
        _check(o[n], qkv[n:n + 1], k0[n:n + 1], v0[n:n + 1], pos, 1, H, hd, f"o of sequence {n}", ks, vs)
    assert torch.equal(gk, k0) and torch.equal(gv, v0)
    assert int(gk[1, 17, 5]) == 0x7E and int(gv[2, 299, 7]) == 0x7E
    assert not o[3].any()
    assert_guards_intact(gk, gv)


@pytest.mark.parametrize("splits", [1, 4])
def test_decode_fp8_moving_max(splits):
    """Position 299 of a cache quantised from the spike score case: the running maximum moves inside
    a stream, between lane groups, between waves and between splits."""
    N, H, hd, S, pos = ac.N_SEQ, ac.HEADS, 64, 320, 299
    E = H * hd
    qkv_all = ac.attention_score_case("spike", 12, hd, S, device=dev)
    k0, v0 = Qz(qkv_all[:, E:2 * E]).reshape(N, S, E), Qz(qkv_all[:, 2 * E:]).reshape(N, S, E)
    qkv = qkv_all.reshape(N, S, 3 * E)[:, pos].contiguous()
    gk, gv, kc, vc = _caches(k0, v0)
    gk[:, pos], gv[:, pos] = 0, 0
    o = decode_attention(qkv, kc, vc, torch.full((1,), pos, device=dev), H, hd, splits=splits)
    assert torch.equal(gk, k0) and torch.equal(gv, v0)
    _check(o, qkv, k0, v0, pos, 1, H, hd, "o")
    assert_guards_intact(gk, gv)


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("hd", [32, 64, 128])
def test_append_fp8(hd, splits):
    """Blocks at the cache's start, across a key tile, over two query tiles with a partly valid
    wave, and past the capacity (rows not written, zero output), the second sequence at half the
    first one's start; non-unit scales at (63, 2)."""
    torch.manual_seed(9)
    N, H, Smax = 2, 2, 320
    E = H * hd
    for start, n in [(1, 2), (63, 2), (60, 130), (317, 8)]:
        ks, vs = (0.37, 1.9) if start == 63 else (1.0, 1.0)
        starts = [start, start // 2]
        k0, v0 = Qz(torch.randn(N, Smax, E, device=dev), ks), Qz(torch.randn(N, Smax, E, device=dev), vs)
        gk, gv, kc, vc = _caches(k0, v0)
        qkv = torch.randn(N * n, 3 * E, device=dev).bfloat16()
        o = append_attention(qkv, kc, vc, torch.tensor(starts, device=dev), n, H, hd, per_seq=True, splits=splits,
                             k_scale=ks, v_scale=vs)
        o, rows = o.view(N, n, E), qkv.view(N, n, 3 * E)
        for s, st in enumerate(starts):
            m = min(n, Smax - st)  # the tokens that fit
            k0[s, st:st + m], v0[s, st:st + m] = Qz(rows[s, :m, E:2 * E], ks), Qz(rows[s, :m, 2 * E:], vs)
            assert not o[s, m:].any(), (start, s)
            _check(o[s, :m], rows[s, :m], k0[s:s + 1], v0[s:s + 1], st, m, H, hd, f"o of sequence {s} at {start}", ks, vs)
        assert torch.equal(gk, k0) and torch.equal(gv, v0), start
        assert_guards_intact(gk, gv)


# relative error of the step's logits against the full forward's last row, measured on the MI355X
# for this seeded model (docs/GENERATION.md): fp8 cache FP8_MEASURED, bf16 cache BF16_MEASURED
FP8_MEASURED = 4.21e-3
BF16_MEASURED = 2.11e-3


def test_model_fp8_cache():
    """Prefill 40 tokens, then three graphed steps: bit-equal to the eager one-token step on a
    second fp8 cache (the same kernels), and close to the full forward."""
    torch.manual_seed(0)
    with torch.device(dev):
        m = TransformerDecoderLM(64, 32, 2, 2, 512, 128)
    m.eval()
    ids = torch.randint(0, 512, (1, 43), device=dev)
    pos = torch.arange(43, device=dev)[None]
    with torch.no_grad():
        ca, cb, cbf = m.new_kv_cache(1, 64, kv_dtype="fp8"), m.new_kv_cache(1, 64, kv_dtype="fp8"), m.new_kv_cache(1, 64)
        assert all(t.dtype == FP8 and 2 * t.nbytes == r.nbytes for t, r in zip(ca.k + ca.v, cbf.k + cbf.v))
        for c in (ca, cb, cbf):
            m.decode(ids[:, :40], pos[:, :40], c)
        dec, dec_bf = m.graph_decoder(ca), m.graph_decoder(cbf)
        for t in range(40, 43):
            lg = dec.step(ids[:, t:t + 1]).clone()
            assert torch.equal(lg, m.decode(ids[:, t:t + 1], pos[:, t:t + 1], cb)), t
            ref = m(ids[:, :t + 1], pos[:, :t + 1])[:, -1:].float()
            err = ((lg.float() - ref).norm() / ref.norm()).item()
            err_bf = ((dec_bf.step(ids[:, t:t + 1]).float() - ref).norm() / ref.norm()).item()
            print(f"step {t}: relative error fp8 {err:.4e}, bf16 {err_bf:.4e}")
            assert err < min(1.5 * FP8_MEASURED, 0.25), (t, err)
    prompts = ["The big brown cat ", "One day, ", "She said that nobody would ever "]
    out = generate_batch(m, prompts, ByteTokenizer(vocab_size=512), torch.device(dev), 6, temperature=0.8, top_k=40,
                         kv_dtype="fp8", prefill_chunk=16)
    assert len(out) == 3 and all(isinstance(s, str) for s in out)
