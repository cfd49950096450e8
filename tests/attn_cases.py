"""Attention inputs whose scores move the running max, shared by the CPU and the GPU tests.

``randn`` inputs give scaled scores of N(0, 1): the flash kernels' lazy rescale (the running max
moves only when a tile's max exceeds it by more than 8 log2 units) is then taken once per block,
on the first tile, where every accumulator is zero.  ``attention_score_case`` builds inputs whose
scaled score in log2 units is "small noise + r_j", r_j a profile over the key index j:

* q and k are 0.5 randn, v is randn;
* coordinate 0 of every head's q is the constant A = 16;
* coordinate 0 of every head's k is r_j / (A c), c = log2(e) / sqrt(hd);
* everything is rounded to bf16 (the references use the rounded values: the ramp's bf16 staircase
  is part of the input).

The noise is c times a sum of hd - 1 products of two N(0, 1/4): a standard deviation of about
0.36 log2 units at every head size.

Profiles (G in log2 units per 64-key tile):

  rising   r_j = G j / 64      G = 12: a rescale on every tile after the first, alpha ~ 2^-12;
                               G = 5: on every other tile, P up to 2^8 against a kept max between;
                               G = 70: with the causal mask, future keys up to ~350 above the lse
  spike    r_j = G at key S - 70, 0.75 G at key S / 2 + 3, else 0: one late rescale onto large
           accumulators
  falling  r_j = -G j / 64     G = 12: never rescales, later tiles underflow (the control);
                               G = 70: with ``attention_score_mask``, padded keys ~153 above the lse

``attention_score_mask`` (N = 3): left padding that covers the whole first tile and part of the
next two, an interior run across a tile boundary, and a sequence that is all padding.

``rescale_event_rows`` and ``masked_excess`` say, in f64, what a case reaches; the CPU tests assert
it so that the GPU tests cannot pass vacuously.
"""
from __future__ import annotations

import math
import zlib

import torch

A_Q = 16.0
TILE = 64     # keys per tile of every flash kernel (csrc/attention.hip: KT)
LAZY = 8.0    # the lazy-rescale threshold in log2 units

# (profile, G); the first four are "moderate": every key still carries weight in some row
PROFILES = [("rising", 12), ("rising", 5), ("spike", 12), ("falling", 12), ("rising", 70), ("falling", 70)]
MODERATE = PROFILES[:4]
# (hd, S): the smallest S with two plain tiles before a query block (q0 >= 128, so S > 256), one
# per bf16 forward kernel: fwd3<64>, fwd<128>, fwd2<32> (S < 512) and fwd3<32> (S >= 512)
SHAPES = [(64, 320), (128, 320), (32, 320), (32, 576)]
N_SEQ, HEADS = 3, 2


def profile_ramp(profile: str, G: float, S: int) -> torch.Tensor:
    """r_j, f64 [S]."""
    j = torch.arange(S, dtype=torch.float64)
    if profile == "rising":
        return G * j / TILE
    if profile == "falling":
        return -G * j / TILE
    if profile == "spike":
        r = torch.zeros(S, dtype=torch.float64)
        r[S - 70] = G
        r[S // 2 + 3] = 0.75 * G
        return r
    raise ValueError(f"attention_score_case: unknown profile {profile!r}")


def _seed(*key) -> int:
    return zlib.crc32(repr(key).encode())


def attention_score_case(profile, G, hd, S, N=N_SEQ, H=HEADS, device="cpu"):
    """bf16 qkv [N S, 3 H hd] (drawn on the CPU from a seed of the arguments: the same values on
    every device)."""
    g = torch.Generator().manual_seed(_seed("qkv", profile, G, hd, S, N, H))
    E = H * hd
    qkv = torch.randn(N * S, 3, H, hd, generator=g)
    qkv[:, :2] *= 0.5
    c = math.log2(math.e) / math.sqrt(hd)
    qkv[:, 0, :, 0] = A_Q
    ramp = (profile_ramp(profile, G, S) / (A_Q * c)).float()
    qkv[:, 1, :, 0] = ramp.repeat(N)[:, None]
    return qkv.reshape(N * S, 3 * E).bfloat16().to(device)


def attention_score_dout(profile, G, hd, S, N=N_SEQ, H=HEADS, device="cpu"):
    """bf16 randn dO [N S, H hd] of the case."""
    g = torch.Generator().manual_seed(_seed("dout", profile, G, hd, S, N, H))
    return torch.randn(N * S, H * hd, generator=g).bfloat16().to(device)


def attention_score_mask(N, S, device="cpu"):
    """Key-padding mask [N, S] (True = padded) of the score cases; N = 3, S >= 200."""
    assert N == 3 and S >= 200
    pad = torch.zeros(N, S, dtype=torch.bool, device=device)
    pad[0, :140] = True      # a wholly masked first tile and two more partly; causal: 140 dead query rows
    pad[1, 130:200] = True   # interior keys across a tile boundary
    pad[2, :] = True         # an all-padding sequence
    return pad


def score_references(qkv, do, N, S, H, hd, pad, causal):
    """(o64, lse64, g64, o_ideal, lse32, g_ideal) of a case, on qkv's device: the f64 forward and
    its gradient (the explicit backward of kernel_checks in f64, from the f64 o and lse -- autograd
    through a row of -inf scores is not used), and the ideal kernel: plain f32 math rounded to
    bf16, its backward from what a kernel is handed, the ideal's own rounded o and f32 lse."""
    from kernel_checks import attention_bwd_plain, attention_plain

    o64, lse64 = attention_plain(qkv, N, S, H, hd, pad, causal)
    g64 = attention_bwd_plain(qkv, do, o64, lse64, N, S, H, hd, pad, causal, dtype=torch.float64)
    o32, lse32 = attention_plain(qkv, N, S, H, hd, pad, causal, dtype=torch.float32)
    o_ideal = o32.to(qkv.dtype)
    g_ideal = attention_bwd_plain(qkv, do, o_ideal, lse32, N, S, H, hd, pad, causal, dtype=torch.float32).to(qkv.dtype)
    return o64, lse64, g64, o_ideal, lse32, g_ideal


def _scores_log2(qkv, N, S, H, hd, pad, causal):
    """(scaled scores in log2 units f64 [N, H, S, S], allowed [N, 1 or H, S, S])."""
    E = H * hd
    q, k = (qkv[:, i * E:(i + 1) * E].double().reshape(N, S, H, hd).transpose(1, 2) for i in range(2))
    s = (q @ k.transpose(-1, -2)) * (math.log2(math.e) / math.sqrt(hd))
    allowed = torch.ones(S, S, dtype=torch.bool, device=qkv.device)
    if causal:
        allowed = torch.tril(allowed)
    allowed = allowed.expand(N, 1, S, S)
    if pad is not None:
        allowed = allowed & ~pad.bool()[:, None, None, :]
    return s, allowed.expand(N, H, S, S)


def rescale_event_rows(qkv, N, S, H, hd, pad=None, causal=True) -> float:
    """The fraction of all N H S query rows whose running max, carried over the 64-key tiles as
    the kernels carry it (moved to max(m, tile max) when the tile max exceeds it by more than 8
    log2 units), moves at least once from a FINITE previous max -- that is, with live
    accumulators.  Per row: the kernels move a whole wave's rows together, so they rescale at
    least as often."""
    s, allowed = _scores_log2(qkv, N, S, H, hd, pad, causal)
    s = s.masked_fill(~allowed, -math.inf)
    m = torch.full(s.shape[:-1], -math.inf, dtype=torch.float64, device=s.device)
    event = torch.zeros_like(m, dtype=torch.bool)
    for k0 in range(0, S, TILE):
        mx = s[..., k0:k0 + TILE].amax(-1)
        up = mx > m + LAZY
        event |= up & torch.isfinite(m)
        m = torch.where(up, torch.maximum(m, mx), m)
    return event.double().mean().item()


def masked_excess(qkv, N, S, H, hd, pad=None, causal=True) -> float:
    """The largest (masked score - row lse) in log2 units over the rows with a finite lse;
    above 128 an f32 exp2 of it is inf.  -inf if nothing is masked."""
    s, allowed = _scores_log2(qkv, N, S, H, hd, pad, causal)
    lse2 = torch.logsumexp(s.masked_fill(~allowed, -math.inf) * math.log(2.0), -1) / math.log(2.0)
    live = torch.isfinite(lse2)
    if not live.any() or bool(allowed.all()):
        return -math.inf
    over = (s - torch.where(live, lse2, torch.zeros_like(lse2))[..., None]).masked_fill(allowed | ~live[..., None], -math.inf)
    return over.max().item()
