"""Temperature / top-k / top-p sampling of one token per row of logits ``[N, V]``.

The definition is order-free and keeps ties (bf16 logits over a 50K vocabulary are full of
them, so "sort and cut" is not well defined):

* ``z_i = logit_i / temperature``; ``temperature == 0`` is argmax, lowest index on ties.
* top-k (``k > 0``): keep ``i`` iff ``#{j : z_j > z_i} < k`` -- ties at the k-th value all stay.
* top-p (``p < 1``): softmax ``q`` over the top-k survivors; keep ``i`` iff the mass of the kept
  values strictly greater than ``z_i`` is ``< p``.  The largest value always stays.
* draw: ``w_i = exp(z_i - max)`` over the kept set, ``Z = sum w``; the token is the first kept
  index, in index order, whose inclusive prefix sum exceeds ``u Z`` (if none does -- ``u = 1``, or
  rounding -- the last kept index of positive weight: a kept ``-inf`` is never drawn).
* ``u`` is counter-based: ``sample_uniform(seed, row, counters[row])``, 24 bits of an ``fmix32``
  chain (``csrc/common.h``; the torch twin of the hash is in ``ops/dropout.py``).  The counters
  live on the device and every call advances them, so a replayed HIP graph draws a fresh number
  each step with no host involvement.

``sample_logits`` runs ``csrc/sample.hip`` on bf16 GPU logits and ``sample_reference`` -- the torch
twin of the same definition -- on CPU tensors and f32 logits.
"""
from __future__ import annotations

import torch

from . import _lib
from .dropout import M32, _fmix32_int


MAX_VOCAB = 57344  # csrc/sample.hip: SM_MAX_V


def sample_uniform(seed: int, row: int, counter: int) -> float:
    """The uniform in [0, 1) of draw ``counter`` of ``row``: bit-exact twin of ``sample.hip``."""
    x = _fmix32_int(seed & M32)
    x = _fmix32_int(x ^ ((((seed >> 32) & M32) * 0x9E3779B1) & M32))
    x = _fmix32_int(x ^ ((row * 0x85EBCA77 + 0x632BE5AB) & M32))
    x = _fmix32_int(x ^ (counter & M32))
    x = _fmix32_int(x ^ ((((counter >> 32) & M32) * 0x9E3779B1) & M32))
    return (x >> 8) * 2.0 ** -24


def kept_mask(logits: torch.Tensor, temperature: float, top_k: int = 0, top_p: float = 1.0,
              dtype=torch.float32):
    """(kept [N, V] bool, w [N, V]): the candidates of each row after top-k and top-p, and
    ``exp(z - max)`` in ``dtype``.  ``temperature`` must be positive."""
    z = logits.to(dtype) / temperature
    N, V = z.shape
    zs, order = torch.sort(z, dim=-1, descending=True)
    # the number of strictly greater values = the position of a value's first occurrence
    first = torch.searchsorted(-zs, -zs, right=False)
    keep = torch.ones_like(zs, dtype=torch.bool)
    if 0 < top_k < V:
        keep = first < top_k
    ws = torch.exp(zs - zs[:, :1])
    if top_p < 1.0:
        wk = ws * keep
        excl = torch.cumsum(wk, -1) - wk
        greater = torch.gather(excl, 1, first)  # kept mass strictly above each value
        keep_p = greater < top_p * wk.sum(-1, keepdim=True)
        keep = keep & (keep_p | (first == 0))  # (the largest value, ties included, always stays)
    kept = torch.zeros_like(keep).scatter_(1, order, keep)
    w = torch.empty_like(ws).scatter_(1, order, ws)
    return kept, w


def sample_reference(logits: torch.Tensor, temperature: float, top_k: int, top_p: float, u: torch.Tensor,
                     dtype=torch.float32) -> torch.Tensor:
    """Tokens int64 [N] of the definition above, computed in ``dtype`` from uniforms ``u`` [N]."""
    if temperature <= 0:
        z = logits.to(dtype)
        return torch.argmax((z == z.amax(-1, keepdim=True)).to(torch.uint8), dim=-1)  # (the first maximum)
    kept, w = kept_mask(logits, temperature, top_k, top_p, dtype)
    w = w * kept
    cum = torch.cumsum(w, -1)
    hit = kept & (cum > u.to(dtype).reshape(-1, 1) * cum[:, -1:])
    V = logits.shape[1]
    idx = torch.arange(V, device=logits.device)
    last = torch.where(w > 0, idx, torch.zeros_like(idx)).amax(-1)  # (the maximum's weight is 1)
    return torch.where(hit.any(-1), torch.argmax(hit.to(torch.uint8), dim=-1), last)


def sample_logits(logits: torch.Tensor, *, temperature: float, top_k: int = 0, top_p: float = 1.0, seed: int = 0,
                  counters: torch.Tensor, out_tok: torch.Tensor, done: torch.Tensor | None = None, eos: int = -1,
                  u: torch.Tensor | None = None, seq: torch.Tensor | None = None, step: torch.Tensor | None = None,
                  lens: torch.Tensor | None = None) -> torch.Tensor:
    """Sample one token per row of ``logits`` [N, V] (row stride >= V) into ``out_tok`` [N, 1] int64.

    ``counters`` int64 [N]: draws so far, advanced here.  ``u`` f32 [N] overrides the hash (tests).
    ``done`` bool [N]: a set row emits ``eos``; a row that draws ``eos`` is set.  A decode loop also
    passes ``seq`` int64 [N, max_new] with ``step`` int64 [N] (the token goes to column ``step[n]``,
    which then advances; a column past the buffer is dropped) and ``lens`` int64 [N] (advanced)."""
    N, V = logits.shape
    if out_tok.dtype != torch.int64 or out_tok.numel() != N or not out_tok.is_contiguous():
        raise ValueError("sample_logits: out_tok must be a contiguous int64 [N, 1]")
    if counters.dtype != torch.int64 or counters.shape != (N,):
        raise ValueError("sample_logits: counters must be int64 [N]")
    if (seq is None) != (step is None):
        raise ValueError("sample_logits: seq and step go together")
    if not (logits.is_cuda and logits.dtype == torch.bfloat16):
        return _sample_torch(logits, temperature, top_k, top_p, seed, counters, out_tok, done, eos, u, seq, step, lens)
    for t, dt, shape in ((u, torch.float32, (N,)), (done, torch.bool, (N,)), (step, torch.int64, (N,)),
                         (lens, torch.int64, (N,))):
        if t is not None and (t.dtype != dt or t.shape != shape or not t.is_contiguous() or not t.is_cuda):
            raise ValueError("sample_logits: u f32 [N], done bool [N], step / lens int64 [N] on the device")
    if logits.stride(1) != 1 or (N > 1 and logits.stride(0) < V):
        raise ValueError("sample_logits: logits rows must be contiguous")
    if V > MAX_VOCAB:
        raise ValueError(f"sample_logits: at most {MAX_VOCAB} columns (the kernel keeps a row in registers)")
    if seq is not None and (seq.dtype != torch.int64 or seq.dim() != 2 or seq.shape[0] != N or not seq.is_contiguous()):
        raise ValueError("sample_logits: seq must be a contiguous int64 [N, max_new]")
    args = _lib.SampleArgs(
        logits=logits.data_ptr(), counters=counters.data_ptr(), u=_lib.ptr(u), out_tok=out_tok.data_ptr(),
        done=_lib.ptr(done), seq=_lib.ptr(seq), step=_lib.ptr(step), len=_lib.ptr(lens),
        ld=logits.stride(0) if N > 1 else max(logits.stride(0), V), seq_ld=0 if seq is None else seq.shape[1],
        eos=int(eos), N=N, V=V, top_k=int(top_k), temperature=float(temperature), top_p=float(top_p),
        seed_lo=seed & M32, seed_hi=(seed >> 32) & M32)
    _lib.call("dpc_sample", args, logits.device)
    return out_tok


def _sample_torch(logits, temperature, top_k, top_p, seed, counters, out_tok, done, eos, u, seq, step, lens):
    N = logits.shape[0]
    if u is None:
        u = torch.tensor([sample_uniform(seed, n, c) for n, c in enumerate(counters.tolist())],
                         dtype=torch.float32, device=logits.device)
    tok = sample_reference(logits.float(), temperature, top_k, top_p, u)
    if done is not None:
        tok = torch.where(done, torch.full_like(tok, eos), tok)
        done |= tok == eos
    out_tok.copy_(tok.view_as(out_tok))
    counters += 1
    if seq is not None:
        ok = (step >= 0) & (step < seq.shape[1])
        rows = torch.arange(N, device=seq.device)[ok]
        seq[rows, step[ok]] = tok[ok]
        step += 1
    if lens is not None:
        lens += 1
    return out_tok


class Sampler:
    """The sampling parameters and the state of a generation loop over N sequences: the token
    buffer ``tok`` [N, 1] the next step reads, the draw ``counters``, the ``done`` flags, the
    ``[N, max_new]`` output ``seq`` (pre-filled with ``eos``) and its column counter ``step``.
    Calling it samples one token per row of ``logits`` [N, V] and advances all of them (and
    ``lens``, the cache lengths of a decode loop, if given)."""

    def __init__(self, N: int, max_new: int, device, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0,
                 seed: int = 0, eos: int = -1):
        self.temperature, self.top_k, self.top_p, self.seed, self.eos = temperature, top_k, top_p, seed, eos
        self.tok = torch.zeros(N, 1, device=device, dtype=torch.int64)
        self.counters = torch.zeros(N, device=device, dtype=torch.int64)
        self.done = torch.zeros(N, device=device, dtype=torch.bool)
        self.seq = torch.full((N, max(max_new, 1)), eos, device=device, dtype=torch.int64)
        self.step = torch.zeros(N, device=device, dtype=torch.int64)

    def __call__(self, logits: torch.Tensor, lens: torch.Tensor | None = None) -> torch.Tensor:
        return sample_logits(logits, temperature=self.temperature, top_k=self.top_k, top_p=self.top_p,
                             seed=self.seed, counters=self.counters, out_tok=self.tok, done=self.done, eos=self.eos,
                             seq=self.seq, step=self.step, lens=lens)

    def state(self) -> list:
        """The tensors a call advances (a graph capture saves and restores them around its warm-up)."""
        return [self.tok, self.counters, self.done, self.seq, self.step]

    def sequences(self) -> list:
        """The generated tokens of each sequence, cut at its first ``eos``."""
        out = []
        for row in self.seq.tolist():
            out.append(row[:row.index(self.eos)] if self.eos in row else row)
        return out
