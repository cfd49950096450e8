"""KV-cache decoding of ``TransformerDecoderLM``: the cache, the incremental forward behind
``model.decode`` and the one-token step captured as a HIP graph.

Same kernels as the training forward (``models/fused.py``: LayerNorm, QKV / FFN GEMMs with fused
epilogues, the LM head) with the layers' self-attention replaced by one of two attends over the
cache: a block of new tokens with the length on the host (prefill, eager steps), or one token per
sequence with the lengths on the device (the graphed step).
"""
from __future__ import annotations

import math

import torch

from ..ops.attention import attention_fwd, decode_attention
from ..ops.gemm import act_code
from .fused import _layer_forward, ensure_store, head_logits, last_rows, run_embeddings


class KVCache:
    """Keys / values of every layer for the tokens decoded so far: ``[N, S_max, H*hd]`` each
    in the compute dtype (GPT-2 XL at S_max = 1024: 2 x 48 x 1024 x 1600 x 2 B = 315 MB per
    sequence).  ``ragged``: one length per sequence -- ``len_t`` is ``[N]`` with the host copy
    ``lens``, so right-padded prompts of different lengths share the batch.  ``len`` is the
    (longest) length on the host; only the methods below assign the lengths' host copies."""

    def __init__(self, model, N, S_max, device, dtype, ragged=False):
        self.k, self.v = [], []
        for layer in model.decoder.layers:
            E = layer.attn.heads * layer.attn.head_dim
            # zeroed: the graphed step reads the whole capacity (masked, but 0 * NaN = NaN)
            self.k.append(torch.zeros(N, S_max, E, device=device, dtype=dtype))
            self.v.append(torch.zeros(N, S_max, E, device=device, dtype=dtype))
        self.len = 0
        self.capacity = S_max
        self.ragged = bool(ragged)
        self.len_t = torch.zeros(N if ragged else 1, device=device, dtype=torch.int64)  # device copy for the graph
        self.lens = [0] * N if ragged else None

    def check_room(self, n: int) -> None:
        if self.len + n > self.capacity:
            raise ValueError(f"KV cache full ({self.len} + {n} > {self.capacity})")

    def advance(self, n: int = 1) -> None:
        """Host copies of the lengths after a step that advanced ``len_t`` on the device."""
        self.len += n
        if self.ragged:
            self.lens = [l + n for l in self.lens]

    def set_lengths(self, lens) -> None:
        """Host and device lengths after a block: one per sequence, ``[L]`` for a shared length."""
        self.len = max(lens)
        if self.ragged:
            self.lens = list(lens)
            self.len_t.copy_(torch.tensor(lens, dtype=torch.int64))
        else:
            self.len_t.fill_(self.len)

    def positions(self, N: int) -> torch.Tensor:
        """Position ids [N, 1] of the next token, read from the device lengths."""
        return self.len_t.view(N, 1) if self.ragged else self.len_t.expand(N, 1)


def _block_attend(qkv, cache, li, H, hd):
    """Append the K/V of the n new tokens per sequence (qkv [N*n, 3*H*hd]) to layer li's cache at
    the host length ``cache.len`` and attend to every cached key.

    Prefill (empty cache) is the flash-attention kernel over the n tokens; a decode step is
    n queries against ``start + n`` keys -- a memory-bound read of the cache (GEMV-shaped,
    no tiles to fill), done as two batched products in f32."""
    E = H * hd
    N = cache.k[li].shape[0]
    n = qkv.shape[0] // N
    start = cache.len
    L = start + n
    q3 = qkv.view(N, n, 3, E)
    cache.k[li][:, start:L] = q3[:, :, 1]
    cache.v[li][:, start:L] = q3[:, :, 2]
    if start == 0:
        return attention_fwd(qkv, N, n, H, hd, None, causal=True)
    q = q3[:, :, 0].float().reshape(N, n, H, hd).transpose(1, 2)             # [N, H, n, hd]
    k = cache.k[li][:, :L].float().reshape(N, L, H, hd).transpose(1, 2)     # [N, H, L, hd]
    v = cache.v[li][:, :L].float().reshape(N, L, H, hd).transpose(1, 2)
    sc = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(hd))                  # [N, H, n, L]
    if n > 1:  # causal inside the new block: query i sees keys < start + i + 1
        qi = torch.arange(n, device=qkv.device)[:, None] + start
        sc = sc.masked_fill(torch.arange(L, device=qkv.device)[None, :] > qi, float("-inf"))
    o = torch.softmax(sc, -1) @ v                                            # [N, H, n, hd]
    return o.transpose(1, 2).reshape(N * n, E).to(qkv.dtype), None


def _step_attend(qkv, cache, li, H, hd):
    """One query per sequence against the cache, the new key / value appended at the
    device-side length(s) by the decode kernel: no shape depends on a length, so the step
    can be graphed."""
    return decode_attention(qkv, cache.k[li], cache.v[li], cache.len_t, H, hd, per_seq=cache.ragged), None


def _run_layers(model, store, x, N, n, cache, attend):
    """Every layer on the n new tokens of each sequence, ``attend(qkv, cache, li, H, hd) -> (o, lse)``
    in place of the self-attention; the unit boundaries are reported to the store (a sharded
    store gathers its weights there)."""
    act = act_code(model.activation)
    for li, layer in enumerate(model.decoder.layers):
        H, hd = layer.attn.heads, layer.attn.head_dim
        u = layer._unit_id
        store.pre_forward(u)
        x, _ = _layer_forward(x, None, layer, store, N, n, act, False, (None, None),
                              attend=lambda qkv: attend(qkv, cache, li, H, hd))
        store.post_forward(u, False)
    return x


def decode_step(model, store, cache, tok, sampler=None):
    """One token ``tok`` [N, 1] per sequence with every length on the device: embedding at positions
    ``len_t``, the layers with the decode attention (appends at ``len_t``), the LM head and -- with
    ``sampler`` -- the sampler, which writes the next token into ``sampler.tok`` and advances the
    lengths.  No shape depends on a length, so the step can be graphed; the caller advances the
    host lengths (``cache.advance``).  Returns logits [N, 1, V]."""
    N = tok.shape[0]
    x = run_embeddings(model, store, tok, cache.positions(N), False)
    x = _run_layers(model, store, x, N, 1, cache, _step_attend)
    logits = head_logits(model, x, store)
    if sampler is not None:
        sampler(logits, lens=cache.len_t)
    else:
        cache.len_t.add_(1)
    return logits.reshape(N, 1, -1)


def kv_decode_forward(model, input_ids, position_ids, cache, lens=None):
    """Incremental forward for decoding: runs only the new tokens (the whole prompt on the first
    call, then one token per call) through the layers, extends ``cache`` and returns the logits
    of the last new token, ``[N, 1, V]``; the reference recomputes the whole sequence for every
    token (its ``utils.py:57-65``).

    A ragged cache first takes right-padded prompts ``input_ids`` [N, S] with their true lengths
    ``lens``: the causal flash-attention forward over all S positions (no pad mask -- a valid row
    never sees a later key), K / V of every position into the cache, the logits of row
    ``lens[n] - 1`` of each sequence.  The padded positions land in the cache beyond ``lens[n]``;
    the decode kernel reads only ``j < len[n]`` and overwrites them one by one.  After that it
    takes one token per sequence at its own position (``position_ids`` unused)."""
    store = ensure_store(model)
    N, n = input_ids.shape
    dev = input_ids.device
    if cache.ragged and cache.len > 0:
        if n != 1:
            raise ValueError("ragged KV cache: one token per step after the prefill")
        cache.check_room(1)
        logits = decode_step(model, store, cache, input_ids)
        cache.advance(1)
        return logits
    if cache.ragged:
        lens = [int(l) for l in lens]
        if len(lens) != N or min(lens) < 1 or max(lens) > n:
            raise ValueError("ragged prefill: one length in 1..S per sequence")
        position_ids = torch.arange(n, device=dev).expand(N, n)
    else:
        lens = [cache.len + n]
    cache.check_room(n)
    x = run_embeddings(model, store, input_ids, position_ids, False)
    x = _run_layers(model, store, x, N, n, cache, _block_attend)
    cache.set_lengths(lens)
    if cache.ragged:
        last = (torch.tensor(lens, dtype=torch.int64) - 1).to(dev)
        rows = x.view(N, n, -1)[torch.arange(N, device=dev), last].contiguous()
    else:
        rows = last_rows(x, N, n)
    return head_logits(model, rows, store).reshape(N, 1, -1)


class GraphDecoder:
    """The one-token decode step (``decode_step``: embedding, every layer, LM head, cache append
    and, with ``sampler`` (``ops/sample.py:Sampler``, a ragged cache), the sampler) captured once
    as a HIP graph and replayed per token: a GPT-2 decode step is a few hundred small launches, so
    eager decoding is launch-bound (measured in ``bench/generate.py``).  The sampler writes the
    next token straight into the graph's own ``tok`` buffer and into its column of the output
    buffer, and advances the lengths: a replay then needs nothing from the host, ``step()`` with
    no argument.  Needs a non-sharded parameter store (single GPU / DDP); FSDP decodes eagerly."""

    def __init__(self, model, cache, sampler=None):
        self.model, self.cache, self.sampler = model, cache, sampler
        self.store = ensure_store(model)
        N = cache.k[0].shape[0]
        self.tok = sampler.tok if sampler is not None else torch.zeros(N, 1, device=cache.len_t.device,
                                                                       dtype=torch.int64)
        self.graph = None
        self.out = None

    def step(self, tok=None):
        """Append one token per sequence at the cache's current lengths (``tok`` [N, 1]; None: the
        sampler's last draw, already in place); logits [N, 1, V], a view of the graph's output
        buffer, overwritten by the next step."""
        cache = self.cache
        cache.check_room(1)
        if tok is not None:
            self.tok.copy_(tok)
        if self.graph is None:
            # eager warm-up (lazy library init), then undo what it advanced; the cache rows it
            # appended are rewritten with the same values by the first replay
            state = [cache.len_t] + (self.sampler.state() if self.sampler is not None else [])
            saved = [t.clone() for t in state]
            decode_step(self.model, self.store, cache, self.tok, self.sampler)
            for t, v in zip(state, saved):
                t.copy_(v)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self.out = decode_step(self.model, self.store, cache, self.tok, self.sampler)
            self.graph = g
        self.graph.replay()
        cache.advance(1)
        return self.out
