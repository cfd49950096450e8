"""KV-cache decoding of ``TransformerDecoderLM``: the cache, the incremental forward behind
``model.decode`` and the one-token step captured as a HIP graph.

Same kernels as the training forward (``models/fused.py``: LayerNorm, QKV / FFN GEMMs with fused
epilogues, the LM head) with the layers' self-attention replaced by one of two attends over the
cache: a block of new tokens (prefill into an empty cache, a block appended to a cache that holds
tokens, eager steps), or one token per sequence with the lengths on the device (the graphed step).
"""
from __future__ import annotations

import math

import torch

from ..ops.attention import FP8, append_attention, attention_fwd, decode_attention, kv_cache_store_fp8
from ..ops.gemm import _SKINNY_MAX_ROWS, act_code, quantize_weight
from .fused import (_layer_forward, _layer_forward_ln_linear, _qkv_weight, ensure_store, head_logits, last_rows,
                    ln_linear_step, run_embeddings)


class KVCache:
    """Keys / values of every layer for the tokens decoded so far: ``[N, S_max, H*hd]`` each
    in the compute dtype (GPT-2 XL at S_max = 1024: 2 x 48 x 1024 x 1600 x 2 B = 315 MB per
    sequence).  ``ragged``: one length per sequence -- ``len_t`` is ``[N]`` with the host copy
    ``lens``, so right-padded prompts of different lengths share the batch.  ``len`` is the
    (longest) length on the host; only the methods below assign the lengths' host copies.

    ``kv_dtype="fp8"``: the tensors are ``torch.float8_e4m3fn``, half the bytes (GPT-2 XL at
    S_max = 1024: 157 MB per sequence), holding ``x / k_scale`` and ``x / v_scale`` (one host
    float per cache each, ``ops/attention.py:kv_quantize_ref``); every attend over the cache is then
    a HIP kernel that dequantises on the way in.  ``models/gpt.py:new_kv_cache`` checks what that
    needs (CUDA, a bf16 local store, head_dim 32 / 64 / 128)."""

    def __init__(self, model, N, S_max, device, dtype, ragged=False, kv_dtype=None, k_scale=1.0, v_scale=1.0):
        if kv_dtype not in (None, "bf16", "fp8"):
            raise ValueError(f"KV cache: kv_dtype must be None, 'bf16' or 'fp8', not {kv_dtype!r}")
        self.fp8 = kv_dtype == "fp8"
        self.k_scale, self.v_scale = float(k_scale), float(v_scale)
        if not self.fp8 and (self.k_scale != 1.0 or self.v_scale != 1.0):
            raise ValueError("KV cache: k_scale / v_scale belong to the fp8 cache")
        if self.fp8:
            dtype = FP8  # (zeros: byte 0 is +0)
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

    def set_shared_start(self, start: int) -> None:
        """Every sequence at ``start`` (a ragged cache too): where the next block of a chunked
        prefill goes; ``set_lengths`` gives the sequences their own lengths afterwards."""
        self.len = start
        if self.ragged:
            self.lens = [start] * len(self.lens)
        self.len_t.fill_(start)

    def positions(self, N: int) -> torch.Tensor:
        """Position ids [N, 1] of the next token, read from the device lengths."""
        return self.len_t.view(N, 1) if self.ragged else self.len_t.expand(N, 1)


class QuantDecodeStore:
    """The model's parameter store with a quantised copy of the Linear weights a one-token step
    streams: each layer's fused QKV, ``to_out``, ``up_proj`` and ``down_proj`` and the LM head.
    ``dtype="fp8"``: e4m3 with one f32 scale per output row, as ``ops/gemm.py:QWeight`` --
    ``linear_fwd`` then runs ``dpc_gemm_wq8`` (csrc/wq_gemm.hip); ``"fp4"``: MXFP4, as
    ``ops/gemm.py:MxWeight`` -- ``dpc_gemm_wq4`` (csrc/wq4_gemm.hip).  LayerNorm weights, biases and
    embeddings are the wrapped store's, as is everything else.  The copy is extra memory beside the
    bf16 weights (prefill and blocks of tokens keep those: about 1.6 GB for GPT-2 XL in fp8, 0.8 GB
    in fp4), and a snapshot: it does not follow later updates of the weights."""

    def __init__(self, model, store, dtype="fp8"):
        self._store = store
        self.dtype = dtype
        self._q, self._qkv = {}, {}
        for layer in model.decoder.layers:
            self._qkv[id(layer.attn)] = quantize_weight(_qkv_weight(store, layer.attn), dtype)
            for lin in (layer.attn.to_out, layer.fc.up_proj, layer.fc.down_proj):
                self._q[id(lin.weight)] = quantize_weight(store.weight(lin.weight), dtype)
        self._q[id(model.lm_head.weight)] = quantize_weight(store.weight(model.lm_head.weight), dtype)

    def weight(self, p):
        q = self._q.get(id(p))
        return q if q is not None else self._store.weight(p)

    def qkv_weight(self, attn):
        return self._qkv[id(attn)]

    def __getattr__(self, name):
        return getattr(self._store, name)


Fp8DecodeStore = QuantDecodeStore  # (its name while fp8 was the only dtype)


def quantize_decode_weights(model, dtype="fp8") -> QuantDecodeStore:
    """A ``QuantDecodeStore`` (``dtype`` "fp8" or "fp4") of the model's weights as they are now, for
    ``decode_step`` / ``GraphDecoder`` / ``model.decode(..., weights=)``.  Needs CUDA and a bf16
    non-sharded store (``ValueError`` otherwise); the step takes at most 64 sequences."""
    if dtype not in ("fp8", "fp4"):
        raise ValueError(f"quantised decode weights: dtype must be 'fp8' or 'fp4', not {dtype!r}")
    from ..parallel.store import LocalStore

    store = ensure_store(model)
    device = next(model.parameters()).device
    if device.type != "cuda" or not isinstance(store, LocalStore) or store.compute_dtype != torch.bfloat16:
        raise ValueError(f"{dtype} decode weights: need CUDA and a bf16 non-sharded parameter store "
                         f"(device {device}, {type(store).__name__} {store.compute_dtype})")
    return QuantDecodeStore(model, store, dtype)


def check_fp8_weight_batch(N: int) -> None:
    if N > _SKINNY_MAX_ROWS:
        raise ValueError(f"fp8 / fp4 decode weights: a batch of at most {_SKINNY_MAX_ROWS} sequences, not {N}")


def _block_attend(qkv, cache, li, H, hd):
    """Append the K/V of the n new tokens per sequence (qkv [N*n, 3*H*hd]) to layer li's cache at
    the host length ``cache.len`` and attend to every cached key.

    Prefill (empty cache) is the flash-attention kernel over the n tokens; a block of n > 1 tokens
    into a cache that holds some is the append kernel, which reads the start(s) from ``len_t``
    (``ops/attention.py:append_attention``); an eager one-token step is one query against
    ``start + 1`` keys -- a memory-bound read of the cache, done as two batched products in f32."""
    E = H * hd
    N = cache.k[li].shape[0]
    n = qkv.shape[0] // N
    start = cache.len
    scales = dict(k_scale=cache.k_scale, v_scale=cache.v_scale) if cache.fp8 else {}
    if start > 0 and n > 1:
        return append_attention(qkv, cache.k[li], cache.v[li], cache.len_t, n, H, hd, per_seq=cache.ragged,
                                **scales), None
    if cache.fp8:
        # prefill: quantised rows into the cache (len_t holds the start, 0), flash attention over the
        # prompt's own bf16 k / v; the one-token step: the decode kernel (no torch path over fp8)
        if start > 0:
            return decode_attention(qkv, cache.k[li], cache.v[li], cache.len_t, H, hd, per_seq=cache.ragged,
                                    **scales), None
        kv_cache_store_fp8(qkv, cache.k[li], cache.v[li], cache.len_t, n, H, hd, per_seq=cache.ragged, **scales)
        return attention_fwd(qkv, N, n, H, hd, None, causal=True)
    L = start + n
    q3 = qkv.view(N, n, 3, E)
    cache.k[li][:, start:L] = q3[:, :, 1]
    cache.v[li][:, start:L] = q3[:, :, 2]
    if start == 0:
        return attention_fwd(qkv, N, n, H, hd, None, causal=True)
    q = q3[:, :, 0].float().reshape(N, n, H, hd).transpose(1, 2)             # [N, H, n, hd]
    k = cache.k[li][:, :L].float().reshape(N, L, H, hd).transpose(1, 2)     # [N, H, L, hd]
    v = cache.v[li][:, :L].float().reshape(N, L, H, hd).transpose(1, 2)
    sc = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(hd))                  # [N, H, 1, L]
    o = torch.softmax(sc, -1) @ v                                            # [N, H, n, hd]
    return o.transpose(1, 2).reshape(N * n, E).to(qkv.dtype), None


def _step_attend(qkv, cache, li, H, hd):
    """One query per sequence against the cache, the new key / value appended at the
    device-side length(s) by the decode kernel: no shape depends on a length, so the step
    can be graphed."""
    scales = dict(k_scale=cache.k_scale, v_scale=cache.v_scale) if cache.fp8 else {}
    return decode_attention(qkv, cache.k[li], cache.v[li], cache.len_t, H, hd, per_seq=cache.ragged, **scales), None


def _run_layers(model, store, x, N, n, cache, attend):
    """Every layer on the n new tokens of each sequence, ``attend(qkv, cache, li, H, hd) -> (o, lse)``
    in place of the self-attention; the unit boundaries are reported to the store (a sharded
    store gathers its weights there).  One token per sequence (n = 1) runs each LayerNorm inside
    the Linear that consumes it where ``ln_linear_step`` holds for the layer's weights."""
    act = act_code(model.activation)
    for li, layer in enumerate(model.decoder.layers):
        H, hd = layer.attn.heads, layer.attn.head_dim
        u = layer._unit_id
        store.pre_forward(u)
        if n == 1 and ln_linear_step(store, x, _qkv_weight(store, layer.attn), store.weight(layer.fc.up_proj.weight)):
            x = _layer_forward_ln_linear(x, layer, store, act, lambda qkv: attend(qkv, cache, li, H, hd))
        else:
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
    logits = head_logits(model, x, store, one_token=True)
    if sampler is not None:
        sampler(logits, lens=cache.len_t)
    else:
        cache.len_t.add_(1)
    return logits.reshape(N, 1, -1)


def _last_valid_rows(x, N, n, lens, dev):
    """Row ``lens[s] - 1`` of each sequence's n rows of x [N*n, D]: [N, D]."""
    last = (torch.tensor(lens, dtype=torch.int64) - 1).to(dev)
    return x.view(N, n, -1)[torch.arange(N, device=dev), last].contiguous()


def prefill_chunked(model, store, input_ids, position_ids, cache, lens, chunk):
    """The prompt into an empty cache in blocks of ``chunk`` tokens, which bounds the activations
    to one block's: block 0 through the flash forward, block c through the append kernel at the
    shared start ``c * chunk`` (a ragged cache too: right-padded positions land beyond ``lens[s]``
    as in the one-shot prefill).  The hidden row ``lens[s] - 1`` of each sequence is kept from the
    block that holds it and the LM head runs once on [N, D]; the lengths are set at the end."""
    N, n = input_ids.shape
    dev = input_ids.device
    rows = None
    try:
        for c0 in range(0, n, chunk):
            c1 = min(n, c0 + chunk)
            cache.set_shared_start(c0)
            x = run_embeddings(model, store, input_ids[:, c0:c1], position_ids[:, c0:c1], False)
            x = _run_layers(model, store, x, N, c1 - c0, cache, _block_attend).view(N, c1 - c0, -1)
            if rows is None:
                rows = torch.empty(N, x.shape[-1], device=dev, dtype=x.dtype)
            for s, l in enumerate(lens):
                if c0 < l <= c1:
                    rows[s] = x[s, l - 1 - c0]
    except BaseException:
        cache.set_shared_start(0)  # a failed prefill leaves the cache empty, as it found it
        raise
    cache.set_lengths(lens if cache.ragged else [n])
    return head_logits(model, rows, store).reshape(N, 1, -1)


def kv_decode_forward(model, input_ids, position_ids, cache, lens=None, prefill_chunk=0, weights=None):
    """Incremental forward for decoding: runs only the new tokens (the whole prompt on the first
    call, then one token or a block of tokens per call) through the layers, extends ``cache`` and
    returns the logits of the last new token, ``[N, 1, V]``; the reference recomputes the whole
    sequence for every token (its ``utils.py:57-65``).

    A ragged cache first takes right-padded prompts ``input_ids`` [N, S] with their true lengths
    ``lens``: the causal flash-attention forward over all S positions (no pad mask -- a valid row
    never sees a later key), K / V of every position into the cache, the logits of row
    ``lens[n] - 1`` of each sequence.  The padded positions land in the cache beyond ``lens[n]``;
    the decode kernel reads only ``j < len[n]`` and overwrites them one by one.  After that it
    takes one token per sequence at its own position, or -- with ``lens``, the valid new tokens
    1..n of each sequence -- a right-padded block of n tokens per sequence, each sequence's at its
    own positions (``position_ids`` unused); pad rows past the capacity are not written.

    ``prefill_chunk``: with an empty cache and ``0 < prefill_chunk < n``, the prompt runs in
    blocks of that many tokens (``prefill_chunked``).

    ``weights``: a ``QuantDecodeStore`` (``quantize_decode_weights``) for the one-token step; the
    prompt and blocks of tokens run on the bf16 weights."""
    store = ensure_store(model)
    N, n = input_ids.shape
    if weights is not None and n == 1 and cache.len > 0:
        check_fp8_weight_batch(N)
        store = weights
    dev = input_ids.device
    if cache.ragged and cache.len > 0:
        if lens is not None:
            lens = [int(l) for l in lens]
            if len(lens) != N or min(lens) < 1 or max(lens) > n:
                raise ValueError("ragged block: one length in 1..n per sequence")
        elif n != 1:
            raise ValueError("ragged KV cache: one token per step, or a block with lens")
        if n == 1:  # (with lens too: every length is 1) the one-token step, each sequence at its own position
            cache.check_room(1)
            logits = decode_step(model, store, cache, input_ids)
            cache.advance(1)
            return logits
        new = [old + l for old, l in zip(cache.lens, lens)]
        if max(new) > cache.capacity:
            raise ValueError(f"KV cache full ({max(new)} > {cache.capacity})")
        max_pos = model.max_position_embeddings - 1
        position_ids = (cache.len_t[:, None] + torch.arange(n, device=dev)).clamp_(max=max_pos)  # (pad rows)
        x = run_embeddings(model, store, input_ids, position_ids, False)
        x = _run_layers(model, store, x, N, n, cache, _block_attend)
        cache.set_lengths(new)
        return head_logits(model, _last_valid_rows(x, N, n, lens, dev), store).reshape(N, 1, -1)
    if cache.ragged:
        lens = [int(l) for l in lens]
        if len(lens) != N or min(lens) < 1 or max(lens) > n:
            raise ValueError("ragged prefill: one length in 1..S per sequence")
        position_ids = torch.arange(n, device=dev).expand(N, n)
    else:
        lens = [cache.len + n]
    cache.check_room(n)
    if cache.len == 0 and 0 < prefill_chunk < n:
        return prefill_chunked(model, store, input_ids, position_ids, cache, lens if cache.ragged else [n] * N,
                               prefill_chunk)
    x = run_embeddings(model, store, input_ids, position_ids, False)
    x = _run_layers(model, store, x, N, n, cache, _block_attend)
    cache.set_lengths(lens)
    if cache.ragged:
        rows = _last_valid_rows(x, N, n, lens, dev)
    else:
        rows = last_rows(x, N, n)
    return head_logits(model, rows, store, one_token=n == 1).reshape(N, 1, -1)


class GraphDecoder:
    """The one-token decode step (``decode_step``: embedding, every layer, LM head, cache append
    and, with ``sampler`` (``ops/sample.py:Sampler``, a ragged cache), the sampler) captured once
    as a HIP graph and replayed per token: a GPT-2 decode step is a few hundred small launches, so
    eager decoding is launch-bound (measured in ``bench/generate.py``).  The sampler writes the
    next token straight into the graph's own ``tok`` buffer and into its column of the output
    buffer, and advances the lengths: a replay then needs nothing from the host, ``step()`` with
    no argument.  Needs a non-sharded parameter store (single GPU / DDP); FSDP decodes eagerly.
    ``weights``: a ``QuantDecodeStore`` (``quantize_decode_weights``) to run the step's Linears on."""

    def __init__(self, model, cache, sampler=None, weights=None):
        self.model, self.cache, self.sampler = model, cache, sampler
        self.store = ensure_store(model) if weights is None else weights
        N = cache.k[0].shape[0]
        if weights is not None:
            check_fp8_weight_batch(N)
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
