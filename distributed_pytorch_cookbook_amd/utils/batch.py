"""Batch preparation and greedy generation (reference ``/root/reference/utils.py``).

``prepare_batch`` keeps the reference contract -- shift by one for next-token targets,
targets equal to ``pad_id`` become -100, position ids 0..S-2, ``mask = ~attention_mask``
(True = padded key) -- with two changes: an all-valid batch gets ``mask=None`` (decided
on the host before the copy, so no device sync; an all-False padding mask is a no-op)
and the position ids are built on the device instead of being copied.

``generate`` is the reference's greedy argmax loop (``utils.py:42-91``): full
recompute per token (``_recompute``), stop at EOS, decode with ``skip_special_tokens``; the LM
head runs on the last position only (``last_only``) where the model supports it, and a model with
``decode`` (``TransformerDecoderLM``, ``models/decode.py``) runs a KV-cache decode instead while
the context fits.  ``model`` is any callable ``model(input_ids=..., position_ids=...) -> logits
[1, s, V]`` (an LM or a parallel engine's forward), so FSDP / pipeline engines run it on every rank.

``generate_batch`` generates for several prompts at once with temperature / top-k / top-p sampling
(``ops/sample.py``; ``temperature=0`` is greedy): right-padded prompts share one ragged KV cache
(a length per sequence), and on a GPU the whole step -- embedding, layers, LM head, sampler --
is one replayed HIP graph (``models/decode.py:GraphDecoder``) that needs nothing from the host;
the loop reads the ``done`` flags every 8 steps only.  Finished sequences keep stepping and emit
EOS; each is cut at its first EOS.  Without ``decode`` it is the same ``_recompute`` loop, prompt
by prompt, sampling with the torch twin.
"""
from __future__ import annotations

import inspect

import torch


def prepare_batch(batch, pad_id: int, device):
    input_ids = batch["input_ids"]
    attention_mask = batch["attention_mask"][:, :-1]
    S = input_ids.shape[1]
    inputs, targets = input_ids[:, :-1].clone(), input_ids[:, 1:].clone()
    targets[targets == pad_id] = -100
    has_pad = not bool(attention_mask.all()) if attention_mask.device.type == "cpu" else True
    device = torch.device(device)
    nb = device.type == "cuda"
    position_ids = torch.arange(S - 1, device=device).unsqueeze(0).expand(inputs.shape[0], -1)
    out = dict(
        input_ids=inputs.to(device, non_blocking=nb),
        position_ids=position_ids,
        mask=(~attention_mask.to(dtype=torch.bool)).to(device, non_blocking=nb) if has_pad else None,
    )
    return out, targets.to(device, non_blocking=nb)


@torch.inference_mode()
def generate(model, prompt: str, tokenizer, device, max_new_tokens: int = 20, use_cache: bool = True,
             temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0) -> str:
    if temperature > 0 or top_k > 0 or top_p < 1.0:  # sampling: the batched loop with one prompt
        return generate_batch(model, [prompt], tokenizer, device, max_new_tokens, temperature, top_k, top_p, seed)[0]
    batch = tokenizer([prompt], truncation=True, max_length=256, return_tensors="pt")
    input_ids = batch["input_ids"].to(device)
    # the learned position table bounds the context: slide a window past it
    max_pos = getattr(model, "max_position_embeddings", None) or 1 << 30
    if use_cache and hasattr(model, "decode") and input_ids.shape[1] + max_new_tokens <= max_pos:
        return _generate_cached(model, input_ids, tokenizer, device, max_new_tokens)
    new = _recompute(model, input_ids, device, max_new_tokens, max_pos, tokenizer.eos_token_id,
                     lambda logits, i: int(logits.argmax(dim=-1)))
    return tokenizer.decode(input_ids[0].tolist() + new, skip_special_tokens=True)


def _generate_cached(model, input_ids, tokenizer, device, max_new_tokens):
    """KV-cache greedy decode: one prefill of the prompt, then one token per forward (same
    tokens as the full-recompute loop while the context fits the position table)."""
    cache = model.new_kv_cache(1, input_ids.shape[1] + max_new_tokens)
    s = input_ids.shape[1]
    logits = model.decode(input_ids, torch.arange(s, device=device).unsqueeze(0), cache)
    out = input_ids[0].tolist()
    step = None
    if device.type == "cuda" and hasattr(model, "graph_decoder"):
        step = model.graph_decoder(cache)  # None if the store is sharded (FSDP)
    for i in range(max_new_tokens):
        new_token = int(logits[0, -1].argmax(dim=-1))
        if new_token == tokenizer.eos_token_id:
            break
        out.append(new_token)
        if i + 1 == max_new_tokens:
            break
        tok = torch.tensor([[new_token]], dtype=input_ids.dtype, device=device)
        if step is not None:
            logits = step.step(tok)
        else:
            logits = model.decode(tok, torch.full((1, 1), len(out) - 1, device=device, dtype=torch.long), cache)
    return tokenizer.decode(out, skip_special_tokens=True)


def _last_only(model) -> bool:
    """Whether the model's forward can run the LM head on the last position only."""
    try:
        fwd = model.forward if isinstance(model, torch.nn.Module) else model
        return "last_only" in inspect.signature(fwd).parameters
    except (TypeError, ValueError):
        return False


def _recompute(model, input_ids, device, max_new_tokens, max_pos, eos, pick) -> list:
    """The reference's loop for one prompt ``input_ids`` [1, s]: the whole context again for every
    token, through any callable (an LM, an FSDP / pipeline engine's forward).  ``pick(logits, i)``
    chooses token i from the last position's logits [V]; returns the new tokens, stopping before
    ``eos``."""
    # only the last position's logits are used: skip the [T, V] head GEMM where the model can
    # (the reference computes every position's logits, utils.py:57-65)
    head = {"last_only": True} if _last_only(model) else {}
    out = []
    for i in range(max_new_tokens):
        ctx = input_ids[:, -max_pos:]
        position_ids = torch.arange(ctx.shape[1], device=device).unsqueeze(0)
        tok = pick(model(input_ids=ctx, position_ids=position_ids, **head)[0, -1], i)
        if tok == eos:
            break
        out.append(tok)
        input_ids = torch.cat([input_ids, torch.tensor([[tok]], dtype=input_ids.dtype, device=device)], 1)
    return out


DONE_POLL = 8  # steps between two reads of the done flags


@torch.inference_mode()
def generate_batch(model, prompts, tokenizer, device, max_new_tokens: int = 20, temperature: float = 0.0,
                   top_k: int = 0, top_p: float = 1.0, seed: int = 0) -> list:
    """Continuations of ``prompts`` (a list of strings), sampled with ``temperature`` / ``top_k`` /
    ``top_p`` from the counter-based stream of ``seed`` (row n of the batch draws
    ``sample_uniform(seed, n, step)``: the same arguments give the same text, on every rank)."""
    from ..ops.sample import Sampler

    device = torch.device(device)
    ids = [tokenizer([p], truncation=True, max_length=256, return_tensors="pt")["input_ids"][0] for p in prompts]
    lens = [int(t.numel()) for t in ids]
    N = len(ids)
    if N == 0 or max_new_tokens <= 0:
        return [tokenizer.decode(t.tolist(), skip_special_tokens=True) for t in ids]
    eos = tokenizer.eos_token_id
    eos = -1 if eos is None else int(eos)
    max_pos = getattr(model, "max_position_embeddings", None) or 1 << 30
    sampler = Sampler(N, max_new_tokens, device, temperature, top_k, top_p, seed, eos)
    if hasattr(model, "decode") and max(lens) + max_new_tokens <= max_pos:
        _sample_cached(model, ids, lens, sampler, device, max_new_tokens)
        new = sampler.sequences()
    else:
        new = [_recompute(model, t.view(1, -1).to(device), device, max_new_tokens, max_pos, eos,
                          _sampled_pick(sampler, n)) for n, t in enumerate(ids)]
    return [tokenizer.decode(t.tolist() + g, skip_special_tokens=True) for t, g in zip(ids, new)]


def _sample_cached(model, ids, lens, sampler, device, max_new_tokens):
    """One prefill of the right-padded prompts into a ragged KV cache, then one token per sequence
    per step: a replayed HIP graph ending in the sampler where the model has one, else eagerly."""
    N, S = len(ids), max(lens)
    padded = torch.zeros(N, S, dtype=torch.int64)
    for n, t in enumerate(ids):
        padded[n, :lens[n]] = t
    cache = model.new_kv_cache(N, S + max_new_tokens, ragged=True)
    logits = model.decode(padded.to(device), None, cache, lens=lens)
    sampler(logits[:, 0])  # (the prefill has set the lengths: token 0 goes to position lens[n])
    dec = None
    if device.type == "cuda" and hasattr(model, "graph_decoder"):
        dec = model.graph_decoder(cache, sampler)  # None if the store is sharded (FSDP) or f32
    for i in range(1, max_new_tokens):
        if i % DONE_POLL == 0 and bool(sampler.done.all()):
            break
        if dec is not None:
            dec.step()
        else:
            sampler(model.decode(sampler.tok, None, cache)[:, 0])


def _sampled_pick(sampler, row):
    """The token rule of ``_recompute`` that samples with the torch twin; ``row`` is the prompt's row
    of the batch, which its uniforms depend on."""
    from ..ops.sample import sample_reference, sample_uniform

    def pick(logits, i):
        u = torch.tensor([sample_uniform(sampler.seed, row, i)], dtype=torch.float32, device=logits.device)
        return int(sample_reference(logits[None].float(), sampler.temperature, sampler.top_k, sampler.top_p, u))

    return pick
