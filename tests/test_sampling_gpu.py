"""The sampler kernel (``csrc/sample.hip``), the per-sequence decode attention and the graphed,
sync-free generation loop on the GPU."""
import math

import pytest
import torch

import sample_cases as sc
from kernel_checks import MARGIN_ATTN, assert_guards_intact, assert_local_close, guarded
from sample_cases import CONFIGS, ROWS, config_rows

from distributed_pytorch_cookbook_amd.models.fused import vocab_ld
from distributed_pytorch_cookbook_amd.models.gpt import TransformerDecoderLM
from distributed_pytorch_cookbook_amd.ops import _lib
from distributed_pytorch_cookbook_amd.ops.attention import decode_attention
from distributed_pytorch_cookbook_amd.ops.sample import MAX_VOCAB, sample_logits, sample_uniform
from distributed_pytorch_cookbook_amd.utils.batch import generate_batch
from distributed_pytorch_cookbook_amd.utils.tokenizer import ByteTokenizer

pytestmark = pytest.mark.gpu
dev = "cuda"
BF, F32 = torch.bfloat16, torch.float32

TEMPERATURE, TOP_K, TOP_P = 0.8, 50, 0.9


def strided(rows):
    """The rows in a ``vocab_ld``-strided device buffer whose padding columns hold +1e4 (a sampler
    that reads them as candidates draws them at once)."""
    N, V = rows.shape
    buf = torch.full((N, vocab_ld(V)), 1e4, dtype=BF, device=dev)
    buf[:, :V] = rows.to(dev)
    return buf[:, :V]


def draw(logits, counters=None, **kw):
    N = logits.shape[0]
    counters = torch.zeros(N, dtype=torch.int64, device=dev) if counters is None else counters
    out = torch.full((N, 1), -7, dtype=torch.int64, device=dev)
    sample_logits(logits, counters=counters, out_tok=out, **kw)
    return out[:, 0].cpu()


@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_sampler_exact_draw_against_f64(ci):
    rows = config_rows(ci)
    u = torch.tensor([sample_uniform(1234, r, 7) for r in range(ROWS)], dtype=F32)
    tok = draw(strided(rows), temperature=TEMPERATURE, top_k=TOP_K, top_p=TOP_P, u=u.to(dev)).tolist()
    assert all(0 <= t < rows.shape[1] for t in tok), "a padding column was drawn"
    # the same rows packed tight (an odd row stride at V = 50257: rows off the 16-B boundary)
    assert draw(rows.to(dev), temperature=TEMPERATURE, top_k=TOP_K, top_p=TOP_P, u=u.to(dev)).tolist() == tok
    n_ambiguous, largest = sc.check_interval_rows(rows, u, tok, TEMPERATURE, TOP_K, TOP_P, what=str(CONFIGS[ci]))
    print(f"config {CONFIGS[ci]}: {n_ambiguous} ambiguous rows, kept sets up to {largest}")
    assert n_ambiguous <= 4


@pytest.mark.parametrize("ci,setting", sc.MATRIX, ids=str)
def test_sampler_random_row_matrix(ci, setting):
    """The exact-draw check over the parameters: each cut alone, top_k on both sides of the
    shortcut's limit and past V, both cuts, a cold and a hot temperature."""
    rows = config_rows(ci)
    temperature, top_k, top_p = setting
    u = torch.tensor([sample_uniform(1234, r, 7) for r in range(ROWS)], dtype=F32)
    kw = dict(temperature=temperature, top_k=top_k, top_p=top_p, u=u.to(dev))
    tok = draw(strided(rows), **kw).tolist()
    assert draw(rows.to(dev), **kw).tolist() == tok
    n_ambiguous, largest = sc.check_interval_rows(rows, u, tok, *setting, what=f"{CONFIGS[ci]} {setting}")
    print(f"config {CONFIGS[ci]} {setting}: {n_ambiguous} ambiguous rows, kept sets up to {largest}")


# ---------------------------------------------------------------- constructed cases: no row excused
def run_case(c, tight):
    rows = c.row.to(dev).expand(len(c.u), c.V)
    logits = rows.contiguous() if tight else strided(rows)
    return draw(logits, temperature=c.temperature, top_k=c.top_k, top_p=c.top_p, u=c.u.to(dev))


def check_cases(cases, what):
    """Every case in a ``vocab_ld`` buffer with +1e4 in the padding and packed tight (rows on and
    off the 16-B boundary): the same tokens, and the f64 oracle's."""
    n_rows = excused = 0
    for c in cases:
        tok = run_case(c, tight=False)
        excused += sc.check_tokens(c, tok)
        assert torch.equal(run_case(c, tight=True), tok), f"{c.name}: the packed rows draw other tokens"
        n_rows += len(tok)
    print(f"{what}: {len(cases)} cases, {n_rows} rows in each layout, {excused} rows excused")
    assert excused == 0


@pytest.mark.parametrize("V", sc.LATTICE_VOCABS)
def test_sampler_lattice_cases(V):
    """Rows of a dozen tied levels: each cut alone and both, top_k just below and just inside every
    level, top_p midway between the cumulative masses, with the threshold key in every position
    of the two histogram passes (tests/sample_cases.py)."""
    check_cases(sc.lattice_cases(V), f"lattice V = {V}")


@pytest.mark.parametrize("V", sc.WALK_VOCABS)
def test_sampler_walk_cases(V):
    """Draws aimed at every edge of the walk (row ends, wave segments, iterations, lanes,
    elements), over a dense and a sparse kept set, and u = 0 / u = 1 over -inf ends."""
    check_cases(sc.walk_cases(V), f"walk V = {V}")


@pytest.mark.parametrize("V", sc.WIDTH_VOCABS)
def test_sampler_width_cases(V):
    check_cases(sc.width_cases(V), f"width V = {V}")


# ---------------------------------------------------------------- invariants, bit for bit
@pytest.mark.parametrize("V", sc.LATTICE_VOCABS)
def test_sampler_top_k_past_the_vocabulary_is_off(V):
    """top_k = 0, V and V + 7 draw the same tokens (the hash path: every row its own uniform)."""
    logits = strided(sc.lattice_row(V).expand(ROWS, V))
    for top_p in (1.0, 0.7):
        toks = [draw(logits, temperature=sc.LATTICE_T, top_k=k, top_p=top_p, seed=21) for k in (0, V, V + 7)]
        assert torch.equal(toks[0], toks[1]) and torch.equal(toks[0], toks[2]), top_p
        assert len(set(toks[0].tolist())) > ROWS // 2  # (the rows draw different uniforms)


@pytest.mark.parametrize("ci", [0, 2])
def test_sampler_top_k_past_the_vocabulary_is_off_random_rows(ci):
    logits = strided(config_rows(ci))
    V = logits.shape[1]
    toks = [draw(logits, temperature=1.5, top_k=k, top_p=0.95, seed=22) for k in (0, V, V + 7)]
    assert torch.equal(toks[0], toks[1]) and torch.equal(toks[0], toks[2])


@pytest.mark.parametrize("V", sc.LATTICE_VOCABS)
def test_sampler_hash_path_is_the_explicit_uniform(V):
    """One case of each instantiation: the hash of (seed, row, counter) on the device draws what
    the host twin's uniform draws when it is passed in."""
    logits = strided(sc.lattice_row(V).expand(ROWS, V))
    seed = (0x1234 << 32) | 77
    kw = dict(temperature=sc.LATTICE_T, top_k=2525, top_p=0.9)
    counters = torch.full((ROWS,), 3, dtype=torch.int64, device=dev)
    by_hash = draw(logits, counters, seed=seed, **kw)
    assert counters.tolist() == [4] * ROWS
    u = torch.tensor([sample_uniform(seed, r, 3) for r in range(ROWS)], dtype=F32, device=dev)
    assert torch.equal(draw(logits, u=u, **kw), by_hash)
    assert len(set(by_hash.tolist())) > ROWS // 2


def test_sampler_distribution_chi2_wide_kernel():
    """8192 hash draws from one V = 8200 vector (sample_kernel<7>) at top_k = 5: Pearson's
    chi-squared against the f64 probabilities below 33.4, the 1 - 1e-6 quantile at 4 degrees of
    freedom.  8200 columns span the segments of waves 0, 1 and 2 only (3584 columns each): the
    five survivors lie in all three, in five different (wave, iteration) registers."""
    V, n = 8200, 8192
    cols = [5, 3000, 4613, 7167, 8199]
    where = [sc.walk_position(c, V)[:2] for c in cols]
    assert where == [(0, 0), (0, 5), (1, 2), (1, 6), (2, 2)]
    vec = torch.tensor([-0.5, -1.0, -3.0, -1.5]).repeat(V // 4).bfloat16()
    vec[cols] = torch.tensor([1.5, 0.0, 2.0, 0.5, 1.0]).bfloat16()
    p = torch.zeros(V, dtype=torch.float64)
    p[cols] = torch.softmax(vec.double()[cols], 0)
    tok = draw(vec.to(dev).repeat(n, 1), temperature=1.0, top_k=5, seed=5)
    counts = torch.bincount(tok, minlength=V).double()
    assert counts[cols].sum() == n == counts.sum()
    chi2 = (((counts - n * p) ** 2)[cols] / (n * p[cols])).sum().item()
    print(f"chi2 = {chi2:.2f}")
    assert chi2 < 33.4


# ---------------------------------------------------------------- refusals
def test_sampler_refuses_bad_shapes():
    """A row past MAX_VOCAB raises in the wrapper; the native entry refuses V = 0, ld < V and a
    sequence buffer without its step counters.  Nothing is written in any of them."""
    assert MAX_VOCAB == sc.MAX_VOCAB
    N = 3
    out = guarded((N, 1), torch.int64, dev, fill=-7)
    counters = guarded(N, torch.int64, dev, fill=0)
    seq = guarded((N, 3), torch.int64, dev, fill=-1)

    def untouched():
        torch.cuda.synchronize()
        assert (out == -7).all() and (counters == 0).all() and (seq == -1).all()
        assert_guards_intact(out, counters, seq)

    wide = torch.zeros(N, MAX_VOCAB + 1, dtype=BF, device=dev)
    with pytest.raises(ValueError, match=f"at most {MAX_VOCAB} columns"):
        sample_logits(wide, temperature=1.0, counters=counters, out_tok=out)
    untouched()
    V = 1000
    logits = strided(config_rows(2)[:N])
    ld = logits.stride(0)

    def native(**over):
        kw = dict(logits=logits.data_ptr(), counters=counters.data_ptr(), u=None, out_tok=out.data_ptr(), done=None,
                  seq=None, step=None, len=None, ld=ld, seq_ld=0, eos=-1, N=N, V=V, top_k=0, temperature=1.0,
                  top_p=1.0, seed_lo=0, seed_hi=0)
        kw.update(over)
        _lib.call("dpc_sample", _lib.SampleArgs(**kw), logits.device)

    for over in (dict(V=0), dict(V=MAX_VOCAB + 1, ld=MAX_VOCAB + 64), dict(ld=V - 1),
                 dict(seq=seq.data_ptr(), seq_ld=3)):
        with pytest.raises(RuntimeError, match="dpc_sample launch failed: hipError 1$"):
            native(**over)
        untouched()
    native()  # the same arguments without the fault are taken
    torch.cuda.synchronize()
    assert (counters == 1).all() and ((out >= 0) & (out < V)).all() and (seq == -1).all()
    assert_guards_intact(out, counters, seq)


@pytest.mark.parametrize("V", [7, 1000, 50257])
def test_sampler_greedy_lowest_index_on_ties(V):
    torch.manual_seed(V)
    x = (torch.randn(5, V) * 2).bfloat16()
    top = x.max() + 1
    x[0, V - 1] = top
    x[1, 0] = x[1, V - 1] = top
    x[2, V // 2] = x[2, V // 2 + 1] = x[2, V - 2] = top
    x[3, 3] = x[3, 5] = top
    want = torch.tensor([V - 1, 0, V // 2, 3, int((x[4] == x[4].max()).nonzero()[0])])
    assert torch.equal(draw(strided(x), temperature=0.0), want)
    # top_k = 1 at u = 0: the first of the ties again
    assert torch.equal(draw(strided(x), temperature=0.8, top_k=1, u=torch.zeros(5, device=dev)), want)


def test_sampler_distribution_chi2():
    """8192 hash draws from one V = 8 vector at top_k = 5: Pearson's chi-squared against the f64
    probabilities below 33.4, the 1 - 1e-6 quantile at 4 degrees of freedom."""
    vec = torch.tensor([2.0, 1.0, 0.5, 0.0, -0.5, -1.0, -3.0, 1.5]).bfloat16()
    kept = [0, 1, 2, 3, 7]
    p = torch.zeros(8, dtype=torch.float64)
    p[kept] = torch.softmax(vec.double()[kept], 0)
    n = 8192
    tok = draw(vec.repeat(n, 1).to(dev), temperature=1.0, top_k=5, seed=3)
    counts = torch.bincount(tok, minlength=8).double()
    assert counts[[4, 5, 6]].sum() == 0 and counts.sum() == n
    chi2 = (((counts - n * p) ** 2)[kept] / (n * p[kept])).sum().item()
    print(f"chi2 = {chi2:.2f}")
    assert chi2 < 33.4


def test_sampler_counters_and_reproducibility():
    logits = strided(config_rows(2))
    kw = dict(temperature=TEMPERATURE, top_k=TOP_K, top_p=TOP_P, seed=9)
    counters = torch.zeros(ROWS, dtype=torch.int64, device=dev)
    a = draw(logits, counters, **kw)
    b = draw(logits, counters, **kw)
    assert counters.tolist() == [2] * ROWS
    assert not torch.equal(a, b)
    counters.zero_()
    assert torch.equal(draw(logits, counters, **kw), a) and torch.equal(draw(logits, counters, **kw), b)
    # the hash is the host twin's: an explicit u from it draws the same tokens
    u = torch.tensor([sample_uniform(9, r, 1) for r in range(ROWS)], dtype=F32, device=dev)
    assert torch.equal(draw(logits, u=u, **{k: v for k, v in kw.items() if k != "seed"}), b)


def test_sampler_done_flags_and_sequence_buffer():
    logits = strided(config_rows(2))
    kw = dict(temperature=TEMPERATURE, top_k=TOP_K, top_p=TOP_P, seed=9)
    free = draw(logits, **kw)
    eos = int(free[5])  # the token row 5 draws: it (and every row that draws the same) must set its flag
    done = torch.zeros(ROWS, dtype=torch.bool, device=dev)
    done[[0, 7]] = True
    seq = guarded((ROWS, 3), torch.int64, dev, fill=-1)
    step = torch.tensor([1] * (ROWS - 1) + [3], dtype=torch.int64, device=dev)  # the last row: past the buffer
    lens = torch.arange(ROWS, dtype=torch.int64, device=dev)
    tok = draw(logits, done=done, eos=eos, seq=seq, step=step, lens=lens, **kw)
    want = free.clone()
    want[[0, 7]] = eos
    assert torch.equal(tok, want)
    assert torch.equal(done.cpu(), want == eos) and done[5]
    assert torch.equal(seq[:-1, 1].cpu(), want[:-1]) and (seq[:, [0, 2]] == -1).all() and seq[-1, 1] == -1
    assert_guards_intact(seq)
    assert step.tolist() == [2] * (ROWS - 1) + [4] and torch.equal(lens.cpu(), torch.arange(ROWS) + 1)


# ---------------------------------------------------------------- ragged decode attention
def _decode_ref(qkv, k0, v0, n, L, H, hd, dt):
    E = H * hd
    q = qkv[n, :E].to(dt).reshape(H, 1, hd)
    k = k0[n, :L].to(dt).reshape(L, H, hd).transpose(0, 1)
    v = v0[n, :L].to(dt).reshape(L, H, hd).transpose(0, 1)
    return (torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), -1) @ v).reshape(H, hd)


@pytest.mark.parametrize("hd", [40, 64, 256])
def test_decode_attention_ragged_edges(hd):
    """Lengths 0, 17 and 299 in one launch over guarded caches: row ``len[n]`` of sequence n
    receives the new key / value and nothing else changes."""
    torch.manual_seed(7)
    N, H, Smax = 3, 3, 300
    E = H * hd
    lens = [0, 17, 299]
    k0 = torch.randn(N, Smax, E, device=dev).bfloat16()
    v0 = torch.randn(N, Smax, E, device=dev).bfloat16()
    kc, vc = guarded((N, Smax, E), BF, dev, fill=k0), guarded((N, Smax, E), BF, dev, fill=v0)
    qkv = torch.randn(N, 3 * E, device=dev).bfloat16()
    length = torch.tensor(lens, device=dev, dtype=torch.int64)
    o = decode_attention(qkv, kc, vc, length, H, hd, per_seq=True)
    for n, pos in enumerate(lens):
        k0[n, pos], v0[n, pos] = qkv[n, E:2 * E], qkv[n, 2 * E:]
    assert torch.equal(kc, k0) and torch.equal(vc, v0)
    assert_guards_intact(kc, vc)
    for n, pos in enumerate(lens):
        ref, ideal = (_decode_ref(qkv, k0, v0, n, pos + 1, H, hd, dt) for dt in (torch.float64, F32))
        assert_local_close(o[n].reshape(H, hd), ref, ideal.bfloat16(), MARGIN_ATTN, axes="rows",
                           what=f"ragged decode o, sequence {n}")

    # one shared length == the same length per sequence, bit for bit
    outs = []
    for per_seq in (False, True):
        ka, va = k0.clone(), v0.clone()
        ln = torch.full((N if per_seq else 1,), 37, device=dev, dtype=torch.int64)
        outs.append((decode_attention(qkv, ka, va, ln, H, hd, per_seq=per_seq), ka, va))
    assert all(torch.equal(a, b) for a, b in zip(*outs))

    # a full cache: nothing is appended and that row's output is zero
    kc2, vc2 = guarded((N, Smax, E), BF, dev, fill=k0), guarded((N, Smax, E), BF, dev, fill=v0)
    full = torch.tensor([5, Smax, Smax + 3], device=dev, dtype=torch.int64)
    o2 = decode_attention(qkv, kc2, vc2, full, H, hd, per_seq=True)
    k1, v1 = k0.clone(), v0.clone()
    k1[0, 5], v1[0, 5] = qkv[0, E:2 * E], qkv[0, 2 * E:]
    assert torch.equal(kc2, k1) and torch.equal(vc2, v1)
    assert_guards_intact(kc2, vc2)
    assert torch.count_nonzero(o2[1:]) == 0 and torch.count_nonzero(o2[0]) > 0


# ---------------------------------------------------------------- end to end
def _model():
    torch.manual_seed(0)
    with torch.device(dev):
        m = TransformerDecoderLM(256, 64, 4, 2, 50257, 128, activation="gelu")
    m.eval()
    return m


def test_ragged_prefill_and_graphed_steps_match_single_sequences():
    """Three right-padded prompts of lengths 5, 20 and 33 share a ragged cache; the logits after
    the prefill and after each of 6 teacher-forced graphed steps are those of each sequence alone."""
    m = _model()
    lens, steps = [5, 20, 33], 6
    g = torch.Generator().manual_seed(1)
    full = [torch.randint(0, 50257, (l + steps,), generator=g).to(dev) for l in lens]
    padded = torch.zeros(3, max(lens), dtype=torch.int64, device=dev)
    for n, l in enumerate(lens):
        padded[n, :l] = full[n][:l]

    def check(lg, t):
        for n, l in enumerate(lens):
            ids = full[n][None, :l + t]
            ref = m(ids, torch.arange(l + t, device=dev)[None])[:, -1:]
            err = ((lg[n:n + 1].float() - ref.float()).norm() / ref.float().norm()).item()
            assert err < 2e-2, (n, t, err)

    with torch.no_grad():
        cache = m.new_kv_cache(3, max(lens) + steps, ragged=True)
        check(m.decode(padded, None, cache, lens=lens), 0)
        dec = m.graph_decoder(cache)
        assert dec is not None
        for t in range(steps):
            tok = torch.stack([full[n][l + t] for n, l in enumerate(lens)]).view(3, 1)
            check(dec.step(tok), t + 1)
        assert cache.lens == [l + steps for l in lens] and cache.len_t.tolist() == cache.lens
        # the longest sequence has filled the cache: a further step is refused and changes nothing
        with pytest.raises(ValueError):
            dec.step(tok)
        assert cache.lens == [l + steps for l in lens] and cache.len_t.tolist() == cache.lens
    assert _lib.is_loaded()


def test_graphed_sampler_steps_read_their_own_draws():
    """A graph that ends in the sampler: the warm-up before the capture leaves no draw behind, and
    the logits of every replay are those of the prompt followed by the tokens the sampler wrote."""
    from distributed_pytorch_cookbook_amd.ops.sample import Sampler

    m = _model()
    lens, steps = [5, 20, 33], 4
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, 50257, (l,), generator=g).to(dev) for l in lens]
    padded = torch.zeros(3, max(lens), dtype=torch.int64, device=dev)
    for n, l in enumerate(lens):
        padded[n, :l] = prompts[n]
    sampler = Sampler(3, 8, dev, temperature=0.8, top_k=40, top_p=0.95, seed=1, eos=-1)
    with torch.no_grad():
        cache = m.new_kv_cache(3, max(lens) + 8, ragged=True)
        logits = m.decode(padded, None, cache, lens=lens)
        sampler(logits[:, 0])
        first = sampler.tok[:, 0].clone()
        dec = m.graph_decoder(cache, sampler)
        assert dec is not None
        outs = []
        for _ in range(steps):
            dec.step()
            outs.append(dec.out.clone())
        assert sampler.counters.tolist() == sampler.step.tolist() == [steps + 1] * 3
        assert torch.equal(sampler.seq[:, 0], first)
        assert cache.len_t.tolist() == cache.lens == [l + steps for l in lens]
        for t, out in enumerate(outs):
            for n, l in enumerate(lens):
                ids = torch.cat([prompts[n], sampler.seq[n, :t + 1]])[None]
                ref = m(ids, torch.arange(l + t + 1, device=dev)[None])[:, -1:]
                err = ((out[n:n + 1].float() - ref.float()).norm() / ref.float().norm()).item()
                assert err < 2e-2, (n, t, err)


class Ids(ByteTokenizer):
    """Decodes to the token ids themselves, so that the texts compared below hide no token."""

    def decode(self, ids, skip_special_tokens=False):
        return " ".join(str(int(i)) for i in ids)


def _new_tokens(text, prompt):
    ids = [int(t) for t in text.split()]
    n = len(prompt.encode())
    assert ids[:n] == ByteTokenizer().encode(prompt)
    return ids[n:]


def test_generate_batch_seeded_text_and_eos_cut():
    m, tok = _model(), Ids()
    prompts = ["The big brown cat ", "One day, ", "She said that nobody would ever "]
    kw = dict(max_new_tokens=12, temperature=0.8, top_k=40, top_p=0.95, seed=1)
    a = generate_batch(m, prompts, tok, torch.device(dev), **kw)
    assert a == generate_batch(m, prompts, tok, torch.device(dev), **kw)
    new = [_new_tokens(t, p) for t, p in zip(a, prompts)]
    assert all(len(x) == 12 and all(0 <= t < 50257 for t in x) for x in new)
    assert a != generate_batch(m, prompts, tok, torch.device(dev), **dict(kw, seed=2))
    # the 4th token of sequence 1 as EOS: that sequence is cut there, the others are unchanged
    # (up to their own first occurrence of it)
    tok.eos_token_id = new[1][3]
    cut = [x[:x.index(tok.eos_token_id)] if tok.eos_token_id in x else x for x in new]
    assert len(cut[1]) <= 3
    b = generate_batch(m, prompts, tok, torch.device(dev), **kw)
    assert [_new_tokens(t, p) for t, p in zip(b, prompts)] == cut
