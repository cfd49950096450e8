"""Cases and checks for the memory-bound kernels (pure host code; shared by test_mem_cases_cpu.py,
test_kernel_edges_gpu.py and test_kernel_trips_gpu.py).

* trip geometry: the sizes at which the flat kernels and the LayerNorm backward take a second
  loop trip, stated once with the source line they come from;
* ``run_layout``: token / position ids whose sorted runs meet every chunk phase and piece length
  of the sorted embedding backward, with the host description of the sorted layout;
* ``scaler_script``: a found-inf pattern and the loss scaler's state after every step, from a
  plain transcription of torch's GradScaler rule;
* the assertions the GPU tests make on the embedding tables, the scaler state and the
  cross-entropy rows, written for any device so that the CPU test can run them on the ops' own
  CPU paths."""
from __future__ import annotations

import struct

import torch

from kernel_checks import MARGIN, assert_local_close

# ---------------------------------------------------------------- trip geometry
FLAT_MAX_BLOCKS = 8192   # csrc/misc.hip: grid_for() caps the grid of adamw / cast / dropout_residual / amp_check
FLAT_BLOCK = 256         # threads per block of those kernels, one 16-B vector (4 f32) per thread per trip
flat_trip_elems = FLAT_MAX_BLOCKS * FLAT_BLOCK * 4   # elements one trip of the capped grid covers
LN_BWD_MIN_BLOCKS = 256  # csrc/layernorm.hip: dpc_layernorm_bwd clamps the grid up to 256 workgroups
ln_bwd_sweep_rows = LN_BWD_MIN_BLOCKS * 4            # rows one trip of that grid covers (4 waves, a row each)
EB_CH = 8                # csrc/embed_bwd.hip: EB_CH, sorted positions per chunk


def flat_trips(n_vec, vecs_per_trip=1):
    """Loop trips of the busiest thread of a grid_for() launch over ``n_vec`` 16-B vectors."""
    blocks = min(max((n_vec + FLAT_BLOCK - 1) // FLAT_BLOCK, 1), FLAT_MAX_BLOCKS)
    per_trip = blocks * FLAT_BLOCK * vecs_per_trip
    return (n_vec + per_trip - 1) // per_trip


def ln_bwd_rows_per_wave(T, blocks=LN_BWD_MIN_BLOCKS):
    """(fewest, most) rows a wave of the persistent LayerNorm backward does (waves with none left out)."""
    waves = min(blocks, (T + 3) // 4) * 4
    most = (T + waves - 1) // waves
    fewest = T // waves if T >= waves else 1
    return fewest, most


# ---------------------------------------------------------------- sorted embedding backward
RUN_LENGTHS = list(range(1, 21)) + [33, 64, 65]  # 372 rows
RUN_TAIL = [4]                                   # variant 1: 376 rows = 47 chunks; the last run fits and ends at T
BAD_IDS = (lambda V: V + 3, lambda V: -1, lambda V: 2 ** 40)
BAD_FROM = (2, 3, 65)                            # the runs (by length) that lose a row to a bad id


def sorted_layout(ids, n_keys):
    """What the stable sort of csrc/embed_bwd.hip makes of ``ids``: out-of-range ids get key
    ``n_keys`` and sort last.  Returns (sorted keys, sorted rows, runs) with runs the
    (key, start, length) of every run of a valid key, in sorted order."""
    ids = ids.reshape(-1).to(torch.int64)
    valid = (ids >= 0) & (ids < n_keys)
    key = torch.where(valid, ids, torch.full_like(ids, n_keys))
    skeys, rows = torch.sort(key, stable=True)
    runs = []
    ks = skeys.tolist()
    i = 0
    while i < len(ks) and ks[i] < n_keys:
        j = i
        while j < len(ks) and ks[j] == ks[i]:
            j += 1
        runs.append((ks[i], i, j - i))
        i = j
    return skeys, rows, runs


def run_pieces(start, length):
    """The lengths of the pieces a run is cut into at every EB_CH-th sorted position."""
    out, i, end = [], start, start + length
    while i < end:
        cut = min(end, (i // EB_CH + 1) * EB_CH)
        out.append(cut - i)
        i = cut
    return out


def layout_conditions(runs):
    """What the runs of a sorted layout exercise in eb_segsum_kernel / eb_runsum_kernel."""
    c = dict(phases=set(), pieces=set(), fits=0, fits_to_chunk_end=0, crosses_one=0, crosses_three=0,
             starts_on_chunk_and_crosses=0, starts_in_last_slot_and_crosses=0, crosses_to_chunk_end=0,
             one_row_into_next_chunk=0)
    for _, start, length in runs:
        end = start + length
        crossed = (end - 1) // EB_CH - start // EB_CH
        c["phases"].add(start % EB_CH)
        c["pieces"].update(run_pieces(start, length))
        c["fits"] += crossed == 0
        c["fits_to_chunk_end"] += crossed == 0 and end % EB_CH == 0
        c["crosses_one"] += crossed == 1
        c["crosses_three"] += crossed >= 3
        c["starts_on_chunk_and_crosses"] += crossed > 0 and start % EB_CH == 0
        c["starts_in_last_slot_and_crosses"] += crossed > 0 and start % EB_CH == EB_CH - 1
        c["crosses_to_chunk_end"] += crossed > 0 and end % EB_CH == 0
        c["one_row_into_next_chunk"] += crossed > 0 and end % EB_CH == 1
    return c


def assert_layout_complete(runs, what=""):
    c = layout_conditions(runs)
    assert c["phases"] == set(range(EB_CH)), (what, "start phases", sorted(c["phases"]))
    assert c["pieces"] == set(range(1, EB_CH + 1)), (what, "piece lengths", sorted(c["pieces"]))
    for k, v in c.items():
        if not isinstance(v, set):
            assert v > 0, (what, k)
    return c


def run_layout(variant):
    """Ids for the sorted embedding backward whose runs have the lengths RUN_LENGTHS (variant 0,
    T = 372) or RUN_LENGTHS + RUN_TAIL (variant 1, T = 376 = 47 chunks, the last run ending on
    the last chunk's end).  Keys rise with the list and leave gaps (3 k + 1: two of every three
    table rows are named by no token); rows are dealt to the keys through a fixed permutation.

    ``pos`` is that layout as it stands (another permutation); ``ids`` is the same with three
    rows overwritten by out-of-range values (V + 3, -1, 2^40), which sort behind every valid key:
    one row each is taken from the runs of BAD_FROM, which shifts every later run by up to three
    positions and still leaves a layout that meets every condition of ``layout_conditions`` in
    both variants (of the 1,540 choices of three runs, 53 do).  Both layouts are described
    (``tok_runs``, ``pos_runs``) and test_mem_cases_cpu.py asserts what they exercise."""
    lengths = RUN_LENGTHS + (RUN_TAIL if variant else [])
    keys = [3 * k + 1 for k in range(len(lengths))]
    V = P = 3 * len(lengths)
    T = sum(lengths)
    by_sorted_pos = torch.repeat_interleave(torch.tensor(keys, dtype=torch.int64), torch.tensor(lengths))

    def deal(seed):
        perm = torch.randperm(T, generator=torch.Generator().manual_seed(seed))
        out = torch.empty(T, dtype=torch.int64)
        out[perm] = by_sorted_pos
        return out

    ids, pos = deal(101 + variant), deal(202 + variant)
    bad_rows = []
    for length, bad in zip(BAD_FROM, BAD_IDS):
        key = keys[lengths.index(length)]
        row = int((ids == key).nonzero()[1])  # the run's second row
        ids[row] = bad(V)
        bad_rows.append(row)
    _, tok_rows, tok_runs = sorted_layout(ids, V)
    _, pos_rows, pos_runs = sorted_layout(pos, P)
    return dict(T=T, V=V, P=P, ids=ids, pos=pos, bad_rows=bad_rows, lengths=lengths, keys=keys,
                tok_runs=tok_runs, tok_rows=tok_rows, pos_runs=pos_runs, pos_rows=pos_rows)


def embedding_refs(base, dout, idx, n_keys):
    """(f64 reference, plain f32 ideal, rows named by a valid index) of table ``base`` after
    ``base[idx] += dout`` over the rows whose own index is in range."""
    idx = idx.reshape(-1)
    ok = (idx >= 0) & (idx < n_keys)
    ref64 = base.double().index_add_(0, idx[ok], dout[ok].double())
    ideal = base.clone().index_add_(0, idx[ok], dout[ok])
    named = torch.zeros(n_keys, dtype=torch.bool, device=base.device)
    named[idx[ok]] = True
    return ref64, ideal, named


def check_embedding_table(table, base, dout, idx, what, family="embedding bwd"):
    """One gradient table after embedding_bwd: rows no valid index names are bit-unchanged, the
    others within MARGIN x the f32 index_add's own error against the f64 one, per row."""
    ref64, ideal, named = embedding_refs(base, dout, idx, base.shape[0])
    assert torch.equal(table[~named].view(torch.int32), base[~named].view(torch.int32)), f"{what}: an unnamed row changed"
    assert_local_close(table[named], ref64[named], ideal[named], MARGIN, axes="rows", what=what, family=family)


# ---------------------------------------------------------------- loss scaling
def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


SCALER_PATTERN = [0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0]
SCALER_INTERVAL = 3
SCALER_INIT = 2.0 ** 16


def scaler_script(growth=2.0, backoff=0.5, pattern=SCALER_PATTERN, interval=SCALER_INTERVAL, init=SCALER_INIT):
    """(pattern, interval, init, states): ``states[i]`` = (scale, 1 / scale, tracker) after the
    update of step i, whose found-inf flag is ``pattern[i]``.  torch's GradScaler rule
    (_amp_update_scale_): on overflow scale *= backoff and the tracker returns to 0; otherwise the
    tracker counts, and when it reaches the interval scale *= growth and the tracker returns to 0.
    The scale is an f32 (the factors too: each product is rounded once); 1 / scale is the f64
    reciprocal of that f32."""
    scale, tracker, states = _f32(init), 0, []
    g, b = _f32(growth), _f32(backoff)
    for found in pattern:
        if found:
            scale, tracker = _f32(scale * b), 0
        else:
            tracker += 1
            if tracker >= interval:
                scale, tracker = _f32(scale * g), 0
        states.append((scale, 1.0 / scale, tracker))
    return list(pattern), interval, init, states


def check_scaler_state(scaler, state, exact_inv, what=""):
    """The scaler's tensors after an update against one state of the script: scale and tracker
    exactly, found_inf consumed; inv_scale bit-equal to the f32 reciprocal (``exact_inv``: powers
    of two) or within 2^-22 relative of the f64 reciprocal (1 ulp of the device's f32 reciprocal,
    doubled)."""
    scale, inv, tracker = state
    assert float(scaler.scale_t) == scale, (what, "scale", float(scaler.scale_t), scale)
    assert float(scaler.tracker) == tracker, (what, "tracker", float(scaler.tracker), tracker)
    assert float(scaler.found_inf) == 0.0, (what, "found_inf not cleared")
    got = float(scaler.inv_scale_t)
    if exact_inv:
        assert got == _f32(inv), (what, "inv_scale", got, inv)
    else:
        assert abs(got - inv) <= 2.0 ** -22 * inv, (what, "inv_scale", got, inv)


AMP_SMALL = [1, 3, 4, 5, 1023, 1027]
AMP_LARGE = 4 * (FLAT_MAX_BLOCKS * FLAT_BLOCK + 300) + 3  # 300 threads take a second trip; a tail of 3
AMP_BAD = [float("inf"), float("-inf"), float("nan")]
# finite values a check must let through: the largest magnitudes, subnormals, both zeros
AMP_CLEAN = [3.4028235e38, -3.4028235e38, 1e-45, -1e-40, -0.0, 0.0]


def amp_positions(n):
    """Where the one non-finite element is planted: the first element, the last (in the scalar
    tail when n & 3), both ends of the last full vector, the middle, and for a buffer past one
    trip of the capped grid an element that only the second trip reads."""
    pos = {0, n - 1, n // 2}
    if n >= 4:
        pos.update({(n // 4) * 4 - 1, (n // 4) * 4 - 4})
    if n > flat_trip_elems:
        pos.add(flat_trip_elems + 4 * 7 + 2)
    return sorted(pos)


def amp_clean_fill(g):
    """Fills ``g`` with AMP_CLEAN, repeated."""
    n = g.numel()
    pat = torch.tensor(AMP_CLEAN, dtype=torch.float32, device=g.device)
    g.copy_(pat.repeat((n + len(AMP_CLEAN) - 1) // len(AMP_CLEAN))[:n])


def check_amp_matrix(scaler, g):
    """GradScaler.check over the flat f32 buffer ``g`` (holding clean values): the flag stays 0 on
    the clean buffer, becomes 1 for every planted value at every position of ``amp_positions``
    (the element is restored after each), and a flag already 1 stays 1 after a clean buffer.
    Returns the number of checks made."""
    n = g.numel()
    flag = scaler.found_inf
    flag.zero_()
    scaler.check(g)
    assert float(flag) == 0.0, f"n {n}: flag raised on a clean buffer"
    checks = 1
    for p in amp_positions(n):
        old = g[p].clone()
        for v in AMP_BAD:
            g[p] = v
            flag.zero_()
            scaler.check(g)
            assert float(flag) == 1.0, f"n {n}: {v} at {p} not seen"
            checks += 1
        g[p] = old
    flag.zero_()
    scaler.check(g)
    assert float(flag) == 0.0, f"n {n}: flag raised after the buffer was restored"
    flag.fill_(1.0)
    scaler.check(g)
    assert float(flag) == 1.0, f"n {n}: a clean buffer cleared a raised flag"
    flag.zero_()
    return checks + 2


# ---------------------------------------------------------------- cross-entropy rows
def first_argmax(vals):
    """The lowest index among each row's maxima (bf16 logits over tens of thousands of columns tie
    at the maximum; torch.argmax does not say which of them it returns)."""
    V = vals.shape[1]
    cols = torch.arange(V, device=vals.device)
    top = vals.amax(-1, keepdim=True)
    return torch.where(vals == top, cols, torch.full_like(cols, V)).amin(-1)


def cross_entropy_refs(vals, tg, inv, dtype):
    """(row loss, gradient rows) of mean cross-entropy over the valid rows in ``dtype``; a target
    of -100 marks an ignored row."""
    valid = tg != -100
    safe = torch.where(valid, tg, torch.zeros_like(tg))
    rows = torch.arange(vals.shape[0], device=vals.device)
    lsm = torch.log_softmax(vals.to(dtype), -1)
    loss = torch.where(valid, -lsm[rows, safe], torch.zeros_like(lsm[:, 0]))
    p = torch.exp(lsm)
    p[rows, safe] -= 1.0
    return loss, p * (valid.to(dtype) * inv.to(dtype))[:, None]


def check_cross_entropy(row_loss, grad, pad_cols, row_correct, vals, tg, inv):
    """Per-row loss and gradient rows against f64 within MARGIN x the plain f32 floor, ignored
    rows and padded columns exactly zero, and the argmax hit against the first maximum."""
    valid = tg != -100
    loss64, grad64 = cross_entropy_refs(vals, tg, inv, torch.float64)
    loss32, grad32 = cross_entropy_refs(vals, tg, inv, torch.float32)
    # The row loss is one f32 per row, and one plain f32 evaluation of it is one sample: at T = 1
    # the floor is a single element, and at V = 4104 it lands 2.8e-8 from the f64 value in either
    # column order (about a quarter of an ulp) where the kernel returns the next float, 8.6e-8
    # away.  So the ideal is, per row, the further of two summation orders (columns first to
    # last, last to first) and never closer than 2^-24 |loss| -- the half ulp of
    # assert_elem_close(ulp_floor=True): no f32 output can be held below its own rounding.
    flipped = torch.where(valid, vals.shape[1] - 1 - tg, tg)
    loss32r = cross_entropy_refs(vals.flip(1), flipped, inv, torch.float32)[0]
    worse = (loss32r.double() - loss64).abs() > (loss32.double() - loss64).abs()
    loss32 = torch.where(worse, loss32r, loss32).double()
    half_ulp = loss64.abs() * 2.0 ** -24
    loss32 = torch.where((loss32 - loss64).abs() < half_ulp, loss64 + half_ulp, loss32)
    assert_local_close(row_loss, loss64, loss32, MARGIN, axes="cols", what="row loss", family="cross-entropy loss")
    assert_local_close(grad, grad64, grad32.to(grad.dtype), MARGIN, axes="rows", what="dlogits",
                       family="cross-entropy grad")
    assert torch.count_nonzero(grad[~valid]) == 0      # ignored rows: exactly zero
    assert torch.count_nonzero(pad_cols) == 0          # padded columns: exactly zero
    hit = ((first_argmax(vals) == tg) & valid).float()
    assert torch.equal(row_correct, hit), (row_correct - hit).nonzero().flatten().tolist()
