"""Cases and checks for the sampler (pure host code; shared by test_sample_cases_cpu.py and
test_sampling_gpu.py).

* ``oracle_row``: the definition of ``ops/sample.py`` in f64 for one row, with the bands inside
  which a kernel that sums in another precision may differ (1e-4 of mass at the top-p cut,
  1e-5 Z at the draw);
* ``key_of``: the Python twin of ``csrc/sample.hip:key_of`` (bf16 payload -> 16-bit ordered key), by
  which the cases say in which (high byte, low byte) bin of the two histogram passes a cut lands;
* constructed cases -- lattice, walk and width rows -- whose right token is not in doubt: every
  row of a case is the same vector, drawn at chosen uniforms, and the test demands the oracle's
  token and excuses no row.  ``check_preconditions`` states why the answer is not in doubt;
* the random-row matrix: the ``randn`` rows and the parameter settings at which the oracle itself
  finds at most MAX_AMBIGUOUS rows of 64 inside its bands;
* the assertions the GPU tests make, written for token lists so that the CPU test can run them
  on the twin and on small mutations of a right answer."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field

import torch

BF = torch.bfloat16
NEG_INF = float("-inf")

# ---------------------------------------------------------------- the kernel's geometry
# (csrc/sample.hip; test_sample_cases_cpu.py reads these out of its text)
SM_NT = 1024            # threads per row; also the largest top_k that takes the thread-maxima shortcut
SM_NW = SM_NT // 64     # waves, each owning one segment of the row
SPLIT_V = SM_NW * 512   # 8192: sample_kernel<1> up to here, sample_kernel<7> beyond
MAX_ITERS = 7
MAX_VOCAB = SM_NW * 512 * MAX_ITERS  # 57344

P_BAND = 1e-4           # of mass, at the top-p cut
U_BAND = 1e-5           # of Z, at the draw
MAX_AMBIGUOUS = 4       # rows of 64 a random-row test may excuse


def iters_for(V):
    return 1 if V <= SPLIT_V else MAX_ITERS


def walk_position(col, V):
    """(wave, iteration, lane, element) of the register that holds ``col`` in the kernel that
    serves a row of V columns: column = wave * SEG + iteration * 512 + lane * 8 + element."""
    seg = 512 * iters_for(V)
    r = col % seg
    return col // seg, r // 512, (r % 512) // 8, r % 8


# ---------------------------------------------------------------- keys
def bf16_bits(x):
    """The 16-bit payload of the bf16 nearest to ``x`` (which must be that bf16)."""
    t = torch.tensor(float(x)).to(BF)
    assert float(t) == float(x) or (math.isinf(x) and math.isinf(float(t))), f"{x} is no bf16"
    return int(t.view(torch.int16)) & 0xFFFF


def key_of(b):
    """csrc/sample.hip:key_of -- payload -> key with the order of the values; -0 is +0."""
    if b == 0x8000:
        b = 0
    return (~b & 0xFFFF) if b & 0x8000 else (b | 0x8000)


def bits_to_bf16(bits):
    """A bf16 tensor with the given payloads (a list of ints): -0.0 survives."""
    t = torch.tensor([b - 65536 if b >= 32768 else b for b in bits], dtype=torch.int16)
    return t.view(BF)


# ---------------------------------------------------------------- the f64 oracle
def oracle_row(row, temperature, top_k, top_p):
    """The definition in f64 for one row: (kept, w, ambiguous) -- the kept mask, exp(z - max), and
    the top-k survivors below the maximum whose strictly-greater mass lies within P_BAND of top_p.
    ``top_k <= 0`` or ``>= V`` and ``top_p >= 1`` turn a cut off, as in the kernel and the twin."""
    z = row.double() / temperature
    V = z.numel()
    vals, inv, counts = torch.unique(z, return_inverse=True, return_counts=True)  # ascending
    count_gt = counts.sum() - torch.cumsum(counts, 0)
    keep_k = count_gt[inv] < top_k if 0 < top_k < V else torch.ones_like(z, dtype=torch.bool)
    w = torch.exp(z - z.max())
    if top_p >= 1.0:
        return keep_k, w, torch.zeros_like(keep_k)
    mass = torch.zeros_like(vals).index_add_(0, inv, w * keep_k)
    q_gt = ((mass.sum() - torch.cumsum(mass, 0)) / mass.sum())[inv]
    top = z == z.max()  # always stays; at top_p = 0 its strictly-greater mass is 0 = top_p
    kept = keep_k & ((q_gt < top_p) | top)
    ambiguous = keep_k & ~top & ((q_gt - top_p).abs() <= P_BAND)
    return kept, w, ambiguous


def oracle_tokens(kept, w, u):
    """The draw in f64: the first kept index whose inclusive prefix exceeds u Z; where none does
    (u = 1), the last kept index of positive weight."""
    wk = w * kept
    cum = torch.cumsum(wk, 0)
    idx = torch.searchsorted(cum, u.double() * cum[-1], right=True)
    last = int((wk > 0).nonzero()[-1])
    return torch.where(idx < cum.numel(), idx, torch.full_like(idx, last))


# ---------------------------------------------------------------- constructed cases
@dataclass
class Case:
    """One launch: ``row`` [V] bf16 repeated ``len(u)`` times, drawn at ``u``; ``want`` the tokens.
    ``kind``: 'mid' (u at the middle of the target's interval, U_BAND inside it), 'equal' (every
    kept weight is exactly 1, u at the middle of the target's slot), 'end' (u = 0 or 1 over -inf
    ends), 'sole' (one column of positive weight), 'greedy'."""
    name: str
    row: torch.Tensor
    temperature: float
    top_k: int
    top_p: float
    u: torch.Tensor
    want: torch.Tensor
    kind: str
    tags: set = field(default_factory=set)

    @property
    def V(self):
        return self.row.numel()

    def rows(self):
        return self.row.expand(len(self.u), self.V)

    @functools.cached_property
    def oracle(self):
        if self.temperature <= 0:
            top = self.row == self.row.max()
            return top, top.double(), torch.zeros_like(top)
        return oracle_row(self.row, self.temperature, self.top_k, self.top_p)

    def __repr__(self):
        return self.name


def _f32(x):
    return torch.as_tensor(x, dtype=torch.float64).float()


def _mid_case(name, row, temperature, top_k, top_p, pick, tags=()):
    """A 'mid' case: ``pick(kept, w)`` names the target columns; those whose interval is too
    narrow for U_BAND (twice over) are left out."""
    c = Case(name, row, temperature, top_k, top_p, None, None, "mid", set(tags))
    kept, w, _ = c.oracle
    wk = w * kept
    cum = torch.cumsum(wk, 0)
    Z = cum[-1]
    targets = [t for t in dict.fromkeys(pick(kept, w)) if kept[t] and wk[t] >= 4 * U_BAND * Z]
    assert targets, name
    t = torch.tensor(targets)
    c.u = _f32((cum[t] - wk[t] / 2) / Z)
    c.want = t
    return c


def check_preconditions(c):
    """Why the token of a constructed case is not in doubt."""
    kept, w, amb = c.oracle
    assert not amb.any(), (c.name, "a candidate within P_BAND of top_p")
    assert c.u.dtype == torch.float32 and c.want.dtype == torch.int64 and len(c.u) == len(c.want) > 0
    assert not torch.isnan(c.row.float()).any() and not torch.isposinf(c.row.float()).any()
    wk = w * kept
    cum = torch.cumsum(wk, 0)
    Z = cum[-1].item()
    pos = (wk > 0).nonzero().flatten()
    if c.kind == "mid":
        x = c.u.double() * Z
        lo, hi = cum[c.want] - wk[c.want], cum[c.want]
        assert ((x - lo >= U_BAND * Z) & (hi - x >= U_BAND * Z)).all(), (c.name, "u within U_BAND of an end")
    elif c.kind == "equal":
        assert torch.equal(wk[kept], torch.ones(int(kept.sum()), dtype=torch.float64)), c.name
        slot = c.u.double() * Z  # = u n: the weights are exactly 2^40 in the kernel too
        rank = torch.cumsum(kept, 0)[c.want] - 1
        assert ((slot - rank - 0.5).abs() < 0.25).all(), c.name
    elif c.kind == "end":
        assert c.u.tolist() == [0.0, 1.0] and c.want.tolist() == [int(pos[0]), int(pos[-1])]
        assert kept[0] and kept[-1] and pos[0] > 0 and pos[-1] < c.V - 1, (c.name, "no -inf end")
    elif c.kind == "sole":
        assert pos.tolist() == [c.V - 1] and set(c.want.tolist()) == {c.V - 1}
    elif c.kind == "greedy":
        assert c.temperature == 0.0 and int(kept.sum()) == 1 and c.want.tolist() == [c.V - 1] and kept[-1]
    else:
        raise AssertionError(c.kind)
    if c.kind != "greedy":
        assert torch.equal(oracle_tokens(kept, w, c.u), c.want), c.name


def check_tokens(c, tok):
    """The assertion of the GPU tests on a constructed case: the oracle's token in every row."""
    tok = [int(t) for t in tok]
    kept, w, _ = c.oracle
    assert len(tok) == len(c.want), (c.name, len(tok))
    for r, (t, want) in enumerate(zip(tok, c.want.tolist())):
        assert 0 <= t < c.V, f"{c.name} row {r}: column {t} drawn, past the {c.V} of the row (padding)"
        if c.kind == "greedy":
            assert kept[t], f"{c.name}: greedy took column {t}, which is no maximum"
            assert t == want, f"{c.name}: greedy took the maximum at {t}, the first is at {want}"
            continue
        assert kept[t], f"{c.name} row {r}: column {t} drawn, which the cuts drop (want {want})"
        assert w[t] > 0, f"{c.name} row {r}: column {t} of weight 0 (-inf) drawn (want {want})"
        assert t == want, f"{c.name} row {r}: column {t} drawn at u = {float(c.u[r])!r}, want {want}"
    return 0  # rows excused


# ---- lattice rows
# (value, columns): a dozen bf16-exact levels; the rest of the row is -inf.  Keys: 7.5 0xc0f0,
# 6.0 0xc0c0, 2.0 0xc000, 1.9921875 0xbfff, 1.0 0xbf80, 0.5 0xbf00, +-0 0x8000, -1.0 0x407f,
# -2.5 0x3fdf, -inf 0x007f.  1024 columns lie above the 0.5 level.
LATTICE = [(7.5, 3), (6.0, 20), (2.0, 100), (1.9921875, 300), (1.0, 601), (0.5, 1500), (0.0, 1000), (-1.0, 1500),
           (-2.5, 2000)]
LATTICE_FINITE = sum(n for _, n in LATTICE)  # 7024
LATTICE_VOCABS = (SPLIT_V, 50257)            # sample_kernel<1>, sample_kernel<7>
LATTICE_T = 4.0                              # every finite level keeps >= 8e-5 of Z per column
PLACEMENTS = ("same_hi", "lower_hi", "lo00", "loff", "negative", "zero", "neg_inf")
K_REGIMES = ("k<=1024", "k==1024", "k==1025", "k>1024", "k>=V")


def lattice_levels(V):
    return LATTICE + [(NEG_INF, V - LATTICE_FINITE)]


@functools.lru_cache(maxsize=None)
def lattice_row(V):
    """The levels of LATTICE and V - 7024 columns of -inf, dealt over the row by a fixed
    permutation.  Every other column of the zero level holds -0.0."""
    bits = []
    for v, n in lattice_levels(V):
        b = bf16_bits(v)
        bits += [b if v != 0.0 or i % 2 == 0 else 0x8000 for i in range(n)]
    perm = torch.randperm(V, generator=torch.Generator().manual_seed(V))
    row = torch.empty(V, dtype=BF)
    row[perm] = bits_to_bf16(bits)
    return row


def placement_of(thr_value, max_value):
    """Where the key of the lowest kept value lies in the two histogram passes."""
    k, kmax = key_of(bf16_bits(thr_value)), key_of(bf16_bits(max_value))
    tags = {"same_hi" if k >> 8 == kmax >> 8 else "lower_hi"}
    if k & 0xFF == 0x00:
        tags.add("lo00")
    if k & 0xFF == 0xFF:
        tags.add("loff")
    if thr_value == 0.0:
        tags.add("zero")
    elif math.isinf(thr_value):
        tags.add("neg_inf")
        assert k >> 8 == 0  # bin 0: lane 0 of hist_search
    elif thr_value < 0:
        tags.add("negative")
        assert k < 0x8000
    return tags


def _level_ends(row, value):
    idx = (row.float() == value).nonzero().flatten()
    return [int(idx[0]), int(idx[-1])]


def _lattice_case(name, V, temperature, top_k, top_p, tags=()):
    row = lattice_row(V)

    def pick(kept, w):
        kv = row.float()[kept]
        finite = kv[torch.isfinite(kv)]
        ends = kept.nonzero().flatten()
        return (_level_ends(row, float(kv.max())) + _level_ends(row, float(kv.min()))
                + _level_ends(row, float(finite.min())) + [int(ends[0]), int(ends[-1])])

    c = _mid_case(name, row, temperature, top_k, top_p, pick, tags)
    kept, w, _ = c.oracle
    keep_k = oracle_row(row, temperature, top_k, 1.0)[0]
    thr = float(row.float()[kept].min())
    # (a top_k past the finite columns keeps everything and still puts the threshold key at -inf)
    cut = "k" if 0 < top_k < V and torch.equal(kept, keep_k) else "" if torch.equal(kept, keep_k) else "p"
    if cut:
        c.tags |= placement_of(thr, float(row.float().max())) | {"cut_" + cut}
        if any(float(row[t]) == thr for t in c.want.tolist()):
            c.tags.add("thr_target")  # a target inside the lowest kept level: dropping its ties shows
    if top_k > 0:
        c.tags.add("k>=V" if top_k >= V else "k<=1024" if top_k <= SM_NT else "k>1024")
        if top_k in (SM_NT, SM_NT + 1):
            c.tags.add(f"k=={top_k}")
    return c


@functools.lru_cache(maxsize=None)
def lattice_cases(V):
    levels = lattice_levels(V)
    above = [sum(n for _, n in levels[:i]) for i in range(len(levels))]  # count_gt of each level
    T = LATTICE_T
    out = []
    # top-k alone: just below and just inside every level (the whole level stays)
    for i in range(1, len(levels)):
        out.append(_lattice_case(f"V{V}-k{above[i]}-below", V, T, above[i], 1.0, {"below"}))
        out.append(_lattice_case(f"V{V}-k{above[i] + 1}-inside", V, T, above[i] + 1, 1.0, {"inside"}))
    for k in (0, V, V + 7):
        out.append(_lattice_case(f"V{V}-k{k}-off", V, T, k, 1.0))
    # top-p alone: midway between consecutive cumulative masses, and 0

    def cum_mass(temperature, n_levels):
        m = [n * math.exp((v - levels[0][0]) / temperature) for v, n in levels[:n_levels]]
        return [sum(m[:i]) / sum(m) for i in range(n_levels + 1)]

    q = cum_mass(T, len(LATTICE))
    out.append(_lattice_case(f"V{V}-p0", V, T, 0, 0.0))
    for i in range(len(LATTICE)):
        out.append(_lattice_case(f"V{V}-p-level{i}", V, T, 0, (q[i] + q[i + 1]) / 2))
    # both: top-p over the survivors of top-k (through the zero level: 2524 columns), at each
    # level of theirs; and a top-k that is the tighter cut
    q = cum_mass(T, 7)
    for i in (0, 3, 5, 6):
        out.append(_lattice_case(f"V{V}-k2525-p-level{i}", V, T, 2525, (q[i] + q[i + 1]) / 2))
    out.append(_lattice_case(f"V{V}-k124-p0.99", V, T, 124, 0.99))
    # the regimes in which random rows are too often ambiguous, and the ends of the temperature:
    # at T = 0.05 every weight below the maximum is under the kernel's 2^-40, at T = 100 the
    # finite levels are nearly uniform
    for temperature, k, p in ((0.8, 2000, 0.95), (1.0, 0, 0.999), (5.0, 0, 0.999), (5.0, 0, 0.5), (100.0, 0, 0.999),
                              (100.0, 0, 0.5), (100.0, 2000, 0.5), (100.0, 0, 1.0), (0.05, 50, 0.9), (0.05, 50, 1.0),
                              (0.05, 0, 1.0)):
        out.append(_lattice_case(f"V{V}-T{temperature}-k{k}-p{p}", V, temperature, k, p, {"regime"}))
    return out


# ---- walk rows
WALK_VOCABS = (SPLIT_V, 50257, MAX_VOCAB)
SPARSE_STRIDE = 513


def walk_targets(V):
    """Columns at every edge of the kernel's walk: the row's ends, both ends of every wave's
    segment, of every iteration inside wave 3, and lanes 0 / 31 / 63 x elements 0 / 3 / 7 of one
    iteration of wave 5."""
    iters = iters_for(V)
    seg = 512 * iters
    t = {0, V - 1}
    for wv in range(SM_NW):
        if wv * seg < V:
            t |= {wv * seg, min((wv + 1) * seg, V) - 1}
    for it in range(iters):
        t |= {3 * seg + it * 512, 3 * seg + it * 512 + 511}
    base = 5 * seg + min(2, iters - 1) * 512
    t |= {base + lane * 8 + e for lane in (0, 31, 63) for e in (0, 3, 7)}
    assert max(t) < V
    return sorted(t)


@functools.lru_cache(maxsize=None)
def walk_cases(V):
    ones = torch.ones(V, dtype=BF)
    t = torch.tensor(walk_targets(V))
    dense = Case(f"V{V}-walk-dense", ones, 1.0, 0, 1.0, _f32((t.double() + 0.5) / V), t, "equal")
    # every 513th column one level up, top_k = 1: the tie is wider than k, and the walk steps
    # over 512 dropped columns between two kept ones
    row = ones.clone()
    cols = torch.arange(0, V, SPARSE_STRIDE)
    row[cols] = 2.0
    n = len(cols)
    sparse = Case(f"V{V}-walk-sparse", row, 1.0, 1, 1.0, _f32((torch.arange(n).double() + 0.5) / n), cols, "equal",
                  {"sparse"})
    # u = 0 and u = 1 over -inf ends: the first and the last column of positive weight
    row = ones.clone()
    row[:3] = NEG_INF
    row[-5:] = NEG_INF
    ends = Case(f"V{V}-walk-ends", row, 1.0, 0, 1.0, torch.tensor([0.0, 1.0]), torch.tensor([3, V - 6]), "end")
    # the same on a lattice row whose -inf columns top-k keeps (a sparse kept set of unequal weights)
    out = [dense, sparse, ends]
    if V in LATTICE_VOCABS:
        row = lattice_row(V).clone()
        row[:3] = NEG_INF
        row[-5:] = NEG_INF
        finite = torch.isfinite(row.float()).nonzero().flatten()
        out.append(Case(f"V{V}-lattice-ends", row, LATTICE_T, int(len(finite)) + 1, 1.0, torch.tensor([0.0, 1.0]),
                        torch.tensor([int(finite[0]), int(finite[-1])]), "end"))
    return out


# ---- width rows
WIDTH_VOCABS = (1, 7, 8, 9, 511, 512, 513, SPLIT_V - 1, SPLIT_V, SPLIT_V + 1, MAX_VOCAB - 1, MAX_VOCAB)


@functools.lru_cache(maxsize=None)
def width_cases(V):
    sole = torch.full((V,), NEG_INF, dtype=BF)
    sole[V - 1] = 1.5
    u = torch.tensor([0.0, 0.37, 1.0])
    out = [Case(f"V{V}-width-sole", sole, 0.7, 0, 1.0, u, torch.full((3,), V - 1), "sole")]
    g = (torch.randn(V, generator=torch.Generator().manual_seed(V)) * 2).to(BF)
    g[V - 1] = g.max() + 1
    out.append(Case(f"V{V}-width-greedy", g, 0.0, 0, 1.0, torch.tensor([0.5]), torch.tensor([V - 1]), "greedy"))
    # 3.0 in the middle, 2.0 in the first and the last column, 1.0 elsewhere; top_k = 2 keeps the
    # pair of 2.0 whole
    small = torch.ones(V, dtype=BF)
    if V >= 3:
        small[0] = small[V - 1] = 2.0
    small[V // 2] = 3.0
    out.append(_mid_case(f"V{V}-width-lattice", small, 1.0, 2, 1.0, lambda kept, w: kept.nonzero().flatten().tolist()))
    return out


def all_cases():
    out = []
    for V in LATTICE_VOCABS:
        out += lattice_cases(V)
    for V in WALK_VOCABS:
        out += walk_cases(V)
    for V in WIDTH_VOCABS:
        out += width_cases(V)
    return out


# ---------------------------------------------------------------- random rows
ROWS = 64
CONFIGS = [(3.0, 50257), (1.0, 50257), (6.0, 1000)]
_rows_cache = {}


def config_rows(i):
    """The 64 rows of configuration i, drawn row after row from one CPU stream over the three
    configurations in order (made once, never modified)."""
    if not _rows_cache:
        gen = torch.Generator().manual_seed(0)
        for c, (scale, V) in enumerate(CONFIGS):
            _rows_cache[c] = torch.stack([(torch.randn(V, generator=gen) * scale).bfloat16() for _ in range(ROWS)])
    return _rows_cache[i]


# (configuration, (temperature, top_k, top_p)): each cut alone, top_k on both sides of the
# shortcut's limit (and >= V at V = 1000), both cuts, a cold and a hot temperature.  At each the
# f64 oracle itself excuses at most MAX_AMBIGUOUS of the 64 rows (test_sample_cases_cpu.py); the
# settings where it excuses more -- top_p = 0.999, top-p alone at T >= 5, (0.8, 2000, 0.95), and
# (100, 2000, 0.5) on the 1000 nearly uniform columns of configuration 2, 15 rows -- are lattice cases.
MATRIX_SETTINGS = [(0.8, 0, 1.0), (0.8, 1, 1.0), (0.8, 1024, 1.0), (0.8, 1025, 1.0), (0.8, 5000, 1.0), (0.8, 0, 0.05),
                   (0.8, 0, 0.5), (0.8, 0, 0.9), (0.8, 5, 0.3), (0.05, 50, 0.9), (100.0, 2000, 0.5)]
MATRIX = [(ci, s) for ci in (0, 2) for s in MATRIX_SETTINGS if (ci, s) != (2, (100.0, 2000, 0.5))]


def check_interval_rows(rows, u, tok, temperature, top_k, top_p, what=""):
    """The assertion on random rows: every token is a kept column whose interval of the f64
    prefix sums holds u Z within U_BAND; a row with a candidate within P_BAND of top_p may draw
    that candidate instead and is counted.  At most MAX_AMBIGUOUS such rows.  Returns (ambiguous
    rows, the largest kept set)."""
    N, V = rows.shape
    tok = [int(t) for t in tok]
    assert all(0 <= t < V for t in tok), f"{what}: a padding column was drawn"
    n_ambiguous, largest = 0, 0
    for r in range(N):
        kept, w, amb = oracle_row(rows[r], temperature, top_k, top_p)
        largest = max(largest, int(kept.sum()))
        t = tok[r]
        if amb.any():
            n_ambiguous += 1
            assert kept[t] or amb[t], (what, r, t)
            continue
        assert kept[t], (what, r, t)
        cum = torch.cumsum(w * kept, 0)
        Z = cum[-1].item()
        lo, hi = (cum[t] - w[t]).item() - U_BAND * Z, cum[t].item() + U_BAND * Z
        assert lo <= u[r].double().item() * Z <= hi, (what, r, t, lo / Z, u[r].item(), hi / Z)
    assert n_ambiguous <= MAX_AMBIGUOUS, (what, n_ambiguous)
    return n_ambiguous, largest
