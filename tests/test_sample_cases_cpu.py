"""The cases of tests/sample_cases.py reach what they are for, and its assertions bite, on the CPU:
every constructed case meets the preconditions that put its token beyond doubt, together they
land a cut in every bin position and a draw at every edge of the kernel's walk (else
test_sampling_gpu.py would pass without running those arms), the geometry is the kernel's own,
the torch twin passes the assertions the GPU tests make, and small mutations of a right answer
fail them."""
import os
import re

import pytest
import torch

import sample_cases as sc

from distributed_pytorch_cookbook_amd.ops import sample as ops_sample
from distributed_pytorch_cookbook_amd.ops.sample import sample_logits, sample_reference

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "distributed_pytorch_cookbook_amd",
                    "ops", "csrc")
CASES = sc.all_cases()


def by_name(name):
    return next(c for c in CASES if c.name == name)


# ---------------------------------------------------------------- geometry and keys
def test_geometry_is_the_kernels():
    with open(os.path.join(CSRC, "sample.hip")) as f:
        src = f.read()
    assert f"constexpr int SM_NT = {sc.SM_NT};" in src and "constexpr int SM_NW = SM_NT / 64;" in src
    assert f"constexpr int SM_MAX_ITERS = {sc.MAX_ITERS};" in src
    assert "constexpr int SM_MAX_V = SM_NW * 512 * SM_MAX_ITERS;" in src
    assert "if (p.top_k <= SM_NT) {" in src  # the shortcut's limit
    launch = re.search(r"if \(a->V <= SM_NW \* 512\) hipLaunchKernelGGL\(sample_kernel<(\d+)>.*\n\s*else "
                       r"hipLaunchKernelGGL\(sample_kernel<(\w+)>", src)
    assert launch and launch.groups() == ("1", "SM_MAX_ITERS")
    assert "a->V > SM_MAX_V || a->ld < a->V" in src
    assert "const int base = wv * SEG + lane * 8;" in src and "SEG = ITERS * 512" in src
    assert sc.SPLIT_V == 8192 and sc.MAX_VOCAB == 57344 == ops_sample.MAX_VOCAB
    assert sc.iters_for(8192) == 1 and sc.iters_for(8193) == 7
    assert sc.walk_position(3 * 3584 + 2 * 512 + 63 * 8 + 7, 50257) == (3, 2, 63, 7)
    assert sc.walk_position(8191, 8192) == (15, 0, 63, 7)


def test_key_of_orders_the_values():
    vals = [sc.NEG_INF, -300.0, -2.5, -1.0, -2.0 ** -126, 0.0, 2.0 ** -126, 0.5, 1.0, 1.9921875, 2.0, 7.5, 3e38]
    keys = [sc.key_of(sc.bf16_bits(torch.tensor(v).bfloat16().item())) for v in vals]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and min(keys) > 0
    assert sc.key_of(0x8000) == sc.key_of(0x0000) == 0x8000  # -0 is +0
    assert sc.key_of(0xFFFF) == 0                              # the marker of a column that is not there
    assert [hex(sc.key_of(sc.bf16_bits(v))) for v, _ in sc.lattice_levels(8192)] == [
        "0xc0f0", "0xc0c0", "0xc000", "0xbfff", "0xbf80", "0xbf00", "0x8000", "0x407f", "0x3fdf", "0x7f"]
    row = sc.bits_to_bf16([0x0000, 0x8000, 0x3F80, 0xFF80])
    assert row.tolist() == [0.0, 0.0, 1.0, sc.NEG_INF] and row.view(torch.int16)[1] == -32768


# ---------------------------------------------------------------- the oracle
def test_oracle_repairs():
    row = torch.tensor([1.0, 3.0, 2.0, 3.0, 2.0, 0.0, -1.0]).bfloat16()

    def kept(k, p):
        return sc.oracle_row(row, 1.0, k, p)[0].nonzero().flatten().tolist()

    assert kept(3, 1.0) == [1, 2, 3, 4] and kept(2, 1.0) == [1, 3]
    assert kept(7, 1.0) == kept(9, 1.0) == kept(0, 1.0) == list(range(7))  # top_k >= V is off
    assert kept(0, 0.69) == [1, 2, 3, 4] and kept(3, 0.73) == [1, 3]
    # top_p = 0: the maximum stays and is not "ambiguous" for it
    k, _, amb = sc.oracle_row(row, 1.0, 0, 0.0)
    assert k.nonzero().flatten().tolist() == [1, 3] and not amb.any()
    # the band still marks a candidate below the maximum: above the 2s lies 0.68041
    assert sc.oracle_row(row, 1.0, 0, 0.68045)[2].nonzero().flatten().tolist() == [2, 4]
    assert not sc.oracle_row(row, 1.0, 0, 0.6806)[2].any()
    # -0.0 and +0.0 are one value; -inf has weight 0 and is never the draw, not even at u = 1
    row = sc.bits_to_bf16([0x8000, 0x0000, 0xBF80, 0xFF80, 0xFF80])
    k, w, _ = sc.oracle_row(row, 1.0, 1, 1.0)
    assert k.tolist() == [True, True, False, False, False]
    k, w, _ = sc.oracle_row(row, 1.0, 4, 1.0)
    assert k.all() and w[3:].tolist() == [0.0, 0.0]
    assert sc.oracle_tokens(k, w, torch.tensor([0.0, 0.99, 1.0])).tolist() == [0, 2, 2]


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize("c", CASES, ids=repr)
def test_case_preconditions(c):
    sc.check_preconditions(c)
    assert sc.check_tokens(c, c.want) == 0


@pytest.mark.parametrize("V", sc.LATTICE_VOCABS)
def test_lattice_cases_cover_every_placement(V):
    cases = sc.lattice_cases(V)
    assert sc.iters_for(V) == (1, 7)[V > 8192]
    row = sc.lattice_row(V)
    bits = (row.view(torch.int16).int() & 0xFFFF).tolist()
    assert bits.count(0x8000) == bits.count(0x0000) == 500  # both zeros are in the row
    assert [int((row.float() == v).sum()) for v, _ in sc.lattice_levels(V)] == [n for _, n in sc.lattice_levels(V)]
    assert all(n >= 100 for _, n in sc.LATTICE[2:]) and len(sc.LATTICE) <= 12
    for cut in ("cut_k", "cut_p"):
        seen = set().union(*(c.tags for c in cases if cut in c.tags and "regime" not in c.tags))
        want = set(sc.PLACEMENTS) - ({"neg_inf"} if cut == "cut_p" else set())  # (top-p never keeps weight 0)
        assert want <= seen, (cut, want - seen)
        # ... each with a target inside the lowest kept level (-inf has none to draw)
        seen = set().union(*(c.tags for c in cases if cut in c.tags and "thr_target" in c.tags))
        assert want - {"neg_inf"} <= seen, (cut, want - seen)
    assert set(sc.K_REGIMES) <= set().union(*(c.tags for c in cases))
    below = {c.top_k for c in cases if "below" in c.tags}
    inside = {c.top_k for c in cases if "inside" in c.tags}
    assert inside == {k + 1 for k in below} and {1024} <= below and {1025, sc.LATTICE_FINITE + 1} <= inside
    # just inside a level: the whole tie stays -- hundreds of columns more than top_k
    c = by_name(f"V{V}-k2525-inside")
    assert int(c.oracle[0].sum()) == 3524
    c = by_name(f"V{V}-k{sc.LATTICE_FINITE + 1}-inside")
    assert c.oracle[0].all() and (c.oracle[1] == 0).sum() == V - sc.LATTICE_FINITE
    # at T = 0.05 only the maximum is above the kernel's 2^-40; at T = 100 the row is nearly uniform
    w = by_name(f"V{V}-T0.05-k0-p1.0").oracle[1]
    assert int((w >= 2.0 ** -40).sum()) == 3 and int((w > 0).sum()) > 3
    w = by_name(f"V{V}-T100.0-k0-p1.0").oracle[1]
    assert w[w > 0].min() > 0.9


@pytest.mark.parametrize("V", sc.WALK_VOCABS)
def test_walk_cases_cover_every_position(V):
    dense, sparse, ends = sc.walk_cases(V)[:3]
    iters = sc.iters_for(V)
    seg = 512 * iters
    pos = [sc.walk_position(t, V) for t in dense.want.tolist()]
    t = set(dense.want.tolist())
    assert {0, V - 1} <= t
    n_seg = (V + seg - 1) // seg
    assert n_seg == (16 if V != 50257 else 15)  # (V = 57344 fills the 16 segments of sample_kernel<7>)
    for wv in range(n_seg):
        assert {wv * seg, min((wv + 1) * seg, V) - 1} <= t, wv
    assert {(it, lane, e) for wv, it, lane, e in pos if wv == 3} >= (
        {(it, 0, 0) for it in range(iters)} | {(it, 63, 7) for it in range(iters)})
    assert {(lane, e) for wv, it, lane, e in pos if wv == 5} >= {(l, e) for l in (0, 63) for e in (0, 7)}
    assert {it for _, it, _, _ in pos} == set(range(iters))
    # the sparse row: every kept column is a target, 512 dropped columns lie between two, and
    # they fall on every element and iteration, in every wave with a full segment
    assert sparse.top_k == 1 and int(sparse.oracle[0].sum()) == len(sparse.want) == (V + 512) // 513 > 1
    pos = [sc.walk_position(t, V) for t in sparse.want.tolist()]
    assert {e for *_, e in pos} == set(range(8)) and {wv for wv, *_ in pos} >= set(range(V // seg))
    if iters > 1:
        assert {it for _, it, _, _ in pos} == set(range(iters))
    assert ends.u.tolist() == [0.0, 1.0] and torch.isinf(ends.row[[0, -1]].float()).all()


def test_width_cases_cover_every_edge():
    assert {1, 7, 8, 9, 511, 512, 513, 8191, 8192, 8193, 57343, 57344} == set(sc.WIDTH_VOCABS)
    for V in sc.WIDTH_VOCABS:
        kinds = [c.kind for c in sc.width_cases(V)]
        assert kinds == ["sole", "greedy", "mid"]
        lattice = sc.width_cases(V)[2]
        assert V - 1 in lattice.want.tolist() and 0 in lattice.want.tolist()
        if V >= 3:  # the pair of 2.0 is wider than top_k - 1
            assert lattice.top_k == 2 and int(lattice.oracle[0].sum()) == 3


# ---------------------------------------------------------------- the twin passes the GPU tests' assertions
def _twin_tokens(c, f64):
    rows = c.rows()
    if f64:
        return sample_reference(rows, c.temperature, c.top_k, c.top_p, c.u, dtype=torch.float64)
    N = len(c.u)
    counters = torch.zeros(N, dtype=torch.int64)
    out = torch.full((N, 1), -7, dtype=torch.int64)
    sample_logits(rows, temperature=c.temperature, top_k=c.top_k, top_p=c.top_p, u=c.u, counters=counters, out_tok=out)
    assert counters.tolist() == [1] * N
    return out[:, 0]


@pytest.mark.parametrize("f64", [True, False], ids=["reference-f64", "cpu-path"])
@pytest.mark.parametrize("c", CASES, ids=repr)
def test_twin_passes_the_exact_checks(c, f64):
    assert sc.check_tokens(c, _twin_tokens(c, f64)) == 0


@pytest.mark.parametrize("ci,setting", sc.MATRIX, ids=str)
def test_matrix_oracle_stays_inside_the_cap(ci, setting):
    """The f64 reference's own tokens on the 64 random rows of a setting pass the interval check
    with at most MAX_AMBIGUOUS rows excused (the count is printed: it is the oracle's, whatever
    sampler is checked)."""
    rows = sc.config_rows(ci)
    u = torch.tensor([ops_sample.sample_uniform(1234, r, 7) for r in range(sc.ROWS)], dtype=torch.float32)
    tok = sample_reference(rows, *setting, u, dtype=torch.float64)
    n, largest = sc.check_interval_rows(rows, u, tok, *setting, what=f"{sc.CONFIGS[ci]} {setting}")
    print(f"config {sc.CONFIGS[ci]} {setting}: {n} ambiguous rows, kept sets up to {largest}")


# ---------------------------------------------------------------- mutations
def _draw_from(c, kept):
    return sc.oracle_tokens(kept, c.oracle[1], c.u)


def _mutant_exact_k(c):
    """top-k keeps exactly k columns (the first k of a stable descending sort), not the whole tie."""
    order = torch.sort(c.row.double(), descending=True, stable=True)[1]
    kept = torch.zeros(c.V, dtype=torch.bool)
    kept[order[:c.top_k]] = True
    return _draw_from(c, kept)


def _mutant_inclusive_p(c):
    """top-p keeps a value iff the mass down to and including it is <= p (the maximum always):
    the comparison of the cut moved from the mass above a value to the mass that reaches it."""
    z = c.row.double() / c.temperature
    keep_k = sc.oracle_row(c.row, c.temperature, c.top_k, 1.0)[0]
    w = c.oracle[1] * keep_k
    q_ge = torch.stack([w[z >= v].sum() for v in z[keep_k].unique()]) / w.sum()
    ok = z[keep_k].unique()[q_ge <= c.top_p]
    kept = keep_k & (torch.isin(z, ok) | (z == z.max()))
    return _draw_from(c, kept)


@pytest.mark.parametrize("V", sc.LATTICE_VOCABS)
def test_mutations_fail_the_exact_checks(V):
    cases = sc.lattice_cases(V)
    n = 0
    for c in cases:
        if {"cut_k", "inside", "thr_target"} <= c.tags:
            with pytest.raises(AssertionError, match="which the cuts drop|drawn at u"):
                sc.check_tokens(c, _mutant_exact_k(c))
            n += 1
    assert n >= 8
    n = 0
    for c in cases:
        if {"cut_p", "thr_target"} <= c.tags and int(c.oracle[0].sum()) > 3:  # (the maximum stays either way)
            with pytest.raises(AssertionError, match="drawn at u"):
                sc.check_tokens(c, _mutant_inclusive_p(c))
            n += 1
    assert n >= 9
    for c in cases + sc.walk_cases(V) + sc.width_cases(V - 1)[::2]:
        kept, w, _ = c.oracle
        ok = (kept & (w > 0)).nonzero().flatten()
        if len(ok) > 1:
            # the token moves one kept column later (the last wraps to the first)
            nxt = torch.stack([ok[(int((ok == t).nonzero()) + 1) % len(ok)] for t in c.want])
            with pytest.raises(AssertionError, match="drawn at u"):
                sc.check_tokens(c, nxt)
        with pytest.raises(AssertionError, match="padding"):
            sc.check_tokens(c, [c.V] + c.want.tolist()[1:])
        with pytest.raises(AssertionError, match="padding"):
            sc.check_tokens(c, c.want.tolist()[:-1] + [-1])
        dropped = (~kept).nonzero().flatten()
        if len(dropped):
            with pytest.raises(AssertionError, match="which the cuts drop"):
                sc.check_tokens(c, [int(dropped[0])] + c.want.tolist()[1:])
    # a -inf column that the cuts keep is drawn: at u = 1 without the clamp, the last kept index
    for name in (f"V{V}-k{sc.LATTICE_FINITE + 1}-inside", f"V{V}-walk-ends", f"V{V}-lattice-ends"):
        c = by_name(name)
        banned = (c.oracle[0] & torch.isinf(c.row.float())).nonzero().flatten()
        with pytest.raises(AssertionError, match="weight 0"):
            sc.check_tokens(c, c.want.tolist()[:-1] + [int(banned[-1])])


def test_mutations_fail_the_greedy_and_interval_checks():
    for V in (7, 513, 8193):
        c = sc.width_cases(V)[1]
        tied = sc.Case(c.name + "-tied", c.row.clone(), 0.0, 0, 1.0, c.u, torch.tensor([2]), "greedy")
        tied.row[2] = tied.row[V - 1]
        assert sc.check_tokens(tied, [2]) == 0
        with pytest.raises(AssertionError, match="the first is at 2"):
            sc.check_tokens(tied, [V - 1])  # greedy returns the last maximum
        with pytest.raises(AssertionError, match="no maximum"):
            sc.check_tokens(c, [0])
    # random rows: the token one kept column later, and a dropped column, fail the interval check
    rows = sc.config_rows(2)
    setting = (0.8, 0, 0.5)
    u = torch.tensor([ops_sample.sample_uniform(1234, r, 7) for r in range(sc.ROWS)], dtype=torch.float32)
    tok = sample_reference(rows, *setting, u, dtype=torch.float64)
    kept = sc.oracle_row(rows[0], *setting)[0].nonzero().flatten()
    assert len(kept) > 1
    later = tok.clone()
    later[0] = kept[(int((kept == tok[0]).nonzero()) + 1) % len(kept)]
    with pytest.raises(AssertionError):
        sc.check_interval_rows(rows, u, later, *setting)
    stray = tok.clone()
    stray[0] = int((~sc.oracle_row(rows[0], *setting)[0]).nonzero()[0])
    with pytest.raises(AssertionError):
        sc.check_interval_rows(rows, u, stray, *setting)
    with pytest.raises(AssertionError, match="padding"):
        sc.check_interval_rows(rows, u, [1000] + tok.tolist()[1:], *setting)
