"""The cases of tests/mem_cases.py reach what they are for, and its assertions bite, on the CPU:
the run layouts meet every chunk phase and piece length of the sorted embedding backward (else
test_kernel_trips_gpu.py would pass without running those arms), the scaler script is torch's
rule, the trip geometry is the dispatchers', and the ops' own CPU paths pass the assertions the
GPU tests make while small mutations of their results fail them."""
import os

import pytest
import torch

import mem_cases as mc
from kernel_checks import guarded

from distributed_pytorch_cookbook_amd.ops.amp import GradScaler
from distributed_pytorch_cookbook_amd.ops.embedding import embedding_bwd
from distributed_pytorch_cookbook_amd.ops.loss import cross_entropy_fused

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "distributed_pytorch_cookbook_amd",
                    "ops", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ---------------------------------------------------------------- geometry
def test_trip_geometry_is_the_dispatchers():
    misc, ln, eb = _src("misc.hip"), _src("layernorm.hip"), _src("embed_bwd.hip")
    assert f"if (b > {mc.FLAT_MAX_BLOCKS}) b = {mc.FLAT_MAX_BLOCKS};" in misc
    assert f"cap = cap < {mc.LN_BWD_MIN_BLOCKS} ? {mc.LN_BWD_MIN_BLOCKS}" in ln
    assert f"constexpr int EB_CH = {mc.EB_CH};" in eb
    assert mc.flat_trip_elems == 8192 * 256 * 4 and mc.ln_bwd_sweep_rows == 256 * 4
    # the sizes of test_kernel_trips_gpu.py: a second trip for 300 threads (AdamW moves two
    # vectors per thread per trip, the others one), none at the sizes of the edge tests
    assert mc.flat_trips(2 * 8192 * 256 + 300, vecs_per_trip=2) == 2
    assert mc.flat_trips(2 * 8192 * 256, vecs_per_trip=2) == 1
    assert mc.flat_trips(8192 * 256 + 300) == 2 and mc.flat_trips(8192 * 256) == 1
    assert mc.flat_trips(2049 * (4100 // 4)) == 2
    assert mc.flat_trips((4096 + 12) // 4) == 1 and mc.flat_trips(67 * 100 // 4) == 1
    assert mc.AMP_LARGE > mc.flat_trip_elems and mc.AMP_LARGE % 4 == 3
    assert any(p >= mc.flat_trip_elems for p in mc.amp_positions(mc.AMP_LARGE)[:-1])  # beside n - 1
    assert mc.ln_bwd_rows_per_wave(517) == (1, 1)  # the largest T of the kernel tests before these
    assert mc.ln_bwd_rows_per_wave(1026) == (1, 2) and mc.ln_bwd_rows_per_wave(2051) == (2, 3)


@pytest.mark.parametrize("n", mc.AMP_SMALL + [mc.AMP_LARGE])
def test_amp_positions(n):
    pos = mc.amp_positions(n)
    assert all(0 <= p < n for p in pos) and 0 in pos and n - 1 in pos
    if n & 3 and n > 4:
        assert pos[-1] >= (n // 4) * 4 > pos[-2]  # one in the scalar tail, one in the last full vector


# ---------------------------------------------------------------- run layouts
@pytest.mark.parametrize("variant", [0, 1])
def test_run_layout(variant):
    L = mc.run_layout(variant)
    T, V = L["T"], L["V"]
    assert T == (372, 376)[variant] and (T % mc.EB_CH == 0) == bool(variant)
    assert L["keys"] == sorted(L["keys"]) and max(L["keys"]) < V
    assert len(set(range(V)) - set(L["keys"])) >= V // 2  # table rows that no token names
    for rows in (L["tok_rows"], L["pos_rows"]):
        assert not torch.equal(rows, torch.arange(T))      # rows[] is not the identity
    assert not torch.equal(L["ids"], L["pos"])
    assert L["ids"][L["bad_rows"]].tolist() == [V + 3, -1, 2 ** 40]
    assert sorted(L["tok_rows"][-3:].tolist()) == sorted(L["bad_rows"])  # out-of-range ids sort last
    # the position table has the lengths as listed; the token table the same with three runs a row shorter
    assert [n for _, _, n in L["pos_runs"]] == L["lengths"]
    short = [n - (n in mc.BAD_FROM) for n in L["lengths"]]
    assert [n for _, _, n in L["tok_runs"]] == short
    mc.assert_layout_complete(L["tok_runs"], "token table")
    c = mc.layout_conditions(L["pos_runs"])
    if variant:
        mc.assert_layout_complete(L["pos_runs"], "position table")
        key, start, n = L["pos_runs"][-1]
        assert n == 4 and start + n == T and start // mc.EB_CH == (T - 1) // mc.EB_CH  # fits, ends at T
    else:
        # (the listed lengths alone have no run that fits and ends on a chunk end: variant 1 adds it)
        c.pop("fits_to_chunk_end")
        assert c.pop("phases") == set(range(8)) and c.pop("pieces") == set(range(1, 9)) and all(c.values()), c
        assert T % mc.EB_CH and L["pos_runs"][-1][1] + 65 == T  # the last chunk is partial, inside a run


def test_run_pieces():
    assert mc.run_pieces(0, 8) == [8] and mc.run_pieces(7, 2) == [1, 1] and mc.run_pieces(5, 20) == [3, 8, 8, 1]
    assert mc.layout_conditions([(0, 7, 11)])["one_row_into_next_chunk"] == 0
    assert mc.layout_conditions([(0, 7, 2)])["starts_in_last_slot_and_crosses"] == 1
    assert mc.layout_conditions([(0, 7, 2)])["one_row_into_next_chunk"] == 1


def test_embedding_cpu_path_passes_the_table_check():
    """ops.embedding.embedding_bwd on CPU tensors (index_add_) through check_embedding_table, and
    two mutations it must refuse: a run that lost its last piece, an unnamed row written."""
    L = mc.run_layout(1)
    D = 8
    g = torch.Generator().manual_seed(9)
    dout = torch.randn(L["T"], D, generator=g)
    bt, bp = torch.randn(L["V"], D, generator=g), torch.randn(L["P"], D, generator=g)
    dt, dp = guarded((L["V"], D), torch.float32, fill=bt), guarded((L["P"], D), torch.float32, fill=bp)
    embedding_bwd(dout, L["pos"], L["pos"], dt, dp)  # (the CPU path takes no out-of-range id)
    mc.check_embedding_table(dt, bt, dout, L["pos"], "dtok")
    mc.check_embedding_table(dp, bp, dout, L["pos"], "dpos")
    # the references leave out a row whose own index is out of range, and only that table's
    ref64, _, named = mc.embedding_refs(bt, dout, L["ids"], L["V"])
    ok = torch.ones(L["T"], dtype=torch.bool)
    ok[L["bad_rows"]] = False
    assert torch.equal(ref64, bt.double().index_add_(0, L["ids"][ok], dout[ok].double()))
    assert named.sum() == len(L["keys"])
    key, start, n = next(r for r in L["pos_runs"] if r[2] == 65)
    lost = dt.clone()
    lost[key] -= dout[L["pos_rows"][start + n - 1]]
    with pytest.raises(AssertionError):
        mc.check_embedding_table(lost, bt, dout, L["pos"], "dtok")
    stray = dt.clone()
    stray[0, 0] += 1e-6  # key 0 is named by no row
    with pytest.raises(AssertionError, match="unnamed"):
        mc.check_embedding_table(stray, bt, dout, L["pos"], "dtok")


# ---------------------------------------------------------------- loss scaling
@pytest.mark.parametrize("growth,backoff", [(2.0, 0.5), (1.7, 0.6)])
def test_scaler_script_is_the_cpu_scaler(growth, backoff):
    pattern, interval, init, states = mc.scaler_script(growth, backoff)
    assert len(pattern) == 12 and interval == 3 and init == 2.0 ** 16
    trackers = [s[2] for s in states]
    assert trackers == [1, 2, 0, 1, 2, 0, 0, 0, 1, 2, 0, 1]
    grew = [i for i in range(1, 12) if states[i][0] > states[i - 1][0]]
    assert grew == [5, 10]  # the growth branch runs twice, first at the step the count reaches 3
    sc = GradScaler("cpu", init_scale=init, growth_factor=growth, backoff_factor=backoff, growth_interval=interval)
    for i, found in enumerate(pattern):
        sc.found_inf.fill_(float(found))
        sc.update()
        mc.check_scaler_state(sc, states[i], exact_inv=True, what=f"step {i}")  # (CPU division is exact)
        mc.check_scaler_state(sc, states[i], exact_inv=False, what=f"step {i}")


def test_scaler_state_check_refuses_an_off_by_one_interval():
    pattern, interval, init, states = mc.scaler_script()
    sc = GradScaler("cpu", init_scale=init, growth_interval=interval + 1)  # 't > interval'
    with pytest.raises(AssertionError):
        for i, found in enumerate(pattern):
            sc.found_inf.fill_(float(found))
            sc.update()
            mc.check_scaler_state(sc, states[i], exact_inv=True)


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("n", mc.AMP_SMALL)
def test_amp_check_cpu_path_passes_the_matrix(n, offset):
    sc = GradScaler("cpu")
    g = guarded(n, torch.float32, offset=offset)
    mc.amp_clean_fill(g)
    assert mc.check_amp_matrix(sc, g) == 3 + 3 * len(mc.amp_positions(n))
    sc.check(g[:0])  # n == 0: nothing to read
    assert float(sc.found_inf) == 0.0


def test_amp_matrix_refuses_a_check_without_the_tail():
    class NoTail(GradScaler):
        def check(self, grad):
            super().check(grad[:grad.numel() & ~3])

    g = torch.empty(1027)
    mc.amp_clean_fill(g)
    with pytest.raises(AssertionError, match="at 1026 not seen"):
        mc.check_amp_matrix(NoTail("cpu"), g)


# ---------------------------------------------------------------- cross-entropy
def test_cross_entropy_cpu_path_passes_the_row_check():
    """ops.loss.cross_entropy_fused on CPU tensors gives the gradient rows; with the plain f32 row
    losses they pass check_cross_entropy.  A tie at the maximum counts for the first index only."""
    T, V, ld = 5, 21, 24
    g = torch.Generator().manual_seed(3)
    vals = (torch.randn(T, V, generator=g) * 2).bfloat16()
    vals[1, 4] = vals[1, 17] = 9.0
    vals[2, 4] = vals[2, 17] = 9.0
    tg = torch.tensor([3, 4, 17, -100, V - 1])
    assert mc.first_argmax(vals)[1:3].tolist() == [4, 4]
    buf = torch.zeros(T, ld)
    buf[:, :V] = vals.float()
    inv = torch.tensor([1.0 / 4])
    cross_entropy_fused(buf, tg, V, write_grad=True)
    row_loss = mc.cross_entropy_refs(vals, tg, inv, torch.float32)[0]
    hit = torch.tensor([float(vals[0].argmax() == 3), 1.0, 0.0, 0.0, float(vals[4].argmax() == V - 1)])
    mc.check_cross_entropy(row_loss, buf[:, :V].bfloat16(), buf[:, V:], hit, vals, tg, inv)
    wrong = hit.clone()
    wrong[2] = 1.0  # the second of two equal maxima taken for the argmax
    with pytest.raises(AssertionError):
        mc.check_cross_entropy(row_loss, buf[:, :V].bfloat16(), buf[:, V:], wrong, vals, tg, inv)
