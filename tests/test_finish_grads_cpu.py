"""The shared end of a step on the CPU engines: what ``store.finish_grads`` reports to its
consumer (``Engine._finish_and_step`` feeds it to ``FlatAdamW.update``), and the skip decision
of a step whose gradients are non-finite on one rank only."""
import pytest
import torch

from dist_helpers import run_workers
from finish_workers import build, readiness, worker_poisoned, worker_readiness


def check_contract(res):
    """The reported ranges are disjoint, tile [0, numel) of the optimizer's buffer, start and
    end on multiples of 4 (FlatAdamW.update's kernel path), and are the same every step; the
    consumer does not change the gradients."""
    first, second = res["ranges"]
    assert first == second
    assert all(lo % 4 == 0 and (hi - lo) % 4 == 0 and hi > lo for lo, hi in first)
    edge = 0
    for lo, hi in sorted(first):
        assert lo == edge, (lo, edge)  # no gap, no overlap
        edge = hi
    assert edge == res["numel"]
    for a, b in zip(res["grads0c"], res["grads0"]):
        assert a.abs().max() > 0 and torch.equal(a, b)
    return first


def test_local_store_reports_the_whole_buffer():
    eng, dp, idx = build("local", 1)
    assert check_contract(readiness(eng, dp, idx)) == [(0, eng.store.numel)]


def test_fsdp_one_rank_forced_sharded_reports_every_unit():
    eng, dp, idx = build("fsdp", 1, force_sharded=True)
    ranges = check_contract(readiness(eng, dp, idx))
    # every unit had a reduce-scatter: the last unit first
    assert ranges == sorted(ranges, reverse=True) and len(ranges) == eng.store.nunits


@pytest.mark.slow
@pytest.mark.parametrize("kind,kw", [("ddp", {"reduce_dtype": "float32"}), ("ddp", {"reduce_dtype": "bfloat16"}),
                                     ("fsdp", {})], ids=["ddp-f32", "ddp-bf16", "fsdp"])
def test_two_rank_stores_report_ranges_that_tile_the_buffer(tmp_path, kind, kw):
    out = tmp_path / "ready.pt"
    run_workers(worker_readiness, 2, str(out), kind, kw)
    for r in range(2):
        ranges = check_contract(torch.load(f"{out}.{r}", weights_only=True))
        assert len(ranges) >= 3  # bucket by bucket / unit by unit


@pytest.mark.slow
@pytest.mark.parametrize("kind", ["fsdp", "pipe"])
def test_step_poisoned_on_one_rank_is_skipped_on_both(tmp_path, kind):
    """FSDP shards and pipeline stages differ per rank: the skip flag is reduced over the
    engine's group, so a non-finite gradient on rank 1 alone makes rank 0 skip too -- parameters
    and moments untouched, the step out of the bias-correction count -- and both ranks back
    off to the same scale."""
    out = tmp_path / "poisoned.pt"
    run_workers(worker_poisoned, 2, str(out), kind)
    recs = [torch.load(f"{out}.{r}", weights_only=True) for r in range(2)]
    for before, after, last in recs:
        assert before["step_t"] == [1.0] * len(before["step_t"])
        assert after["step_t"] == before["step_t"]
        for key in ("param", "exp_avg", "exp_avg_sq"):
            for a, b, c in zip(before[key], after[key], last[key]):
                assert torch.equal(a, b)
                assert not torch.equal(b, c)  # the clean step after it moves them again
        assert (before["scale"], after["scale"], last["scale"]) == (65536.0, 32768.0, 32768.0)
        assert (before["tracker"], after["tracker"], last["tracker"]) == (1.0, 0.0, 1.0)
        assert last["step_t"] == [2.0] * len(last["step_t"])
    assert recs[0][2]["scale"] == recs[1][2]["scale"]
