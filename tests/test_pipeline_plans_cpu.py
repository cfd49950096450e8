"""The pipeline's host-side plans are pinned: unit / stage costs (bit for bit), partitions and
zero-bubble orders of every architecture preset, recorded in ``golden/pipeline_plans.json``.

A tie between equal-cost layers decides where ``partition`` cuts and when ``simulate_orders``
runs a W pass, so a cost that moves by one ulp can move a stage boundary: the costs are compared
as ``float.hex()`` strings.  ``PYTHONPATH=. python tests/test_pipeline_plans_cpu.py`` re-records
the file (golden/README.md).
"""
import json
import os
from types import SimpleNamespace

from distributed_pytorch_cookbook_amd.models.gpt import PRESETS
from distributed_pytorch_cookbook_amd.parallel.pipeline import (p2p_deadlock_free, partition, schedule_zb,
                                                                stage_costs, unit_costs)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_plans.json")
PPS = (2, 4, 8)
VOCAB = 50257


def _ops(order):
    return " ".join(f"{k}{m}" for k, m in order)


def compute_plans():
    """{preset: {seq_len, unit_costs, pp: {pp: {partition, stage_costs, orders: {"zb/M8": [stage
    order strings]}}}}} from the functions under test."""
    out = {}
    for name, cfg in PRESETS.items():
        model = SimpleNamespace(dim=cfg["dim"], heads=cfg["heads"], head_dim=cfg["head_dim"],
                                num_layers=cfg["num_layers"], vocab_size=VOCAB)
        S = cfg["sequence_length"]
        units = unit_costs(model, S)
        case = {"seq_len": S, "unit_costs": [c.hex() for c in units], "pp": {}}
        for pp in PPS:
            groups = partition(units, pp)
            costs = stage_costs(model, S, groups)
            orders = {}
            for sched, mem in (("zb", 1), ("zb2", 2)):
                for M in (2 * pp, 4 * pp):
                    orders[f"{sched}/M{M}"] = [_ops(schedule_zb(M, s, pp, costs=costs, mem=mem)) for s in range(pp)]
            case["pp"][str(pp)] = {"partition": groups, "stage_costs": [[c.hex() for c in t] for t in costs],
                                   "orders": orders}
        out[name] = case
    return out


def _parse(ops):
    return [(op[0], int(op[1:])) for op in ops.split()]


def test_recorded_pipeline_plans():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = compute_plans()
    assert sorted(got) == sorted(want) == sorted(PRESETS)
    n_sets = 0
    for name in want:
        w, g = want[name], got[name]
        assert g["seq_len"] == w["seq_len"], name
        assert g["unit_costs"] == w["unit_costs"], name
        assert sorted(w["pp"]) == sorted(str(pp) for pp in PPS), name
        for pp in w["pp"]:
            wp, gp = w["pp"][pp], g["pp"][pp]
            assert gp["partition"] == wp["partition"], (name, pp)
            assert gp["stage_costs"] == wp["stage_costs"], (name, pp)
            assert sorted(gp["orders"]) == sorted(wp["orders"]), (name, pp)
            for key, stages in wp["orders"].items():
                assert gp["orders"][key] == stages, (name, pp, key)
                assert len(stages) == int(pp)
                assert p2p_deadlock_free([_parse(o) for o in stages]), (name, pp, key)
                n_sets += 1
    assert n_sets == len(PRESETS) * len(PPS) * 4


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump(compute_plans(), f, indent=0, sort_keys=True)
        f.write("\n")
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
