"""Every compiled instantiation of the persistent GEMM family (ops/csrc/gemm_parts.txt) runs
and matches an fp32 product.

``test_gemm_plan_cpu.py::test_every_compiled_kernel_is_reached`` proves that every identity is
named by some recorded plan; here each one is executed.  Per identity:

* ``smallest``: the smallest recorded case (tests/golden/gemm_plan_cases.txt) that names it and
  whose settings a running process can apply (tests/gemm_cases.py);
* ``two_units``: that case on the smallest grid (a CU reserve beyond the CU count: 8 workgroups,
  16 slots for v8), grown a tile at a time along M and N until one workgroup streams at least
  two units -- the ring's carry-over across a tile boundary, the store credit and, for v7d, a
  deferred tile.  Every identity has such a case (checked without a GPU by
  test_gemm_plan_cpu.py::test_every_compiled_kernel_has_gpu_cases); the SCHED 2 kernels, whose
  smallest case may be id 17 (one unit per workgroup by design) or v8 with a k-major A (17 row
  tiles needed, the other operand's rows kept short), get theirs from id 20 / 21 and more tiles.

The plan the dispatcher explains for the call must name exactly the identity under test, and the
outputs are held to the bounds of test_table_signature_matches_fp32 (1.5e-2 bf16 outputs and
aux_out, 5e-3 f32 outputs and colsum, relative to the largest magnitude).
"""
import pytest

import gemm_cases as gc

pytestmark = pytest.mark.gpu

IDENTITIES = gc.identities()
CASES = gc.cases_by_identity()  # per identity, the smallest first


@pytest.mark.parametrize("ident", IDENTITIES)
def test_instantiation_smallest_case_matches_fp32(monkeypatch, ident):
    gc.run_case(CASES[ident][0], ident, monkeypatch)


@pytest.mark.parametrize("ident", IDENTITIES)
def test_instantiation_two_units_per_workgroup_matches_fp32(monkeypatch, ident):
    case = gc.two_unit_case(ident, CASES[ident], gc.explain_on_device)
    assert case is not None, f"no two-unit case within {gc.MAX_GROW} tiles of {CASES[ident]}"
    plan = gc.run_case(case, ident, monkeypatch)
    assert gc.streams_two_units(ident, plan), (case, plan)
