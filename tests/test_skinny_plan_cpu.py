"""The skinny-Linear planner (host only): an instantiated plan for every shape, from the shape alone."""
import pytest

from distributed_pytorch_cookbook_amd.ops.gemm import SKINNY_PLANS, skinny_plan


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_skinny_plan(cus):
    for N in (1, 15, 16, 17, 104, 768, 2304, 6400, 16 * cus - 1, 16 * cus, 16 * cus + 1, 50304, 1 << 20):
        for M in (1, 17, 64):
            for K in (8, 64, 520, 6400):
                nb, nw = plan = skinny_plan(M, N, K, cus)
                assert plan in SKINNY_PLANS and nw >= 1 and -(-N // nb) * nb >= N
                # the wider strip only while every second compute unit still gets a workgroup
                assert (nb == 32) == (2 * -(-N // 32) >= cus)
