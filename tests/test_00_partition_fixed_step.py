"""A fixed-step membrane integrator on a cell partition, rehearsed on one card (the pattern of
test_00_partition_device.py): two child processes each step their slab with DeviceStepper(ode_method="rk4"), the ghost
membrane dofs integrated redundantly; the method is deterministic, so every owned membrane field, ODE state and
right-hand-side row equals the single-rank run bit for bit (tools/check_partition_steps.py --ode-method).

Runs early (file name): the children are started before this process has touched the GPU.
"""
import pytest

from partition_ranks import run_ranks


@pytest.mark.gpu
@pytest.mark.parametrize("family,method", [("idealized", "slabgen"), ("astro", "rcb")])
def test_two_rank_rk4_steps_equal_single_rank_bit_for_bit(family, method):
    args = ["--kind", "tet", "--steps", "4", "--method", method, "--family", family, "--ode-method", "rk4",
            "--ode-substeps", "25"]
    rcs, outs = run_ranks("check_partition_steps.py", args)
    assert rcs == [0, 0], "\n".join(outs)
    assert "PARTITION STEPS OK" in outs[0], outs[0]
    assert "ode_method rk4" in outs[0], outs[0]
