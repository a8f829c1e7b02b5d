"""Ion fluxes and membrane exchange on cell-partitioned runs (DeviceStepper.fluxes / exchange with halo=...), rehearsed on
one card: fresh child processes (gloo, all on GPU 0, at most 3) each step their part with both recorders attached, fields
on; every rank must hold the same series, and rank 0 compares them with the same recorders on one rank holding the whole
mesh -- maxima and the per-item fields of the recorded items (matched by centroid) bit for bit, sums within
2 n 2^-53 sum |term| (tools/check_partition_fluxes.py).

Runs early (file name): the children are started before this process has touched the GPU.
"""
import pytest

from partition_ranks import run_ranks

TOOL = "check_partition_fluxes.py"

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind,method,world,every,capacity", [
    ("tet", "rcb", 2, 1, 4), ("tet", "rcb", 3, 3, 1), ("hex", "slab", 2, 2, 2), ("tet", "slabgen", 2, 1, 8),
    ("tet", "far", 2, 2, 1)])
def test_partitioned_series_equal_single_rank(kind, method, world, every, capacity):
    """Six steps without solves: the partitioned steps are bit-identical to the single-rank ones
    (test_00_partition_device), so the series differ only by the order of summation.  A capacity below the number of
    records drains mid-run (the first case: four of six).  "far": rank 0 holds no intracellular cell and no membrane
    facet, and contributes zeros for them."""
    rcs, outs = run_ranks(TOOL, ["--kind", kind, "--method", method, "--steps", "6", "--every", str(every),
                                 "--capacity", str(capacity)], world=world)
    assert rcs == [0] * world, "\n".join(outs)
    assert "PARTITION FLUXES OK" in outs[0], outs[0]


def test_three_subdomain_driver_series():
    """The astrocyte driver's set-up (ECS + neuron + glia, two membrane models, pulsed ECS source) on an RCB partition,
    both cells watched."""
    rcs, outs = run_ranks(TOOL, ["--family", "astro", "--kind", "tet", "--method", "rcb", "--steps", "4", "--every", "1",
                                 "--capacity", "3"])
    assert rcs == [0, 0], "\n".join(outs)
    assert "PARTITION FLUXES OK" in outs[0], outs[0]


def test_partitioned_series_and_budget_with_distributed_solves():
    """Whole time steps with the distributed Krylov solves: the series agree with the single-rank run to the solver
    tolerance of check_partition_steps.py --solves, and the mass budget of the partitioned run -- the global exchange
    series with the partitioned observables' masses -- closes to the single-rank residual blocks."""
    rcs, outs = run_ranks(TOOL, ["--kind", "tet", "--method", "rcb", "--steps", "4", "--every", "1", "--solves"])
    assert rcs == [0, 0], "\n".join(outs)
    assert "the mass budget of the partitioned run closes" in outs[0] and "PARTITION FLUXES OK" in outs[0], outs[0]


def test_two_partitioned_runs_are_bit_identical():
    rcs, outs = run_ranks(TOOL, ["--kind", "tet", "--method", "rcb", "--steps", "4", "--every", "1", "--repeat"])
    assert rcs == [0, 0], "\n".join(outs)
    assert "two partitioned runs give identical series" in outs[0] and "PARTITION FLUXES OK" in outs[0], outs[0]


def test_library_rccl_record_matches_unpartitioned_rows():
    """One rank, nccl backend: the halo runs on the library's communicator and every record sums the exchange buffer
    with knpemi_comm_allreduce; the rows equal those of the plain recorders bit for bit."""
    rcs, outs = run_ranks(TOOL, ["--kind", "tet", "--method", "rcb", "--steps", "4", "--every", "1", "--capacity", "3",
                                 "--rccl"], world=1)
    assert rcs == [0], outs[0]
    assert "library RCCL" in outs[0] and "PARTITION FLUXES OK" in outs[0], outs[0]
