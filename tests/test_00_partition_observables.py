"""Observables on cell-partitioned runs (DeviceStepper.observe(obs, halo=...)), rehearsed on one card: fresh child
processes (gloo, all on GPU 0) each step their part and record the observables of tests/test_observables_gpu.py plus a
point on a rank boundary; every rank must hold the same series, and rank 0 compares it with DeviceStepper.observe on one
rank holding the whole mesh -- points, minima and maxima bit for bit, sums within 1e-13 of sum |w u| / denom
(tools/check_partition_observables.py).

Runs early (file name): the children are started before this process has touched the GPU.
"""
import pytest

from partition_ranks import run_ranks

TOOL = "check_partition_observables.py"

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind,method,world,every,capacity", [
    ("tet", "rcb", 2, 1, 4), ("tet", "rcb", 3, 3, 1), ("hex", "slab", 2, 3, 1), ("tet", "slabgen", 2, 1, 4)])
def test_partitioned_series_equal_single_rank(kind, method, world, every, capacity):
    """Without solves: the partitioned steps are bit-identical to the single-rank ones (test_00_partition_device), so
    the series differ only by the order of summation.  A capacity below the number of records drains mid-run."""
    rcs, outs = run_ranks(TOOL, ["--kind", kind, "--method", method, "--steps", "6", "--every", str(every),
                                 "--capacity", str(capacity)], world=world)
    assert rcs == [0] * world, "\n".join(outs)
    assert "PARTITION OBSERVABLES OK" in outs[0], outs[0]


def test_three_subdomain_driver_series():
    """The astrocyte driver's set-up (ECS + neuron + glia, two membrane models, pulsed ECS source) on an RCB partition,
    with points and membrane points in both cells."""
    rcs, outs = run_ranks(TOOL, ["--family", "astro", "--kind", "tet", "--method", "rcb", "--steps", "4", "--every", "1",
                                 "--capacity", "3"])
    assert rcs == [0, 0], "\n".join(outs)
    assert "PARTITION OBSERVABLES OK" in outs[0], outs[0]


def test_partitioned_series_with_distributed_solves():
    """Whole time steps with the distributed Krylov solves: the series agree with the single-rank run to the solver
    tolerance of check_partition_steps.py --solves."""
    rcs, outs = run_ranks(TOOL, ["--kind", "tet", "--method", "rcb", "--steps", "4", "--every", "1", "--solves"])
    assert rcs == [0, 0], "\n".join(outs)
    assert "PARTITION OBSERVABLES OK" in outs[0], outs[0]


def test_two_partitioned_runs_are_bit_identical():
    rcs, outs = run_ranks(TOOL, ["--kind", "tet", "--method", "rcb", "--steps", "4", "--every", "1", "--repeat"])
    assert rcs == [0, 0], "\n".join(outs)
    assert "two partitioned runs give identical series" in outs[0] and "PARTITION OBSERVABLES OK" in outs[0], outs[0]


def test_library_rccl_record_matches_unpartitioned_rows():
    """One rank, nccl backend: the halo runs on the library's communicator and every record sums the exchange buffer
    with knpemi_comm_allreduce; the rows equal those of the plain observe bit for bit."""
    rcs, outs = run_ranks(TOOL, ["--kind", "tet", "--method", "rcb", "--steps", "4", "--every", "1", "--capacity", "3",
                                 "--rccl"], world=1)
    assert rcs == [0], outs[0]
    assert "library RCCL" in outs[0] and "PARTITION OBSERVABLES OK" in outs[0], outs[0]
