"""Field snapshots on a cell-partitioned problem (DeviceStepper.snapshot, Snapshots.select_owned / global_ids), rehearsed
on one card: fresh child processes (gloo, all on GPU 0) each push an analytic field at their local coordinates and
snapshot the items they own; rank 0 gathers every rank's frames and compares their union, ordered by the global numbers,
with the frames of one rank holding the whole mesh -- no item missing or duplicated, every watch bit for bit
(tools/check_partition_snapshots.py).  Each child has its own time limit, and nothing is started after a child fails.

Runs early (file name): the children are started before this process has touched the GPU.
"""
import pytest

from partition_ranks import run_ranks

TOOL = "check_partition_snapshots.py"

pytestmark = pytest.mark.gpu


def test_partitioned_snapshots_equal_single_rank():
    """Tetrahedra, RCB, two ranks, 3 records of an analytic field on the vertices of the ECS (the solver's c, the vertex
    records as doubles and as floats), of cell 1 (the eliminated ion) and on its membrane."""
    rcs, outs = run_ranks(TOOL, ["--kind", "tet", "--method", "rcb", "--records", "3"], timeout=240)
    assert rcs == [0, 0], "\n".join(outs)
    assert "PARTITION SNAPSHOTS OK" in outs[0], outs[0]
