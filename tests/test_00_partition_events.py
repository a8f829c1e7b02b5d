"""Membrane events on cell-partitioned runs (DeviceStepper.detect with step(halo)), rehearsed on one card: fresh child
processes (gloo, all on GPU 0) each step their part and record the events of cell 1; rank 0 gathers every rank's owned
maps and compares their union, matched by the dof coordinates, with the maps of one rank holding the whole mesh -- no
dof missing or duplicated, every map bit for bit (tools/check_partition_events.py).

Runs early (file name): the children are started before this process has touched the GPU.
"""
import pytest

from partition_ranks import run_ranks

TOOL = "check_partition_events.py"

pytestmark = pytest.mark.gpu


def test_partitioned_maps_equal_single_rank():
    """Tetrahedra, RCB, two ranks, 6 steps without solves: the partitioned steps are bit-identical to the single-rank
    ones (test_00_partition_device), so the maps are too."""
    rcs, outs = run_ranks(TOOL, ["--kind", "tet", "--method", "rcb", "--steps", "6"])
    assert rcs == [0, 0], "\n".join(outs)
    assert "PARTITION EVENTS OK" in outs[0], outs[0]
