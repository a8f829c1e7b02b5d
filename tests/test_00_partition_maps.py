"""Field maps on a cell-partitioned problem (DeviceStepper.track, FieldMaps.maps(halo=...)), rehearsed on one card: fresh
child processes (gloo, all on GPU 0) each push an analytic field at their local coordinates and record it; rank 0 gathers
every rank's owned maps and compares their union, matched by the coordinates, with the maps of one rank holding the whole
mesh -- no item missing or duplicated, every map bit for bit -- and step(halo) refuses a series watch
(tools/check_partition_maps.py).

Runs early (file name): the children are started before this process has touched the GPU.
"""
import pytest

from partition_ranks import run_ranks

TOOL = "check_partition_maps.py"

pytestmark = pytest.mark.gpu


def test_partitioned_field_maps_equal_single_rank():
    """Tetrahedra, RCB, two ranks, 8 records of an analytic field on the vertices of the ECS (the solver's c and the
    vertex records), of cell 1 (the eliminated ion) and on its membrane."""
    rcs, outs = run_ranks(TOOL, ["--kind", "tet", "--method", "rcb", "--records", "8"])
    assert rcs == [0, 0], "\n".join(outs)
    assert "PARTITION MAPS OK" in outs[0], outs[0]
