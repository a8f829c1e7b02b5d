"""Field maps on a cell-partitioned problem (DeviceStepper.track, FieldMaps.maps(halo=...)), rehearsed on one card: fresh
child processes (gloo, all on GPU 0) each push an analytic field at their local coordinates and record it; rank 0 gathers
every rank's owned maps and compares their union, matched by the coordinates, with the maps of one rank holding the whole
mesh -- no item missing or duplicated, every map bit for bit -- and step(halo) refuses a series watch
(tools/check_partition_maps.py).

Runs early (file name): the children are started before this process has touched the GPU.
"""
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "check_partition_maps.py")

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(args, world=2, timeout=420):
    port = _free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, TOOL] + args, env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=timeout)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return [p.returncode for p in procs], outs


def test_partitioned_field_maps_equal_single_rank():
    """Tetrahedra, RCB, two ranks, 8 records of an analytic field on the vertices of the ECS (the solver's c and the
    vertex records), of cell 1 (the eliminated ion) and on its membrane."""
    rcs, outs = _run_ranks(["--kind", "tet", "--method", "rcb", "--records", "8"])
    assert rcs == [0, 0], "\n".join(outs)
    assert "PARTITION MAPS OK" in outs[0], outs[0]
