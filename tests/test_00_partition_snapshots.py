"""Field snapshots on a cell-partitioned problem (DeviceStepper.snapshot, Snapshots.select_owned / global_ids), rehearsed
on one card: fresh child processes (gloo, all on GPU 0) each push an analytic field at their local coordinates and
snapshot the items they own; rank 0 gathers every rank's frames and compares their union, ordered by the global numbers,
with the frames of one rank holding the whole mesh -- no item missing or duplicated, every watch bit for bit
(tools/check_partition_snapshots.py).  Each child has its own time limit, and nothing is started after a child fails.

Runs early (file name): the children are started before this process has touched the GPU.
"""
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "check_partition_snapshots.py")

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(args, world=2, timeout=240):
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


def test_partitioned_snapshots_equal_single_rank():
    """Tetrahedra, RCB, two ranks, 3 records of an analytic field on the vertices of the ECS (the solver's c, the vertex
    records as doubles and as floats), of cell 1 (the eliminated ion) and on its membrane."""
    rcs, outs = _run_ranks(["--kind", "tet", "--method", "rcb", "--records", "3"])
    assert rcs == [0, 0], "\n".join(outs)
    assert "PARTITION SNAPSHOTS OK" in outs[0], outs[0]
