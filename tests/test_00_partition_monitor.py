"""Membrane monitors and the maps' series on a cell-partitioned problem (DeviceStepper.monitor(halo=...), track(halo=...)),
rehearsed on one card: fresh child processes (gloo, all on GPU 0) record the two-cell-type box -- a shipped
Hodgkin-Huxley slot and a plug-in slot whose monitor runs through hipRTC -- and rank 0 compares with one rank holding the
whole mesh: every rank the same series bit for bit; points, minima and maxima bit for bit, integrals and averages within
the derived bound n 2^-52 sum |w_q v_q|; the union of the ranks' owned per-dof values the single-rank values bit for bit;
the n column of a maps series exact and its measure within the same kind of bound (tools/check_partition_monitor.py).

Runs early (file name): the children are started before this process has touched the GPU.
"""
import pytest

from partition_ranks import run_ranks

TOOL = "check_partition_monitor.py"

pytestmark = pytest.mark.gpu


def _check(rcs, outs, world):
    assert rcs == [0] * world, "\n".join(outs)
    assert "PARTITION MONITOR OK" in outs[0], outs[0]


def test_partitioned_monitors_and_map_series_equal_single_rank_on_an_analytic_state():
    """Tetrahedra, RCB, two ranks, 8 records of an analytic state: both watches with points and every reduction, the K_ecs
    and phi_M series watches of the maps and their per-item maps."""
    rcs, outs = run_ranks(TOOL, ["--kind", "tet", "--method", "rcb", "--records", "8"])
    _check(rcs, outs, 2)
    assert "maps series: largest" in outs[0] and "per-item maps" in outs[0], outs[0]


def test_a_rank_without_a_membrane_dof_of_a_watch_takes_part():
    """Three ranks cut across z: ranks 0 and 2 hold no membrane dof of one of the two cells (no workgroup, no recorded
    facet, the operations' identities in their slots) and still append every row."""
    rcs, outs = run_ranks(TOOL, ["--kind", "tet", "--method", "rcbz", "--records", "3"], world=3)
    _check(rcs, outs, 3)


def test_one_rank_records_a_whole_cell():
    """Two ranks cut across z: rank 0 records every facet of cell 1 (the divisor of its averages is that rank's sum of
    weights plus zeros, formed in another order than the library's own sum), rank 1 holds no dof of it."""
    rcs, outs = run_ranks(TOOL, ["--kind", "tet", "--method", "rcbz", "--records", "3"])
    _check(rcs, outs, 2)


def test_a_rank_without_any_membrane_dof_takes_part():
    """Three ranks, rank 0 with ECS cells away from every membrane only: it launches no record, holds the operations'
    identities in its slots, takes part in every all-reduce and appends every row."""
    rcs, outs = run_ranks(TOOL, ["--kind", "tet", "--method", "far", "--records", "3"], world=3)
    _check(rcs, outs, 3)


def test_partitioned_monitors_equal_single_rank_on_stepped_states():
    """Two ranks, 5 steps of the device-resident stepper (LSODA, no solves: bit-identical fields), a record after each."""
    rcs, outs = run_ranks(TOOL, ["--kind", "tet", "--method", "rcb", "--steps", "5"])
    _check(rcs, outs, 2)
