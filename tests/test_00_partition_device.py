"""The x-slab partition on the HIP path (BASELINE.json configs[2] in its stated form, rehearsed on one card): two
fresh child processes (gloo, both on GPU 0) each step their slab with `DeviceStepper(halo)` -- halo pack / unpack
kernels, ghost membrane dofs integrated redundantly -- and rank 0 compares every OWNED membrane field, ODE state and
row of b_emi / b_knp with a single-rank run of the whole box, bit for bit (tools/check_partition_steps.py).

Runs first (file name): the children are started before this process has touched the GPU.
"""
import os
import subprocess
import sys

import pytest

from partition_ranks import ROOT, free_port, run_ranks

TOOL = "check_partition_steps.py"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["tet", "hex"])
@pytest.mark.parametrize("mem_halo", [True, False])
def test_two_rank_device_steps_equal_single_rank_bit_for_bit(kind, mem_halo):
    rcs, outs = run_ranks(TOOL, ["--kind", kind, "--steps", "6"] + ([] if mem_halo else ["--no-mem-halo"]))
    assert rcs == [0, 0], "\n".join(outs)
    assert "PARTITION STEPS OK" in outs[0], outs[0]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,method,world", [("tet", "rcb", 2), ("tet", "rcb", 3), ("hex", "slab", 2)])
def test_general_partition_device_steps_equal_single_rank_bit_for_bit(kind, method, world):
    """The same check with the general cell partitioner (recursive coordinate bisection / layer slabs on the global
    mesh, id-keyed halo: knpemi.fem.distributed), also on three ranks."""
    rcs, outs = run_ranks(TOOL, ["--kind", kind, "--steps", "4", "--method", method], world=world)
    assert rcs == [0] * world, "\n".join(outs)
    assert "PARTITION STEPS OK" in outs[0], outs[0]


@pytest.mark.gpu
def test_jittered_shuffled_tetrahedra_on_two_ranks_equal_single_rank_bit_for_bit():
    """The same check on general tetrahedra: the r = 0 box with every vertex moved by up to 20 % of the smallest spacing and
    vertices, cells and the vertex order inside every cell shuffled (tests/unstructured_meshes.py), cut in two by recursive
    coordinate bisection.  The general row kernels and the strips of knpemi_create see each cell in another position on a
    rank than on the whole mesh; owned rows of both right-hand sides and the owned membrane fields agree bit for bit."""
    rcs, outs = run_ranks(TOOL, ["--kind", "tet", "--steps", "3", "--method", "rcb", "--mesh", "jittered"])
    assert rcs == [0, 0], "\n".join(outs)
    assert "PARTITION STEPS OK" in outs[0], outs[0]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,method", [("tet", "rcb"), ("tet", "slabgen"), ("hex", "slab")])
def test_two_rank_time_steps_with_distributed_solves(kind, method):
    """Whole time steps on a partitioned problem: knpemi_solve_emi / knpemi_solve_knp as distributed solves (halo'd
    SpMV, all-reduced dot products, each rank's AMG V-cycle on its diagonal block) give the fields, membrane
    potentials, currents and ODE states of the single-rank run to solver tolerance (pdeSolver.py:24-35,74-78,99-110
    run the reference's KSP solves on the mesh communicator)."""
    rcs, outs = run_ranks(TOOL, ["--kind", kind, "--steps", "4", "--method", method, "--solves"])
    assert rcs == [0, 0], "\n".join(outs)
    assert "PARTITION STEPS OK" in outs[0], outs[0]


@pytest.mark.gpu
@pytest.mark.parametrize("method,world,solves", [("rcb", 2, False), ("slab", 3, False), ("rcb", 2, True)])
def test_three_subdomain_driver_on_a_cell_partition(method, world, solves):
    """BASELINE configs[4]'s set-up on a partition: ECS + neuron (HH, mV / ms) + glia (Kir4.1 / pump), two membrane
    models, the pulsed ECS source on -- the reference runs this driver under MPI on DOLFINx's cell partition
    (/root/reference/examples/local_astrocyte_depolarization/run_stim_duration.py:127-134,168-211).  Without solves the
    partitioned run reproduces the single-rank run bit for bit (three sub-domain halos, ghost membrane dofs of both
    models integrated redundantly); with the distributed solves to solver tolerance."""
    args = ["--family", "astro", "--kind", "tet", "--steps", "4", "--method", method] + (["--solves"] if solves else [])
    rcs, outs = run_ranks(TOOL, args, world=world)
    assert rcs == [0] * world, "\n".join(outs)
    assert "PARTITION STEPS OK" in outs[0], outs[0]


@pytest.mark.gpu
def test_two_rank_solves_with_jacobi_preconditioning_match_single_rank():
    """KNPEMI_PC_JACOBI on a partitioned problem: the scaled SpMV A (D^-1 p) needs the owners' 1 / a_ii on the ghost
    columns (round-2 advisor finding: ghost rows are identity rows, their local inverse diagonal is 1)."""
    rcs, outs = run_ranks(TOOL, ["--kind", "tet", "--steps", "3", "--method", "rcb", "--solves", "--jacobi"])
    assert rcs == [0, 0], "\n".join(outs)
    assert "PARTITION STEPS OK" in outs[0], outs[0]


@pytest.mark.gpu
def test_coarse_space_of_the_distributed_emi_solve_lowers_the_iteration_count(monkeypatch):
    """knpemi_set_distributed_coarse (hat functions over slices of every rank's sub-domains along the cable) on a cable cut in
    three (BASELINE configs[1] per rank; the global modes along the cable only matter once the cable is long in cells:
    at resolution 0 both counts are equal), solved to the reference's tolerances (pdeSolver.py:9,84: rtol 1e-5, the example drivers pass 1e-7 for KNP;
    the correction removes the smooth error the first iterations spend their time on, at 1e-8 the interface modes of
    the non-overlapping blocks set the count and the gain is 10 %): fewer CG iterations than the block-Jacobi AMG
    alone, fields within what those tolerances leave (I_K is a small remainder of channel and pump currents).  Six steps:
    39, 40, 39, 23, 22, 21 iterations against 54, 55, 62, 49, 49, 42 without the coarse space (piecewise constants over
    the same slices, the round-2 version: 52, 52, 31, 29, 28, 19); one rank needs 11, 11, 11, 9, 8, 7 -- what remains are
    the interface modes of the non-overlapping blocks."""
    import re
    mean = {}
    for off in ("", "1"):
        if off:
            monkeypatch.setenv("KNPEMI_NO_COARSE", "1")
        rcs, outs = run_ranks(TOOL, ["--kind", "tet", "--steps", "6", "--method", "slabgen", "--solves", "--resolution", "1",
                                     "--rtol", "1e-5", "1e-7", "--tol", "1e-2"], world=3)
        assert rcs == [0, 0, 0], "\n".join(outs)
        assert "PARTITION STEPS OK" in outs[0], outs[0]
        mean[off] = float(re.search(r"EMI iterations per solve, mean: ([0-9.]+)", outs[0]).group(1))
    # (end of round 3: 16.8 against 19.3 -- the ranks' hierarchies now end on a dense level of up to 2 048 unknowns and run
    # through the merged transfer operators, which brought both counts down from 30.7 / 51.8 and narrowed the gap)
    assert mean[""] < mean["1"] and mean[""] < 22, mean


@pytest.mark.gpu
@pytest.mark.parametrize("world,cell", [(2, "tetrahedron"), (3, "tetrahedron"), (2, "hexahedron")])
def test_dg_variant_cell_partition_equals_single_rank_bit_for_bit(world, cell):
    """The DG + SIP variant (broken P1 on tetrahedra, broken Q1 on hexahedra) on x-slabs with one ghost-cell layer (knpemi.dg.DGSlab): after three steps (facet-node ODE
    sweep, both assemblies, update, ghost refresh through knpemi_dg_halo_pack/unpack with the ghosts poisoned before
    every exchange) the matrix rows, right-hand sides and fields of the owned cells and the potentials, currents and
    ODE states of the owned membrane nodes equal those of the whole box on one rank, bit for bit."""
    rcs, outs = run_ranks("check_dg_partition.py", ["--steps", "3", "--cell", cell], world=world)
    assert rcs == [0] * world, "\n".join(outs)
    assert "DG PARTITION OK" in outs[0], outs[0]


@pytest.mark.gpu
@pytest.mark.parametrize("cell", ["tetrahedron", "hexahedron"])
def test_dg_variant_distributed_solves_match_single_rank(cell):
    """knpemi_dg_set_distributed (knpemi.dg.DGSlab.enable_solves): CG on the potential system and BiCGStab on the
    concentration systems of the DG variant solved GLOBALLY on two slabs -- owned rows, ghost refresh of every SpMV argument,
    all-reduced dot products, per-rank auxiliary-space AMG -- agree with the single-rank solves of the whole box to solver
    accuracy (the reference runs these KSP solves under MPI)."""
    rcs, outs = run_ranks("check_dg_partition.py", ["--steps", "2", "--cell", cell, "--solves"], world=2)
    assert rcs == [0, 0], "\n".join(outs)
    assert "DG PARTITION OK" in outs[0] and "distributed solves" in outs[0], outs[0]


@pytest.mark.gpu
def test_rccl_halo_transport_rehearsal_on_one_gpu():
    """Real RCCL on one GPU (a world-size-1 group sending the packed halo to itself, tools/check_async_halo.py): the
    stream-ordered exchange through torch.distributed and the library's own transport (knpemi_comm_init / _sendrecv /
    _allreduce) deliver the packed halo without any host synchronisation, over 300 + 5 exchanges; the Krylov solves run
    through the library's own hooks (knpemi_comm_allreduce_hook / knpemi_comm_halo_hook) and solve the same systems."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_async_halo.py")], env=env, capture_output=True,
                       text=True, timeout=420)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "ALL OK" in out, out[-3000:]
    assert out.count("library RCCL exchange") == 5 and "correct: False" not in out, out[-3000:]
    assert "distributed solves through the library's hooks" in out and "WRONG" not in out, out[-3000:]


@pytest.mark.gpu
def test_bench_self_launch_two_ranks_on_one_gpu():
    """`python bench.py --gpus 2` without a launcher (WORLD_SIZE unset): bench.py starts torch.distributed.run itself as a
    child process; rehearsed with both ranks on this one card and gloo as the process-group backend.  The line must carry
    n_gpus = 2, the x-slab partition and a positive value."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(KNPEMI_BENCH_BACKEND="gloo", KNPEMI_BENCH_TRAJ_MIN="8", HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2",
                        "--repeats", "2", "--cpu-steps", "0", "--solve-steps", "0", "--no-dg", "--no-config3"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 2 and out["value"] > 0 and out["config"]["partition"] == "x-slabs", out["config"]
