"""Observables on a cell-partitioned run against a single-rank run of the whole mesh (rehearsal with gloo, 2+ ranks on
one card; started by tests/test_00_partition_observables.py):

    torchrun --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29534 tools/check_partition_observables.py \\
        --kind tet --method rcb --every 1 --capacity 4

Every rank steps its part with the device-resident stepper (as tools/check_partition_steps.py) and records the same
observables through `DeviceStepper.observe(obs, halo=halo)`; every rank must hold the same series, and rank 0 compares
it with `DeviceStepper.observe` on one rank holding the whole mesh: points, minima and maxima bit for bit, sums within
1e-13 of sum |w u| / denom (to --tol with --solves), the times equal.  --repeat: a second partitioned run from the same
start (DeviceStepper.reset) must give the identical series.  --rccl: one rank, backend nccl, the halo on the library's
communicator: the record goes through knpemi_comm_allreduce and the rows must equal the non-partitioned rows bit for bit.
"""
import argparse, contextlib, io, os, sys
import numpy as np

import partition_common as pc

from check_partition_steps import init_fields, membrane_models  # noqa: E402

# ECS, ICS of cell 1 and membrane of cell 1 (axon 1 of make_mesh_3D), as in tests/test_observables_gpu.py; cell 2 of
# the astrocyte driver is axon 4 (axon_tags (1, 2, 1, 2), y in [0.2, 0.4], z in [0.5, 0.7] um)
POINTS = dict(ECS=[16.1e-6, 0.45e-6, 0.13e-6], ICS=[16.1e-6, 0.31e-6, 0.27e-6], mem=[16.1e-6, 0.4e-6, 0.33e-6],
              ICS2=[16.1e-6, 0.31e-6, 0.61e-6], mem2=[16.1e-6, 0.33e-6, 0.5e-6])


def define(obs, scale, cells, bpoint):
    """The observables of tests/test_observables_gpu.py::_observables, plus a point on a rank boundary."""
    P = {k: np.array(v) * scale for k, v in POINTS.items()}
    obs.point("ECS", tag=0, x=P["ECS"])
    obs.point("ICS", tag=1, x=P["ICS"])
    obs.membrane_point("mem", tag=1, x=P["mem"])
    obs.point("cut", tag=0, x=bpoint)
    obs.reduce("K_ecs_max", "c", ion="K", tag=0, op="max")
    obs.reduce("Na_ecs_min", "c", ion="Na", tag=0, op="min")
    obs.reduce("phi_ecs_int", "phi", tag=0, op="integral")
    obs.reduce("K_ics_avg", "c", ion="K", tag=1, op="average")
    for t in cells:
        obs.reduce(f"phi_M_{t}", "phi_M", tag=t, op="nodal_mean")
        obs.reduce(f"phi_M_{t}_max", "phi_M", tag=t, op="max")
        obs.reduce(f"phi_M_{t}_int", "phi_M", tag=t, op="integral")
    if 2 in cells:
        obs.point("ICS2", tag=2, x=P["ICS2"])
        obs.membrane_point("mem2", tag=2, x=P["mem2"])
    return obs


def boundary_point(mesh, ct, part):
    """A vertex of the ECS whose cells belong to ranks 0 and 1: a point on the cut between them."""
    nv = mesh.cells.shape[1]
    lo = np.full(mesh.num_vertices, 1 << 30)
    hi = np.full(mesh.num_vertices, -1)
    tag = np.zeros(mesh.num_vertices, np.int64)
    np.minimum.at(lo, mesh.cells.ravel(), np.repeat(part, nv))
    np.maximum.at(hi, mesh.cells.ravel(), np.repeat(part, nv))
    np.maximum.at(tag, mesh.cells.ravel(), np.repeat(ct.dense(), nv))
    ok = np.flatnonzero((lo == 0) & (hi == 1) & (tag == 0))
    return mesh.x[ok[len(ok) // 2]].copy()


def run(s, K, halo, defs, every, capacity, solves, partitioned, repeat=False):
    """Series of K steps with the observables recorded; with repeat also the series of a second run from the start."""
    from knpemi import Observables
    from knpemi.stepper import DeviceStepper
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev,
                       device_solves=solves)
    for _, mm in membrane_models(s):
        st.add_membrane_model(mm['ode'], s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
    src = getattr(s, "f_source_K", None)
    if src is not None:
        s.set_source(s.cfg["delay"])
        st.set_source(0, s.f_source_K.x._a)
    if halo is not None:
        halo.attach(st.dp)
        halo.exchange_bulk()
        halo.exchange_membrane()
        if solves is not None:
            halo.enable_solves()
    obs = defs(Observables(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list, partitioned=partitioned))
    st.observe(obs, every=every, capacity=capacity, halo=halo if partitioned else None)
    out = []
    for _ in range(2 if repeat else 1):
        if out:
            st.reset()
        for _ in range(K):
            st.step(halo)
        out.append(obs.series())
    if halo is not None and getattr(halo, "_hook_error", None) is not None:
        raise halo._hook_error
    return obs, out, st


def compare(obs, got, ref, tol, scale_of):
    from knpemi import _lib as L
    assert list(got) == list(ref), (list(got), list(ref))
    assert np.array_equal(got["t"], ref["t"]), (got["t"], ref["t"])
    worst = {}
    for j, o in enumerate(obs.items):
        a, b = got[o.key], ref[o.key]
        assert a.shape == b.shape and a.shape[0] > 0, o.key
        if tol == 0.0 and (o.op in (L.OBS_MIN, L.OBS_MAX) or o.src[0] == "point"):
            assert np.array_equal(a, b), (o.key, a, b)
            worst[o.key] = 0.0
        else:
            worst[o.key] = float((np.abs(a - b) / scale_of(o, b)).max())
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="tet")
    ap.add_argument("--method", default="rcb", choices=["slabgen", "slab", "rcb"])
    ap.add_argument("--family", default="idealized", choices=["idealized", "astro"])
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--capacity", type=int, default=1024)
    ap.add_argument("--solves", action="store_true", help="distributed device solves (check_partition_steps --solves)")
    ap.add_argument("--rtol", type=float, nargs=2, default=(1e-8, 1e-10), metavar=("EMI", "KNP"))
    ap.add_argument("--tol", type=float, default=1e-5, help="bound on the relative differences with --solves")
    ap.add_argument("--repeat", action="store_true", help="a second partitioned run must give the identical series")
    ap.add_argument("--rccl", action="store_true", help="one rank, nccl backend, the library's own communicator")
    a = ap.parse_args()
    rank, world = pc.start("nccl" if a.rccl else "gloo")
    from knpemi.fem import make_mesh_3D
    from knpemi.fem.distributed import make_partitioned_astro, make_partitioned_problem, rcb_partition, slab_partition
    from knpemi.fem.partition import make_slab_problem
    from setup_problem import Setup
    solves = tuple(a.rtol) if a.solves else None
    astro = a.family == "astro"
    scale, v_rest = (100.0, -70.0) if astro else (1.0, -0.0744)
    cells = (1, 2) if astro else (1,)
    if astro:
        sys.path.insert(0, os.path.join(pc.ROOT, "examples", "local_astrocyte_depolarization"))
        import run_stim_duration as rsd
        cfg = dict(rsd.DEFAULTS)
        cfg["mesh"] = dict(kind="box3d", resolution_factor=0, cell_type="tetrahedron" if a.kind == "tet" else "hexahedron",
                           length=2 * world)
        cfg.update(delay=0.0, pulse_width=1.0, period=10.0, end_time=100.0, x_L=15e-4, x_U=17e-4, y_L=-1.0, y_U=0.2e-4,
                   z_L=-1.0, z_U=0.2e-4)
        gm, gct, gft = rsd.read_mesh(cfg)
    else:
        gm, gct, gft = make_mesh_3D(0, {"tet": "tetrahedron", "hex": "hexahedron"}[a.kind], l=2 * world)
    with contextlib.redirect_stdout(io.StringIO()):
        if astro:
            s = make_partitioned_astro(cfg, rank, world, method=a.method)
        elif a.method == "slabgen":
            s = make_slab_problem(a.kind, 0, rank, world, g_syn=10.0)
        else:
            s = make_partitioned_problem(a.kind, 0, rank, world, g_syn=10.0, method=a.method)
    cent = gm.x[gm.cells].mean(axis=1)
    if world > 1:
        part = rcb_partition(cent, world) if a.method == "rcb" else slab_partition(cent, world)
        bpoint = boundary_point(gm, gct, part)
    else:
        bpoint = np.array(POINTS["ECS"]) * scale + np.array([1e-6, 0.0, 0.0]) * scale
    defs = lambda obs: define(obs, scale, cells, bpoint)       # noqa: E731
    L_x = s.global_length
    init_fields(s, L_x, scale, v_rest)
    obs, series, st = run(s, a.steps, s.halo, defs, a.every, a.capacity, solves, True, a.repeat)
    print(f"rank {rank}: transport {s.halo.mode}, {len(obs.items)} observables, {series[0]['t'].shape[0]} rows",
          flush=True)
    if a.repeat:
        for k in series[0]:
            assert np.array_equal(series[0][k], series[1][k]), ("repeat", k)
        print("two partitioned runs give identical series", flush=True)
    gathered = pc.gather(series[0])
    for r, other in enumerate(gathered):            # every rank holds the same (global) series
        for k in series[0]:
            assert np.array_equal(other[k], series[0][k]), ("rank", r, k)
    if rank == 0:
        with contextlib.redirect_stdout(io.StringIO()):
            if astro:
                g = rsd.Problem(cfg)
            else:
                g = Setup(a.kind, 0, g_syn=10.0, mesh_data=(gm, gct, gft))
        init_fields(g, L_x, scale, v_rest)
        ref_st = {}

        def fields_scale(o, b):
            return np.maximum(ref_st["scale"][o.key], 1e-300)
        gobs, ref, st1 = run(g, a.steps, None, defs, a.every, a.capacity, solves, False)
        # sum |w u| / denom at the last step, from the single-rank fields: the size of the rounding of a sum
        st1.download()
        from knpemi import _lib as L
        ref_st["scale"] = {}
        for o in gobs.items:
            u = gobs._fields(o, g.phi, g.c, g.phi_M_prev)
            sc = np.abs(o.w * u[o.ids]).sum() / abs(o.denom)
            ref_st["scale"][o.key] = sc if o.op == L.OBS_SUM else np.abs(u).max()
        if a.solves:
            worst = compare(gobs, series[0], ref[0], 1.0, lambda o, b: np.maximum(np.abs(b).max(), 1e-300))
            print("max relative differences (distributed solves):", worst)
            assert max(worst.values()) < a.tol, worst
        else:
            worst = compare(gobs, series[0], ref[0], 0.0, fields_scale)
            print("max differences of the sums, relative to sum |w u| / denom:", worst)
            assert max(worst.values()) <= (0.0 if a.rccl else 1e-13), worst
        print("rows compared:", ref[0]["t"].shape[0], "every", a.every, "capacity", a.capacity)
        print("PARTITION OBSERVABLES OK", flush=True)
    pc.finish()


if __name__ == "__main__":
    main()
