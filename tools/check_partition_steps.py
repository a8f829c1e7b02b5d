"""Multi-step consistency of the x-slab partition on the GPU (rehearsal with gloo, 2+ ranks on one card):

    torchrun --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 tools/check_partition_steps.py [--no-mem-halo]

Every rank steps its slab of the (32 * world) um box K times with the device-resident stepper (bench flow: no
linear solves) and compares its OWNED membrane fields / ODE states with a single-rank run of the whole box.
"""
import argparse, contextlib, io, os, sys
import numpy as np

import partition_common as pc


def init_fields(s, L_x, scale=1.0, v_rest=-0.0744):
    """Deterministic functions of the coordinates, so every rank and the global run start from the same state.
    scale: coordinate unit (1: metres, 100: the centimetres of the astrocyte driver); v_rest in the driver's unit."""
    for tag in s.subdomain_list:
        x = s.subdomain_list[tag]['mesh_sub'].x
        w = np.sin(2 * np.pi * x[:, 0] / L_x) * np.cos(3e6 / scale * x[:, 1]) * np.cos(2e6 / scale * x[:, 2])
        for k in range(2):
            s.c_prev[tag][k].x.array[:] *= 1.0 + 1e-3 * w * (1 + k)
            s.c[tag][k].x.array[:] = s.c_prev[tag][k].x._a
        rho = s.physical_parameters.get('rho', {})
        rho_term = float(getattr(rho.get(tag, 0.0), 'value', rho.get(tag, 0.0))) * float(rho.get('z', 0.0)) if rho else 0.0
        s.ion_list[-1][f'c_{tag}'].x.array[:] = -(1.0 / s.ion_list[-1]['z']) * (rho_term + sum(
            ion['z'] * f.x._a for ion, f in zip(s.ion_list[:-1], s.c_prev[tag])))
        s.phi[tag].x.array[:] = (v_rest if tag > 0 else 0.0) * (1.0 + 1e-2 * w)


def membrane_models(s):
    """[(tag, model dict)] in the stepper's registration order"""
    return [(tag, mm) for tag, sd in s.subdomain_list.items() if tag > 0 for mm in sd.get('mem_models', [])]


def run(s, K, halo, mem_halo, solves=None, jacobi=False, ode_method="lsoda", ode_substeps=None):
    from knpemi.stepper import DeviceStepper
    from knpemi import _lib as L
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev,
                       device_solves=solves, ode_method=ode_method, ode_substeps=ode_substeps)
    if jacobi:
        st.dp.solver_setup(L.B_EMI, L.PC_JACOBI)
        st.dp.solver_setup(L.B_KNP, L.PC_JACOBI)
    for _, mm in membrane_models(s):
        st.add_membrane_model(mm['ode'], s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
    src = getattr(s, "f_source_K", None)
    if src is not None:          # pulsed ECS source of the astrocyte driver: on from the first step
        s.set_source(s.cfg["delay"])
        st.set_source(0, s.f_source_K.x._a)
    if halo is not None:
        halo.attach(st.dp)
        halo.exchange_bulk()
        halo.exchange_membrane()
        if not mem_halo:
            halo.exchange_membrane = lambda: None
        if solves is not None:
            halo.enable_solves()
    for _ in range(K):
        st.step(halo)
    st.download()
    if halo is not None and getattr(halo, "_hook_error", None) is not None:
        raise halo._hook_error
    # membrane fields of every cellular sub-domain, concatenated in sub-domain order (the order of the halo's keys)
    xs, phiM, states, cur = [], [], [], {}
    for tag, mm in membrane_models(s):
        ode = mm['ode']
        xs.append(np.hstack([ode.dof_locations, np.full((ode.nodes, 1), float(tag))]))
        phiM.append(s.phi_M_prev[tag].x._a.copy())
        st_pad = np.zeros((ode.nodes, 4))
        st_pad[:, :ode.states.shape[1]] = ode.states
        states.append(st_pad)
        for n, f in mm['I_ch_k'].items():
            cur.setdefault("I_" + n, []).append(f.x._a.copy())
    out = dict(x=np.concatenate(xs), phiM=np.concatenate(phiM), states=np.concatenate(states))
    out.update({k: np.concatenate(v) for k, v in cur.items()})
    out["iterations"] = list(getattr(st, "iterations", []))
    # right-hand sides of the last step (they see the ghost membrane dofs through the facets of ghost cells)
    from knpemi import _lib as L
    dp = st.dp
    b_emi, b_knp = dp.rhs(L.B_EMI), dp.rhs(L.B_KNP)
    rows = dict(x=[], b_emi=[], b_knp0=[], b_knp1=[])
    off = koff = 0
    for tag in s.subdomain_list:
        xs = s.subdomain_list[tag]['mesh_sub'].x
        n = len(xs)
        rows["x"].append(np.hstack([xs, np.full((n, 1), float(tag))]))
        rows["b_emi"].append(b_emi[off:off + n])
        rows["b_knp0"].append(b_knp[koff:koff + n])
        rows["b_knp1"].append(b_knp[koff + n:koff + 2 * n])
        off += n
        koff += 2 * n
    out["rows"] = {k: np.concatenate(v) for k, v in rows.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-mem-halo", action="store_true")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--kind", default="tet")
    ap.add_argument("--method", default="slabgen", choices=["slabgen", "slab", "rcb"],
                    help="slabgen: slab meshes generated directly (knpemi.fem.partition); slab / rcb: the general cell "
                         "partitioner of knpemi.fem.distributed on the global mesh")
    ap.add_argument("--solves", action="store_true",
                    help="whole time steps: distributed CG / BiCGStab (halo'd SpMV, all-reduced dots, per-rank AMG) "
                         "against the single-rank solves, to solver tolerance instead of bit for bit")
    ap.add_argument("--resolution", type=int, default=0, help="resolution factor of the idealized 3D geometry")
    ap.add_argument("--rtol", type=float, nargs=2, default=(1e-8, 1e-10), metavar=("EMI", "KNP"),
                    help="relative tolerances of the two solves (the reference's are 1e-5 1e-7)")
    ap.add_argument("--tol", type=float, default=1e-5, help="bound on the relative field differences with --solves")
    ap.add_argument("--jacobi", action="store_true", help="with --solves: Jacobi instead of AMG preconditioning for both systems")
    ap.add_argument("--family", default="idealized", choices=["idealized", "astro"],
                    help="astro: the three-sub-domain driver (ECS + neuron HH + glia Kir4.1/pump, pulsed ECS source) of "
                         "examples/local_astrocyte_depolarization on a general cell partition (rcb / slab)")
    ap.add_argument("--ode-method", default="lsoda", choices=["lsoda", "euler", "rk4", "rush_larsen"],
                    help="membrane integrator of both runs (DeviceStepper(ode_method=...))")
    ap.add_argument("--ode-substeps", type=int, default=None)
    ap.add_argument("--mesh", default="box", choices=["box", "jittered"],
                    help="jittered (with --method rcb / slab, --kind tet): the box with every vertex moved and vertices, cells "
                         "and the vertex order inside the cells shuffled (tests/unstructured_meshes.py: jittered_tet_box)")
    a = ap.parse_args()
    rank, world = pc.start()
    from knpemi.fem.partition import make_slab_problem
    from knpemi.fem import make_mesh_3D
    from setup_problem import Setup
    solves = tuple(a.rtol) if a.solves else None
    astro = a.family == "astro"
    scale, v_rest = (100.0, -70.0) if astro else (1.0, -0.0744)
    if astro:
        sys.path.insert(0, os.path.join(pc.ROOT, "examples", "local_astrocyte_depolarization"))
        import run_stim_duration as rsd
        cfg = dict(rsd.DEFAULTS)
        cfg["mesh"] = dict(kind="box3d", resolution_factor=a.resolution, cell_type="tetrahedron" if a.kind == "tet" else "hexahedron",
                           length=2 * world)
        cfg.update(delay=0.0, pulse_width=1.0, period=10.0, end_time=100.0, x_L=15e-4, x_U=17e-4, y_L=-1.0, y_U=0.2e-4,
                   z_L=-1.0, z_U=0.2e-4)
        if a.method == "slabgen":
            a.method = "slab"
    mesh_data = None
    if a.mesh == "jittered":
        assert not astro and a.kind == "tet" and a.method != "slabgen"
        sys.path.insert(0, os.path.join(pc.ROOT, "tests"))
        from unstructured_meshes import jittered_tet_box
        mesh_data = jittered_tet_box(r=a.resolution, l=2 * world)      # seeded: the same mesh on every rank
    with contextlib.redirect_stdout(io.StringIO()):
        if astro:
            from knpemi.fem.distributed import make_partitioned_astro
            s = make_partitioned_astro(cfg, rank, world, method=a.method)
        elif a.method == "slabgen":
            s = make_slab_problem(a.kind, a.resolution, rank, world, g_syn=10.0)
        else:
            from knpemi.fem.distributed import make_partitioned_problem
            s = make_partitioned_problem(a.kind, a.resolution, rank, world, g_syn=10.0, method=a.method, mesh_data=mesh_data)
    L_x = s.global_length
    init_fields(s, L_x, scale, v_rest)
    loc = run(s, a.steps, s.halo, not a.no_mem_halo, solves, a.jacobi, a.ode_method, a.ode_substeps)
    its_local = loc.pop("iterations")
    rows = loc.pop("rows")
    hx = L_x / (2 * world * 16 * 2 ** a.resolution)
    if a.method == "slabgen":
        lay = s.layout
        plane = np.rint(loc["x"][:, 0] / hx).astype(int)
        own = (plane >= lay.own_lo) & (plane <= lay.own_hi)
        rplane = np.rint(rows["x"][:, 0] / hx).astype(int)
        rown = (rplane >= lay.own_lo) & (rplane <= lay.own_hi)
    else:
        halo = s.halo
        own = np.concatenate([ow == rank for _, (gid, ow, _) in sorted(halo.keys["mem"].items())])
        rown = np.concatenate([ow == rank for _, (gid, ow, _) in sorted(halo.keys["bulk"].items())])
    gathered = pc.gather(({k: v[own] for k, v in loc.items()}, {k: v[rown] for k, v in rows.items()}))
    if rank == 0:
        with contextlib.redirect_stdout(io.StringIO()):
            ctype = {"tet": "tetrahedron", "hex": "hexahedron"}[a.kind]
            if astro:
                g = rsd.Problem(cfg)
            else:
                g = Setup(a.kind, a.resolution, g_syn=10.0,
                          mesh_data=mesh_data or make_mesh_3D(a.resolution, ctype, l=2 * world))
                if mesh_data is not None:
                    import ctypes
                    flags = ctypes.c_int(-1)
                    g.a_emi.dp.lib.knpemi_debug_geometry(g.a_emi.dp.h, ctypes.byref(flags))
                    assert not flags.value & 1, "the jittered mesh must run the general tetrahedron kernels"
        init_fields(g, L_x, scale, v_rest)
        ref = run(g, a.steps, None, True, solves, a.jacobi, a.ode_method, a.ode_substeps)
        its_ref = ref.pop("iterations")
        ref_rows = ref.pop("rows")
        key = lambda x: tuple(np.rint(x / (hx / 64)).astype(np.int64))
        lookup = {key(x): i for i, x in enumerate(ref["x"])}
        rlookup = {key(x): i for i, x in enumerate(ref_rows["x"])}
        worst = {}
        n = nr = 0
        for _, part in gathered:
            idx = np.array([rlookup[key(x)] for x in part["x"]])
            nr += len(idx)
            for k in part:
                if k == "x":
                    continue
                d = np.abs(part[k] - ref_rows[k][idx]).max() / max(np.abs(ref_rows[k]).max(), 1e-300)
                worst[k] = max(worst.get(k, 0.0), d)
        print("matrix rows compared:", nr, "of", len(ref_rows["x"]))
        assert nr == len(ref_rows["x"])
        for part, _ in gathered:
            idx = np.array([lookup[key(x)] for x in part["x"]])
            n += len(idx)
            for k in part:
                if k == "x":
                    continue
                d = np.abs(part[k] - ref[k][idx]).max() / max(np.abs(ref[k]).max(), 1e-300)
                worst[k] = max(worst.get(k, 0.0), d)
        print("membrane dofs compared:", n, "of", len(ref["x"]), "mem halo:", not a.no_mem_halo)
        print("max relative differences:", worst)
        assert n == len(ref["x"])
        if a.solves:
            # distributed Krylov (block-Jacobi AMG over the ranks) vs the single-rank solve, both to rtol 1e-8 / 1e-10
            # (one-level block Jacobi has no global coarse space: its attainable accuracy on the 35:1 cables ends
            # near 1e-9 relative, far below the reference's rtol 1e-5 / 1e-7)
            print("iterations per solve, partitioned:", [it[1] for it in its_local], "single rank:",
                  [it[1] for it in its_ref])
            emi = [it[1] for it in its_local if it[0] == "emi"]
            print("EMI iterations per solve, mean:", sum(emi) / max(len(emi), 1))
            worst.pop("b_emi", None)          # right-hand sides of the LAST step see the solutions through phi_M only
            assert max(worst.values()) < a.tol, worst
        else:
            # owner-computes rows + deterministic kernels: the partitioned run reproduces the single-rank run bit for bit
            assert max(worst.values()) == 0.0, worst
        print(f"ode_method {a.ode_method}" + (f", {a.ode_substeps} sub-steps" if a.ode_substeps else ""))
        print("PARTITION STEPS OK")
    pc.finish()


if __name__ == "__main__":
    main()
