"""Ion fluxes and membrane exchange on a cell-partitioned run against a single-rank run of the whole mesh (rehearsal with
gloo, 2+ ranks on one card; started by tests/test_00_partition_fluxes.py):

    torchrun --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29534 tools/check_partition_fluxes.py \\
        --kind tet --method rcb --every 1 --capacity 4

Every rank steps its part with the device-resident stepper (as tools/check_partition_steps.py) with both recorders
attached, fields on: `DeviceStepper.fluxes(fl, halo=halo)` and `DeviceStepper.exchange(ex, halo=halo)`.  Every rank must
hold the same two series bit for bit, and rank 0 compares them with the same recorders on one rank holding the whole mesh:
  * maxima bit for bit;
  * the per-item fields of every recorded item, matched by centroid, bit for bit (each item recorded exactly once);
  * sums within 2 n 2^-53 sum |term|: without solves the partitioned steps are bit-identical to the single-rank ones
    (tests/test_00_partition_device.py), so both sides add the same n terms in two orders, each within
    (n - 1) 2^-53 sum |term| of the exact sum; sum |term| from the single-rank per-item fields of that record times the
    volumes (areas).
--method far: two ranks by hand, rank 0 without an intracellular cell and without a membrane facet.
--solves: distributed device solves; the series agree to --tol, the tolerance of tools/check_partition_steps.py --solves,
which holds the FIELDS of the two runs to tol x the field's largest magnitude.  A column's own magnitude is no scale for
that: several columns cancel (the capacitive current of a closed cell to 1e-9 of its largest term, the integral of a
gradient to its boundary terms).  The exchange columns are held to tol x sum |term| of the same record (single-rank
per-facet means times areas), what the column sums.  A flux is a gradient, which divides a field difference by the cell
size, so the fluxes are held to the field tolerance carried through the formulas (`flux_solve_bounds`).  The mass budget `ex.budget(obs.series())` of the partitioned run, with
partitioned observables, stays within sqrt(n_block) |r_block|_2 + floor x sum_facets |int j dS| with r the true residual
of the SINGLE-RANK KNP solve of that step (tests/test_exchange_gpu.py::test_mass_budget_closes_to_the_residual_of_the_solve).
--repeat: a second partitioned run from the same start (DeviceStepper.reset) must give the identical series.
--rccl: one rank, backend nccl, the halo on the library's communicator: the records go through knpemi_comm_allreduce and
the rows must equal the non-partitioned rows bit for bit.
--cost N: after the run, alternating windows of N partitioned steps with both taps switched off and on; prints the median
ms per step of each as one JSON line.  The difference is two partitioned records per step (launch, all-reduce, combine,
twice) as this rehearsal runs them: with gloo the all-reduce synchronises the stream and goes through the host.
"""
import argparse, contextlib, io, json, os, sys, time
import numpy as np

import torch.distributed as dist

import partition_common as pc
sys.path.insert(0, os.path.join(pc.ROOT, "tests"))

from check_partition_steps import init_fields, membrane_models  # noqa: E402
# the hand-made partition, sum |term| of every sum column and 2^-53: shared with the host test of the same checks
from test_partition_fluxes_host import U, far_partition, sum_abs_terms  # noqa: E402

BUDGET_FLOOR = 5.7e-11      # tests/test_exchange_gpu.py


def recorders(s):
    from knpemi import IonFluxes, MembraneExchange
    fl = IonFluxes(s.subdomain_list, s.ion_list, s.physical_parameters)
    for tag in s.subdomain_list:
        fl.watch(tag)
    ex = MembraneExchange(s.subdomain_list, s.ion_list, s.physical_parameters, ft=s.ft)
    for tag in list(s.subdomain_list)[1:]:
        ex.watch(tag)
    return fl, ex


def run(s, K, halo, every, capacity, solves, partitioned, repeat=False, budget=False):
    """K steps with both recorders attached.  Returns the recorders, per run (flux series, exchange series, the per-item
    fields of every record), the stepper; with budget also the observables and, single rank only, the true residuals
    of the recorded KNP solves."""
    from knpemi import Observables
    from knpemi import _lib as L
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
    fl, ex = recorders(s)
    h = halo if partitioned else None
    st.fluxes(fl, every=every, capacity=capacity, fields=True, halo=h)
    st.exchange(ex, every=every, capacity=capacity, fields=True, halo=h)
    obs, resid = None, []
    if budget:
        obs = Observables(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list, partitioned=partitioned)
        ex.observe_masses(obs)
        st.observe(obs, every=1, halo=h)
        if halo is None:
            solve = st.solve_knp

            def solve_knp(dp):
                solve(dp)
                if (st.k + 1) % every == 0:
                    A, b = dp.csr(L.A_KNP), dp.rhs(L.B_KNP)
                    resid.append(A @ dp.get_solution(L.B_KNP, A.shape[0]) - b)
            st.solve_knp = solve_knp
    out = []
    for _ in range(2 if repeat else 1):
        if out:
            st.reset()
        fields = []
        for k in range(K):
            st.step(halo)
            if (k + 1) % every == 0:      # both recorders have just recorded: the fluxes at the end of this step
                fields.append(({t: fl.fields(t, halo=h) for t in fl.watched}, {t: ex.fields(t, halo=h) for t in ex.watched}))
        out.append((fl.series(), ex.series(), fields))
    if halo is not None and getattr(halo, "_hook_error", None) is not None:
        raise halo._hook_error
    return fl, ex, out, st, obs, resid


def field_magnitudes(s):
    """{tag: (max |phi|, [max |c_k|], [min |c_k|])} of the host fields (c_prev of the solved ions, the eliminated ion's c)."""
    out = {}
    for tag in s.subdomain_list:
        ck = [np.abs(f.x._a) for f in s.c_prev[tag]] + [np.abs(s.ion_list[-1][f"c_{tag}"].x._a)]
        out[tag] = (float(np.abs(s.phi[tag].x._a).max()), [float(c.max()) for c in ck], [float(c.min()) for c in ck])
    return out


def flux_solve_bounds(fl, mags, f_fl, tol):
    """{column key: bound} on the difference of a flux row between two runs whose nodal fields agree to tol x the field's
    largest magnitude, to first order in tol.  With g = E^-1 d and |d_t| <= 2 max |u| for a nodal field u (differences of
    vertex values; on hexahedra 1/4 of eight signed values), a field difference of tol max |u| moves component a of the
    gradient by at most tol max |u| G_a, G_a = 2 sum_t |E^-1[a, t]|.  Hence per cell
        |dJ_diff_a|  <= D tol max |c| G_a
        |dJ_drift_a| <= tol (max |c| / min |c|) |J_drift_a| + |z psi D| max |c| tol max |phi| G_a
    (the centroid value of c moves by at most tol max |c|, and J_drift is proportional to it), the current by
    F sum_k |z_k| of both, a sum column by sum_T vol_T of the cell bounds, and a maximum by the largest norm of a cell's
    bound.  mags: `field_magnitudes`, the larger of the start and the end of the run; f_fl: the single-rank per-cell
    fields of the record."""
    out = {}
    for tag, (idx, cur) in fl.watched.items():
        cells, kind, E, vol = fl._geometry(tag)
        G = 2.0 * np.abs(np.linalg.inv(E)).sum(axis=2)
        phimax, cmax, cmin = mags[tag]
        bi = np.zeros_like(G)
        for k in range(fl.K):
            n, D, z = fl.names[k], fl.D[tag][k], fl.z[k]
            bd = D * tol * cmax[k] * G
            br = tol * (cmax[k] / cmin[k]) * np.abs(f_fl[tag][f"{n}/drift"]) + abs(z * fl.psi * D) * cmax[k] * tol * phimax * G
            bi += fl.F * abs(z) * (bd + br)
            out[f"{tag}/{n}/diffusive"] = (vol[:, None] * bd).sum(axis=0)
            out[f"{tag}/{n}/drift"] = (vol[:, None] * br).sum(axis=0)
            out[f"{tag}/{n}/max"] = np.sqrt(((bd + br) ** 2).sum(axis=1)).max()
        out[f"{tag}/current"] = (vol[:, None] * bi).sum(axis=0)
        out[f"{tag}/current_max"] = np.sqrt((bi ** 2).sum(axis=1)).max()
    return out


def keyed(s, fl, ex, fields, h, gdim):
    """{("cell" | "facet", tag): (centroid keys, {name: values})} of the items this rank records, from the fields of one
    record (with their "recorded" masks; all items when there is none)."""
    out = {}
    for what, rec, f in (("cell", fl, fields[0]), ("facet", ex, fields[1])):
        for tag in rec.watched:
            m = s.subdomain_list[tag]["mesh_sub" if what == "cell" else "mesh_mem"]
            mask = f[tag].get("recorded", np.ones(m.cells.shape[0], bool))
            cent = m.x[m.cells[mask]].mean(axis=1).reshape(-1, gdim)
            keys = [tuple(r) for r in np.rint(cent / h).astype(np.int64)]
            out[(what, tag)] = (keys, {k: v[mask] for k, v in f[tag].items() if k not in ("recorded", "facet")})
    return out


def compare_items(all_keyed, ref_keyed):
    """Every item of the single-rank run is recorded by exactly one rank, with the same bits in every field."""
    n = 0
    for key, (ref_keys, ref_vals) in ref_keyed.items():
        got_keys = [k for part in all_keyed for k in part[key][0]]
        assert len(got_keys) == len(set(got_keys)) == len(ref_keys) and set(got_keys) == set(ref_keys), key
        pos = {k: i for i, k in enumerate(ref_keys)}
        for part in all_keyed:
            keys, vals = part[key]
            if not keys:
                continue
            idx = np.array([pos[k] for k in keys])
            for name, v in vals.items():
                assert np.array_equal(v, ref_vals[name][idx]), (key, name)
        n += len(ref_keys)
    return n


def compare_series(rec, got, ref, count, terms_by_row, tol):
    """Maxima bit for bit and sums within the derived bound (tol None).  With tol, terms_by_row holds per record the scale
    of every column at tolerance 1 (sum |term|, or the bound of `flux_solve_bounds` at tol = 1): the largest difference
    of every column relative to it is printed, and the caller holds the largest of them against tol.  Returns the
    largest ratio to the bound (to the scale)."""
    assert list(got) == list(ref), (list(got), list(ref))
    assert np.array_equal(got["t"], ref["t"]) and got["t"].shape[0] > 0, (got["t"], ref["t"])
    is_max, j, worst = rec.max_columns(), 0, 0.0
    for key, w in rec.columns():
        a, b = got[key].reshape(len(got["t"]), w), ref[key].reshape(len(ref["t"]), w)
        if tol is not None:
            scale = np.array([np.atleast_1d(t[key]) * np.ones(w) for t in terms_by_row])
            ratio = float((np.abs(a - b) / np.maximum(scale, 1e-300)).max())
            print(f"  {key}: {ratio:.3e} of its scale ({float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)):.3e} of "
                  "its own largest magnitude)", flush=True)
            worst = max(worst, ratio)
        elif is_max[j]:
            assert np.array_equal(a, b), (key, a, b)
        else:
            for i in range(a.shape[0]):
                bound = 2.0 * count(int(key.split("/")[0])) * U * np.atleast_1d(terms_by_row[i][key])
                assert np.all(np.abs(a[i] - b[i]) <= bound), (key, i, np.abs(a[i] - b[i]), bound)
                worst = max(worst, float((np.abs(a[i] - b[i]) / np.where(bound > 0, bound, 1.0)).max()))
        j += w
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="tet")
    ap.add_argument("--method", default="rcb", choices=["slabgen", "slab", "rcb", "far"])
    ap.add_argument("--family", default="idealized", choices=["idealized", "astro"])
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--capacity", type=int, default=1024)
    ap.add_argument("--solves", action="store_true", help="distributed device solves (check_partition_steps --solves)")
    ap.add_argument("--rtol", type=float, nargs=2, default=(1e-8, 1e-10), metavar=("EMI", "KNP"))
    ap.add_argument("--tol", type=float, default=1e-5, help="bound on the relative differences with --solves")
    ap.add_argument("--repeat", action="store_true", help="a second partitioned run must give the identical series")
    ap.add_argument("--rccl", action="store_true", help="one rank, nccl backend, the library's own communicator")
    ap.add_argument("--cost", type=int, default=0, metavar="N", help="time windows of N steps with the taps off and on")
    a = ap.parse_args()
    rank, world = pc.start("nccl" if a.rccl else "gloo")
    from knpemi.fem import make_mesh_3D
    from knpemi.fem.distributed import LocalPart, VertexHalo, make_partitioned_astro, make_partitioned_problem
    from knpemi.fem.partition import make_slab_problem
    from setup_problem import Setup
    solves = tuple(a.rtol) if a.solves else None
    astro = a.family == "astro"
    scale, v_rest = (100.0, -70.0) if astro else (1.0, -0.0744)
    gather = pc.gather
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
        elif a.method == "far":
            local = LocalPart(gm, gct, gft, far_partition(gm, gct), rank, world)
            s = Setup(a.kind, 0, g_syn=10.0, mesh_data=(local.mesh, local.ct, local.ft), build_forms=True)
            s.halo = VertexHalo(local, s.subdomain_list)
            s.halo.build(gather)
            s.global_length = 2 * world * 16e-6
        else:
            s = make_partitioned_problem(a.kind, 0, rank, world, g_syn=10.0, method=a.method)
    L_x = s.global_length
    init_fields(s, L_x, scale, v_rest)
    fl, ex, runs, st, obs, _ = run(s, a.steps, s.halo, a.every, a.capacity, solves, True, a.repeat, budget=a.solves)
    ser_fl, ser_ex, fields = runs[0]
    print(f"rank {rank}: transport {s.halo.mode}, {fl.n_cols} + {ex.n_cols} columns, {ser_fl['t'].shape[0]} rows, "
          f"cells {[fl.n_cells(t) for t in fl.watched]}, facets {[ex.n_facets(t) for t in ex.watched]}", flush=True)
    if a.repeat:
        for one, two in zip(runs[0][:2], runs[1][:2]):
            for k in one:
                assert np.array_equal(one[k], two[k]), ("repeat", k)
        print("two partitioned runs give identical series", flush=True)
    for r, other in enumerate(gather((ser_fl, ser_ex))):            # every rank holds the same (global) series
        for mine, theirs in zip((ser_fl, ser_ex), other):
            for k in mine:
                assert np.array_equal(theirs[k], mine[k]), ("rank", r, k)
    h = np.ptp(gm.x[gm.cells], axis=1).min() / 64
    all_keyed = gather(keyed(s, fl, ex, fields[-1], h, gm.gdim))
    bud = ex.budget(obs.series()) if a.solves else None
    if a.cost:
        taps = [st.taps["fluxes"], st.taps["exchange"]]

        def window(on):
            for tap in taps:
                tap.enabled = on
            st.dp.sync()
            dist.barrier()
            t0 = time.perf_counter()
            for _ in range(a.cost):
                st.step(s.halo)
            st.dp.sync()
            return (time.perf_counter() - t0) * 1e3 / a.cost
        window(False), window(True)
        ms = {False: [], True: []}
        for _ in range(5):
            for on in (False, True):
                ms[on].append(window(on))
        print(json.dumps(dict(rank=rank, world=world, steps=a.cost, every=a.every, fields=True,
                              ms_per_step_plain=float(np.median(ms[False])), ms_per_step_recorded=float(np.median(ms[True])),
                              us_per_step_two_records=float(np.median(np.array(ms[True]) - np.array(ms[False])) * 1e3),
                              windows_ms={"plain": ms[False], "recorded": ms[True]})), flush=True)
    if rank == 0:
        with contextlib.redirect_stdout(io.StringIO()):
            if astro:
                g = rsd.Problem(cfg)
            else:
                g = Setup(a.kind, 0, g_syn=10.0, mesh_data=(gm, gct, gft))
        init_fields(g, L_x, scale, v_rest)
        mags0 = field_magnitudes(g)
        gfl, gex, ref, st1, _, resid = run(g, a.steps, None, a.every, a.capacity, solves, False, budget=a.solves)
        ref_fl, ref_ex, ref_fields = ref[0]
        terms = [sum_abs_terms(gfl, gex, g, f[0], f[1]) for f in ref_fields]
        tol = a.tol if a.solves else None
        flux_scale = terms
        if a.solves:      # the scale of a flux column at tolerance 1, from the fields' magnitudes at the start and the end
            st1.download()
            mags1 = field_magnitudes(g)
            mags = {t: (max(mags0[t][0], mags1[t][0]), list(np.maximum(mags0[t][1], mags1[t][1])),
                        list(np.minimum(mags0[t][2], mags1[t][2]))) for t in mags0}
            flux_scale = [flux_solve_bounds(gfl, mags, f[0], 1.0) for f in ref_fields]
        worst = (compare_series(gfl, ser_fl, ref_fl, gfl.n_cells, flux_scale, tol),
                 compare_series(gex, ser_ex, ref_ex, gex.n_facets, terms, tol))
        if a.solves:
            print("max relative differences (distributed solves): fluxes, exchange", worst)
            assert max(worst) < a.tol, worst
            dp = st1.dp
            names = [n for n in gex.names[:-1]]
            assert len(resid) == len(ser_ex["t"]) and set(bud) == {"t"} | {f"{t}/{n}" for t in [0] + list(gex.watched) for n in names}
            checked = 0
            for i, (r, f) in enumerate(zip(resid, ref_fields)):
                if i == 0:      # the first row has no mass at t - dt (the observables record at the ends of the steps)
                    assert all(np.isnan(bud[key][0]) for key in bud if key != "t")
                    continue
                checked += 1
                for k, name in enumerate(names):
                    for tag in [0] + list(gex.watched):
                        sub = dp.sub_index[tag]
                        n = int(dp.n_vert[sub])
                        r_block = r[len(names) * int(dp.voff[sub]) + k * n:][:n]
                        side = "ecs" if tag == 0 else "ics"
                        flux = sum(float((f[1][c]["area"] * np.abs(f[1][c][f"{name}/{side}"])).sum())
                                   for c in (gex.watched if tag == 0 else [tag]))
                        bound = np.sqrt(n) * np.linalg.norm(r_block) + BUDGET_FLOOR * flux
                        defect = bud[f"{tag}/{name}"][i]
                        print("row", i, name, tag, "defect", defect, "bound", bound, "sqrt(n) |r|", bound - BUDGET_FLOOR * flux,
                              flush=True)
                        assert abs(defect) <= bound, (i, name, tag, defect, bound)
            assert checked == a.steps // a.every - 1 and checked > 0
            print("the mass budget of the partitioned run closes to the single-rank residuals")
        else:
            print("largest |difference of a sum| / bound: fluxes, exchange", worst)
            if a.rccl:      # one rank: the same order of summation, the plain recorder's bits
                for got, want in ((ser_fl, ref_fl), (ser_ex, ref_ex)):
                    for k in want:
                        assert np.array_equal(got[k], want[k]), ("rccl", k)
            n = compare_items(all_keyed, keyed(g, gfl, gex, ref_fields[-1], h, gm.gdim))
            print("items matched by centroid, fields bit for bit:", n)
        print("rows compared:", ref_fl["t"].shape[0], "every", a.every, "capacity", a.capacity)
        print("PARTITION FLUXES OK", flush=True)
    pc.finish()


if __name__ == "__main__":
    main()
