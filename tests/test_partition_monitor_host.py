"""CPU tests (gloo ranks) of the membrane monitors and of the maps' series on a cell-partitioned mesh: every rank builds its
table from its local mesh (MembraneMonitor.partition, FieldMaps.partition), evaluates its partial row from host data
(evaluate_partial_host, series_partial_host), and the rows folded in rank order (recording.combine_partials) equal the
single-rank evaluation of the whole mesh (compute_host, record_host).

The problem: ECS + cell 1 (Hodgkin-Huxley) + cell 2 (glial) on the tetrahedral r = 0 box -- the two-cell-type problem of
exchange_cases.three_problem -- with the two cell types stacked in z (axons 1 and 3 are cell 1, axons 2 and 4 cell 2), so
that a cut across z ("rcbz": recursive bisection of the z coordinate alone) leaves the outer ranks without a membrane facet
of one of the cells.  The state is analytic: concentrations, phi_M and the gates are polynomials of the coordinates formed
with multiplications and additions only, so a dof has the same bits on every rank that holds it.

Points, minima and maxima agree bit for bit.  Sums: both sides add the same n terms w_q v_q (a dof's weight is itself a sum
of at most a handful of facet areas, split among the ranks) in two orders, so they differ by at most
n 2^-52 sum_q |w_q v_q| (`sum_bound`, the derivation of test_partition_fluxes_host); an average by that over the sum of
weights plus 2^-52 |average| for the differing bits of the sum of weights.  The bounds are derived, not measured."""
import contextlib
import io
import math
import os

import numpy as np
import pytest

from partition_ranks import free_port
import test_partition_observables_host as po

EPS = 2.0 ** -52
OMEGA = 2.0 * math.pi * 180.0
T0 = 0.7e-3
AXON_TAGS = (1, 2, 1, 2)
INIT = {"Na": (100.7, 12.8), "K": (3.3, 124.2), "Cl": (104.0, 137.0)}
OPS = ("integral", "average", "min", "max")
LEVEL = {"K_ecs": 3.4, "phi_M": -0.06}       # inside the ranges of the analytic fields at every record


def two_type_mesh(length=2):
    from knpemi.fem import make_mesh_3D
    return make_mesh_3D(0, "tetrahedron", l=length, axon_tags=AXON_TAGS)


def cut(mesh, method, world, ct=None):
    """The owner rank of every cell: "rcb" on the centroids, "rcbz" on their z coordinate alone, "slab" along x, "far"
    (needs the cell tags ct) by hand."""
    from knpemi.fem.distributed import rcb_partition, slab_partition
    cent = mesh.x[mesh.cells].mean(axis=1)
    if method == "rcbz":
        return rcb_partition(np.ascontiguousarray(cent[:, 2:]), world)
    if method == "far":      # rank 0: the ECS cells two cell layers away from every membrane; the rest bisected
        from test_partition_fluxes_host import far_partition
        near = far_partition(mesh, ct) == 1
        part = np.zeros(mesh.num_cells, np.int32)
        part[near] = 1 + rcb_partition(cent[near], world - 1)
        return part
    return rcb_partition(cent, world) if method == "rcb" else slab_partition(cent, world)


def build(mesh_data, forms=False, plug_in=False):
    """The two-cell-type problem on the mesh (mesh, ct, ft), with the parameters of exchange_cases.three_problem;
    plug_in: cell 2 carries examples/benchmark/mm_glial.py, which is bound from source and brings its own monitor."""
    from setup_problem import C_M, FARADAY, PSI, load_model
    from knpemi import (create_functions_emi, create_functions_knp, emi_system, knp_system, set_initial_conditions,
                        setup_membrane_model)
    from knpemi.fem import Constant, extract_submesh
    mesh, ct, ft = mesh_data
    glial = load_model("glial")
    if plug_in:
        import importlib.util
        spec = importlib.util.spec_from_file_location(
            "mm_glial_benchmark", os.path.join(po.ROOT, "examples", "benchmark", "mm_glial.py"))
        glial = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(glial)
    dt, models, subs = 1e-4, {1: load_model("hh_si"), 2: glial}, {}
    with contextlib.redirect_stdout(io.StringIO()):
        for t in (0, 1, 2):
            sm, e2p, v2p, _, _ = extract_submesh(mesh, ct, t)
            subs[t] = dict(tag=t, name=f"sub{t}", mesh_sub=sm, sub_to_parent=e2p, sub_vertex_to_parent=v2p)
            if t > 0:
                g, g2p, _, _, _ = extract_submesh(mesh, ft, [t])
                subs[t].update(mesh_mem=g, mem_to_parent=g2p, membrane_tags=[t], ode_models={t: models[t]})
        rho = {'z': -1, **{t: Constant(subs[t]['mesh_sub'], 0.1 * t) for t in subs}}
        pp = {'dt': Constant(mesh, dt), 'F': Constant(mesh, FARADAY), 'psi': Constant(mesh, PSI),
              'C_phi': Constant(mesh, C_M / dt), 'C_M': Constant(mesh, C_M), 'rho': rho}
        Dv = {"Na": 1.33e-9, "K": 1.96e-9, "Cl": 2.03e-9}
        ions = [dict(name=n, z=z, D={t: Constant(None, Dv[n] * (1 + 0.1 * t)) for t in subs},
                     c_init={t: Constant(None, INIT[n][0 if t == 0 else 1]) for t in subs})
                for n, z in (("K", 1.0), ("Cl", -1.0), ("Na", 1.0))]
        phi, phi_M_prev = create_functions_emi(subs, degree=1)
        c, c_prev = create_functions_knp(subs, ions, degree=1)
        set_initial_conditions(ions, subs, c_prev)
        for t in (1, 2):
            subs[t]['mem_models'] = setup_membrane_model({'stimulus': {}, 'stimulus_locator': None}, pp,
                                                         subs[t]['ode_models'], ft, phi_M_prev[t].function_space, ions)
        s = type("S", (), {})()
        s.__dict__.update(mesh=mesh, ct=ct, ft=ft, subdomain_list=subs, ion_list=ions, physical_parameters=pp, dt=dt,
                          phi=phi, phi_M_prev=phi_M_prev, c=c, c_prev=c_prev, entity_maps=[],
                          stim_params={'stimulus': {}, 'stimulus_locator': None})
        if forms:
            s.a_emi, s.p_emi, s.L_emi = emi_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c_prev, dt)
            s.a_knp, s.p_knp, s.L_knp = knp_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c, c_prev, dt)
    return s


def local_problem(gmesh, method, rank, world, gather, forms=False, plug_in=False):
    """(set-up, halo) of one rank of the cut `method` of the global mesh data gmesh."""
    from knpemi.fem.distributed import LocalPart, VertexHalo
    gm, gct, gft = gmesh
    local = LocalPart(gm, gct, gft, cut(gm, method, world, gct), rank, world)
    s = build((local.mesh, local.ct, local.ft), forms, plug_in)
    halo = VertexHalo(local, s.subdomain_list)
    halo.build(gather)
    return s, halo


def shape(x, L_x, t, k):
    """A smooth function of the coordinates x (n, 3) and t in about [-1, 1.5], different for every k; multiplications
    and additions only, the factors of t scalars: the same bits wherever a vertex is held."""
    u = x[:, 0] * (1.0 / L_x)
    v = x[:, 1] * 1.0e6
    w = x[:, 2] * 1.0e6
    g = u * (1.0 - u) * 4.0 + v * w * (0.5 + 0.125 * k)
    q = (u * u) * (1.0 + w) - v * (0.25 + 0.0625 * k)
    return g * math.cos(OMEGA * t + k) + q * math.sin(OMEGA * t + k)


def analytic_state(s, L_x, t):
    """The `state` of MembraneMonitor.compute_host at time t: {"c", "phi_M", "tables"}; the gates of the state tables are
    analytic too (at t = 0: they do not move between the records), every other column is the model's."""
    names = [ion["name"] for ion in s.ion_list]
    c, phi_M, tables = {}, {}, {}
    for tag, sd in s.subdomain_list.items():
        x = np.asarray(sd["mesh_sub"].x, np.float64)
        c[tag] = [INIT[n][0 if tag == 0 else 1] * (1.0 + shape(x, L_x, t, k) * 0.05) for k, n in enumerate(names)]
        if tag > 0:
            xm = np.asarray(sd["mesh_mem"].x, np.float64)
            phi_M[tag] = shape(xm, L_x, t, 4 + tag) * 0.01 + (-0.07)
            for j, mm in enumerate(sd["mem_models"]):
                ode = mm["ode"]
                st, pa = np.array(ode.states, np.float64), np.array(ode.parameters, np.float64)
                for col in range(st.shape[1]):
                    if col != ode.V_index:
                        st[:, col] = shape(xm, L_x, 0.0, 7 + col) * 0.2 + 0.4
                tables[(tag, j)] = (st, pa)
    return dict(c=c, phi_M=phi_M, tables=tables)


def membrane_points(gs):
    """{name: (tag, x)}: two points per cell inside facets of the global membrane meshes, one of them in the middle."""
    out = {}
    for tag in (1, 2):
        mem = gs.subdomain_list[tag]["mesh_mem"]
        cells = np.asarray(mem.cells)
        for j, name in ((3, f"a{tag}"), (cells.shape[0] // 2, f"b{tag}")):
            X = np.asarray(mem.x)[cells[j]]
            w = np.array([0.5, 0.3, 0.2])
            out[name] = (tag, w @ X)
    return out


def define(mon, points, quantities=None):
    """Both cells watched (all quantities of the first, those named for the second), the points, every reduction."""
    mon.watch(1)
    mon.watch(2, quantities=quantities)
    for name, (tag, x) in points.items():
        mon.point(name, tag, x)
    for tag in (1, 2):
        for op in OPS:
            mon.reduce(f"{op}{tag}", tag, op=op)
    return mon


def sum_bound(mon, values, weights, wsum):
    """{column key: bound on |partitioned - single|} of the integral and average columns of one record, from the
    single-rank per-dof values: n 2^-52 sum_q |w_q v_q| over the n dofs with w_q > 0, for an average divided by the sum
    of weights plus 2^-52 |average|."""
    from knpemi import _lib as L
    out = {}
    for ckey, kind, key, i, _ in mon._cols:
        if kind not in (L.MON_INTEGRAL, L.MON_AVERAGE):
            continue
        w = weights[key]
        on = w > 0.0
        v = values[key][mon.names(*key)[i]]
        b = int(on.sum()) * EPS * float(np.abs(w[on] * v[on]).sum())
        if kind == L.MON_AVERAGE:
            b = b / wsum[key] + EPS * abs(float(np.sum(w[on] * v[on])) / wsum[key])
        out[ckey] = b
    return out


def compare_row(mon, got, ref, bounds):
    """Points, minima and maxima bit for bit, sums within `bounds`; returns the largest |difference| / bound."""
    worst = 0.0
    for c, (ckey, *_) in enumerate(mon._cols):
        if ckey in bounds:
            assert abs(got[c] - ref[ckey]) <= bounds[ckey], (ckey, got[c], ref[ckey], bounds[ckey])
            if bounds[ckey] > 0.0:      # (a quantity that is zero everywhere, the stimulus conductance: 0 <= 0)
                worst = max(worst, abs(got[c] - ref[ckey]) / bounds[ckey])
        else:
            assert got[c] == ref[ckey], (ckey, got[c], ref[ckey])
    return worst


def series_maps(s):
    from knpemi import FieldMaps
    fm = FieldMaps(s.subdomain_list, s.ion_list)
    fm.watch("K_ecs", "c", tag=0, ion="K", threshold=LEVEL["K_ecs"], series=True)
    fm.watch("phi_M", "phi_M", tag=2, threshold=LEVEL["phi_M"], series=True)
    return fm


def _gather(world):
    import torch.distributed as dist

    def gather(obj):
        res = [None] * world
        dist.all_gather_object(res, obj)
        return res
    return gather


def _worker(rank, world, port, method, out_dir):
    po._paths()
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    from knpemi import MembraneMonitor
    from knpemi import _lib as L
    from knpemi.recording import combine_partials
    gather = _gather(world)
    gmesh = two_type_mesh()
    gm = gmesh[0]
    L_x = float(np.ptp(gm.x[:, 0]))
    h = np.ptp(gm.x[gm.cells], axis=1).min() / 64
    g = build(gmesh)
    points = membrane_points(g)
    s, halo = local_problem(gmesh, method, rank, world, gather)
    mon = define(MembraneMonitor(s.subdomain_list, s.ion_list, ft=s.ft, partitioned=True), points)
    tab = mon.partition(halo, gather, every=1, capacity=8)
    assert tab["world"] == world and tab["rank"] == rank
    assert all(np.array_equal(mon.weights(*key, halo=halo), tab["weights"][key]) for key in mon.watched)
    state = analytic_state(s, L_x, T0)
    rows = gather(mon.evaluate_partial_host(T0, state))
    got = combine_partials(mon, rows)
    mine = {}
    for key in mon.watched:
        mem = s.subdomain_list[key[0]]["mesh_mem"]
        rec = tab["recorded"][key[0]]
        cent = np.asarray(mem.x)[np.asarray(mem.cells)[rec]].mean(axis=1).reshape(-1, 3)
        mine[key] = dict(facets=po._key(cent, h), w=dict(zip(po._key(np.asarray(mem.x).reshape(-1, 3), h), tab["weights"][key])),
                         n_recorded=int(rec.sum()), n_local=int(rec.shape[0]))
    everything = gather((mine, tab["taker"], [len(q) for _, _, q, _ in mon._points]))
    # a NaN in one rank's minimum (maximum) reaches the folded row, whichever rank it comes from
    kinds = [kind for _, kind, *_ in mon._cols]
    for r in (0, world - 1):
        for kind in (L.MON_MIN, L.MON_MAX_OP):
            bad = [row.copy() for row in rows]
            c = kinds.index(kind)
            bad[r][c] = np.nan
            folded = combine_partials(mon, bad)
            assert np.isnan(folded[c]) and np.array_equal(np.delete(folded, c), np.delete(got, c))
    if rank == 0:
        gmon = define(MembraneMonitor(g.subdomain_list, g.ion_list, ft=g.ft), points)
        values, ref = gmon.compute_host(T0, analytic_state(g, L_x, T0))
        assert [k for k, *_ in gmon._cols] == [k for k, *_ in mon._cols]
        wg = {key: gmon.weights(*key) for key in gmon.watched}
        worst = compare_row(mon, got, ref, sum_bound(gmon, values, wg, {k: float(w.sum()) for k, w in wg.items()}))
        print("monitors", method, world, "largest |difference| / bound of a sum column:", worst)
        empty = whole = none = 0
        for key in gmon.watched:
            mem = g.subdomain_list[key[0]]["mesh_mem"]
            # every facet is recorded once
            ref_keys = po._key(np.asarray(mem.x)[np.asarray(mem.cells)].mean(axis=1), h)
            keys = [k for m, _, _ in everything for k in m[key]["facets"]]
            assert len(keys) == len(set(keys)) == len(ref_keys) and set(keys) == set(ref_keys), key
            # the rank weights sum over the ranks to the single-rank weights
            tot = dict.fromkeys(po._key(np.asarray(mem.x), h), 0.0)
            for m, _, _ in everything:
                for k, v in m[key]["w"].items():
                    tot[k] += v
            wsum = np.array([tot[k] for k in po._key(np.asarray(mem.x), h)])
            assert np.abs(wsum - wg[key]).max() <= 4 * world * EPS * wg[key].sum(), key
            assert abs(tab["wsum"][key] - wg[key].sum()) <= 4 * world * EPS * wg[key].sum(), key
            empty += sum(m[key]["n_recorded"] == 0 for m, _, _ in everything)
            whole += sum(m[key]["n_recorded"] == len(ref_keys) for m, _, _ in everything)
        none = sum(all(m[key]["n_local"] == 0 for key in gmon.watched) for m, _, _ in everything)
        # every point lands on one rank: the taker holds its dofs, nobody else does
        for p in range(len(mon._points)):
            assert [r for r, (_, _, nq) in enumerate(everything) if nq[p] > 0] == [everything[0][1][p]]
        with open(os.path.join(out_dir, "ok_0"), "w") as f:
            f.write(f"{empty} {whole} {none}")
    dist.barrier()
    dist.destroy_process_group()


# ("rcbz", 3): ranks 0 and 2 hold no membrane facet of cell 2 and of cell 1; ("rcbz", 2): rank 0 records every facet of
# cell 1, rank 1 holds none of it; ("far", 3): rank 0 holds no membrane facet at all
CASES = [("rcb", 2), ("rcb", 3), ("rcbz", 3), ("rcbz", 2), ("far", 3)]


@pytest.mark.parametrize("method,world", CASES)
def test_partial_rows_combine_to_the_single_rank_row(tmp_path, hip_lib, method, world):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(world, free_port(), method, str(tmp_path)), nprocs=world, join=True)
    empty, whole, none = map(int, (tmp_path / "ok_0").read_text().split())
    if method == "rcbz":      # a rank without a recorded facet of a watch
        assert empty >= 1, empty
    if (method, world) == ("rcbz", 2):      # one rank records a whole watched cell
        assert whole >= 1, whole
    if method == "far":      # a rank without a membrane facet of any watch
        assert none == 1 and empty >= 2, (none, empty)


def test_the_z_cut_leaves_ranks_without_a_cell():
    """The cut of ("rcbz", 3), read off the global mesh: rank 0 owns no vertex of a cell-2 membrane facet and its ghost
    layer holds none, rank 2 none of cell 1."""
    po._paths()
    gm, gct, gft = two_type_mesh()
    part = cut(gm, "rcbz", 3)
    ct = gct.dense()
    for rank, tag in ((0, 2), (2, 1)):
        mine = np.zeros(gm.num_vertices, bool)
        mine[gm.cells[part == rank].ravel()] = True
        local = mine[gm.cells].any(axis=1)            # the rank's cells and its ghost layer
        assert local.any() and not (ct[local] == tag).any(), (rank, tag)


def _series_worker(rank, world, port, method, out_dir):
    po._paths()
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    from knpemi.recording import combine_partials
    gather = _gather(world)
    gmesh = two_type_mesh()
    L_x = float(np.ptp(gmesh[0].x[:, 0]))
    s, halo = local_problem(gmesh, method, rank, world, gather)
    fm = series_maps(s)
    tab = fm.partition(halo, gather, every=1, capacity=8)
    assert set(tab["weights"]) == set(tab["owned"]) == {"K_ecs", "phi_M"}
    state = analytic_state(s, L_x, T0)
    c = {t: state["c"][t][:2] for t in state["c"]}
    rows = gather(fm.series_partial_host(None, c, state["phi_M"]))
    got = combine_partials(fm, rows)
    owned = gather({n: int(o.sum()) for n, o in tab["owned"].items()})
    if rank == 0:
        g = build(gmesh)
        gfm = series_maps(g)
        gstate = analytic_state(g, L_x, T0)
        ref = gfm.record_host(T0, None, {t: gstate["c"][t][:2] for t in gstate["c"]}, gstate["phi_M"])
        assert 0 < ref[1] < gfm.watches["K_ecs"].n and 0 < ref[3] < gfm.watches["phi_M"].n, ref      # the levels separate
        for j, name in enumerate(("K_ecs", "phi_M")):
            w = gfm.watches[name]
            assert sum(o[name] for o in owned) == w.n                                                # every item owned once
            assert got[2 * j + 1] == ref[2 * j + 1], (name, got, ref)                                 # n: exact
            v = gstate["c"][0][0] if name == "K_ecs" else gstate["phi_M"][2]
            beyond = v >= LEVEL[name]
            assert beyond.sum() == ref[2 * j + 1]
            bound = int(beyond.sum()) * EPS * float(w.w[beyond].sum())      # n terms w_q, the items beyond the level
            assert abs(got[2 * j] - ref[2 * j]) <= bound, (name, got, ref, bound)
        with open(os.path.join(out_dir, "ok_0"), "w") as f:
            f.write("ok")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("method,world", [("rcb", 2), ("rcbz", 3), ("far", 3)])
def test_series_partials_combine_to_the_single_rank_row(tmp_path, hip_lib, method, world):
    import torch.multiprocessing as mp
    mp.spawn(_series_worker, args=(world, free_port(), method, str(tmp_path)), nprocs=world, join=True)
    assert (tmp_path / "ok_0").exists()


def _error_worker(rank, world, port, case, out_dir):
    po._paths()
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    from knpemi import MembraneMonitor
    gather = _gather(world)
    gmesh = two_type_mesh()
    points = membrane_points(build(gmesh))
    s, halo = local_problem(gmesh, "rcb", rank, world, gather)
    odd = rank == 1
    try:
        if case.startswith("maps"):
            fm = series_maps(s)
            if case == "maps_watches" and odd:
                fm.watch("extra", "phi", tag=0, stats=("peak",))
            fm.partition(halo, gather, every=2 if case == "maps_every" and odd else 1, capacity=8)
        else:
            mon = MembraneMonitor(s.subdomain_list, s.ion_list, ft=s.ft, partitioned=True)
            define(mon, points, quantities=("E_K",) if case == "watches" and odd else None)
            if case == "columns" and odd:
                mon.reduce("extra", 1, op="max", quantities=("E_K",))
            if case == "outside":
                mon.point("far", 1, [1.0, 1.0, 1.0])
            mon.partition(halo, gather, every=2 if case == "every" and odd else 1, capacity=4 if case == "capacity" and odd else 8)
        msg = "no error"
    except ValueError as exc:
        msg = str(exc)
    with open(os.path.join(out_dir, f"msg_{rank}"), "w") as f:
        f.write(msg)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case,text", [("watches", "watches of rank 1"), ("columns", "columns of rank 1"),
                                       ("every", "every of rank 1"), ("capacity", "capacity of rank 1"),
                                       ("outside", "is not on the membrane of model 0 of cell 1 on any rank"),
                                       ("maps_watches", "watches of rank 1"), ("maps_every", "every of rank 1")])
def test_mismatched_definitions_raise_on_every_rank(tmp_path, hip_lib, case, text):
    import torch.multiprocessing as mp
    mp.spawn(_error_worker, args=(2, free_port(), case, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        msg = (tmp_path / f"msg_{r}").read_text()
        assert text in msg, (r, msg)


def test_the_fold_keeps_a_nan_and_divides_the_averages():
    """recording.combine_partials with a recorder's own folds: minimum and maximum keep a NaN of either side, as mon_min /
    mon_max of the record kernel do, start from +-inf, and only sums are divided."""
    po._paths()
    from knpemi.recording import FOLD_MAX, FOLD_MIN, FOLD_SUM, combine_partials

    class Rec:
        def column_folds(self):
            return [FOLD_MIN, FOLD_MAX, FOLD_SUM, FOLD_MIN, FOLD_MAX], [1.0, 1.0, 4.0, 1.0, 1.0]
    nan, inf = np.nan, np.inf
    out = combine_partials(Rec(), [[nan, -3.0, 1.0, inf, -inf], [1.0, nan, 2.0, -2.0, -5.0], [0.5, 7.0, 3.0, inf, -inf]])
    assert np.isnan(out[0]) and np.isnan(out[1]) and out[2] == 1.5 and out[3] == -2.0 and out[4] == -5.0
    out = combine_partials(Rec(), [[1.0, 2.0, 0.0, 0.0, 0.0], [0.5, nan, 0.0, nan, 0.0]])
    assert out[0] == 0.5 and np.isnan(out[1]) and np.isnan(out[3])


def test_a_partitioned_monitor_defers_points_and_empty_reductions(hip_lib):
    """A partitioned rank may hold neither a point nor a facet that carries the model: the definitions do not look."""
    po._paths()
    from knpemi import MembraneMonitor
    g = build(two_type_mesh())
    mon = MembraneMonitor(g.subdomain_list, g.ion_list, ft=g.ft, partitioned=True)
    mon.watch(1)
    mon.point("far", 1, [1.0, 1.0, 1.0])
    assert mon._points[0][2].size == 0 and mon.columns()[0][0].startswith("far/")
    plain = MembraneMonitor(g.subdomain_list, g.ion_list, ft=g.ft)
    plain.watch(1)
    with pytest.raises(ValueError):
        plain.point("far", 1, [1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="partitioned=True"):
        plain.partition(None)
