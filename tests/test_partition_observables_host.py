"""CPU tests (gloo ranks) of the observables on a cell-partitioned mesh: every rank builds its table from its local mesh
(Observables(partitioned=True).partition), evaluates its partial row from host fields (evaluate_partial_host), and the
rows folded in rank order (combine_partials) equal the single-rank evaluation of the whole mesh (evaluate_host): points,
minima and maxima bit for bit, sums to rounding."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

from partition_ranks import free_port

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

POINTS = {
    2: dict(ECS=[25e-6, 3.5e-6], ICS=[25e-6, 2e-6], mem=[25.3e-6, 3e-6]),
    3: dict(ECS=[16.1e-6, 0.45e-6, 0.13e-6], ICS=[16.1e-6, 0.31e-6, 0.27e-6], mem=[16.1e-6, 0.4e-6, 0.33e-6]),
}


def _paths():
    for p in ("knp-emi-fenics-x_amd", "oracle", "examples/idealized_geometries", "tests"):
        sys.path.insert(0, os.path.join(ROOT, p))


def _global_mesh(kind):
    from knpemi.fem import make_mesh_2D, make_mesh_3D
    if kind == "2d":
        return make_mesh_2D(1)
    return make_mesh_3D(0, {"tet": "tetrahedron", "hex": "hexahedron"}[kind])


def _partition(mesh, method, world):
    from knpemi.fem.distributed import rcb_partition, slab_partition
    cent = mesh.x[mesh.cells].mean(axis=1)
    return rcb_partition(cent, world) if method == "rcb" else slab_partition(cent, world)


def boundary_point(mesh, ct, part):
    """A vertex of the ECS whose cells belong to two ranks (ranks 0 and 1): a point on the cut between them."""
    nv = mesh.cells.shape[1]
    lo = np.full(mesh.num_vertices, 1 << 30)
    hi = np.full(mesh.num_vertices, -1)
    tag = np.zeros(mesh.num_vertices, np.int64)
    np.minimum.at(lo, mesh.cells.ravel(), np.repeat(part, nv))
    np.maximum.at(hi, mesh.cells.ravel(), np.repeat(part, nv))
    np.maximum.at(tag, mesh.cells.ravel(), np.repeat(ct.dense(), nv))
    ok = np.flatnonzero((lo == 0) & (hi == 1) & (tag == 0))
    return mesh.x[ok[len(ok) // 2]]


def define(obs, gdim, bpoint=None):
    """The observables of tests/test_observables_gpu.py::_observables, plus the eliminated ion's reductions."""
    P = POINTS[gdim]
    obs.point("ECS", tag=0, x=P["ECS"])
    obs.point("ICS", tag=1, x=P["ICS"])
    obs.membrane_point("mem", tag=1, x=P["mem"])
    if bpoint is not None:
        obs.point("cut", tag=0, x=bpoint)
    obs.reduce("K_ecs_max", "c", ion="K", tag=0, op="max")
    obs.reduce("Na_ecs_min", "c", ion="Na", tag=0, op="min")
    obs.reduce("Na_ics_max", "c", ion="Na", tag=1, op="max")
    obs.reduce("phi_ecs_int", "phi", tag=0, op="integral")
    obs.reduce("K_ics_avg", "c", ion="K", tag=1, op="average")
    obs.reduce("Na_ecs_mean", "c", ion="Na", tag=0, op="nodal_mean")
    obs.reduce("phi_M_1", "phi_M", tag=1, op="nodal_mean")
    obs.reduce("phi_M_1_max", "phi_M", tag=1, op="max")
    obs.reduce("phi_M_1_min", "phi_M", tag=1, op="min")
    obs.reduce("phi_M_1_int", "phi_M", tag=1, op="integral")
    obs.reduce("phi_M_1_avg", "phi_M", tag=1, op="average")
    return obs


def fill_fields(s, scale):
    """Smooth synthetic fields of the coordinates (the eliminated ion included): the same values at a vertex on every
    rank and in the single-rank set-up.  `scale`: coordinate extent, so that the fields do not depend on the local mesh."""
    for tag, sd in s.subdomain_list.items():
        x = sd["mesh_sub"].x / scale
        s.phi[tag].x.array[:] = 1e-3 * _f(x, 0)
        for k in range(2):
            s.c[tag][k].x.array[:] = 10.0 + _f(x, k + 1)
        s.ion_list[-1][f"c_{tag}"].x.array[:] = 100.0 + _f(x, 3)
        if tag > 0:
            s.phi_M_prev[tag].x.array[:] = -0.07 + 1e-3 * _f(sd["mesh_mem"].x / scale, 4)


def _f(x, k):
    return sum(np.sin((2.0 + d + k) * x[:, d] + 0.3 * k) * (1.0 + 0.1 * d) for d in range(x.shape[1]))


def abs_scale(obs, s):
    """sum |w u| / denom of every observable on the single-rank set-up (the size of the rounding)."""
    row = np.empty(len(obs.items))
    for j, o in enumerate(obs.items):
        u = obs._fields(o, s.phi, s.c, s.phi_M_prev)
        row[j] = np.abs(o.w * u[o.ids]).sum() / abs(o.denom)
    return row


def _key(x, h):
    return [tuple(r) for r in np.rint(x / h).astype(np.int64)]


def _local_setup(kind, method, rank, world, gather):
    from setup_problem import Setup
    from knpemi.fem.distributed import LocalPart, VertexHalo
    if method == "slabgen":
        from knpemi.fem.partition import build_halo, make_slab_layout_and_mesh
        lay, mesh_data = make_slab_layout_and_mesh(kind, 0, rank, world, length=2)
        with contextlib.redirect_stdout(io.StringIO()):
            s = Setup(kind, 0, mesh_data=mesh_data, build_forms=False)
        halo, _ = build_halo(lay, s.subdomain_list, gather)
        return s, halo
    gm, gct, gft = _global_mesh(kind)
    local = LocalPart(gm, gct, gft, _partition(gm, method, world), rank, world)
    with contextlib.redirect_stdout(io.StringIO()):
        s = Setup(kind, 1 if kind == "2d" else 0, mesh_data=(local.mesh, local.ct, local.ft), build_forms=False)
    halo = VertexHalo(local, s.subdomain_list)
    halo.build(gather)
    return s, halo


def _worker(rank, world, port, kind, method, out_dir):
    _paths()
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    from setup_problem import Setup
    from knpemi import Observables
    from knpemi import _lib as L
    from knpemi.fem.probe import integral_weights
    from knpemi.observables import combine_partials

    def gather(obj):
        res = [None] * world
        dist.all_gather_object(res, obj)
        return res
    gm, gct, gft = _global_mesh(kind)
    scale = np.ptp(gm.x, axis=0)
    h = np.ptp(gm.x[gm.cells], axis=1).min() / 64
    s, halo = _local_setup(kind, method, rank, world, gather)
    method_part = "slab" if method == "slabgen" else method
    bpoint = boundary_point(gm, gct, _partition(gm, method_part, world))
    obs = define(Observables(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list, partitioned=True), gm.gdim, bpoint)
    tab = obs.partition(halo, gather, every=1, capacity=8)
    # ownership read off the plans: membrane dofs have the owner of their vertex in the ECS
    own_b, own_m = halo.vertex_owner("bulk"), halo.vertex_owner("mem")
    ecs = s.subdomain_list[0]["mesh_sub"]
    mem = s.subdomain_list[1]["mesh_mem"]
    pos = np.searchsorted(ecs.parent_vertices, mem.parent_vertices)
    assert np.array_equal(own_m[:mem.num_vertices], own_b[pos])
    fill_fields(s, scale)
    part_row = obs.evaluate_partial_host(s.phi, s.c, s.phi_M_prev)
    rows = gather(part_row)
    row = combine_partials(obs, rows)
    # what each rank counts, keyed by coordinates (vertices) and centroids (cells, facets)
    counted = {}
    for key, ow in tab["owner"].items():
        msh = s.subdomain_list[key[1]]["mesh_mem" if key[0] else "mesh_sub"]
        rec = tab["recorded"][key]
        w = integral_weights(msh, rec)
        counted[key] = dict(v=_key(msh.x[ow == rank], h), c=_key(msh.x[msh.cells[rec]].mean(axis=1), h),
                            w=dict(zip(_key(msh.x, h), w)))
    takes = [int(sum(tab["entries"][j][0].shape[0] > 0 for j, o in enumerate(obs.items)
                     if o.src[0] == "point" and o.src[1] == k)) > 0 for k in range(len(obs._points))]
    everything = gather((counted, takes))
    if rank == 0:
        with contextlib.redirect_stdout(io.StringIO()):
            g = Setup(kind, 1 if kind == "2d" else 0, mesh_data=(gm, gct, gft), build_forms=False)
        gobs = define(Observables(gm, gct, gft, g.subdomain_list, g.ion_list), gm.gdim, bpoint)
        fill_fields(g, scale)
        ref = gobs.evaluate_host(g.phi, g.c, g.phi_M_prev)
        sc = abs_scale(gobs, g)
        assert gobs.keys == obs.keys
        for j, o in enumerate(obs.items):
            if o.op in (L.OBS_MIN, L.OBS_MAX) or o.src[0] == "point":
                assert row[j] == ref[j], (o.key, row[j], ref[j])
            else:
                assert abs(row[j] - ref[j]) <= 1e-13 * sc[j], (o.key, abs(row[j] - ref[j]) / sc[j])
        # every global vertex and cell (facet) counted by exactly one rank; the weights of the ranks sum to the global
        for key in counted:
            msh = g.subdomain_list[key[1]]["mesh_mem" if key[0] else "mesh_sub"]
            for what, ref_keys in (("v", _key(msh.x, h)), ("c", _key(msh.x[msh.cells].mean(axis=1), h))):
                got = [k for c, _ in everything for k in c[key][what]]
                assert len(got) == len(set(got)) == len(ref_keys) and set(got) == set(ref_keys), (key, what)
            wg = integral_weights(msh)
            tot = dict.fromkeys(_key(msh.x, h), 0.0)
            for c, _ in everything:
                for k, v in c[key]["w"].items():
                    tot[k] += v
            wsum = np.array([tot[k] for k in _key(msh.x, h)])
            assert np.abs(wsum - wg).max() <= 1e-13 * wg.max(), key
        # each point taken by exactly one rank
        assert all(sum(t[k] for _, t in everything) == 1 for k in range(len(obs._points)))
        open(os.path.join(out_dir, "ok_0"), "w").write("ok")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("kind,method,world", [
    ("tet", "rcb", 2), ("tet", "rcb", 3), ("tet", "rcb", 4), ("tet", "slab", 3), ("tet", "slabgen", 2),
    ("hex", "rcb", 2), ("hex", "slab", 2), ("hex", "slabgen", 4), ("2d", "rcb", 3), ("2d", "slab", 4)])
def test_partial_rows_combine_to_the_single_rank_row(tmp_path, kind, method, world):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(world, free_port(), kind, method, str(tmp_path)), nprocs=world, join=True)
    assert (tmp_path / "ok_0").exists()


def _error_worker(rank, world, port, case, out_dir):
    _paths()
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    from knpemi import Observables

    def gather(obj):
        res = [None] * world
        dist.all_gather_object(res, obj)
        return res
    s, halo = _local_setup("tet", "rcb", rank, world, gather)
    obs = define(Observables(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list, partitioned=True), 3)
    every = 1
    if case == "outside":
        obs.point("far", tag=1, x=[1.0, 1.0, 1.0])
    elif case == "keys" and rank == 1:
        obs.reduce("extra", "phi", tag=0, op="max")
    elif case == "every" and rank == 1:
        every = 2
    try:
        obs.partition(halo, gather, every=every, capacity=8)
        msg = "no error"
    except ValueError as exc:
        msg = str(exc)
    open(os.path.join(out_dir, f"msg_{rank}"), "w").write(msg)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case,text", [("outside", "point [1.0, 1.0, 1.0] is not in sub-domain 1 on any rank"),
                                       ("keys", "keys of rank 1"), ("every", "every of rank 1")])
def test_bad_definitions_raise_on_every_rank(tmp_path, case, text):
    import torch.multiprocessing as mp
    mp.spawn(_error_worker, args=(2, free_port(), case, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        msg = (tmp_path / f"msg_{r}").read_text()
        assert text in msg, (r, msg)


def test_partitioned_definitions_defer_point_location():
    """A partitioned rank may not hold a point: the definition does not locate it (partition does)."""
    _paths()
    from setup_problem import Setup
    from knpemi import Observables
    with contextlib.redirect_stdout(io.StringIO()):
        s = Setup("2d", 1, build_forms=False)
    obs = Observables(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list, partitioned=True)
    obs.point("far", tag=1, x=[1.0, 1.0])
    assert obs.keys[0] == "far/phi" and obs.items[0].ids.size == 0
    with pytest.raises(ValueError, match="not in sub-domain 1"):
        Observables(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list).point("far", tag=1, x=[1.0, 1.0])
