"""CPU tests (gloo ranks) of the ion fluxes and the membrane exchange on a cell-partitioned mesh: every rank builds its
recorded masks from its local mesh (WatchedIons.partition), evaluates its partial row from host fields
(compute_host(recorded=...)), and the rows folded in rank order (recording.combine_partials) equal the single-rank
compute_host of the whole mesh.

Maxima agree bit for bit.  Sums: a cell's (facet's) term is computed from the same vertex values on the rank that records
it and on the single rank, so the two sides add the same n numbers in two orders; each order is off the exact sum by at
most (n - 1) u sum |term| to first order (u = 2^-53), so they differ by at most 2 n 2^-53 sum |term|, with sum |term|
from the single-rank per-item fields times the volumes (areas).  The bound is derived, not measured."""
import contextlib
import io
import os

import numpy as np
import pytest

from partition_ranks import free_port
import test_partition_observables_host as po

DT = 1e-4
U = 2.0 ** -53


def far_partition(mesh, ct):
    """Two ranks by hand: rank 0 owns the ECS cells at least two cell layers away from the membrane (no vertex in common
    with a cell that touches an intracellular vertex), rank 1 the rest.  Rank 0's ghost layer then stops short of the
    cells at the membrane: its local mesh has no intracellular cell and no membrane facet."""
    inside = np.zeros(mesh.num_vertices, bool)
    inside[mesh.cells[ct.dense() > 0].ravel()] = True
    layer1 = inside[mesh.cells].any(axis=1)
    near = np.zeros(mesh.num_vertices, bool)
    near[mesh.cells[layer1].ravel()] = True
    layer2 = near[mesh.cells].any(axis=1)
    return np.where(layer2, 1, 0).astype(np.int32)


def local_setup(kind, method, rank, world, gather):
    if method != "far":
        return po._local_setup(kind, method, rank, world, gather)
    from setup_problem import Setup
    from knpemi.fem.distributed import LocalPart, VertexHalo
    gm, gct, gft = po._global_mesh(kind)
    local = LocalPart(gm, gct, gft, far_partition(gm, gct), rank, world)
    with contextlib.redirect_stdout(io.StringIO()):
        s = Setup(kind, 1 if kind == "2d" else 0, mesh_data=(local.mesh, local.ct, local.ft), build_forms=False)
    halo = VertexHalo(local, s.subdomain_list)
    halo.build(gather)
    return s, halo


def fill_fields(s, scale):
    """The smooth synthetic fields of test_partition_observables_host, plus the channel currents."""
    po.fill_fields(s, scale)
    for tag, sd in s.subdomain_list.items():
        for mm in sd.get("mem_models", []) if tag > 0 else []:
            x = sd["mesh_mem"].x / scale
            for k, f in enumerate(mm["I_ch_k"].values()):
                f.x.array[:] = 1e-2 * po._f(x, 5 + k)


def recorders(s):
    from knpemi import IonFluxes, MembraneExchange
    fl = IonFluxes(s.subdomain_list, s.ion_list, s.physical_parameters)
    for tag in s.subdomain_list:
        fl.watch(tag)
    ex = MembraneExchange(s.subdomain_list, s.ion_list, s.physical_parameters, ft=s.ft)
    for tag in list(s.subdomain_list)[1:]:
        ex.watch(tag)
    return fl, ex


def host_rows(s, fl, ex, rec_fl=None, rec_ex=None):
    """((flux fields, flux row), (exchange fields, exchange row)) of compute_host on the set-up's host fields."""
    tags = list(s.subdomain_list)
    phi = {t: s.phi[t] for t in tags}
    c = {t: s.c[t] for t in tags}
    return (fl.compute_host(phi, c, recorded=rec_fl),
            ex.compute_host(phi, c, phi_M_prev={t: s.phi_M_prev[t] for t in tags[1:]}, dt=DT, recorded=rec_ex))


def sum_abs_terms(fl, ex, g, f_fl, f_ex):
    """{column key: sum over the items of |term|} of every sum column, from the single-rank per-item fields."""
    out = {}
    for tag, (idx, cur) in fl.watched.items():
        vol = fl.volumes(tag)[:, None]
        for k in idx:
            for p in ("diffusive", "drift"):
                out[f"{tag}/{fl.names[k]}/{p}"] = (vol * np.abs(f_fl[tag][f"{fl.names[k]}/{p}"])).sum(axis=0)
        if cur:
            out[f"{tag}/current"] = (vol * np.abs(f_fl[tag]["current"])).sum(axis=0)
    for tag, (idx, cur) in ex.watched.items():
        area = f_ex[tag]["area"]
        for k in idx:
            for p in ("ecs", "ics", "channel"):
                out[f"{tag}/{ex.names[k]}/{p}"] = (area * np.abs(f_ex[tag][f"{ex.names[k]}/{p}"])).sum()
        if cur:
            out[f"{tag}/capacitive"] = (area * np.abs(f_ex[tag]["capacitive"])).sum()
            # the total channel current: its terms are the sums of the ions' per-facet channel integrals
            out[f"{tag}/channel"] = sum(out[f"{tag}/{ex.names[k]}/channel"] for k in range(ex.K))
            out[f"{tag}/area"] = area.sum()
    return out


def _worker(rank, world, port, kind, method, out_dir):
    po._paths()
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    from setup_problem import Setup
    from knpemi.recording import combine_partials

    def gather(obj):
        res = [None] * world
        dist.all_gather_object(res, obj)
        return res
    gm, gct, gft = po._global_mesh(kind)
    scale = np.ptp(gm.x, axis=0)
    h = np.ptp(gm.x[gm.cells], axis=1).min() / 64
    s, halo = local_setup(kind, method, rank, world, gather)
    fill_fields(s, scale)
    fl, ex = recorders(s)
    tab_fl = fl.partition(halo, gather, every=1, capacity=8)
    tab_ex = ex.partition(halo, gather, every=1, capacity=8)
    assert tab_fl["world"] == world and tab_ex["rank"] == rank
    for tag in fl.watched:
        assert tab_fl["recorded"][tag].shape == (fl.n_cells(tag),)
    for tag in ex.watched:
        assert tab_ex["recorded"][tag].shape == (ex.n_facets(tag),)
    if method == "far" and rank == 0:
        assert fl.n_cells(1) == 0 and ex.n_facets(1) == 0 and fl.recorded_mask().shape == (fl.n_cells(0),)
    (_, row_fl), (_, row_ex) = host_rows(s, fl, ex, tab_fl["recorded"], tab_ex["recorded"])
    got_fl = combine_partials(fl, gather(fl.row_vector(row_fl)))
    got_ex = combine_partials(ex, gather(ex.row_vector(row_ex)))
    counted = {}
    for tag in fl.watched:
        m = s.subdomain_list[tag]["mesh_sub"]
        counted[("cell", tag)] = po._key(m.x[m.cells[tab_fl["recorded"][tag]]].mean(axis=1).reshape(-1, gm.gdim), h)
    for tag in ex.watched:
        m = s.subdomain_list[tag]["mesh_mem"]
        counted[("facet", tag)] = po._key(m.x[m.cells[tab_ex["recorded"][tag]]].mean(axis=1).reshape(-1, gm.gdim), h)
    everything = gather(counted)
    if rank == 0:
        with contextlib.redirect_stdout(io.StringIO()):
            g = Setup(kind, 1 if kind == "2d" else 0, mesh_data=(gm, gct, gft), build_forms=False)
        fill_fields(g, scale)
        gfl, gex = recorders(g)
        (f_fl, ref_fl), (f_ex, ref_ex) = host_rows(g, gfl, gex)
        terms = sum_abs_terms(gfl, gex, g, f_fl, f_ex)
        worst = 0.0
        for rec, got, ref, count in ((gfl, got_fl, ref_fl, gfl.n_cells), (gex, got_ex, ref_ex, gex.n_facets)):
            is_max, j = rec.max_columns(), 0
            for key, w in rec.columns():
                a, b = got[j:j + w], np.atleast_1d(np.asarray(ref[key], np.float64))
                if is_max[j]:
                    assert np.array_equal(a, b), (key, a, b)
                else:
                    bound = 2.0 * count(int(key.split("/")[0])) * U * np.atleast_1d(terms[key])
                    assert np.all(bound > 0) and np.all(np.abs(a - b) <= bound), (key, np.abs(a - b), bound)
                    worst = max(worst, float((np.abs(a - b) / bound).max()))
                j += w
        print(kind, method, world, "largest |difference| / bound of a sum column:", worst)
        # every global cell and every global facet is recorded by exactly one rank
        for (what, tag) in counted:
            m = g.subdomain_list[tag]["mesh_sub" if what == "cell" else "mesh_mem"]
            ref_keys = po._key(m.x[m.cells].mean(axis=1), h)
            keys = [k for c in everything for k in c[(what, tag)]]
            assert len(keys) == len(set(keys)) == len(ref_keys) and set(keys) == set(ref_keys), (what, tag)
        open(os.path.join(out_dir, "ok_0"), "w").write("ok")
    dist.barrier()
    dist.destroy_process_group()


# "far": the hand-made partition, on the meshes large enough for it (the 2-D mesh has no cell that far from the membrane)
CASES = [(k, m, w) for k in ("2d", "tet", "hex") for m, w in (("rcb", 2), ("rcb", 3), ("slab", 2))]
CASES += [("tet", "far", 2), ("hex", "far", 2)]


@pytest.mark.parametrize("kind,method,world", CASES)
def test_partial_rows_combine_to_the_single_rank_row(tmp_path, kind, method, world):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(world, free_port(), kind, method, str(tmp_path)), nprocs=world, join=True)
    assert (tmp_path / "ok_0").exists()


def test_mesh_counts():
    """The meshes of the cases above: cells, ECS cells, intracellular cells."""
    po._paths()
    want = {"2d": (496, 256, 240), "tet": (15552, 13440, 2112), "hex": (2592, 2240, 352)}
    for kind, counts in want.items():
        gm, gct, _ = po._global_mesh(kind)
        ct = gct.dense()
        assert (gm.num_cells, int((ct == 0).sum()), int((ct > 0).sum())) == counts, kind
        if (kind, "far", 2) in CASES:
            part = far_partition(gm, gct)
            assert (part == 0).any() and not (ct[part == 0] > 0).any()


def _error_worker(rank, world, port, case, out_dir):
    po._paths()
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    from knpemi import IonFluxes, MembraneExchange

    def gather(obj):
        res = [None] * world
        dist.all_gather_object(res, obj)
        return res
    s, halo = local_setup("2d", "rcb", rank, world, gather)
    every, capacity = 1, 8
    if case.startswith("flux"):
        rec = IonFluxes(s.subdomain_list, s.ion_list, s.physical_parameters)
        rec.watch(0)
        if not (case == "flux_watches" and rank == 1):
            rec.watch(1, ions=["K"] if case == "flux_masks" and rank == 1 else None)
    else:
        rec = MembraneExchange(s.subdomain_list, s.ion_list, s.physical_parameters, ft=s.ft)
        rec.watch(1, current=not (case == "exchange_masks" and rank == 1))
        every = 2 if case == "exchange_every" and rank == 1 else 1
        capacity = 4 if case == "exchange_capacity" and rank == 1 else 8
    try:
        rec.partition(halo, gather, every=every, capacity=capacity)
        msg = "no error"
    except ValueError as exc:
        msg = str(exc)
    open(os.path.join(out_dir, f"msg_{rank}"), "w").write(msg)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case,text", [("flux_watches", "watches of rank 1"), ("flux_masks", "watches of rank 1"),
                                       ("exchange_masks", "watches of rank 1"), ("exchange_every", "every of rank 1"),
                                       ("exchange_capacity", "capacity of rank 1")])
def test_ranks_that_disagree_raise_on_every_rank(tmp_path, case, text):
    import torch.multiprocessing as mp
    mp.spawn(_error_worker, args=(2, free_port(), case, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        msg = (tmp_path / f"msg_{r}").read_text()
        assert text in msg, (r, msg)


def test_recorded_none_is_the_plain_restatement_and_masks_fold():
    """Without a mask compute_host is unchanged; with complementary masks the partial rows fold to the whole, and an
    all-false mask gives zeros, maxima included (a rank without items of a watch)."""
    po._paths()
    from setup_problem import Setup
    from knpemi.recording import combine_partials
    with contextlib.redirect_stdout(io.StringIO()):
        s = Setup("2d", 1, build_forms=False)
    fill_fields(s, np.ptp(s.mesh.x, axis=0))
    fl, ex = recorders(s)
    (f0, r0), (g0, q0) = host_rows(s, fl, ex)
    all_fl = {t: np.ones(fl.n_cells(t), bool) for t in fl.watched}
    all_ex = {t: np.ones(ex.n_facets(t), bool) for t in ex.watched}
    (f1, r1), (g1, q1) = host_rows(s, fl, ex, all_fl, all_ex)
    assert np.array_equal(fl.row_vector(r0), fl.row_vector(r1)) and np.array_equal(ex.row_vector(q0), ex.row_vector(q1))
    for t in fl.watched:
        assert all(np.array_equal(f0[t][k], f1[t][k]) for k in f0[t])
    none_fl = {t: np.zeros(fl.n_cells(t), bool) for t in fl.watched}
    none_ex = {t: np.zeros(ex.n_facets(t), bool) for t in ex.watched}
    (f2, r2), (g2, q2) = host_rows(s, fl, ex, none_fl, none_ex)
    assert not fl.row_vector(r2).any() and not ex.row_vector(q2).any()
    assert all(np.array_equal(f0[t][k], f2[t][k]) for t in fl.watched for k in f0[t])       # the fields ignore the mask
    assert np.array_equal(combine_partials(fl, [fl.row_vector(r2), fl.row_vector(r0)]), fl.row_vector(r0))
    is_max = fl.max_columns()
    assert is_max.sum() == 2 * (fl.K + 1) and is_max.shape == (fl.n_cols,) and not ex.max_columns().any()
    thirds = [host_rows(s, fl, ex, {t: np.arange(fl.n_cells(t)) % 3 == j for t in fl.watched}, all_ex)[0][1]
              for j in range(3)]
    got = combine_partials(fl, [fl.row_vector(r) for r in thirds])
    assert np.array_equal(got[is_max], fl.row_vector(r0)[is_max])
    terms, j = sum_abs_terms(fl, ex, s, f0, g0), 0
    for key, w in fl.columns():
        if not is_max[j]:
            bound = 2.0 * fl.n_cells(int(key.split("/")[0])) * U * terms[key]
            assert np.all(np.abs(got[j:j + w] - fl.row_vector(r0)[j:j + w]) <= bound), key
        j += w
