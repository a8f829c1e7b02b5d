"""CPU tests of the field snapshots of a DG run (knpemi/dg_snapshots.py): the numpy restatement `frame_host` on hand-made
fields, the frame layout, the float32 rule, selections and locations, the sinks with the XDMF round trip, and every
refusal that needs no device."""
import os
import re

import numpy as np
import pytest

from knpemi import _lib as L
from knpemi.dg_snapshots import (DGSnapshots, DGXdmfSink, MemorySink, NpzSink, ordered_sum, read_xdmf_series)

IONS = ["Na", "K", "Cl"]


def _mesh(kind="triangle", M=8):
    from knpemi.fem import create_box, create_unit_square
    from knpemi.fem.idealized import _tag
    if kind == "triangle":
        mesh = create_unit_square(None, M, M)
    else:
        mesh = create_box(None, [np.zeros(3), np.ones(3)], (M, M, M), kind)
    ct, ft = _tag(mesh, [([0.25] * mesh.x.shape[1], [0.75] * mesh.x.shape[1])], [1], full_facet_tags=False)
    return mesh, ct, ft


def _snap(kind="triangle", M=8, **kw):
    mesh, ct, ft = _mesh(kind, M)
    return DGSnapshots(mesh, ct, ft, [0, 1], [1], IONS, **kw)


def _fields(s, f):
    """phi = f(x), c_k = (k + 2) f(x) at the broken dofs; phi_M = f at the membrane nodes, I_ch_k = (k + 2) phi_M."""
    X, XM = s.x[s.cells], s.x[s.mem_facets]
    phi, phi_M = f(X), f(XM)
    return dict(phi=phi, c=[(k + 2.0) * phi for k in range(3)], phi_M=phi_M, I_ch=[(k + 2.0) * phi_M for k in range(3)])


@pytest.mark.parametrize("kind,M", [("triangle", 8), ("tetrahedron", 3), ("hexahedron", 3)])
def test_vertex_form_of_a_continuous_function_is_the_function_at_the_vertices(kind, M):
    s = _snap(kind, M)
    s.watch_results(form="vertex")
    s.watch("I", "I_ch", 1, ion="K", form="vertex")
    f = lambda X: np.cos(3.0 * X[..., 0] + 1.0) * np.sin(2.0 * X[..., 1] + 0.5) + X[..., -1] ** 2
    frame = s.frame_host(**_fields(s, f))
    for name in ("phi_0", "phi_1", "Cl_0", "phi_M_1", "I"):
        scale = {"Cl_0": 4.0, "I": 3.0}.get(name, 1.0)
        exact = scale * f(s.locations(name))
        # the coincident dofs hold the same double, up to the rounding of the factor: the mean of n equal numbers is
        # exact up to the n - 1 additions and the division
        assert np.max(np.abs(frame[name] - exact)) <= 16 * np.finfo(float).eps * np.max(np.abs(exact)), name
    # one item per mesh vertex the sub-domain touches, in increasing vertex id
    ids = s.item_ids("phi_1")
    assert np.array_equal(ids, np.unique(s.cells[s.cell_sub == 1])) and np.all(np.diff(ids) > 0)
    assert np.array_equal(s.item_ids("phi_M_1"), np.unique(s.mem_facets))
    # an interface vertex belongs to both sub-domains, and each averages its own cells only
    assert np.intersect1d(s.item_ids("phi_0"), ids).size == np.unique(s.mem_facets).size


@pytest.mark.parametrize("kind,M", [("triangle", 8), ("tetrahedron", 3), ("hexahedron", 3)])
def test_cell_mean_of_a_linear_function_is_its_value_at_the_centroid(kind, M):
    s = _snap(kind, M)
    s.watch("phi", "phi", 0, form="cell_mean")
    s.watch("K", "c", 1, ion="K", form="cell_mean")
    a = np.array([0.7, -1.3, 2.1])[:s.x.shape[1]]
    f = lambda X: 0.25 + X @ a
    frame = s.frame_host(**_fields(s, f))
    cent = s.x[s.cells].mean(axis=1)
    for name, sub, scale in (("phi", 0, 1.0), ("K", 1, 3.0)):
        cells = np.flatnonzero(s.cell_sub == sub)
        assert np.array_equal(s.item_ids(name), cells)
        assert np.allclose(s.locations(name), cent[cells], rtol=0, atol=1e-15)
        assert np.max(np.abs(frame[name] - scale * f(cent[cells]))) < 1e-14
    # the summation order is the local-vertex order, one addition at a time
    v = f(s.x[s.cells])[s.cell_sub == 0]
    acc = v[:, 0].copy()
    for j in range(1, v.shape[1]):
        acc = acc + v[:, j]
    assert np.array_equal(frame["phi"], acc / float(v.shape[1]))


def test_broken_form_is_the_field_in_the_cell_order_of_the_sub_domain():
    s = _snap()
    s.watch_results(form="broken")
    rng = np.random.default_rng(3)
    phi, phi_M = rng.random((s.n_cells, s.nv)), rng.random((s.nmf, s.nf))
    frame = s.frame_host(phi=phi, c=[phi + k for k in range(3)], phi_M=phi_M)
    for sub in (0, 1):
        assert np.array_equal(frame[f"phi_{sub}"], phi[s.cell_sub == sub].ravel())
        assert np.array_equal(frame[f"Cl_{sub}"], (phi + 2)[s.cell_sub == sub].ravel())
        assert np.array_equal(s.locations(f"phi_{sub}"), s.x[s.cells][s.cell_sub == sub].reshape(-1, 2))
    assert np.array_equal(frame["phi_M_1"], phi_M.ravel())
    assert np.array_equal(s.item_ids("phi_M_1"), np.arange(s.nq))


def test_ordered_sum_keeps_the_sign_of_a_lone_negative_zero_and_adds_in_list_order():
    v = np.array([-0.0, 1e16, 1.0, -1e16, 3.0])
    s, cnt = ordered_sum(v, np.array([0, 1, 4, 5]), np.array([0, 1, 2, 3, 4]))
    assert np.signbit(s[0]) and s[0] == 0.0
    assert s[1] == (1e16 + 1.0) + -1e16 and s[1] != 1.0      # not the exact sum: the order of the additions shows
    assert s[2] == 3.0 and np.array_equal(cnt, [1, 3, 1])


def test_high_valence_vertices_are_gathered_with_a_loop():
    from unstructured_meshes import fan_mesh
    mesh, ct, ft = fan_mesh(2)
    s = DGSnapshots(mesh, ct, ft, [0, 1], [1], IONS)
    s.watch("phi", "phi", 0, form="vertex")
    S = s.space(0, "vertex")
    valence = np.diff(S.vptr)
    assert valence.max() >= 12 and valence.min() >= 1
    rng = np.random.default_rng(5)
    phi = rng.standard_normal((s.n_cells, s.nv))
    got = s.frame_host(phi=phi)["phi"]
    flat = phi.ravel()
    for i in (int(np.argmax(valence)), 0, S.n - 1):
        acc = flat[S.vdof[S.vptr[i]]]
        for e in range(S.vptr[i] + 1, S.vptr[i + 1]):
            acc = acc + flat[S.vdof[e]]
        assert got[i] == acc / float(valence[i])
        assert np.all(np.diff(S.vdof[S.vptr[i]:S.vptr[i + 1]]) > 0)
        assert np.all(s.cells.ravel()[S.vdof[S.vptr[i]:S.vptr[i + 1]]] == S.ids[i])


def test_offsets_are_multiples_of_the_alignment_and_the_frame_holds_every_watch():
    s = _snap()
    s.watch_results(form="vertex")
    s.watch("b", "phi", 0, form="broken", dtype="f4")
    s.watch("m", "phi", 1, form="cell_mean", dtype="f4")
    s.watch("st", "state", 1, state=2)
    watches, nbytes = s.layout_host()
    assert [w[0] for w in watches] == list(s.watches)
    end = 0
    for name, dt, off, n in watches:
        assert off % 256 == 0 and off >= end and n == s.locations(name).shape[0]
        end = off + n * np.dtype(dt).itemsize
    assert nbytes % 256 == 0 and nbytes >= end
    spec, space, list_off, lst, sel_space, sel_off, sel_idx = s.table()
    assert spec.shape == (len(watches), 5) and spec.dtype == np.int32 and space.shape[1] == 4
    assert list_off[-1] == lst.shape[0] and sel_space.size == 0
    # every (kind, tag, form) once, in the order of its first watch
    assert len({tuple(r[:3]) for r in space.tolist()}) == space.shape[0] == 6


def test_float32_watches_convert_as_numpy_does():
    """NaN, signed zeros, float32 denormals, ties to even and overflow: `np.float32(v)`, bit for bit."""
    s = _snap()
    s.watch("phi4", "phi", 0, dtype="f4")
    s.watch("phi8", "phi", 0)
    tiny = float(np.finfo(np.float32).tiny)
    special = np.array([np.nan, 0.0, -0.0, tiny / 4, -tiny / 1024, 2.0 ** -149, 2.0 ** -150, 1.5 * 2.0 ** -149,
                        1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 3.5e38, -1e39, np.inf,
                        float(np.finfo(np.float32).max) * (1 + 2.0 ** -25)])
    phi = np.zeros((s.n_cells, s.nv))
    phi.ravel()[:special.size] = special
    frame = s.frame_host(phi=phi)
    assert frame["phi4"].dtype == np.float32 and frame["phi8"].dtype == np.float64
    with np.errstate(over="ignore", invalid="ignore"):
        want = phi[s.cell_sub == 0].ravel().astype(np.float32)
    assert np.array_equal(frame["phi4"].view(np.uint32), want.view(np.uint32))
    got = frame["phi4"][:special.size]            # (cell 0 lies in the ECS: the special values lead the watch)
    assert np.isnan(got[0]) and not np.signbit(got[1]) and np.signbit(got[2]) and got[3] != 0 and got[5] == 2.0 ** -149
    assert got[6] == 0.0 and got[7] == 2.0 ** -148                    # ties go to the even neighbour
    assert got[8] == 1.0 and got[9] == np.float32(1.0 + 2.0 ** -22) and got[10] == np.float32(1.0 + 2.0 ** -23)
    assert np.isinf(got[11]) and got[12] == -np.inf and got[13] == np.inf and got[14] == np.finfo(np.float32).max
    assert np.array_equal(frame["phi8"].view(np.uint64), phi[s.cell_sub == 0].ravel().view(np.uint64))


def test_selections_and_locations():
    s = _snap()
    s.watch_results(form="vertex")
    s.watch("b", "phi", 0, form="broken")
    s.watch("m", "c", 0, ion="K", form="cell_mean")
    s.watch("pm", "phi_M", 1, form="broken")
    lo, hi = (0.0, 0.0), (0.5, 1.0)
    s.select(0, "vertex", box=(lo, hi))
    s.select(0, "broken", indices=[0, 5, 7, 280])
    s.select(0, "cell_mean", box=((0.0, 0.0), (1.0, 0.2)))
    s.select(1, "broken", indices=np.arange(0, s.nq, 3), membrane=True)
    full = _snap()
    full.watch_results(form="vertex")
    full.watch("b", "phi", 0, form="broken")
    full.watch("m", "c", 0, ion="K", form="cell_mean")
    full.watch("pm", "phi_M", 1, form="broken")
    rng = np.random.default_rng(11)
    data = dict(phi=rng.random((s.n_cells, s.nv)), c=[rng.random((s.n_cells, s.nv)) for _ in range(3)],
                phi_M=rng.random((s.nmf, s.nf)))
    a, b = s.frame_host(**data), full.frame_host(**data)
    x = s.locations("phi_0")
    assert x.shape[0] < full.locations("phi_0").shape[0] and np.all((x >= lo) & (x <= hi))
    keep = np.all((full.locations("phi_0") >= lo) & (full.locations("phi_0") <= hi), axis=1)
    for name in ("phi_0", "Na_0", "K_0", "Cl_0"):           # every watch of the space
        assert np.array_equal(a[name], b[name][keep])
    assert np.array_equal(a["phi_1"], b["phi_1"])           # another space: untouched
    assert np.array_equal(a["b"], b["b"][[0, 5, 7, 280]]) and np.array_equal(s.item_ids("b"), full.item_ids("b")[[0, 5, 7, 280]])
    assert np.all(s.locations("m")[:, 1] <= 0.2) and a["m"].shape[0] == s.locations("m").shape[0] < b["m"].shape[0]
    assert np.array_equal(a["pm"], b["pm"][::3]) and np.array_equal(a["phi_M_1"], b["phi_M_1"])
    spec, space, list_off, lst, sel_space, sel_off, sel_idx = s.table()
    assert sel_space.tolist() == [i for i, r in enumerate(space.tolist()) if tuple(r[:3]) in
                                  {(0, 0, L.DG_SNAP_VERTEX), (0, 0, L.DG_SNAP_BROKEN), (0, 0, L.DG_SNAP_CELL_MEAN),
                                   (1, 0, L.DG_SNAP_BROKEN)}]
    assert sel_off[-1] == sel_idx.shape[0] and np.all(np.diff(sel_off) > 0)
    for bad in (dict(indices=[3, 2]), dict(indices=[1, 1]), dict(indices=[-1]), dict(indices=[10 ** 6]), dict(indices=[]),
                dict(box=((2.0, 2.0), (3.0, 3.0))), dict(), dict(box=(lo, hi), indices=[1])):
        with pytest.raises(ValueError):
            s.select(1, "vertex", **bad)
    with pytest.raises(ValueError, match="selection already"):
        s.select(0, "vertex", indices=[1])


def test_sinks_and_the_xdmf_round_trip(tmp_path):
    from knpemi.fem import XDMFFile
    s = _snap(writer="inline")
    s.watch_results(form="vertex")
    s.watch("phi_b", "phi", 0, form="broken")
    mem = MemorySink()
    for sink in (mem, NpzSink(str(tmp_path), compressed=False), DGXdmfSink(s, str(tmp_path))):
        s.add_sink(sink)
    rng = np.random.default_rng(2)
    frames = []
    for k, t in ((5, 0.5), (10, 1.0)):
        data = dict(phi=rng.random((s.n_cells, s.nv)), c=[rng.random((s.n_cells, s.nv)) for _ in range(3)],
                    phi_M=rng.random((s.nmf, s.nf)))
        frames.append(s.record_host(t, k, **data))
    s.close()
    assert s.frames == 2 and [(t, k) for t, k, _ in mem.frames] == [(0.5, 5), (1.0, 10)]
    z = np.load(tmp_path / "step_000010.npz")
    assert float(z["t"]) == 1.0 and all(np.array_equal(z[n], frames[1][n]) for n in s.watches)
    # the vertex watches: the sub-mesh of the sub-domain, vertices in increasing parent id, one collection per watch
    for stem, names in (("results_sub_0", ["phi_0", "Na_0", "K_0", "Cl_0"]), ("results_sub_1", ["phi_1", "Cl_1"]),
                        ("results_mem_1", ["phi_M_1"])):
        path = str(tmp_path / (stem + ".xdmf"))
        with XDMFFile(None, path, "r") as f:
            sub = f.read_mesh()
        assert np.array_equal(sub.x, s.locations(names[0]))
        for n in names:
            times, values = read_xdmf_series(path, n)
            assert times.tolist() == [0.5, 1.0]
            assert np.array_equal(values[0], frames[0][n]) and np.array_equal(values[1], frames[1][n])
    with XDMFFile(None, str(tmp_path / "results_sub_1.xdmf"), "r") as f:
        sub = f.read_mesh()
    cells1 = s.cells[s.cell_sub == 1]
    assert sub.cell_type == "triangle" and np.array_equal(s.item_ids("phi_1")[sub.cells], cells1)
    with XDMFFile(None, str(tmp_path / "results_mem_1.xdmf"), "r") as f:
        assert f.read_mesh().cell_type == "interval"
    # the broken watch: the exploded mesh, so a viewer shows the jumps
    with XDMFFile(None, str(tmp_path / "broken_sub_0.xdmf"), "r") as f:
        ex = f.read_mesh()
    assert np.array_equal(ex.cells, np.arange(ex.num_vertices).reshape(-1, 3))
    assert np.array_equal(ex.x, s.x[s.cells][s.cell_sub == 0].reshape(-1, 2))
    assert np.array_equal(read_xdmf_series(str(tmp_path / "broken_sub_0.xdmf"), "phi_b")[1][1], frames[1]["phi_b"])
    with pytest.raises(KeyError):
        read_xdmf_series(str(tmp_path / "broken_sub_0.xdmf"), "nothing")


def test_xdmf_sink_refuses_what_it_cannot_write(tmp_path):
    for define, text in ((lambda s: s.watch("m", "phi", 0, form="cell_mean"), "cell mean"),
                         (lambda s: s.watch("p", "phi", 0, form="vertex", dtype="f4"), "float32"),
                         (lambda s: (s.watch("p", "phi", 0, form="vertex"), s.select(0, "vertex", indices=[0, 1])), "selection")):
        s = _snap(writer="inline")
        define(s)
        s.add_sink(DGXdmfSink(s, str(tmp_path)))
        with pytest.raises(ValueError, match=text):
            s.record_host(0.0, 0, phi=np.zeros((s.n_cells, s.nv)))


def test_refusals_that_need_no_device():
    s = _snap()
    s.watch("phi", "phi", 0)
    for args, kw in ((("phi", "phi", 0), {}),                                  # the name twice
                     (("p2", "phi", 0), {}),                                   # the watch twice
                     (("x", "rho", 0), {}), (("x", "phi", 7), {}),             # unknown quantity, unknown sub-domain tag
                     (("x", "phi_M", 0), {}), (("x", "phi_M", 2), {}),         # no membrane facets with that tag
                     (("x", "c", 0), {}), (("x", "c", 0), dict(ion="Ca")), (("x", "c", 0), dict(ion=3)),
                     (("x", "I_ch", 1), dict(ion=-1)),
                     (("x", "state", 1), {}), (("x", "state", 1), dict(state=-1)),
                     (("x", "phi", 0), dict(form="nodal")), (("x", "phi", 0), dict(dtype="f2")),
                     (("x", "phi_M", 1), dict(form="cell_mean"))):
        with pytest.raises(ValueError):
            s.watch(*args, **kw)
    assert list(s.watches) == ["phi"]
    with pytest.raises(ValueError, match="no watch"):
        s.locations("nothing")
    with pytest.raises(ValueError, match="needs phi"):
        s.frame_host(c=[None] * 3)
    with pytest.raises(ValueError, match="values for"):
        s.frame_host(phi=np.zeros(5))
    with pytest.raises(ValueError, match="nothing is watched"):
        _snap().record_host(0.0, 0)
    with pytest.raises(ValueError):
        DGSnapshots(*_mesh(), [0, 1], [1], IONS, writer="process")
    from knpemi.fem.idealized import make_mesh_2D
    with pytest.raises(ValueError, match="triangles, tetrahedra and hexahedra"):
        DGSnapshots(*make_mesh_2D(1, cell_type="quadrilateral"), [0, 1], [1], IONS)
    with pytest.raises(NotImplementedError):
        s.select_owned(None)
    from knpemi.dg import DGSlab
    with pytest.raises(NotImplementedError, match="DGSlab.snapshot"):
        DGSlab.snapshot(object(), s)


def test_abi_and_driver_options(hip_lib):
    header = open(os.path.join(os.path.dirname(L.__file__), "..", "..", "include", "knpemi_hip.h")).read()
    for name in ("set", "layout", "record", "take", "pending", "reset", "clear"):
        fn = f"knpemi_dg_snapshot_{name}"
        assert re.search(rf"\b{fn}\s*\(", header) and hasattr(hip_lib, fn) and fn in L.SIGNATURES
    assert L.SIGNATURES["knpemi_dg_snapshot_take"] == L.SIGNATURES["knpemi_snapshot_take"]
    assert L.SIGNATURES["knpemi_dg_snapshot_record"] == L.SIGNATURES["knpemi_snapshot_record"]
    for name, value in (("KNPEMI_DG_ODE_STATE", L.DG_ODE_STATE), ("KNPEMI_DG_SNAP_BROKEN", L.DG_SNAP_BROKEN),
                        ("KNPEMI_DG_SNAP_CELL_MEAN", L.DG_SNAP_CELL_MEAN), ("KNPEMI_DG_SNAP_VERTEX", L.DG_SNAP_VERTEX),
                        ("KNPEMI_DG_SNAPSHOT_MAX_SPACE", L.DG_SNAPSHOT_MAX_SPACE)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value
    import run_2D_dg as D
    a = D.build_parser().parse_args(["--snapshots", "out", "--save-every", "5", "--snapshot-form", "broken"])
    assert (a.snapshots, a.save_every, a.snapshot_form) == ("out", 5, "broken")
    d = D.build_parser().parse_args([])
    assert d.snapshots is None and d.save_every == 1 and d.snapshot_form == "vertex"
    with pytest.raises(SystemExit):
        D.build_parser().parse_args(["--snapshot-form", "nodal"])
