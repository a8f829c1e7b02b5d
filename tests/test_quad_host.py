"""Host tests of the quadrilateral support (no GPU): the 2-D mesh generator's quadrilateral variant, the flattening of a
quadrilateral problem, the oracle's patch test on general bilinear cells (the yardstick tests/test_quad_gpu.py leans on),
the host restatement of the ion fluxes, and the drivers' --cell-type option with the XDMF round trip."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

import quad_meshes as qm
from helpers import Setup
from knpemi.fem import CellType, create_rectangle, make_mesh_2D

EXAMPLES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "idealized_geometries")


def _host_setup(data, r=1):
    with contextlib.redirect_stdout(io.StringIO()):
        return Setup("2d", r, mesh_data=data, build_forms=False)


def interior_rows(s):
    """(rows, x): the dofs of the potential system, numbered [ECS | cell], whose vertex has four incident cells of its
    sub-mesh and does not lie on the membrane, and the coordinates of every dof."""
    mem = s.subdomain_list[1]["mesh_mem"].parent_vertices
    rows, xs, off = [], [], 0
    for tag in s.subdomain_list:
        m = s.subdomain_list[tag]["mesh_sub"]
        count = np.bincount(m.cells.ravel(), minlength=m.num_vertices)
        ok = (count == 4) & ~np.isin(m.parent_vertices, mem)
        rows.append(off + np.flatnonzero(ok))
        xs.append(m.x)
        off += m.num_vertices
    return np.concatenate(rows), np.concatenate(xs)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 2])
def test_make_mesh_2D_quadrilateral_tags(r):
    from knpemi.fem.probe import integral_weights
    from knpemi.fem.mesh import exterior_facet_indices
    mesh, ct, ft = make_mesh_2D(r, cell_type="quadrilateral")
    assert mesh.cell_type == "quadrilateral" and mesh.cells.shape == (31 * 2 ** r * 2 * 2 ** r, 4)
    assert (qm.corner_determinants(mesh.x, mesh.cells) > 0).all()              # [v00, v10, v01, v11], right-handed
    w = integral_weights(mesh, ct.dense() == 1)
    assert abs(w.sum() - 60e-6 * 2e-6) < 1e-13 * 60e-6 * 2e-6
    # the membrane is the boundary of [1, 61] x [1, 3] um, 2 (60 + 2) um long, cut into facets of h = 2 um / 2^r
    assert int((ft.values == 1).sum()) == 2 * (60 + 2) * 2 ** r // 2
    ext = exterior_facet_indices(mesh)
    assert np.array_equal(np.sort(ft.indices[ft.values == 5]), np.sort(ext))
    # the default is what it was: triangles, the cells and tags of create_rectangle(..., triangle)
    tri, ct3, ft3 = make_mesh_2D(r)
    ref = create_rectangle(None, [np.array([0.0, 0.0]), np.array([62.0e-6, 4.0e-6])], (31 * 2 ** r, 2 * 2 ** r),
                           CellType.triangle)
    assert tri.cell_type == "triangle" and np.array_equal(tri.cells, ref.cells) and np.array_equal(tri.x, ref.x)
    mid = tri.x[tri.cells].mean(axis=1)
    inside = (mid[:, 0] > 1e-6) & (mid[:, 0] < 61e-6) & (mid[:, 1] > 1e-6) & (mid[:, 1] < 3e-6)
    assert np.array_equal(ct3.dense() == 1, inside)
    assert int((ft3.values == 1).sum()) == 2 * (60 + 2) * 2 ** r // 2
    with pytest.raises(ValueError):
        make_mesh_2D(r, cell_type="hexahedron")


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rect", "star7"])
def test_flatten_problem_passes_quadrilaterals_through(name):
    from knpemi import _lib as L
    from knpemi.device import _CELL_KIND, flatten_problem
    data = qm.rect(1) if name == "rect" else qm.reorient(qm.star_quad(7, 3), 42)[0]
    s = _host_setup(data)
    flat = flatten_problem(s.mesh, s.ft, s.subdomain_list)
    assert L.QUADRILATERAL == 3 and _CELL_KIND[s.mesh.cell_type] == 3
    for i, tag in enumerate(s.subdomain_list):
        sub = s.subdomain_list[tag]["mesh_sub"]
        assert flat["cells"][i].shape[1] == 4 and flat["cells"][i].dtype == np.int32
        # unchanged in vertex order: local vertex j of sub-mesh cell c is parent vertex mesh.cells[parent cell, j]
        assert np.array_equal(sub.parent_vertices[flat["cells"][i]], s.mesh.cells[sub.parent_entities])
        det = qm.corner_determinants(flat["x"][i], flat["cells"][i])
        assert (np.ptp(np.sign(det), axis=1) == 0).all()
    assert flat["facet_e"][1].shape[1] == 2 and flat["facet_i"][1].shape == flat["facet_q"][1].shape == flat["facet_e"][1].shape
    assert np.array_equal(flat["x"][0][flat["facet_e"][1]], flat["x"][1][flat["facet_i"][1]])
    lh = qm.left_handed_fraction(s.mesh)
    assert lh == 0.0 if name == "rect" else 0.3 < lh < 0.7
    if name == "star7":
        assert s.mesh.num_cells == 63 and np.bincount(s.mesh.cells.ravel()).max() == 7
        assert qm.star_quad(3, 2)[0].num_cells == 12


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def test_oracle_patch_test_on_jittered_quadrilaterals():
    """A_emi of the oracle on jittered(2), general bilinear cells, applied to a linear potential with constant
    concentrations: nothing is left on the 613 interior rows (four incident cells of one sub-domain, off the membrane).
    Measured: 3.2e-16 of max|A| max|u|.  r = 1 has no interior ECS row."""
    s = _host_setup(qm.jittered(2), 2)
    o, P, params, ions = s.oracle()
    c_all, phi, phiM, mm = s.oracle_fields()
    A, _, _ = o.assemble_emi(P, params, ions, c_all, phiM, mm)
    rows, x = interior_rows(s)
    n0 = s.subdomain_list[0]["mesh_sub"].num_vertices
    assert len(rows) == 613 and (rows < n0).any() and (rows >= n0).any()
    u = 3.0 + 2.0e5 * x[:, 0] - 1.5e5 * x[:, 1]
    r = np.abs((A @ u)[rows]).max() / (np.abs(A.data).max() * np.abs(u).max())
    print("patch test residual", r)
    assert r < 1e-13
    assert abs(A - A.T).max() < 1e-14 * np.abs(A.data).max()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def _affine_fluxes(data):
    """IonFluxes on `data` with affine nodal fields: (fl, fields, row, exact per-cell vectors, volumes)."""
    from knpemi import IonFluxes
    s = _host_setup(data)
    fl = IonFluxes(s.subdomain_list, s.ion_list, s.physical_parameters)
    for tag in s.subdomain_list:
        fl.watch(tag)
    gphi = np.array([3.0e2, -1.0e2])
    gc = [np.array([2.0e6, 1.0e6]), np.array([-1.0e6, 3.0e6]), np.array([0.5e6, -2.0e6])]
    phi, c = {}, {}
    for tag in s.subdomain_list:
        x = s.subdomain_list[tag]["mesh_sub"].x
        phi[tag] = -0.07 + x @ gphi
        c[tag] = [100.0 + 10.0 * k + x @ gc[k] for k in range(3)]
    fields, row = fl.compute_host(phi, c)
    return s, fl, fields, row, (gphi, gc, c)


@pytest.mark.parametrize("name", ["rect", "sheared", "left_handed"])
def test_flux_restatement_is_exact_on_affine_fields(name):
    """On parallelograms the Q1 interpolant of an affine field is the field: the gradient is exact, the value at the centre
    is the field's, the midpoint volumes add up to the area -- whatever the orientation of the cells."""
    data = {"rect": lambda: qm.rect(1), "sheared": lambda: qm.sheared(1),
            "left_handed": lambda: qm.reorient(qm.rect(1), 45, symmetry=qm.MIRROR)[0]}[name]()
    s, fl, fields, row, (gphi, gc, c) = _affine_fluxes(data)
    assert qm.left_handed_fraction(s.mesh) == (1.0 if name == "left_handed" else 0.0)
    F, psi = fl.F, fl.psi
    for tag in s.subdomain_list:
        m = s.subdomain_list[tag]["mesh_sub"]
        vol = fl.volumes(tag)
        area = (62e-6 * 4e-6 - 60e-6 * 2e-6) if tag == 0 else 60e-6 * 2e-6
        assert abs(vol.sum() / area - 1.0) < 1e-12
        centre = m.x[m.cells].mean(axis=1)
        total = np.zeros((m.num_cells, 2))
        for k, ion in enumerate(s.ion_list):
            D, z = fl.D[tag][k], fl.z[k]
            Jd = np.broadcast_to(-D * gc[k], total.shape)
            ck = 100.0 + 10.0 * k + centre @ gc[k]
            Jr = -(z * psi * D) * ck[:, None] * gphi
            n = ion["name"]
            for got, want in ((fields[tag][f"{n}/diffusive"], Jd), (fields[tag][f"{n}/drift"], Jr)):
                assert np.abs(got - want).max() < 1e-9 * np.abs(want).max()
            total = total + F * z * (Jd + Jr)
            assert np.abs(row[f"{tag}/{n}/diffusive"] - (vol[:, None] * Jd).sum(axis=0)).max() < 1e-9 * np.abs(vol.sum() * Jd[0]).max()
        assert np.abs(fields[tag]["current"] - total).max() < 1e-9 * np.abs(total).max()


def test_flux_restatement_does_not_depend_on_the_local_vertex_order():
    """jittered(1), general cells, against the same mesh with every cell in another of the 8 tensor orders and shuffled
    numbers: the per-cell vectors move with the cell permutation, the sums and maxima stay."""
    base = qm.jittered(1)
    data, (vperm, cperm, G) = qm.reorient(base, 46)
    s0, s1 = _host_setup(base), _host_setup(data)
    rng = np.random.default_rng(5)
    from knpemi import IonFluxes
    out = []
    nodal = {"phi": rng.standard_normal(base[0].num_vertices), "c": [50.0 + rng.random(base[0].num_vertices) for _ in range(3)]}
    inv = np.argsort(vperm)
    for s, to_old in ((s0, None), (s1, inv)):
        fl = IonFluxes(s.subdomain_list, s.ion_list, s.physical_parameters)
        phi, c = {}, {}
        for tag in s.subdomain_list:
            fl.watch(tag)
            pv = s.subdomain_list[tag]["mesh_sub"].parent_vertices
            old = pv if to_old is None else to_old[pv]
            phi[tag] = nodal["phi"][old]
            c[tag] = [a[old] for a in nodal["c"]]
        out.append((s, fl) + fl.compute_host(phi, c))
    (s0, f0, fields0, row0), (s1, f1, fields1, row1) = out
    for key in row0:
        assert np.abs(np.asarray(row1[key]) - np.asarray(row0[key])).max() <= 1e-12 * np.abs(np.asarray(row0[key])).max(), key
    for tag in s0.subdomain_list:
        # new sub-mesh cell i is old parent cell cperm[parent of i]
        old_parent = cperm[s1.subdomain_list[tag]["mesh_sub"].parent_entities]
        own = s0.subdomain_list[tag]["mesh_sub"].parent_entities
        pos = np.searchsorted(own, old_parent)
        assert np.array_equal(own[pos], old_parent)
        for key in fields0[tag]:
            want = fields0[tag][key][pos]
            assert np.abs(fields1[tag][key] - want).max() <= 1e-11 * np.abs(want).max(), key


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_driver_accepts_the_cell_type_and_mesh_files_round_trip(tmp_path, monkeypatch):
    sys.path.insert(0, EXAMPLES)
    try:
        import importlib
        run_2D_dg = importlib.import_module("run_2D_dg")
        args = run_2D_dg.build_parser().parse_args(["--cell-type", "quadrilateral"])
        assert args.cell_type == "quadrilateral"
        assert run_2D_dg.build_parser().parse_args([]).cell_type == "triangle"
        with pytest.raises(SystemExit):
            run_2D_dg.build_parser().parse_args(["--cell-type", "hexahedron"])
        run_2D = importlib.import_module("run_2D")
        ap = run_2D.build_parser(cell_types=run_2D.CELL_TYPES_2D)
        assert ap.parse_args(["--cell-type", "quadrilateral"]).cell_type == "quadrilateral"
        assert ap.parse_args([]).cell_type == "triangle"
        assert not hasattr(run_2D.build_parser(res=0, steps=20).parse_args([]), "cell_type")      # run_3D.py's parser
        mk = importlib.import_module("make_mesh_2D")
        path = mk.main(str(tmp_path), 1, "quadrilateral")
        assert os.path.basename(path) == "mesh_1_quad.xdmf" and "Quadrilateral" in open(path).read()
        assert os.path.basename(mk.main(str(tmp_path), 1)) == "mesh_1.xdmf"
        mesh, ct, ft = run_2D.read_mesh(path)
    finally:
        sys.path.remove(EXAMPLES)
    from knpemi.dg import DGProblem              # the DG variant keeps refusing the cell kind, before it touches a device
    with pytest.raises(ValueError, match="DG variant"):
        DGProblem(*qm.rect(1), [0, 1], [1])
    m0, ct0, ft0 = qm.rect(1)
    assert mesh.cell_type == "quadrilateral" and np.array_equal(mesh.cells, m0.cells) and np.array_equal(mesh.x, m0.x)
    assert np.array_equal(ct.dense(), ct0.dense())
    assert np.array_equal(ft.dense(fill=0), ft0.dense(fill=0))
