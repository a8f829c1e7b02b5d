"""Host tests of the re-oriented, renumbered and irregular hexahedral meshes of tests/hex_meshes.py: the properties the GPU
tests of tests/test_hex_unstructured_gpu.py rely on, and how far the two numpy restatements themselves depend on the
description of a mesh (which bounds what those GPU tests may blame on the yardstick).

Figures (hex_statistics; the re-oriented boxes share one topology):

                                        box variants   star3 (3, 2, 3)   star7 (7, 3, 4)
    cells                               2 592          36                252
    left-handed cells (per-cell)        49 - 50 %      44 %              49 %
    most cells at one vertex            8              8                 14
    most cells at a sub-mesh vertex     8              8                 12
    longest A_emi row                   33             33                51
    distinct (facet, facet, map)        288 (all)      107               277
    (one global symmetry: 6 triples, 100 % / 0 % left-handed)

Oracle equivariance (the same oracle on the base mesh, mapped through (vperm, cperm, G)), largest over all meshes:
oracle/knpemi_oracle.py 5.7e-14 (b_emi; matrices <= 7.0e-15), DGOracleQ1 3.2e-14 (b_emi; matrices <= 4.1e-15)."""
import contextlib
import io

import numpy as np
import pytest

import hex_meshes as hm
from helpers import Setup, csr_rel_err, rel_err


def test_the_48_symmetries():
    gs = {tuple(g) for _, _, g in hm.SYMMETRIES}
    assert len(hm.SYMMETRIES) == 48 and len(gs) == 48
    corners = np.array([[(j >> a) & 1 for a in range(3)] for j in range(8)], float) * np.array([1.0, 0.7, 1.3])
    left = 0
    for k, (pi, s, g) in enumerate(hm.SYMMETRIES):
        assert sorted(g) == list(range(8))
        det = hm.corner_determinants(corners, g[None, :])[0]
        assert np.all(det > 0) or np.all(det < 0), k                       # the eight-corner sign test of knpemi_dg_create
        assert bool(det[0] < 0) == hm.symmetry_is_left_handed(k)
        left += det[0] < 0
    assert left == 24
    assert hm.symmetry_is_left_handed(hm.MIRROR) and not hm.symmetry_is_left_handed(hm.CYCLIC)
    # the counter-clockwise (VTK) order is none of them: it folds
    vtk = np.array([[0, 1, 3, 2, 4, 5, 7, 6]])
    det = hm.corner_determinants(corners, vtk)[0]
    assert (det > 0).any() and (det < 0).any()


@pytest.mark.parametrize("name", hm.NAMES)
def test_meshes_are_valid_and_reach_what_they_are_for(name):
    base, data, (vperm, cperm, G) = hm.variant(name)
    mesh, ct, ft = data
    st = hm.hex_statistics(data)
    print(name, st)
    det = hm.corner_determinants(mesh.x, mesh.cells)
    assert np.all((det > 0).all(axis=1) | (det < 0).all(axis=1))
    # the same mesh: coordinates, cells and tags map back
    assert np.array_equal(mesh.x[vperm], base[0].x)
    assert np.array_equal(np.argsort(vperm)[mesh.cells], np.take_along_axis(base[0].cells[cperm], G.astype(np.int32), axis=1))
    assert np.array_equal(ct.dense(), base[1].dense()[cperm])
    assert (ft.values == 1).sum() == (base[2].values == 1).sum() > 0 and (ft.values == 5).sum() == (base[2].values == 5).sum()
    if name in hm.PER_CELL:
        assert 0.35 <= st["left_handed"] <= 0.65
        assert st["neighbour_facets_per_axis"] == [6, 6, 6]
        assert st["position_maps"] > 1
    elif name == "global_mirror":
        assert st["left_handed"] == 1.0
    else:
        assert st["left_handed"] == 0.0
    if name.startswith("star"):
        assert getattr(mesh, "uniform_cell", None) is None
    else:
        assert getattr(mesh, "uniform_cell", None) is not None
        assert not np.array_equal(mesh.cells, base[0].cells)


def test_star_meshes_are_irregular():
    """star_hex(7, 3, 4): 252 cells, 425 vertices, 48 membrane facets, 14 cells at an axis vertex (12 of one sub-domain),
    longest A_emi row 51; star_hex(3, 2, 3): 36 cells, 76 vertices, an edge shared by three hexahedra."""
    st7, st3 = hm.hex_statistics(hm.variant("star7")[1]), hm.hex_statistics(hm.variant("star3")[1])
    print(st7, st3)
    assert st7["cells"] == 252 and st3["cells"] == 36
    assert st7["longest_row"] > 27 and st7["most_cells_at_a_vertex"] > 8 and st7["most_cells_at_a_submesh_vertex"] > 8
    mesh = hm.variant("star3")[0][0]
    axis = np.flatnonzero(np.all(np.abs(mesh.x[:, :2]) < 1e-12, axis=1))
    on_axis = np.isin(mesh.cells, axis).sum(axis=1) == 2
    assert on_axis.sum() == 3 * 3                                          # three cells around the axis in each layer
    s = Setup("hex", 0, mesh_data=hm.variant("star7")[1], build_forms=False)
    _, P, params, ions = s.oracle()
    import knpemi_oracle as o
    c_all, phi, phiM, mm = s.oracle_fields()
    A, _, _ = o.assemble_emi(P, params, ions, c_all, phiM, mm)
    assert np.diff(A.tocsr().indptr).max() == st7["longest_row"]          # the host model of the pattern is the oracle's


def _cg_objects(s, splitting):
    o, P, params, ions = s.oracle()
    c_all, phi, phiM, mm = s.oracle_fields()
    A, Pm, b = o.assemble_emi(P, params, ions, c_all, phiM, mm, splitting_scheme=splitting)
    Ak, bk = o.assemble_knp(P, params, ions, c_all, phi, phiM, mm, s.dt, splitting_scheme=splitting)
    return P, dict(A_emi=A.tocsr(), P_emi=Pm.tocsr(), b_emi=b, A_knp=Ak.tocsr(), b_knp=bk)


def cg_oracle_equivariance(name, splitting=True):
    """Relative differences of the five objects of oracle/knpemi_oracle.py on the re-oriented mesh and on its base mesh
    (the same nodal fields), the latter permuted to the numbering of the former."""
    import knpemi_oracle as o
    base, data, (vperm, cperm, G) = hm.variant(name)
    with contextlib.redirect_stdout(io.StringIO()):
        s0 = Setup("hex", 0, mesh_data=base, build_forms=False)
        s1 = Setup("hex", 0, mesh_data=data, build_forms=False)
    s0.perturb()
    p = hm.transfer_cg_fields(s0, s1, vperm)
    P0, a = _cg_objects(s0, splitting)
    P1, b = _cg_objects(s1, splitting)
    pe = np.concatenate([P0.off[t] + p[t] for t in P0.tags])
    off, _ = o.knp_block_offsets(P0, 2)
    pk = np.concatenate([off[(t, k)] + p[t] for t in P0.tags for k in range(2)])
    out = {}
    for key in a:
        q = pk if key.endswith("knp") else pe
        out[key] = rel_err(b[key], a[key][q]) if key.startswith("b") else csr_rel_err(b[key], a[key][q][:, q].tocsr())
    return out


def _dg_state(nc, nmf, X, K, seed):
    rng = np.random.default_rng(seed)
    smooth = lambda a, b: a + b * np.cos(3.0 * X[:, :, 0] + 1.0) * np.sin(2.0 * X[:, :, 1] + 0.5)
    c_all = [smooth(2.0 + k, 0.4) + 0.05 * rng.random((nc, 8)) for k in range(K)]
    phi = smooth(0.1, 0.3) + 0.02 * rng.random((nc, 8))
    phi_M = 0.2 + 0.1 * rng.random((nmf, 4))
    I_ch = [0.3 * rng.standard_normal((nmf, 4)) for _ in range(K)]
    src = {k: rng.standard_normal((nc, 8)) for k in range(K - 1)}
    return c_all, phi, phi_M, I_ch, src


def dg_oracle_equivariance(name, splitting=True, scale=None):
    """The same for DGOracleQ1: dofs through new (i, j) <-> old (cperm[i], G[i, j]), membrane nodes by their vertices.
    `scale` brings the mesh to unit size (the DG tests use unit parameters)."""
    import knpemi_dg_oracle as dg
    base, data, (vperm, cperm, G) = hm.variant(name)
    K, res = 3, []
    ions = [dict(name=f"i{k}", z=z, D=[1.0 + 0.3 * k, 0.6 + 0.2 * k]) for k, z in enumerate((1.0, -1.0, 2.0))]
    params = dict(dt=0.05, F=1.3, psi=0.8, C_M=0.7)
    mems, state = [], None
    for mesh, ct, ft in (base, data):
        x = mesh.x * (scale or 1.0)
        mem = mesh.facets[np.sort(ft.indices[ft.values == 1])]
        mems.append(mem)
        o = dg.make_dg_oracle(x, mesh.cells, mesh.cell_type, ct.dense().astype(np.int32), mem, np.ones(len(mem), np.int32))
        if state is None:
            state = _dg_state(mesh.num_cells, len(mem), x[mesh.cells], K, 1)
            c_all, phi, phi_M, I_ch, src = state
        else:
            p = hm.dg_dof_map(cperm, G)
            f, t = hm.dg_membrane_map(mems[0], mem, vperm)
            cell = lambda a: a.ravel()[p].reshape(-1, 8)
            memf = lambda a: np.take_along_axis(a[f], t, axis=1)
            c_all, phi, phi_M = [cell(c) for c in state[0]], cell(state[1]), memf(state[2])
            I_ch, src = [memf(i) for i in state[3]], {k: cell(v) for k, v in state[4].items()}
        A, b = o.assemble_emi(params, ions, c_all, phi_M, I_ch, splitting_scheme=splitting, gamma=7.5)
        As, bs = o.assemble_knp(params, ions, c_all, phi, phi_M, I_ch, splitting_scheme=splitting, gamma=7.5, f_source=src)
        res.append(([A.tocsr()] + [a.tocsr() for a in As], [b] + list(bs)))
    (A0, b0), (A1, b1) = res
    out = {}
    for w in range(K):
        out[f"A{w}"] = csr_rel_err(A1[w], A0[w][p][:, p].tocsr())
        out[f"b{w}"] = rel_err(b1[w], b0[w][p])
    return out


@pytest.mark.parametrize("name", hm.NAMES)
def test_cg_oracle_does_not_depend_on_the_description_of_the_mesh(name):
    """Measured: largest 5.7e-14 (b_emi, global_mirror); matrices <= 7.0e-15 (A_knp, reoriented_sheared).  Bound 1e-12."""
    errs = cg_oracle_equivariance(name)
    print(name, errs)
    assert max(errs.values()) < 1e-12, errs


@pytest.mark.parametrize("name", hm.NAMES)
def test_dg_oracle_does_not_depend_on_the_description_of_the_mesh(name):
    """DGOracleQ1 on the same meshes, scaled to unit size (the DG tests use unit parameters).  Measured: largest 3.2e-14
    (b_emi, reoriented_sheared); matrices <= 4.1e-15.  Bound 1e-12."""
    errs = dg_oracle_equivariance(name, scale=1.0 / hm.L_BOX if name.startswith("star") else 1e6)
    print(name, errs)
    assert max(errs.values()) < 1e-12, errs
