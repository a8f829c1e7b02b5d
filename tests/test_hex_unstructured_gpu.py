"""GPU tests of the hexahedral kernels on meshes that create_box does not produce (tests/hex_meshes.py): every cell in its
own one of the 48 tensor orders (half of them left-handed), shuffled vertex and cell numbers, one global symmetry, and
the star meshes with an edge shared by 3 or 7 cells.  On these a facet meets ANY facet of its neighbour with any of the
vertex correspondences, the box-mesh DG kernels see another `box_h` order on either side of a facet, the CG geometry
classes (uniform / affine / general) have to be decided on the coordinates, and rows are longer than 27 entries.
`knpemi_debug_geometry`, `knpemi_debug_layout` and bit comparisons prove in every test that the mesh reached the code it
is there for.  tests/test_hex_meshes_host.py bounds what may be blamed on the two restatements (below 1e-13)."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

import hex_meshes as hm
from helpers import TOL, Setup, assemble_both, check_facet_integrals_of_the_write_back_launch, csr_rel_err, rel_err
from knpemi import _lib as L

pytestmark = pytest.mark.gpu

KN_STAGED = 768        # distinct vertices of a block staged by the batched loads (kernels_assemble.hip: stage_records)
AFFINE, UNIFORM = 2, 4  # knpemi_debug_geometry
# mesh -> (affine, uniform).  reoriented_box: every cell is the same box, but half of them mirrored and with permuted axes,
# so the edge table of the first cell (and the attached uniform_cell) does not describe the others.  The global variants:
# every cell has the SAME edge table, which contradicts the attached uniform_cell (mirror: determinant < 0; permuted: the
# cell's first edge is not along x) -- knpemi_create falls back to the first cell's table, whose metric is diagonal.
GEOMETRY = {"reoriented_box": (True, False), "global_mirror": (True, True), "global_permuted": (True, True),
            "reoriented_sheared": (True, False), "reoriented_jittered": (False, False), "star3": (False, False),
            "star7": (False, False)}


def _setup(name, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        s = Setup("hex", 0, mesh_data=hm.variant(name)[1], **kw)
    s.perturb()
    return s


def _layout(dp):
    out = (ctypes.c_int * 8)()
    L.check(dp.lib.knpemi_debug_layout(dp.h, out, 8))
    return dict(zip(("longest_row", "lanes_per_row", "pairs_per_lane", "block_vertices", "membrane_entries", "lds_emi",
                     "lds_knp", "longest_laplacian_row"), out))


def _geometry(dp):
    flags = ctypes.c_int(-1)
    L.check(dp.lib.knpemi_debug_geometry(dp.h, ctypes.byref(flags)))
    return flags.value


def _values(a):
    return np.asarray(a.data if hasattr(a, "indptr") else a)


# ---- CG path ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hm.NAMES)
def test_assembly_matches_oracle_on_reoriented_hexahedra(hip_lib, name):
    """All five objects, both splitting modes, at 1e-10, and the geometry class knpemi_create decided on (GEOMETRY).
    Largest device-versus-oracle error measured on an MI355X (both modes):
        reoriented_box      A_emi 5.2e-15  P_emi 5.2e-15  b_emi 1.1e-13  A_knp 5.5e-15  b_knp 4.7e-15   flags 2
        reoriented_jittered A_emi 1.9e-15  P_emi 1.9e-15  b_emi 8.4e-14  A_knp 3.0e-15  b_knp 1.7e-15   flags 0
        reoriented_sheared  A_emi 4.6e-15  P_emi 4.6e-15  b_emi 7.5e-14  A_knp 5.9e-15  b_knp 4.7e-15   flags 2
        global_mirror       A_emi 6.6e-15  P_emi 6.6e-15  b_emi 1.1e-13  A_knp 7.0e-15  b_knp 6.3e-15   flags 6
        global_permuted     A_emi 4.2e-15  P_emi 4.2e-15  b_emi 1.0e-13  A_knp 5.3e-15  b_knp 4.1e-15   flags 6
        star3               A_emi 1.1e-15  P_emi 1.1e-15  b_emi 5.4e-14  A_knp 1.4e-15  b_knp 1.1e-15   flags 0
        star7               A_emi 1.3e-15  P_emi 1.3e-15  b_emi 5.9e-14  A_knp 1.8e-15  b_knp 1.2e-15   flags 0
    Layout: the boxes and star3 have a longest row of 33 (Laplacian 27), star7 of 51 (Laplacian 42, 3 pairs per lane)."""
    s = _setup(name)
    for splitting in (True, False):
        errs, _ = assemble_both(s, splitting)
        flags, lay = _geometry(s.a_emi.dp), _layout(s.a_emi.dp)
        print(name, splitting, errs, "flags", flags, lay)
        assert (bool(flags & AFFINE), bool(flags & UNIFORM)) == GEOMETRY[name], flags
        assert max(errs.values()) < TOL, errs
    if not name.startswith("star"):
        assert getattr(s.mesh, "uniform_cell", None) is not None
    if name == "global_mirror":
        assert hm.left_handed_fraction(s.mesh) == 1.0               # uniform with a negative determinant
    if name == "star7":
        assert lay["longest_row"] > 27 and lay["longest_laplacian_row"] > 27
    assert lay["lds_emi"] > 0 and lay["lds_knp"] > 0


def test_oversized_row_blocks_on_the_reoriented_box(hip_lib, monkeypatch):
    """KNPEMI_BLOCK_CLASSIC=1 on the shuffled box: 64 consecutive rows of a random numbering touch up to 27 vertices each,
    more than the 768 the batched loads of stage_records take, so its loop for oversized blocks runs on hexahedra (with the
    x-fastest numbering of create_box it cannot).  Against the oracle, and bit for bit equal to the clustered run.
    Measured block_vertices: classic 1263, clustered 1112 (on a random numbering the clusters are oversized too)."""
    res = {}
    for classic in (False, True):
        if classic:
            monkeypatch.setenv("KNPEMI_BLOCK_CLASSIC", "1")
        else:
            monkeypatch.delenv("KNPEMI_BLOCK_CLASSIC", raising=False)
        s = _setup("reoriented_box")
        errs, objs = assemble_both(s)
        lay = _layout(s.a_emi.dp)
        print("classic" if classic else "clustered", errs, lay)
        assert max(errs.values()) < TOL, errs
        res[classic] = (objs, lay)
    assert res[True][1]["block_vertices"] > KN_STAGED
    for a, b in zip(res[False][0], res[True][0]):
        assert np.array_equal(_values(a), _values(b))


def test_emi_invariants_and_reproducibility_on_the_star_mesh(hip_lib):
    s = _setup("star7")
    _, first = assemble_both(s)
    A = first[0]
    assert np.abs(A @ np.ones(A.shape[0])).max() < 1e-12 * np.abs(A.data).max()
    assert csr_rel_err(A, A.T.tocsr()) < 1e-14
    first = [_values(a).copy() for a in first]
    _, second = assemble_both(s)
    for a, b in zip(first, second):
        assert np.array_equal(a, _values(b))


def test_trace_on_reoriented_jittered_hexahedra_matches_oracle(hip_lib):
    """test_trace_matches_oracle on the shuffled numbering: non-planar membrane quadrilaterals, 864 membrane vertices."""
    from knpemi import interpolate_to_membrane
    s = _setup("reoriented_jittered")
    o, P, params, ions = s.oracle()
    qe, qi = interpolate_to_membrane(s.phi[0], s.phi[1], s.phi_M_prev[1].function_space, s.mesh, s.ct,
                                     s.subdomain_list, 1)
    te, ti = P.trace(1, s.phi[0].x._a, s.phi[1].x._a)
    assert len(te) >= 40 and np.abs(te - ti).max() > 0
    assert np.array_equal(qe.x._a, te) and np.array_equal(qi.x._a, ti)
    assert qe.name == s.phi[0].name


def test_update_pde_on_reoriented_jittered_hexahedra_matches_oracle(hip_lib):
    from knpemi import update_pde_variables
    s = _setup("reoriented_jittered")
    o, P, params, ions = s.oracle()
    c_all, phi, phiM, mm = s.oracle_fields()
    c_new = {t: [f.x._a.copy() for f in s.c[t]] for t in s.subdomain_list}
    s.physical_parameters['rho'][1].value = np.asarray(0.7)
    rho = {'z': -1, 0: 0.0, 1: 0.7}
    update_pde_variables(s.c, s.c_prev, s.phi, s.phi_M_prev, s.physical_parameters, s.ion_list,
                         s.subdomain_list, s.mesh, s.ct)
    o.update_pde_variables(P, ions, rho, c_new, c_all, phi, phiM)
    for t in s.subdomain_list:
        for k in range(2):
            assert np.array_equal(s.c_prev[t][k].x._a, c_all[t][k])
        assert rel_err(s.ion_list[-1][f'c_{t}'].x._a, c_all[t][2]) < 1e-15
    assert rel_err(s.phi_M_prev[1].x._a, phiM[1]) < 1e-15


def test_facet_integrals_of_the_write_back_launch_on_the_star_mesh(hip_lib):
    """test_facet_integrals_formed_in_the_potential_write_back_launch on the 48 membrane quadrilaterals of star7, the
    seven-cell edge among their vertices."""
    s = _setup("star7")
    check_facet_integrals_of_the_write_back_launch(s)
    assert _layout(s.a_emi.dp)["membrane_entries"] >= 4


def test_flux_record_on_reoriented_jittered_hexahedra(hip_lib):
    """One record of the ion fluxes against IonFluxes.compute_host (pinned by tests/test_flux_host.py): knpemi/fluxes.py
    promises that left-handed hexahedra give the same answer.  Tolerance of tests/test_flux_gpu.py.
    Measured: fields 6.7e-16, row 6.1e-15."""
    from knpemi import IonFluxes
    from test_flux_gpu import _host_state, _read, _rel, _row_err, _stepper
    s = _setup("reoriented_jittered")
    st = _stepper(s)
    fl = IonFluxes(s.subdomain_list, s.ion_list, s.physical_parameters)
    for tag in s.subdomain_list:
        fl.watch(tag)
    st.fluxes(fl, fields=True)
    dp = st.dp
    L.check(dp.lib.knpemi_flux_record(dp.h, 1))
    dev = {tag: fl.fields(tag) for tag in s.subdomain_list}
    buf, rows, over = _read(dp, fl.n_cols, 1, reset=1)
    assert rows == 1 and over == 0
    fields, want = fl.compute_host(*_host_state(s))
    worst = 0.0
    for tag in s.subdomain_list:
        assert set(dev[tag]) == set(fields[tag])
        for key in fields[tag]:
            worst = max(worst, _rel(dev[tag][key], fields[tag][key]))
    e_row = _row_err(fl, buf[0], want)
    print("fields", worst, "row", e_row)
    assert 0.35 < hm.left_handed_fraction(s.mesh) < 0.65
    assert worst < TOL and e_row < TOL


# ---- refusal of folded hexahedra in knpemi_create ------------------------------------------------------------------------
def _small_box():
    from knpemi.fem import create_box
    from knpemi.fem.idealized import _tag
    mesh = create_box(None, [np.zeros(3), np.full(3, 2e-6)], (2, 2, 2), "hexahedron")
    ct, ft = _tag(mesh, [([0.0] * 3, [1e-6] * 3)], [1])
    with contextlib.redirect_stdout(io.StringIO()):
        return Setup("hex", 0, mesh_data=(mesh, ct, ft), build_forms=False)


def test_knpemi_create_refuses_hexahedra_in_vtk_order(hip_lib):
    """Local vertices 2 <-> 3 and 6 <-> 7 swapped (the counter-clockwise order of VTK): the trilinear map folds over."""
    from knpemi.device import DeviceProblem
    s = _small_box()
    for t in s.subdomain_list:
        cells = s.subdomain_list[t]["mesh_sub"].cells
        cells[:] = cells[:, [0, 1, 3, 2, 4, 5, 7, 6]]
    with pytest.raises(L.KnpemiError, match="tensor-product vertex order"):
        DeviceProblem(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list)


def test_knpemi_create_accepts_a_cell_in_another_tensor_order(hip_lib):
    from knpemi.device import DeviceProblem
    s = _small_box()
    k = next(k for k in range(48) if hm.symmetry_is_left_handed(k) and hm.SYMMETRIES[k][0] != (0, 1, 2))
    cells = s.subdomain_list[0]["mesh_sub"].cells
    cells[3] = cells[3][hm.SYMMETRIES[k][2]]
    dp = DeviceProblem(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list)
    assert dp.h and not _geometry(dp) & UNIFORM


# ---- DG path ---------------------------------------------------------------------------------------------------------------
IONS = [dict(name=f"i{k}", z=z, D=[1.0 + 0.3 * k, 0.6 + 0.2 * k]) for k, z in enumerate((1.0, -1.0, 2.0, -1.0))]
PARAMS = dict(dt=0.05, F=1.3, psi=0.8, C_M=0.7)


def _dg_problem(data, K, gamma=7.5):
    from knpemi.dg import DGProblem
    import knpemi_dg_oracle as dg
    mesh, ct, ft = data
    dp = DGProblem(mesh, ct, ft, [0, 1], [1], n_ions=K)
    dp.gamma = gamma
    o = dg.make_dg_oracle(mesh.x, mesh.cells, mesh.cell_type, dp.cell_sub, dp.mem_facets, dp.mem_tags)
    return dp, o


def _dg_pair(which, K, seed=41):
    """(base problem, re-oriented problem and its oracle, maps).  which = (M, distort): the unit cube of
    test_dg_gpu._hex_problem; which = "star3" / "star7": the star mesh scaled to unit size."""
    from knpemi.fem import Mesh
    from test_dg_gpu import _hex_problem
    if isinstance(which, str):
        m0, ct0, _ = hm.variant(which)[0]
        mesh0 = Mesh(m0.x / hm.L_BOX, m0.cells, m0.cell_type)
        ct0, ft0 = hm.tag_cells(mesh0, ct0.dense())
        from knpemi.dg import DGProblem
        base = DGProblem(mesh0, ct0, ft0, [0, 1], [1], n_ions=K)
        base.gamma = 7.5
    else:
        stretch = which[1] == "stretch"               # the axis-aligned cube scaled to edge lengths 1 : 0.6 : 1.7
        base, _ = _hex_problem(which[0], True, n_ions=K, gamma=7.5, distort=None if stretch else which[1])
        mesh0 = Mesh(base.mesh.x * np.array([1.0, 0.6, 1.7]), base.mesh.cells, "hexahedron") if stretch else base.mesh
        ct0, ft0 = hm.tag_cells(mesh0, base.cell_sub)
        if stretch:
            base, _ = _dg_problem((mesh0, ct0, ft0), K)
    data, maps = hm.reorient((mesh0, ct0, ft0), seed)
    dp, o = _dg_problem(data, K)
    return base, dp, o, maps


def _dg_assemble(dp, K, state, splitting):
    from test_dg_gpu import _push
    c_all, phi, phi_M, I_ch, src = state
    _push(dp, PARAMS, IONS[:K], c_all, phi, phi_M, I_ch, src)
    dp.assemble_emi(splitting)
    dp.assemble_knp(splitting)
    return [dp.matrix(w) for w in range(K)], [dp.rhs(w) for w in range(K)]


def _dg_errors(o, K, state, splitting, A, b):
    c_all, phi, phi_M, I_ch, src = state
    Ao, bo = o.assemble_emi(PARAMS, IONS[:K], c_all, phi_M, I_ch, splitting_scheme=splitting, gamma=7.5)
    As, bs = o.assemble_knp(PARAMS, IONS[:K], c_all, phi, phi_M, I_ch, splitting_scheme=splitting, gamma=7.5, f_source=src)
    errs = dict(A_emi=csr_rel_err(A[0], Ao), b_emi=rel_err(b[0], bo))
    for k in range(K - 1):
        errs[f"A_knp{k}"], errs[f"b_knp{k}"] = csr_rel_err(A[1 + k], As[k]), rel_err(b[1 + k], bs[k])
    return errs


def _mapped_state(base, dp, K, maps, seed=1):
    """A random state on the base problem and the same state on the re-oriented one."""
    from test_dg_gpu import _random_state
    vperm, cperm, G = maps
    state = _random_state(base, K, seed)
    p = hm.dg_dof_map(cperm, G)
    f, t = hm.dg_membrane_map(base.mem_facets, dp.mem_facets, vperm)
    cell = lambda a: a.ravel()[p].reshape(-1, 8)
    memf = lambda a: np.take_along_axis(a[f], t, axis=1)
    c_all, phi, phi_M, I_ch, src = state
    mapped = ([cell(c) for c in c_all], cell(phi), memf(phi_M), [memf(i) for i in I_ch], {k: cell(v) for k, v in src.items()})
    return state, mapped, p


DG_CASES = [((4, None), 3), ((5, None), 3), ((5, "stretch"), 3), ((4, "shear"), 3), ((5, "shear"), 4), ((4, "random"), 3),
            ((5, "random"), 2), ((4, "random"), 4), ((4, "rotate"), 3), ((5, "rotate"), 3), ("star3", 3), ("star7", 3)]


@pytest.mark.parametrize("splitting", [True, False])
@pytest.mark.parametrize("which,K", DG_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_dg_q1_assembly_on_reoriented_hexahedra_matches_oracle(hip_lib, which, K, splitting):
    """test_dg_q1_assembly_on_hexahedra_matches_oracle on the re-oriented and shuffled unit cube (None, "stretch" and
    "rotate": the box-mesh kernels, each cell with its own order of box_h -- on the cube all three lengths are equal, the
    other two have 1 : 0.6 : 1.7; "shear" and "random": the general ones) and on the star meshes: every facet pairing and
    vertex correspondence that knpemi_dg_create packs into finfo.  1e-10 of the largest entry.  Largest error measured on
    an MI355X over all cases: 1.7e-15 (matrices), 1.2e-14 (right-hand sides).  Tried once with the neighbour's axis replaced
    by the cell's own at decode sites of kernels_dg_hex.hip: in the general kernels (`ao`), "shear", "random" and the star
    meshes fail; in the box kernels (`box_h[nbr * 3 + ao]`), "stretch" and "rotate" fail and the cubes cannot; the tests on
    create_box meshes pass either way."""
    from test_dg_gpu import _random_state
    _, dp, o, _ = _dg_pair(which, K)
    st = hm.hex_statistics((dp.mesh,) + hm.tag_cells(dp.mesh, dp.cell_sub))
    assert st["neighbour_facets_per_axis"] == [6, 6, 6] and st["position_maps"] > 1 and 0.3 < st["left_handed"] < 0.7
    state = _random_state(dp, K, 1)
    A, b = _dg_assemble(dp, K, state, splitting)
    errs = _dg_errors(o, K, state, splitting, A, b)
    print(which, K, splitting, errs, "pairings", st["pairings"])
    assert max(errs.values()) < 1e-10, errs
    assert dp.nv == 8 and dp.nf == 4 and np.all(np.diff(dp.indptr) % 8 == 0)
    for r in (0, dp.n // 2, dp.n - 1):
        cols = dp.indices[dp.indptr[r]:dp.indptr[r + 1]]
        assert np.all(np.diff(cols) > 0) and r in cols


@pytest.mark.parametrize("which", [(5, None), (5, "stretch"), (4, "random"), (5, "rotate"), "star3", "star7"],
                         ids=lambda v: str(v).replace(" ", ""))
def test_dg_q1_device_results_are_equivariant(hip_lib, which):
    """No oracle in the loop: the device matrices and right-hand sides on the re-oriented mesh against the device results
    on the base mesh, through new dof (i, j) <-> old dof (cperm[i], G[i, j]) and the membrane nodes by their vertices.
    Bound: 1e-12 of the largest entry, as in the lanes-per-row test (the restatement's own figure for this comparison is
    3.2e-14 at worst, tests/test_hex_meshes_host.py, so ten times that stays below the bound).
    Largest measured on an MI355X: 1.0e-15 (matrices), 6.5e-15 (right-hand sides)."""
    K = 3
    base, dp, _, maps = _dg_pair(which, K)
    state, mapped, p = _mapped_state(base, dp, K, maps)
    for splitting in (True, False):
        A0, b0 = _dg_assemble(base, K, state, splitting)
        A1, b1 = _dg_assemble(dp, K, mapped, splitting)
        worst = {}
        for w in range(K):
            want = A0[w][p][:, p].tocsr()
            worst[f"A{w}"] = abs(A1[w] - want).max() / abs(want).max()
            worst[f"b{w}"] = np.abs(b1[w] - b0[w][p]).max() / np.abs(b0[w]).max()
        print(which, splitting, worst)
        assert max(worst.values()) <= 1e-12, worst


@pytest.mark.parametrize("splitting", [True, False])
def test_dg_q1_box_kernels_agree_with_the_general_kernels_on_the_reoriented_box(hip_lib, splitting, monkeypatch):
    """The re-oriented 5 x 5 x 5 box (cells 1 : 0.6 : 1.7) with the box-mesh kernels (hex_box is decided cell by cell,
    whatever the orientation; the constant facet frames differ between the two sides of a facet) and with KNPEMI_DG_HEX_GENERAL=1: within 1e-13 on
    the matrices and 1e-12 on the right-hand sides, both against the restatement, and not the same bits (two different
    kernels did run)."""
    from test_dg_gpu import _random_state
    K, out = 3, {}
    for name in ("box", "general"):
        if name == "general":
            monkeypatch.setenv("KNPEMI_DG_HEX_GENERAL", "1")
        else:
            monkeypatch.delenv("KNPEMI_DG_HEX_GENERAL", raising=False)
        _, dp, o, _ = _dg_pair((5, "stretch"), K)
        state = _random_state(dp, K, 1)
        A, b = _dg_assemble(dp, K, state, splitting)
        errs = _dg_errors(o, K, state, splitting, A, b)
        print(name, splitting, errs)
        assert max(errs.values()) < 1e-10, (name, errs)
        out[name] = A + b
    for w in range(K):
        assert csr_rel_err(out["box"][w], out["general"][w]) < 1e-13
        assert rel_err(out["box"][K + w], out["general"][K + w]) < 1e-12
    assert abs(out["box"][0] - out["general"][0]).max() > 0


def test_dg_update_and_membrane_dofs_on_reoriented_hexahedra(hip_lib):
    """The assertions of test_dg_update_matches_oracle on the re-oriented "random" cube."""
    import dg_cases as C
    from test_dg_gpu import _push, _random_state
    _, dp, o, _ = _dg_pair((4, "random"), 3)
    ions = C.ions_unit()
    params = dict(dt=0.1, F=1.0, psi=1.0, C_M=1.0)
    c_all, phi, phi_M, I_ch, _ = _random_state(dp, 3, 3)
    rho = (-1.0, [0.0, 0.4])
    _push(dp, params, ions, c_all, phi, phi_M, I_ch, rho=rho)
    rng = np.random.default_rng(5)
    c_new = [rng.random((dp.n_cells, dp.nv)) + 1.0 for _ in range(2)]
    dp.update(np.array(c_new))
    want, pm = o.update(ions, [rho[0] * r for r in rho[1]], c_new, phi)
    for k in range(3):
        assert rel_err(dp.get_concentration(k), want[k]) < 1e-14
    assert rel_err(dp.get_membrane_potential(), pm) < 1e-14
    e, i = dp.membrane_dofs()
    assert np.all(dp.cell_sub[e // dp.nv] == 0) and np.all(dp.cell_sub[i // dp.nv] == 1)
    assert np.array_equal(dp.X.reshape(-1, 3)[e.ravel()], dp.XM.reshape(-1, 3))
    assert np.array_equal(dp.X.reshape(-1, 3)[i.ravel()], dp.XM.reshape(-1, 3))


def test_dg_membrane_ode_step_on_reoriented_hexahedra(hip_lib):
    """The first step of test_dg_membrane_ode_sweep_matches_scipy_lsoda on the re-oriented "random" cube: the traces the
    sweep reads and the phi_M and I_ch it writes land on the membrane nodes the restatement's `traces` name."""
    import knpemi_oracle as ko
    from setup_problem import C_M, PSI
    _, dp, o, _ = _dg_pair((4, "random"), 3)
    m = ko.MODELS["hh_si"]
    ix = m["pidx"]
    names = ["Na", "K", "Cl"]
    ions = [dict(name=n, z=z, D=[1e-9, 1e-9]) for n, z in zip(names, (1.0, 1.0, -1.0))]
    dp.set_params(dict(dt=1e-4, F=96485.0, psi=PSI, C_M=C_M), ions)
    ins = (dp.cell_sub > 0)[:, None]
    vary = 1.0 + 0.05 * np.cos(6.0 * dp.X[:, :, 0]) * np.cos(4.0 * dp.X[:, :, 2])
    conc = [np.where(ins, 12.0, 100.0) * vary, np.where(ins, 125.0, 4.0) * vary, np.where(ins, 137.0, 104.0) * vary]
    for k in range(3):
        dp.set_concentration(k, conc[k])
    prow = np.array(m["params"], float)
    prow[ix["Cm"]] = C_M
    prow[ix["z_Na"]], prow[ix["z_K"]], prow[ix["z_Cl"]], prow[ix["psi"]] = 1.0, 1.0, -1.0, PSI
    ion_param = sum(([ix[f"{n}_e"], ix[f"{n}_i"], ix[f"I_ch_{n}"]] for n in names), [])
    dp.ode_bind(L.MODEL_HH_SI, m["states"], prow, ion_param, m["V"])
    nq = dp.nmf * dp.nf
    st_o, p_o = np.tile(np.array(m["states"]), (nq, 1)), np.tile(prow, (nq, 1))
    dp.ode_step(0.0, 1e-4, set_v=False)
    for k, n in enumerate(names):
        te, ti = o.traces(conc[k])
        assert np.ptp(te) > 0 and np.ptp(ti) > 0
        p_o[:, ix[f"{n}_e"]], p_o[:, ix[f"{n}_i"]] = te.ravel(), ti.ravel()
    ko.ode_sweep("hh_si", st_o, p_o, 0.0, 1e-4)
    st, pr = dp.ode_tables()
    for n in names:                                              # the traces the sweep read, bit for bit
        assert np.array_equal(pr[:, ix[f"{n}_e"]], p_o[:, ix[f"{n}_e"]]) and np.array_equal(pr[:, ix[f"{n}_i"]], p_o[:, ix[f"{n}_i"]])
    assert rel_err(st, st_o) < 1e-6
    ich = [ix["I_ch_Na"], ix["I_ch_K"], ix["I_ch_Cl"]]
    assert np.abs(pr[:, ich] - p_o[:, ich]).max() / max(np.abs(p_o[:, ich]).max(), 1e-3) < 1e-5
    assert rel_err(dp.get_membrane_potential().ravel(), st[:, m["V"]]) == 0.0
    for k, n in enumerate(names):
        assert np.array_equal(dp.get_channel_current(k).ravel(), pr[:, ix[f"I_ch_{n}"]])
    n_rhs, n_steps, n_failed = dp.ode_stats()
    assert n_failed == 0 and n_rhs > 0
