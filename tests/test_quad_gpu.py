"""GPU tests of the Q1 quadrilateral in 2-D (tests/quad_meshes.py): emi_rows_quad_v2 / knp_rows_quad_v2 in both geometry
variants and both lane counts, knpemi_create's set-up and refusals, the flux kernel's 2-D Q1 cell, whole steps and the
recorders that ride along.  Everything against the oracle (`"quadrilateral"` in oracle/knpemi_oracle.py, pinned by
tests/test_quad_host.py) at the project's tolerances; `knpemi_debug_geometry` and `knpemi_debug_layout` prove in every
test that the mesh reached the code it is there for."""
import contextlib
import ctypes
import functools
import io

import numpy as np
import pytest

import quad_meshes as qm
from helpers import TOL, Setup, assemble_both, csr_rel_err, ion_count_problem, rel_err
from knpemi import _lib as L

pytestmark = pytest.mark.gpu

AFFINE, UNIFORM = 2, 4   # knpemi_debug_geometry
# mesh -> (its data, every cell a parallelogram)
MESHES = {"rect": (lambda: qm.rect(1), True),
          "sheared": (lambda: qm.sheared(1), True),
          "jittered": (lambda: qm.jittered(1), False),
          "reoriented_jittered": (lambda: qm.reorient(qm.jittered(1), 41)[0], False),
          "star7": (lambda: qm.reorient(qm.star_quad(7, 3), 42)[0], False),
          "star3": (lambda: qm.reorient(qm.star_quad(3, 2), 43)[0], False)}


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return MESHES[name][0]()


def _setup(data, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        s = Setup("2d", 1, mesh_data=data, **kw)
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


# ---- 6: parity with the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MESHES))
def test_assembly_matches_oracle_on_quadrilaterals(hip_lib, name):
    """All five objects, both splitting modes, at 1e-10; AFFINE on the parallelogram meshes only, UNIFORM never; two lanes
    per row.  star7 has a vertex of valence 7 on the membrane, star3 one of valence 3.
    Largest device-versus-oracle error measured on an MI355X (both modes):
        rect                A_emi 2.5e-15  P_emi 2.5e-15  b_emi 6.5e-14  A_knp 2.2e-15  b_knp 3.1e-15   flags 2
        sheared             A_emi 2.9e-15  P_emi 2.9e-15  b_emi 6.9e-14  A_knp 2.2e-15  b_knp 3.1e-15   flags 2
        jittered            A_emi 2.6e-15  P_emi 2.6e-15  b_emi 6.3e-14  A_knp 2.2e-15  b_knp 3.2e-15   flags 0
        reoriented_jittered A_emi 2.4e-15  P_emi 2.4e-15  b_emi 6.0e-14  A_knp 1.8e-15  b_knp 2.3e-15   flags 0
        star7               A_emi 7.0e-16  P_emi 7.0e-16  b_emi 5.9e-14  A_knp 1.3e-15  b_knp 9.0e-16   flags 0
        star3               A_emi 8.0e-16  P_emi 8.0e-16  b_emi 3.4e-14  A_knp 2.3e-15  b_knp 1.4e-15   flags 0
    Layout: longest row 11 (Laplacian 9) on the rectangle, 15 (Laplacian 12, 3 pairs per lane) on star7."""
    s = _setup(_mesh(name))
    assert s.mesh.cell_type == "quadrilateral"
    for splitting in (True, False):
        errs, _ = assemble_both(s, splitting)
        flags, lay = _geometry(s.a_emi.dp), _layout(s.a_emi.dp)
        print(name, splitting, errs, "flags", flags, lay)
        assert bool(flags & AFFINE) == MESHES[name][1] and not flags & UNIFORM and not flags & 1, flags
        assert lay["lanes_per_row"] == 2
        assert max(errs.values()) < TOL, errs
    assert lay["lds_emi"] > 0 and lay["lds_knp"] > 0
    if name.startswith("reoriented") or name.startswith("star"):
        assert 0.3 < qm.left_handed_fraction(s.mesh) < 0.7
    if name == "star7":                              # the valence-7 vertex lies on the membrane: 5 of its cells in the ECS
        assert lay["longest_laplacian_row"] == 12 and lay["pairs_per_lane"] == 3


# ---- 7: ion counts, membrane paths, lane counts -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(mesh, n_ions):
    s = ion_count_problem(_mesh(mesh), n_ions)
    o, P, params, ions = s.oracle
    c_all, phi, phiM, mm = s.oracle_fields
    return o.assemble_emi(P, params, ions, c_all, phiM, mm) + o.assemble_knp(P, params, ions, c_all, phi, phiM, mm, s.dt)


def _solvers(s):
    from knpemi.pdeSolver import create_solver_emi, create_solver_knp
    emi = create_solver_emi(s.a_emi, s.L_emi, s.phi, [], s.subdomain_list, None, p=s.p_emi, direct=False)
    knp = create_solver_knp(s.a_knp, s.L_knp, s.c, [], s.subdomain_list, None, p=s.p_knp)
    return emi, knp


def _emi_errors(emi, ref):
    A, b = emi.assemble()
    return dict(A_emi=csr_rel_err(A, ref[0]), P_emi=csr_rel_err(emi.P, ref[1]), b_emi=rel_err(b, ref[2]))


def _knp_errors(dp, ref):
    return dict(A_knp=csr_rel_err(dp.csr(L.A_KNP), ref[3]), b_knp=rel_err(dp.rhs(L.B_KNP), ref[4]))


@pytest.mark.parametrize("n_ions", [2, 3, 4])
@pytest.mark.parametrize("mesh", ["rect", "reoriented_jittered"])
def test_knp_rows_of_every_ion_count_and_membrane_path_match_oracle(hip_lib, monkeypatch, mesh, n_ions):
    """tests/test_launch_table_gpu.py's test on quadrilaterals: K - 1 = 1..3 solved ions x the three sources of the membrane
    integrals of b_knp, in GEO 1 (rect) and GEO 0.  The stored system is overwritten with NaN before each optional path."""
    ref = _oracle(mesh, n_ions)
    for classic in (False, True):
        if classic:
            monkeypatch.setenv("KNPEMI_BLOCK_CLASSIC", "1")
        else:
            monkeypatch.delenv("KNPEMI_BLOCK_CLASSIC", raising=False)
        s = ion_count_problem(_mesh(mesh), n_ions)
        emi, knp = _solvers(s)
        dp = knp.dp
        A, _ = knp.assemble()
        assert _layout(dp)["lanes_per_row"] == 2 and bool(_geometry(dp) & AFFINE) == MESHES[mesh][1]
        assert A.shape[0] == (n_ions - 1) * ref[0].shape[0]
        errs = {"default": _knp_errors(dp, ref)}
        errs["default"].update(_emi_errors(emi, ref))
        dp.set_csr_values(L.A_KNP, np.full(A.nnz, np.nan))
        dp.set_rhs(L.B_KNP, np.full(A.shape[0], np.nan))
        if classic:
            L.check(dp.lib.knpemi_set_option(dp.h, L.OPT_FUSE_MEMBRANE, 1))
            dp.assemble_knp()
            errs["fused"] = _knp_errors(dp, ref)
        else:
            dp.assemble_knp(early_membrane=True)
            errs["early"] = _knp_errors(dp, ref)
        print(mesh, n_ions, "classic blocks" if classic else "clustered blocks", errs)
        for path, e in errs.items():
            assert max(e.values()) < TOL, (path, e)


@pytest.mark.parametrize("lpr", [2, 4])
@pytest.mark.parametrize("mesh", ["rect", "reoriented_jittered"])
def test_both_lane_counts_with_three_ions_match_oracle(hip_lib, monkeypatch, mesh, lpr):
    monkeypatch.setenv("KNPEMI_LPR", str(lpr))
    ref = _oracle(mesh, 3)
    emi, knp = _solvers(ion_count_problem(_mesh(mesh), 3))
    errs = _emi_errors(emi, ref)
    knp.assemble()
    errs.update(_knp_errors(knp.dp, ref))
    print(mesh, lpr, errs)
    assert _layout(knp.dp)["lanes_per_row"] == lpr
    assert max(errs.values()) < TOL, errs


def test_lane_counts_that_are_not_built_are_refused_by_name(hip_lib, monkeypatch):
    """Eight lanes per row: no quadrilateral kernel.  KNPEMI_EINVAL names the combination and the cell kind."""
    monkeypatch.setenv("KNPEMI_LPR", "8")
    emi, knp = _solvers(ion_count_problem(_mesh("rect"), 3))
    with pytest.raises(L.KnpemiError, match="8 lanes per row.*quadrilaterals") as e:
        knp.assemble()
    assert e.value.code == L.EINVAL
    with pytest.raises(L.KnpemiError, match="quadrilaterals"):
        emi.assemble()


# ---- 8: GEO 1 against GEO 0 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sheared", "rect"])
def test_closed_forms_agree_with_the_quadrature_on_parallelograms(hip_lib, monkeypatch, name):
    """The closed forms against KNPEMI_QUAD_GENERAL=1 on the same mesh: matrices within 1e-13, right-hand sides within
    1e-12 (the bounds of the hexahedral counterpart), and not the same bits: two different kernels ran.
    Measured: matrices 1.1e-15 (sheared) / 3.3e-16 (rect), right-hand sides 3.6e-15 / 3.7e-15."""
    out = {}
    for general in (False, True):
        if general:
            monkeypatch.setenv("KNPEMI_QUAD_GENERAL", "1")
        else:
            monkeypatch.delenv("KNPEMI_QUAD_GENERAL", raising=False)
        s = _setup(_mesh(name))
        errs, objs = assemble_both(s)
        assert bool(_geometry(s.a_emi.dp) & AFFINE) == (not general)
        assert max(errs.values()) < TOL, errs
        out[general] = objs
    d = [csr_rel_err(out[False][i], out[True][i]) for i in (0, 1, 3)] + [rel_err(out[False][i], out[True][i]) for i in (2, 4)]
    print(name, d)
    assert max(d[:3]) < 1e-13 and max(d[3:]) < 1e-12
    assert abs(out[False][0] - out[True][0]).max() > 0


# ---- 9: reproducibility, block shapes -------------------------------------------------------------------------------------
def test_bit_reproducibility_and_block_shapes(hip_lib, monkeypatch):
    res = {}
    for classic in (False, True):
        if classic:
            monkeypatch.setenv("KNPEMI_BLOCK_CLASSIC", "1")
        else:
            monkeypatch.delenv("KNPEMI_BLOCK_CLASSIC", raising=False)
        s = _setup(_mesh("reoriented_jittered"))
        _, first = assemble_both(s)
        first = [_values(a).copy() for a in first]
        _, second = assemble_both(s)
        for a, b in zip(first, second):
            assert np.array_equal(a, _values(b))
        res[classic] = first
    for a, b in zip(res[False], res[True]):
        assert np.array_equal(a, b)


# ---- 10: re-orientation invariance on the device -----------------------------------------------------------------------------
def test_device_results_are_invariant_under_reorientation(hip_lib):
    """rect(1) against its re-oriented, renumbered twin, no oracle in the loop: fields moved by the vertex permutation,
    both systems agree after permuting rows and columns, at 1e-12.  The twin takes the closed forms too.
    Measured: matrices 3.3e-16, right-hand sides 3.1e-16."""
    data, (vperm, cperm, G) = qm.reorient(qm.rect(1), 44)
    s0, s1 = _setup(qm.rect(1)), _setup(data)
    p = qm.transfer_cg_fields(s0, s1, vperm)
    _, o0 = assemble_both(s0)
    _, o1 = assemble_both(s1)
    assert _geometry(s1.a_emi.dp) & AFFINE and 0.3 < qm.left_handed_fraction(s1.mesh) < 0.7
    n0 = len(p[0])
    pe = np.concatenate([p[0], n0 + p[1]])                       # EMI dofs: [ECS | cell]
    pk = np.concatenate([k * n0 + p[0] for k in range(2)] + [2 * n0 + k * len(p[1]) + p[1] for k in range(2)])
    worst = dict(A_emi=csr_rel_err(o1[0], o0[0][pe][:, pe].tocsr()), P_emi=csr_rel_err(o1[1], o0[1][pe][:, pe].tocsr()),
                 b_emi=rel_err(o1[2], o0[2][pe]), A_knp=csr_rel_err(o1[3], o0[3][pk][:, pk].tocsr()),
                 b_knp=rel_err(o1[4], o0[4][pk]))
    print(worst)
    assert max(worst.values()) < 1e-12, worst


# ---- 11: patch test on the device ---------------------------------------------------------------------------------------------
def test_patch_test_on_the_device(hip_lib):
    """A_emi of jittered(2), read back from the handle, applied to a linear potential with constant concentrations: the
    rows of vertices whose four cells lie in one sub-domain and off the membrane vanish to 1e-13 of max|A| max|u|.
    Measured: 3.1e-16 on the 613 rows."""
    from test_quad_host import interior_rows
    data = qm.jittered(2)
    with contextlib.redirect_stdout(io.StringIO()):
        s = Setup("2d", 2, mesh_data=data)                        # constant initial concentrations, not perturbed
    from knpemi.pdeSolver import create_solver_emi
    emi = create_solver_emi(s.a_emi, s.L_emi, s.phi, s.entity_maps, s.subdomain_list, None, p=s.p_emi, direct=False)
    A, _ = emi.assemble()
    assert not _geometry(emi.dp) & AFFINE
    rows, x = interior_rows(s)
    u = 3.0 + 2.0e5 * x[:, 0] - 1.5e5 * x[:, 1]
    r = np.abs((A @ u)[rows]).max() / (np.abs(A.data).max() * np.abs(u).max())
    print("interior rows", len(rows), "residual", r)
    assert len(rows) == 613 and r < 1e-13


# ---- 12: refusals ------------------------------------------------------------------------------------------------------------
def _fresh_rect():
    m0, ct0, ft0 = qm.rect(1)
    from knpemi.fem import Mesh, MeshTags
    mesh = Mesh(m0.x.copy(), m0.cells.copy(), "quadrilateral")
    ct = MeshTags(mesh, 2, ct0.indices.copy(), ct0.values.copy())
    ft = MeshTags(mesh, 1, ft0.indices.copy(), ft0.values.copy())
    with contextlib.redirect_stdout(io.StringIO()):
        return Setup("2d", 1, mesh_data=(mesh, ct, ft), build_forms=False)


def test_knpemi_create_refusals_leave_the_process_usable(hip_lib):
    from knpemi.device import DeviceProblem
    s = _fresh_rect()                                # every cell in counter-clockwise order: the bilinear map folds
    for t in s.subdomain_list:
        cells = s.subdomain_list[t]["mesh_sub"].cells
        cells[:] = cells[:, [0, 1, 3, 2]]
    with pytest.raises(L.KnpemiError, match="quadrilateral 0 of sub-domain 0.*tensor-product vertex order") as e:
        DeviceProblem(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list)
    assert e.value.code == L.EINVAL
    s = _fresh_rect()                                # one non-convex cell: vertex v11 of cell 5 pulled past the diagonal
    sub = s.subdomain_list[0]["mesh_sub"]
    c = sub.cells[5]
    sub.x[c[3]] = sub.x[c[0]] + 0.2 * (sub.x[c[3]] - sub.x[c[0]])
    with pytest.raises(L.KnpemiError, match="quadrilateral") as e:
        DeviceProblem(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list)
    assert e.value.code == L.EINVAL and "sub-domain 0" in str(e.value)
    n1 = np.array([1], np.int32)                     # cell_kind 3 with gdim 3
    desc = L.ProblemDesc(gdim=3, cell_kind=L.QUADRILATERAL, n_sub=1, n_ions=3, n_vert=L.iptr(n1), n_cell=L.iptr(n1))
    h = ctypes.c_void_p()
    assert hip_lib.knpemi_create(ctypes.byref(desc), 0, ctypes.byref(h)) == L.EINVAL and not h
    s = _fresh_rect()                                # and a valid problem after the three refusals
    dp = DeviceProblem(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list)
    assert dp.h and _geometry(dp) & AFFINE


# ---- 13: whole steps -----------------------------------------------------------------------------------------------------------
def test_device_resident_time_loop_matches_oracle_on_quadrilaterals(hip_lib):
    """test_device_resident_time_loop_matches_oracle on rect(1): ten steps with device solves (1e-12, 1e-13) against
    OracleRun, that test's tolerances, every solve below 1 000 iterations, and the fused sweep launch declines.
    Measured: 2 CG iterations per EMI solve, 3 BiCGStab iterations per KNP solve (439 unknowns: one AMG level)."""
    import driver
    from knpemi.stepper import DeviceStepper
    with contextlib.redirect_stdout(io.StringIO()):
        s = Setup("2d", 1, g_syn=10.0, mesh_data=qm.rect(1))
    o, P, params, ions = s.oracle()
    c_all, _, _, _ = s.oracle_fields()
    ode = s.mem_models[0]['ode']
    mask = np.array([x[0] < 20e-6 for x in ode.dof_locations])
    run = driver.OracleRun(P, params, ions, "hh_si", c_all, ode.states.copy(), ode.parameters.copy(),
                           ode.dof_locations, mask, {o.MODELS["hh_si"]["pidx"]["stim_amplitude"]: 10.0},
                           {'z': -1, 0: 0.0, 1: 0.0})
    for t in s.subdomain_list:
        for k in range(2):
            s.c[t][k].x.array[:] = s.c_prev[t][k].x._a
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev,
                       device_solves=(1e-12, 1e-13))
    st.add_membrane_model(ode, s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
    fused = []
    for k in range(10):
        st.step()
        fused.append(st.last_fused)
        run.step()
    st.download()
    print("iterations", st.iterations, "fused", fused)
    assert fused[0] == 0 and not any(fused)
    assert rel_err(s.phi_M_prev[1].x._a, run.phiM[1]) < 1e-6
    for t in (0, 1):
        for k in range(2):
            assert rel_err(s.c_prev[t][k].x._a, run.c_all[t][k]) < 1e-8
    assert rel_err(ode.states, run.states) < 1e-6
    assert all(it[1] <= 1000 for it in st.iterations)


def test_device_stepper_matches_dropin_path_on_quadrilaterals(hip_lib):
    """test_device_stepper_matches_dropin_path on rect(1): three steps, bit for bit."""
    from knpemi import update_ode_variables, update_pde_variables
    from knpemi.pdeSolver import create_solver_emi, create_solver_knp
    from knpemi.stepper import DeviceStepper
    res = []
    for mode in ("dropin", "stepper"):
        s = _setup(qm.rect(1), g_syn=10.0)
        for t in s.subdomain_list:
            for k in range(2):
                s.c[t][k].x.array[:] = s.c_prev[t][k].x._a * 1.001
        s.phi[1].x.array[:] += -0.0744
        ode = s.mem_models[0]['ode']
        with contextlib.redirect_stdout(io.StringIO()):
            if mode == "stepper":
                st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi,
                                   s.phi_M_prev)
                st.add_membrane_model(ode, s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
                for _ in range(3):
                    st.step()
                    assert not st.last_fused         # 0: asked and declined (the first step); None: not asked again
                b_emi, b_knp = st.dp.rhs(0), st.dp.rhs(1)
                st.download()
            else:
                emi = create_solver_emi(s.a_emi, s.L_emi, s.phi, s.entity_maps, s.subdomain_list, None, p=s.p_emi, direct=False)
                knp = create_solver_knp(s.a_knp, s.L_knp, s.c, s.entity_maps, s.subdomain_list, None, p=s.p_knp)
                for k in range(3):
                    update_ode_variables(ode, s.c_prev, s.phi_M_prev[1], s.ion_list, s.subdomain_list, s.mesh, s.ct, 1, k)
                    ode.step_lsoda(s.dt, s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
                    ode.get_membrane_potential(s.phi_M_prev[1])
                    for ion, f in s.mem_models[0]['I_ch_k'].items():
                        ode.get_parameter("I_ch_" + ion, f)
                    _, b_emi = emi.assemble()
                    _, b_knp = knp.assemble()
                    update_pde_variables(s.c, s.c_prev, s.phi, s.phi_M_prev, s.physical_parameters, s.ion_list,
                                         s.subdomain_list, s.mesh, s.ct)
        res.append((ode.states.copy(), s.phi_M_prev[1].x._a.copy(), s.c_prev[1][0].x._a.copy(), b_emi, b_knp))
    for a, b in zip(*res):
        assert np.array_equal(a, b)


# ---- 14: fluxes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["jittered", "left_handed_rect"])
def test_flux_fields_and_row_match_the_restatement(hip_lib, name):
    """tests/test_flux_gpu.py::test_fields_and_row_match_the_restatement on general cells and on rect(1) with every cell
    mirrored (left-handed): device fields and row against IonFluxes.compute_host at 1e-10.
    Measured: fields 3.8e-16 / 3.0e-16, row 4.5e-15 / 2.4e-15."""
    from knpemi import IonFluxes
    from test_flux_gpu import _host_state, _read, _rel, _row_err, _stepper
    data = qm.jittered(1) if name == "jittered" else qm.reorient(qm.rect(1), 45, symmetry=qm.MIRROR)[0]
    s = _setup(data)
    assert qm.left_handed_fraction(s.mesh) == (0.0 if name == "jittered" else 1.0)
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
            assert dev[tag][key].shape == (fl.n_cells(tag), 2)
            worst = max(worst, _rel(dev[tag][key], fields[tag][key]))
    e_row = _row_err(fl, buf[0], want)
    print(name, "fields", worst, "row", e_row)
    assert worst < TOL and e_row < TOL


# ---- 15: recorders ride along ---------------------------------------------------------------------------------------------------
def test_recorders_ride_along(hip_lib):
    """Five steps on rect(1) with Observables (the integral of every solved ion, and of a constant) and MembraneExchange
    attached: the mass budget of every solved ion closes to the residual bound of tests/test_exchange_gpu.py, the
    integral of a constant field is the sub-domain's area."""
    import exchange_cases as xc
    from knpemi import Observables
    from test_exchange_gpu import BUDGET_FLOOR
    from test_flux_gpu import _stepper
    with contextlib.redirect_stdout(io.StringIO()):
        s = Setup("2d", 1, g_syn=10.0, mesh_data=qm.rect(1))
    for t in s.subdomain_list:
        for k in range(2):
            s.c[t][k].x.array[:] = s.c_prev[t][k].x._a
    st = _stepper(s, device_solves=(1e-9, 1e-10))
    st.add_membrane_model(s.mem_models[0]["ode"], s.stim_params["stimulus"], s.stim_params["stimulus_locator"])
    dp = st.dp
    ex = xc.exchange(s)
    st.exchange(ex, every=1, capacity=8, t0=0.25, fields=True)
    obs = Observables(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list)
    ex.observe_masses(obs)
    for tag in (0, 1):                               # integral / average = the measure the device integrates over
        obs.reduce(f"mean/{tag}/K", "c", tag, "average", ion="K")
    st.observe(obs, every=1, t0=0.25)
    seen, resid = [], []
    solve = st.solve_knp

    def solve_knp(dp):
        st.download()
        seen.append(xc.host_state(s))
        solve(dp)
        A, b = dp.csr(L.A_KNP), dp.rhs(L.B_KNP)
        resid.append(A @ dp.get_solution(L.B_KNP, A.shape[0]) - b)
    st.solve_knp = solve_knp
    with contextlib.redirect_stdout(io.StringIO()):
        for k in range(5):
            st.step()
    bud = ex.budget(obs.series())
    assert set(bud) == {"t", "1/K", "1/Cl", "0/K", "0/Cl"} and len(bud["t"]) == 5
    checked = 0
    for i, (snap, r) in enumerate(zip(seen, resid)):
        fields, _ = ex.compute_host(**snap)
        for k, name in enumerate(("K", "Cl")):
            for sub, side in ((0, "ecs"), (1, "ics")):
                defect = bud[f"{sub}/{name}"][i]
                if np.isnan(defect):                 # the first row has no mass at t - dt
                    assert i == 0
                    continue
                n = int(dp.n_vert[sub])
                r_block = r[2 * int(dp.voff[sub]) + k * n:][:n]
                flux = float((fields[1]["area"] * np.abs(fields[1][f"{name}/{side}"])).sum())
                bound = np.sqrt(n) * np.linalg.norm(r_block) + BUDGET_FLOOR * flux
                print("step", i + 1, name, side, "defect", defect, "bound", bound)
                assert abs(defect) <= bound
                checked += 1
    assert checked >= 16
    # integral of a constant = the sub-domain's area: the device's integral over its average, and the weights themselves
    ser = obs.series()
    area = {0: 62e-6 * 4e-6 - 60e-6 * 2e-6, 1: 60e-6 * 2e-6}
    for tag in (0, 1):
        got = ser[ex.mass_key(tag, "K")] / ser[f"mean/{tag}/K"]
        assert np.abs(got / area[tag] - 1.0).max() < 1e-12
        assert abs(obs.integral_weights(False, tag).sum() / area[tag] - 1.0) < 1e-12
