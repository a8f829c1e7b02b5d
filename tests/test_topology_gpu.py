"""GPU tests of the membrane topologies of dense tissue (tests/topology_meshes.py) on every cell kind: cells that meet at a
corner or along an edge, a pinched sub-domain, cells sharing facets, a cell cut by the bounding box, the smallest cell, several
membrane tags on one cell, an empty cellular sub-domain -- each plain (lattice, uniform and affine kernels) and jittered
(general kernels).  Everything against the oracle (pinned on these meshes by tests/test_topology_host.py) at the project's
tolerances; `knpemi_debug_geometry` proves in every test which kernels ran.  And the refusal of a tagged facet between two
cells by knpemi_create itself."""
import contextlib
import ctypes as C
import functools
import io

import numpy as np
import pytest

import exchange_cases as xc
import topology_cases as tc
import topology_meshes as tm
from helpers import TOL, check_facet_integrals_of_the_write_back_launch, csr_rel_err, rel_err
from knpemi import _lib as L

pytestmark = pytest.mark.gpu

LATTICE_TETS, AFFINE, UNIFORM = 1, 2, 4     # knpemi_debug_geometry
FLAGS = {"triangle": 0, "quadrilateral": AFFINE, "tetrahedron": LATTICE_TETS, "hexahedron": AFFINE | UNIFORM}   # plain
NAMES = ("A_emi", "P_emi", "b_emi", "A_knp", "b_knp")
FORMS = (False, True)
MEMBRANE_CASES = ("edge_touch", "pinch", "to_boundary", "tags")


def _geometry(dp):
    flags = C.c_int(-1)
    L.check(dp.lib.knpemi_debug_geometry(dp.h, C.byref(flags)))
    return flags.value & (LATTICE_TETS | AFFINE | UNIFORM)


def _layout(dp):
    out = (C.c_int * 8)()
    L.check(dp.lib.knpemi_debug_layout(dp.h, out, 8))
    return dict(zip(("longest_row", "lanes_per_row", "pairs_per_lane", "block_vertices", "membrane_entries", "lds_emi",
                     "lds_knp", "longest_laplacian_row"), out))


def _assert_kernels(dp, kind, jittered):
    """Plain grids reach the lattice (tetrahedra), uniform (hexahedra) and affine (quadrilaterals) kernels, jittered
    ones the general kernels; triangles have one variant."""
    assert _geometry(dp) == (0 if jittered else FLAGS[kind]), (_geometry(dp), kind, jittered)


def _build(kind, case, jittered):
    import adapters
    s = tc.build(kind, case, jittered)
    s.oracle = lambda: adapters.oracle_problem(s)
    s.oracle_fields = lambda: adapters.oracle_fields(s)
    return s


@functools.lru_cache(maxsize=None)
def _reference(kind, case, jittered, splitting=True):
    """The oracle's five objects: computed once per mesh and mode (the fields are seeded), left unchanged."""
    objs = tc.oracle_objects(tc.build(kind, case, jittered, forms=False), splitting)
    for a in objs:
        (a.data if hasattr(a, "indptr") else a).setflags(write=False)
    return objs


def _solvers(s):
    from knpemi.pdeSolver import create_solver_emi, create_solver_knp
    emi = create_solver_emi(s.a_emi, s.L_emi, s.phi, [], s.subdomain_list, None, p=s.p_emi, direct=False)
    knp = create_solver_knp(s.a_knp, s.L_knp, s.c, [], s.subdomain_list, None, p=s.p_knp)
    return emi, knp


def _device_objects(s, splitting=True):
    for f in (s.a_emi, s.a_knp):
        f.shared['splitting_scheme'] = splitting
    emi, knp = _solvers(s)
    A, b = emi.assemble()
    Ak, bk = knp.assemble()
    return (A, emi.P, b, Ak, bk), knp.dp


def _errors(objs, ref):
    return {k: (rel_err(a, r) if isinstance(r, np.ndarray) else csr_rel_err(a, r)) for k, a, r in zip(NAMES, objs, ref)}


def _knp_errors(dp, ref):
    return dict(A_knp=csr_rel_err(dp.csr(L.A_KNP), ref[3]), b_knp=rel_err(dp.rhs(L.B_KNP), ref[4]))


def _values(a):
    return np.asarray(a.data if hasattr(a, "indptr") else a)


# ---- parity with the oracle --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jittered", FORMS)
@pytest.mark.parametrize("case", list(tm.CASES))
@pytest.mark.parametrize("kind", tm.KINDS)
def test_assembly_matches_oracle(hip_lib, kind, case, jittered):
    """The five objects, both splitting modes, at 1e-10 on 4 kinds x 7 cases x {plain, jittered}.
    Largest device-versus-oracle error measured on an MI355X over the seven cases and both modes:
        triangle plain       A_emi 1.7e-15  P_emi 1.7e-15  b_emi 3.4e-13  A_knp 1.5e-15  b_knp 1.4e-15   flags 0
        triangle jittered    A_emi 1.7e-15  P_emi 1.7e-15  b_emi 2.7e-13  A_knp 1.8e-15  b_knp 1.6e-15   flags 0
        quadrilateral plain  A_emi 1.8e-15  P_emi 1.8e-15  b_emi 2.7e-13  A_knp 1.5e-15  b_knp 1.6e-15   flags 2
        quadrilateral jitt.  A_emi 1.3e-15  P_emi 1.3e-15  b_emi 3.5e-13  A_knp 1.6e-15  b_knp 1.3e-15   flags 0
        tetrahedron plain    A_emi 1.7e-15  P_emi 1.7e-15  b_emi 1.7e-13  A_knp 1.7e-15  b_knp 1.7e-15   flags 1
        tetrahedron jitt.    A_emi 2.1e-15  P_emi 2.1e-15  b_emi 1.1e-13  A_knp 2.4e-15  b_knp 2.4e-15   flags 0
        hexahedron plain     A_emi 1.8e-15  P_emi 1.8e-15  b_emi 2.0e-13  A_knp 2.1e-15  b_knp 2.2e-15   flags 6
        hexahedron jittered  A_emi 1.4e-15  P_emi 1.4e-15  b_emi 1.4e-13  A_knp 1.5e-15  b_knp 1.5e-15   flags 0
    Layout: longest row 12 / 13 / 26 / 39 (triangle, quadrilateral, tetrahedron, hexahedron), most membrane entries of a
    row 4 / 4 / 10 / 6, on the pinch vertex -- far from the 255 entries and 8-bit offsets a row can address."""
    s = _build(kind, case, jittered)
    for splitting in (True, False):
        objs, dp = _device_objects(s, splitting)
        errs = _errors(objs, _reference(kind, case, jittered, splitting))
        lay = _layout(dp)
        print(kind, case, "jittered" if jittered else "plain", "splitting" if splitting else "no splitting", errs,
              "flags", _geometry(dp), "longest row", lay["longest_row"], "membrane entries", lay["membrane_entries"])
        _assert_kernels(dp, kind, jittered)
        assert lay["lanes_per_row"] == (2 if s.mesh.gdim == 2 else 4)
        assert max(errs.values()) < TOL, errs
    assert (lay["membrane_entries"] == 0) == (case == "empty")


# ---- the membrane paths of b_knp ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jittered", FORMS)
@pytest.mark.parametrize("case", MEMBRANE_CASES)
@pytest.mark.parametrize("kind", tm.KINDS)
def test_membrane_paths_of_b_knp_match_oracle(hip_lib, monkeypatch, kind, case, jittered):
    """The three sources of the membrane integrals of b_knp: the facet kernel (default), the two-part early form, and the
    integrals inside the row block (KNPEMI_OPT_FUSE_MEMBRANE with KNPEMI_BLOCK_CLASSIC=1).  Before each optional path the
    stored system is overwritten with NaN, so what is compared is what that path wrote."""
    ref = _reference(kind, case, jittered)
    for classic in (False, True):
        if classic:
            monkeypatch.setenv("KNPEMI_BLOCK_CLASSIC", "1")
        else:
            monkeypatch.delenv("KNPEMI_BLOCK_CLASSIC", raising=False)
        s = _build(kind, case, jittered)
        _, knp = _solvers(s)
        dp = knp.dp
        A, _ = knp.assemble()                # pushes every field; the facet kernel
        _assert_kernels(dp, kind, jittered)
        errs = {"facet kernel": _knp_errors(dp, ref)}
        dp.set_csr_values(L.A_KNP, np.full(A.nnz, np.nan))
        dp.set_rhs(L.B_KNP, np.full(A.shape[0], np.nan))
        if classic:
            L.check(dp.lib.knpemi_set_option(dp.h, L.OPT_FUSE_MEMBRANE, 1))
            dp.assemble_knp()
            errs["fused"] = _knp_errors(dp, ref)
        else:
            dp.assemble_knp(early_membrane=True)
            errs["early"] = _knp_errors(dp, ref)
        print(kind, case, "jittered" if jittered else "plain", "classic blocks" if classic else "clustered blocks", errs)
        for path, e in errs.items():
            assert max(e.values()) < TOL, (path, e)


@pytest.mark.parametrize("jittered", FORMS)
@pytest.mark.parametrize("case", MEMBRANE_CASES)
@pytest.mark.parametrize("kind", tm.KINDS)
def test_folded_integrals_of_the_write_back_launch(hip_lib, kind, case, jittered):
    """KNPEMI_OPT_FOLD_MEMBRANE: b_knp with the facet integrals formed by the launch that writes a potential back, bit
    for bit against the facet kernel and at 1e-10 against the oracle (the stored right-hand side is NaN before each)."""
    check_facet_integrals_of_the_write_back_launch(_build(kind, case, jittered))


# ---- the Robin term of b_emi as a launch of its own --------------------------------------------------------------------------
@pytest.mark.parametrize("jittered", FORMS)
@pytest.mark.parametrize("case", ["edge_touch", "pinch"])
@pytest.mark.parametrize("kind", tm.KINDS)
def test_separate_robin_term_kernel_equals_the_fused_one(hip_lib, kind, case, jittered):
    """knpemi_assemble_emi_membrane_rhs (emi_membrane_rhs_kernel) behind KNPEMI_SKIP_MEMBRANE_RHS against the b_emi the
    row kernel forms in one launch: the same bits, as the stepper tests hold it, in both splitting modes -- on ECS rows
    coupled to the membranes of two cells and on the non-manifold membrane."""
    s = _build(kind, case, jittered)
    for splitting in (True, False):
        s.a_emi.shared['splitting_scheme'] = splitting
        emi, _ = _solvers(s)
        _, fused = emi.assemble()            # pushes every field this mode reads; one launch
        fused = np.array(fused)
        dp = emi.dp
        flags = L.WANT_P | (0 if splitting else L.NO_SPLITTING)
        dp.set_rhs(L.B_EMI, np.full(len(fused), np.nan))
        L.check(dp.lib.knpemi_assemble_emi(dp.h, flags | L.SKIP_MEMBRANE_RHS))
        volume = dp.rhs(L.B_EMI).copy()
        L.check(dp.lib.knpemi_assemble_emi_membrane_rhs(dp.h, flags))
        both = dp.rhs(L.B_EMI).copy()
        assert np.isfinite(fused).all() and np.array_equal(both.view(np.uint64), fused.view(np.uint64))
        assert not np.array_equal(volume, fused)
        assert rel_err(fused, _reference(kind, case, jittered, splitting)[2]) < TOL


# ---- traces and the end-of-step update ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["edge_touch", "pinch", "to_boundary"])
@pytest.mark.parametrize("kind", tm.KINDS)
def test_trace_and_end_of_step_update_match_oracle(hip_lib, kind, case):
    """knpemi_trace and knpemi_update_pde on the jittered meshes at the 1e-14 of test_three_subdomains_two_cell_types: the
    eliminated ion from electroneutrality, phi_M <- tr(phi_i) - tr(phi_e) on membranes that share ECS vertices."""
    import adapters
    from knpemi import update_pde_variables
    s = _build(kind, case, True)
    o, P, params, ions = adapters.oracle_problem(s)
    c_all, phi, phiM, _ = adapters.oracle_fields(s)
    dp = s.a_emi.dp
    tags = list(s.subdomain_list)
    for t in tags[1:]:
        qe, qi = dp.trace(dp.sub_index[t], phi[0], c_all[t][0])
        we, wi = P.trace(t, phi[0], c_all[t][0])
        assert len(qe) == P.NQ[t] > 0 and np.array_equal(qe, we) and np.array_equal(qi, wi)
    for t in tags:
        for k in range(2):
            s.c[t][k].x.array[:] = s.c_prev[t][k].x._a * 1.01
    c_new = {t: [f.x._a.copy() for f in s.c[t]] for t in tags}
    update_pde_variables(s.c, s.c_prev, s.phi, s.phi_M_prev, s.physical_parameters, s.ion_list, s.subdomain_list, s.mesh,
                         s.ct)
    o.update_pde_variables(P, ions, {'z': -1, **{t: 0.1 * t for t in tags}}, c_new, c_all, phi, phiM)
    for t in tags:
        assert rel_err(s.ion_list[-1][f'c_{t}'].x._a, c_all[t][2]) < 1e-14
        for k in range(2):
            assert np.array_equal(s.c_prev[t][k].x._a, c_new[t][k])
        if t > 0:
            assert rel_err(s.phi_M_prev[t].x._a, phiM[t]) < 1e-14


# ---- invariants, bit-reproducibility -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("jittered", FORMS)
@pytest.mark.parametrize("case", ["pinch", "face_contact"])
@pytest.mark.parametrize("kind", tm.KINDS)
def test_invariants_and_bit_reproducibility(hip_lib, monkeypatch, kind, case, jittered):
    """The device's own A_emi: symmetric, constants in its null space (1e-13 of max|A|, the oracle's bound on the host);
    P = A on ECS rows, bit for bit; the membrane part of b_emi sums to zero.  Two assemblies of one handle and the two
    block shapes give the same bits."""
    res = {}
    for classic in (False, True):
        if classic:
            monkeypatch.setenv("KNPEMI_BLOCK_CLASSIC", "1")
        else:
            monkeypatch.delenv("KNPEMI_BLOCK_CLASSIC", raising=False)
        s = _build(kind, case, jittered)
        first, dp = _device_objects(s)
        first = [_values(a).copy() for a in first]
        second, _ = _device_objects(s)
        for a, b in zip(first, second):
            assert np.array_equal(a.view(np.uint64), _values(b).view(np.uint64))
        res[classic] = first
    for a, b in zip(res[False], res[True]):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    A, Pm, b = second[:3]
    scale = np.abs(A.data).max()
    assert np.abs(A @ np.ones(A.shape[0])).max() < 1e-13 * scale
    assert csr_rel_err(A, A.T.tocsr()) < 1e-13
    n0 = int(dp.n_vert[0])
    D = (Pm - A).tocsr()
    assert (D[:n0].nnz == 0 or np.abs(D[:n0].data).max() == 0.0) and np.abs(D[n0:].data).max() > 0
    L.check(dp.lib.knpemi_assemble_emi(dp.h, L.WANT_P | L.SKIP_MEMBRANE_RHS))
    b_mem = b - dp.rhs(L.B_EMI)
    assert np.abs(b_mem).max() > 0 and abs(b_mem.sum()) < 1e-13 * np.abs(b_mem).sum()


# ---- three steps: the device stepper against the drop-in sequence ---------------------------------------------------------------
@pytest.mark.parametrize("kind,jittered", [("triangle", True), ("tetrahedron", False), ("quadrilateral", False),
                                            ("hexahedron", True)])
def test_device_stepper_matches_dropin_path_with_two_models(hip_lib, kind, jittered):
    """test_device_stepper_matches_dropin_path_on_quadrilaterals on edge_touch with hh_si bound on cell 1 and glial on
    cell 2: three steps without linear solves, bit for bit.  The ECS vertices where the two cells meet are membrane dofs
    of both cells, and each model integrates every dof of its cell."""
    from knpemi import update_ode_variables, update_pde_variables
    from knpemi.stepper import DeviceStepper
    res = []
    for mode in ("dropin", "stepper"):
        s = _build(kind, "edge_touch", jittered)
        for t in s.subdomain_list:
            for k in range(2):
                s.c[t][k].x.array[:] = s.c_prev[t][k].x._a * 1.001
            if t > 0:
                s.phi[t].x.array[:] += -0.0744
        models = {t: s.subdomain_list[t]['mem_models'][0]['ode'] for t in (1, 2)}
        flat = s.a_emi.dp.flat
        shared = np.intersect1d(flat["q_to_e"][1], flat["q_to_e"][2])
        assert len(shared) == (1 if s.mesh.gdim == 2 else 2)
        for i, t in ((1, 1), (2, 2)):
            assert models[t].nodes == flat["n_q"][i] and np.isin(shared, flat["q_to_e"][i]).all()
            assert np.isin(flat["facet_q"][i], np.arange(models[t].nodes)).all()
            assert (s.a_emi.dp._keep[1][i] == 0).all()                # every facet of the cell is bound to its model
        with contextlib.redirect_stdout(io.StringIO()):
            if mode == "stepper":
                st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi,
                                   s.phi_M_prev)
                for t in (1, 2):
                    st.add_membrane_model(models[t])
                for _ in range(3):
                    st.step()
                    assert st.last_fused is None                      # two models: the fused sweep launch is not asked for
                b_emi, b_knp = st.dp.rhs(0), st.dp.rhs(1)
                st.download()
                _assert_kernels(st.dp, kind, jittered)
            else:
                emi, knp = _solvers(s)
                for k in range(3):
                    for t in (1, 2):
                        update_ode_variables(models[t], s.c_prev, s.phi_M_prev[t], s.ion_list, s.subdomain_list, s.mesh,
                                             s.ct, t, k)
                        models[t].step_lsoda(s.dt, None)
                        models[t].get_membrane_potential(s.phi_M_prev[t])
                        for ion, f in s.subdomain_list[t]['mem_models'][0]['I_ch_k'].items():
                            models[t].get_parameter("I_ch_" + ion, f)
                    _, b_emi = emi.assemble()
                    _, b_knp = knp.assemble()
                    update_pde_variables(s.c, s.c_prev, s.phi, s.phi_M_prev, s.physical_parameters, s.ion_list,
                                         s.subdomain_list, s.mesh, s.ct)
        res.append([models[1].states.copy(), models[2].states.copy(), s.phi_M_prev[1].x._a.copy(),
                    s.phi_M_prev[2].x._a.copy(), s.c_prev[1][0].x._a.copy(), s.c_prev[0][1].x._a.copy(),
                    np.asarray(b_emi).copy(), np.asarray(b_knp).copy()])
    for a, b in zip(*res):
        assert np.isfinite(a).all() and np.array_equal(a, b)
    assert np.ptp(res[0][2]) > 0 and np.ptp(res[0][3]) > 0


# ---- membrane exchange ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jittered", FORMS)
@pytest.mark.parametrize("case", ["edge_touch", "tags", "to_boundary"])
@pytest.mark.parametrize("kind", tm.KINDS)
def test_membrane_exchange_matches_the_restatement(hip_lib, kind, case, jittered):
    """tests/test_exchange_gpu.py::test_fields_and_row_match_the_restatement: device fields and row against
    MembraneExchange.compute_host at 1e-10, both splitting modes.  On `tags` the facets tagged 7 have no model and
    contribute nothing: zero area, zero in every field."""
    from test_exchange_gpu import _read, _set_scheme, _stepper
    s = _build(kind, case, jittered)
    st = _stepper(s)
    ex = xc.exchange(s)
    st.exchange(ex, fields=True)
    dp = st.dp
    _assert_kernels(dp, kind, jittered)
    for splitting in (True, False):
        _set_scheme(dp, splitting)
        L.check(dp.lib.knpemi_exchange_record(dp.h, 1))
        dev = {tag: ex.fields(tag) for tag in ex.watched}
        buf, rows, over = _read(dp, ex.n_cols, 1, reset=1)
        assert rows == 1 and over == 0
        fields, want = ex.compute_host(splitting=splitting, **xc.host_state(s))
        worst = max(xc.fields_err(dev[tag], fields[tag]) for tag in ex.watched)
        e_row = xc.row_err(ex, buf[0], want, fields)
        print(kind, case, "jittered" if jittered else "plain", splitting, "fields", worst, "row", e_row)
        assert worst < TOL and e_row < TOL
        if case == "tags":
            ftag = dp.flat["facet_tag"][1]
            assert (ftag == 7).any() and (dev[1]["area"][ftag != 7] > 0).all()
            for key, v in dev[1].items():
                if key != "facet":
                    assert not v[ftag == 7].any(), key


# ---- a tagged facet between two cells is refused by knpemi_create ---------------------------------------------------------------
def _unverified_tables(mesh, ft, subdomain_list):
    """knpemi.device.flatten_problem without its checks, every looked-up index clipped into its range: what a ctypes caller
    who matches vertices and verifies nothing hands to knpemi_create."""
    tags = list(subdomain_list)
    subs = [subdomain_list[t] for t in tags]
    ecs, ft_dense = subs[0]["mesh_sub"], ft.dense()
    out = dict(tags=tags, x=[np.ascontiguousarray(sd["mesh_sub"].x, np.float64) for sd in subs],
               cells=[np.ascontiguousarray(sd["mesh_sub"].cells, np.int32) for sd in subs], n_q=[0], facet_e=[None],
               facet_i=[None], facet_q=[None], facet_tag=[None], q_to_e=[None], q_to_i=[None], q_x=[None])
    for sd in subs[1:]:
        mem, ics = sd["mesh_mem"], sd["mesh_sub"]

        def find(sub, pv):
            return np.minimum(np.searchsorted(sub.parent_vertices, pv), sub.num_vertices - 1).astype(np.int32)
        pv = mem.parent_vertices[mem.cells]
        out["n_q"].append(mem.num_vertices)
        out["facet_e"].append(np.ascontiguousarray(find(ecs, pv)))
        out["facet_i"].append(np.ascontiguousarray(find(ics, pv)))
        out["facet_q"].append(np.ascontiguousarray(mem.cells, np.int32))
        out["facet_tag"].append(ft_dense[mem.parent_entities].astype(np.int32))
        out["q_to_e"].append(find(ecs, mem.parent_vertices))
        out["q_to_i"].append(find(ics, mem.parent_vertices))
        out["q_x"].append(mem.x)
    return out


@pytest.mark.parametrize("which", list(tm.CONTACTS))
@pytest.mark.parametrize("kind", tm.KINDS)
def test_tagged_contact_facets_are_refused_and_untagged_ones_match_oracle(hip_lib, monkeypatch, kind, which):
    """Cells 1 and 2 share facets that carry membrane tag 1.  DeviceProblem refuses in flatten_problem and names the parent
    facet; with the host check out of the way knpemi_create itself answers KNPEMI_EINVAL and names facet and sub-domain.
    The process stays usable: the same mesh with the contact facets untagged is created, assembled and equal to the
    oracle."""
    import adapters
    import knpemi.device as device
    data = tm.contact(kind, which)
    s = tc.problem(data, tm.CONTACT_SPEC, forms=False)
    with pytest.raises(RuntimeError, match=r"membrane facet \d+ of sub-domain 1 .* tags \[1, 2\]"):
        device.DeviceProblem(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list)
    with monkeypatch.context() as m:
        m.setattr(device, "flatten_problem", _unverified_tables)
        with pytest.raises(L.KnpemiError, match=r"membrane facet \d+ of sub-domain 1 is not a facet of an ECS cell") as e:
            device.DeviceProblem(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list)
    assert e.value.code == L.EINVAL
    s = tc.problem(tm.contact(kind, which, tagged=False), tm.CONTACT_SPEC)
    objs, dp = _device_objects(s)
    ref = tc.oracle_objects(s)
    errs = _errors(objs, ref)
    print(kind, which, errs)
    _assert_kernels(dp, kind, False)
    assert max(errs.values()) < TOL, errs
