"""GPU tests that pin, from outside, which instantiations of the assembly kernels a handle can reach (the
`..._built` predicates of csrc/kernels_assemble.hip and the kn_pick calls of the launchers): every ion count and membrane
path at the default lanes per row on every cell kind and geometry variant, the other lane counts with three ions, the
combinations that are refused -- by name, leaving the handle usable -- and the DG parametrisations tests/test_dg_gpu.py
lacks.  Smallest meshes of the parity tests; everything against the oracles at 1e-10."""
import ctypes
import functools

import numpy as np
import pytest

import hex_meshes as hm
from helpers import TOL, csr_rel_err, ion_count_problem, make_mesh, rel_err
from knpemi import _lib as L

pytestmark = pytest.mark.gpu

LATTICE_TETS, AFFINE, UNIFORM = 1, 2, 4     # knpemi_debug_geometry
# mesh -> (its data, the geometry flags knpemi_create must decide on: the variant the row kernels are picked for)
MESHES = {"2d": (lambda: make_mesh("2d", 1), 0),
          "tet": (lambda: make_mesh("tet", 0), LATTICE_TETS),
          "hex": (lambda: make_mesh("hex", 0), AFFINE | UNIFORM),                    # GEO 2: one box
          "hex_affine": (lambda: hm.variant("reoriented_sheared")[1], AFFINE),      # GEO 1: parallelepipeds
          "hex_general": (lambda: hm.variant("reoriented_jittered")[1], 0)}         # GEO 0: trilinear cells


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return MESHES[name][0]()


def _debug(dp):
    flags, out = ctypes.c_int(-1), (ctypes.c_int * 8)()
    L.check(dp.lib.knpemi_debug_geometry(dp.h, ctypes.byref(flags)))
    L.check(dp.lib.knpemi_debug_layout(dp.h, out, 8))
    return flags.value & (LATTICE_TETS | AFFINE | UNIFORM), out[1]          # geometry variant, lanes per row


def _solvers(s):
    from knpemi.pdeSolver import create_solver_emi, create_solver_knp
    emi = create_solver_emi(s.a_emi, s.L_emi, s.phi, [], s.subdomain_list, None, p=s.p_emi, direct=False)
    knp = create_solver_knp(s.a_knp, s.L_knp, s.c, [], s.subdomain_list, None, p=s.p_knp)
    return emi, knp


@functools.lru_cache(maxsize=None)
def _oracle(mesh, n_ions):
    """(A_emi, P_emi, b_emi, A_knp, b_knp) of ion_count_problem(mesh, n_ions): the fields are seeded, so every problem built
    for the pair has these."""
    s = ion_count_problem(_mesh(mesh), n_ions)
    o, P, params, ions = s.oracle
    c_all, phi, phiM, mm = s.oracle_fields
    return o.assemble_emi(P, params, ions, c_all, phiM, mm) + o.assemble_knp(P, params, ions, c_all, phi, phiM, mm, s.dt)


def _emi_errors(emi, ref):
    A, b = emi.assemble()
    return dict(A_emi=csr_rel_err(A, ref[0]), P_emi=csr_rel_err(emi.P, ref[1]), b_emi=rel_err(b, ref[2]))


def _knp_errors(dp, ref):
    return dict(A_knp=csr_rel_err(dp.csr(L.A_KNP), ref[3]), b_knp=rel_err(dp.rhs(L.B_KNP), ref[4]))


@pytest.mark.parametrize("n_ions", [2, 3, 4])
@pytest.mark.parametrize("mesh", list(MESHES))
def test_knp_rows_of_every_ion_count_and_membrane_path_match_oracle(hip_lib, monkeypatch, mesh, n_ions):
    """K - 1 = 1..3 solved ions x the three sources of the membrane integrals of b_knp -- the facet kernel's partial
    integrals (default), the two-part early form (KNPEMI_MEMBRANE_EARLY), evaluated inside the row block
    (KNPEMI_OPT_FUSE_MEMBRANE, which needs row blocks of consecutive rows) -- at the default lanes per row, on triangles,
    lattice tetrahedra and the three geometry variants of hexahedra.  Before each of the optional paths the stored
    system is overwritten with NaN, so what is compared is what that path wrote."""
    ref = _oracle(mesh, n_ions)
    for classic in (False, True):
        if classic:
            monkeypatch.setenv("KNPEMI_BLOCK_CLASSIC", "1")
        else:
            monkeypatch.delenv("KNPEMI_BLOCK_CLASSIC", raising=False)
        s = ion_count_problem(_mesh(mesh), n_ions)
        _, knp = _solvers(s)
        dp = knp.dp
        A, _ = knp.assemble()                # pushes every field; default path
        geometry, lanes = _debug(dp)
        assert lanes == (2 if mesh == "2d" else 4) and (mesh == "2d" or geometry == MESHES[mesh][1])
        assert A.shape[0] == (n_ions - 1) * ref[0].shape[0]
        errs = {"default": _knp_errors(dp, ref)}
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


@pytest.mark.parametrize("lpr", [1, 8])
@pytest.mark.parametrize("mesh", ["tet", "hex"])
def test_other_lane_counts_with_three_ions_match_oracle(hip_lib, monkeypatch, mesh, lpr):
    """KNPEMI_LPR = 1 and 8 are built for two solved ions and the default membrane path: all five assembled objects."""
    monkeypatch.setenv("KNPEMI_LPR", str(lpr))
    ref = _oracle(mesh, 3)
    emi, knp = _solvers(ion_count_problem(_mesh(mesh), 3))
    errs = _emi_errors(emi, ref)
    knp.assemble()
    errs.update(_knp_errors(knp.dp, ref))
    print(mesh, lpr, errs)
    assert _debug(knp.dp) == (MESHES[mesh][1], lpr)
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("what", ["two_ions", "fused_membrane"])
@pytest.mark.parametrize("mesh", ["tet", "hex"])
def test_combinations_that_are_not_built_are_refused_by_name(hip_lib, monkeypatch, mesh, what):
    """Eight lanes per row with one solved ion, or with the membrane integrals inside the row block: no such knp_rows
    kernel exists.  knpemi_assemble_knp answers KNPEMI_EINVAL and names the combination; the handle stays usable -- the EMI
    system of the same handle assembles and matches the oracle."""
    monkeypatch.setenv("KNPEMI_LPR", "8")
    monkeypatch.setenv("KNPEMI_BLOCK_CLASSIC", "1")
    n_ions = 2 if what == "two_ions" else 3
    ref = _oracle(mesh, n_ions)
    emi, knp = _solvers(ion_count_problem(_mesh(mesh), n_ions))
    dp = knp.dp
    if what == "fused_membrane":
        knp.assemble()                       # three ions, default path: built
        assert max(_knp_errors(dp, ref).values()) < TOL
        L.check(dp.lib.knpemi_set_option(dp.h, L.OPT_FUSE_MEMBRANE, 1))
    with pytest.raises(L.KnpemiError, match="unsupported lanes-per-row / ion-count / membrane-option combination") as e:
        if what == "fused_membrane":
            dp.assemble_knp()
        else:
            knp.assemble()
    assert e.value.code == L.EINVAL
    print(mesh, what, e.value)
    assert _debug(dp)[1] == 8
    errs = _emi_errors(emi, ref)
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("splitting", [True, False])
@pytest.mark.parametrize("cell,M,K", [("tetrahedron", 4, 2), ("hexahedron", 4, 2), ("hexahedron", 4, 4)])
def test_dg_ion_counts_the_dg_tests_lack_match_oracle(hip_lib, cell, M, K, splitting):
    """dg_knp_kernel<4, 1> and the box-mesh kernels dg_knp_hex_box_kernel<1> and <3> (tests/test_dg_gpu.py has tetrahedra
    with 3 and 4 ions, boxes with 3): A_emi, b_emi and the K - 1 concentration systems against the restatement."""
    from test_dg_gpu import _hex_problem, _problem, _push, _random_state
    dp, o = _problem(3, M, True, n_ions=K, gamma=7.5) if cell == "tetrahedron" else _hex_problem(M, True, n_ions=K, gamma=7.5)
    zs = [1.0, -1.0, 2.0, -1.0][:K]
    ions = [dict(name=f"i{k}", z=zs[k], D=[1.0 + 0.3 * k, 0.6 + 0.2 * k]) for k in range(K)]
    params = dict(dt=0.05, F=1.3, psi=0.8, C_M=0.7)
    c_all, phi, phi_M, I_ch, src = _random_state(dp, K, 1)
    _push(dp, params, ions, c_all, phi, phi_M, I_ch, src)
    dp.assemble_emi(splitting)
    dp.assemble_knp(splitting)
    A, b = o.assemble_emi(params, ions, c_all, phi_M, I_ch, splitting_scheme=splitting, gamma=7.5)
    assert csr_rel_err(dp.matrix(0), A) < TOL and rel_err(dp.rhs(0), b) < TOL
    As, bs = o.assemble_knp(params, ions, c_all, phi, phi_M, I_ch, splitting_scheme=splitting, gamma=7.5, f_source=src)
    for k in range(K - 1):
        assert csr_rel_err(dp.matrix(1 + k), As[k]) < TOL, k
        assert rel_err(dp.rhs(1 + k), bs[k]) < TOL, k
    assert dp.nv == (4 if cell == "tetrahedron" else 8)
