"""GPU parity tests: HIP kernels (through the C ABI and the knpemi API) against the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import Setup, csr_rel_err, rel_err
from helpers import assemble_both as _assemble_both
from helpers import check_facet_integrals_of_the_write_back_launch
from knpemi import _lib as L

pytestmark = pytest.mark.gpu

TOL = 1e-10   # stated fp64 tolerance for assembled operators


@pytest.mark.parametrize("kind,r", [("2d", 1), ("2d", 2), ("tet", 0), ("hex", 0)])
@pytest.mark.parametrize("splitting", [True, False])
def test_assembly_matches_oracle(hip_lib, kind, r, splitting):
    s = Setup(kind, r)
    s.perturb()
    errs, _ = _assemble_both(s, splitting)
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("kind,r", [("2d", 1), ("tet", 0), ("hex", 0)])
@pytest.mark.parametrize("splitting", [True, False])
def test_c_phi_is_its_own_parameter(hip_lib, kind, r, splitting):
    """`physical_parameters['C_phi']` is an entry of its own in the reference (run_2D.py:187,208) and only the EMI forms read
    it (emiWeakForm.py:164,231-236): with C_phi != C_M / dt the EMI coupling and Robin datum follow C_phi, the KNP
    membrane terms keep C_M / dt."""
    from setup_problem import C_M, DT
    from knpemi.fem import Constant
    s = Setup(kind, r)
    s.physical_parameters['C_phi'] = Constant(s.mesh, 2.5 * C_M / DT)
    s.perturb()
    errs, (A, _, b, _, _) = _assemble_both(s, splitting)
    assert max(errs.values()) < TOL, errs
    s0 = Setup(kind, r)
    s0.perturb()
    _, (A0, _, b0, _, _) = _assemble_both(s0, splitting)
    assert abs(A - A0).max() > 0 and np.abs(b - b0).max() > 0      # it does change the system


def _distorted_hex_mesh(seed=3):
    """The r = 0 hexahedral box with every vertex moved by up to 15 % of the smallest spacing: trilinear cells
    with a non-constant Jacobian and non-planar membrane quadrilaterals."""
    from setup_problem import make_mesh
    mesh, ct, ft = make_mesh("hex", 0)
    rng = np.random.default_rng(seed)
    mesh.x[:] = mesh.x + 0.15 * 0.1e-6 * (2.0 * rng.random(mesh.x.shape) - 1.0)
    return mesh, ct, ft


@pytest.mark.parametrize("splitting", [True, False])
def test_assembly_matches_oracle_on_distorted_hexahedra(hip_lib, splitting):
    """General Q1 path (Jacobian inverted at every Gauss point) against the oracle's quadrature."""
    s = Setup("hex", 0, mesh_data=_distorted_hex_mesh())
    s.perturb()
    errs, _ = _assemble_both(s, splitting)
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("mirror", [False, True])
def test_assembly_matches_oracle_on_sheared_hexahedra(hip_lib, mirror):
    """Parallelepipeds with a full metric tensor (the box sheared by a constant matrix; mirrored: left-handed cells):
    the closed-form Q1 rows of the affine kernels, off-diagonal terms included, against the oracle's 2 x 2 x 2 rule."""
    from setup_problem import make_mesh
    mesh, ct, ft = make_mesh("hex", 0)
    A = np.array([[1.0, 0.8, -0.5], [0.02, 1.0, 0.3], [-0.01, 0.25, 1.0]])
    if mirror:
        A[:, 1] *= -1.0
    mesh.x[:] = mesh.x @ A.T
    s = Setup("hex", 0, mesh_data=(mesh, ct, ft))
    s.perturb()
    for splitting in (True, False):
        errs, _ = _assemble_both(s, splitting)
        assert max(errs.values()) < TOL, errs


def test_general_hexahedron_kernel_on_box_mesh(hip_lib, monkeypatch):
    """KNPEMI_HEX_GENERAL forces the general Q1 kernels (per-cell affinity test at run time) on a box mesh."""
    monkeypatch.setenv("KNPEMI_HEX_GENERAL", "1")
    s = Setup("hex", 0)
    s.perturb()
    errs, _ = _assemble_both(s)
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("kind", ["2d", "tet", "hex"])
def test_clustered_row_blocks_equal_blocks_of_consecutive_rows_bit_for_bit(hip_lib, monkeypatch, kind):
    """The row blocks are clusters of 16-row (hexahedra: 8-row) chunks chosen by the Laplacian graph (fewer distinct vertices to stage per
    block); KNPEMI_BLOCK_CLASSIC=1 takes 64 consecutive rows.  A row's pairs, their order and its lanes do not depend on
    the block it sits in: all five assembled objects agree bit for bit."""
    res = []
    for classic in (False, True):
        if classic:
            monkeypatch.setenv("KNPEMI_BLOCK_CLASSIC", "1")
        else:
            monkeypatch.delenv("KNPEMI_BLOCK_CLASSIC", raising=False)
        s = Setup(kind, 1 if kind == "2d" else 0)
        s.perturb()
        errs, objs = _assemble_both(s)
        assert max(errs.values()) < TOL, errs
        res.append(objs)
    for a, b in zip(*res):
        a = a.data if hasattr(a, "data") and not isinstance(a, np.ndarray) else a
        b = b.data if hasattr(b, "data") and not isinstance(b, np.ndarray) else b
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_assembly_is_bit_reproducible(hip_lib):
    s = Setup("tet", 0)
    s.perturb()
    _, first = _assemble_both(s)
    _, second = _assemble_both(s)
    for a, b in zip(first, second):
        a = a.data if hasattr(a, "data") and not isinstance(a, np.ndarray) else a
        b = b.data if hasattr(b, "data") and not isinstance(b, np.ndarray) else b
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_emi_invariants(hip_lib):
    """Constant null space and zero-sum membrane RHS."""
    s = Setup("tet", 0)
    s.perturb()
    _, (A, Pm, b, Ak, bk) = _assemble_both(s)
    assert np.abs(A @ np.ones(A.shape[0])).max() < 1e-12 * np.abs(A.data).max()
    assert csr_rel_err(A, A.T.tocsr()) < 1e-14


def test_update_pde_matches_oracle(hip_lib):
    from knpemi import update_pde_variables
    s = Setup("tet", 0)
    s.perturb()
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


def test_write_through_a_retained_array_view_is_uploaded(hip_lib):
    """DOLFINx driver code keeps views (`a = f.x.array`) and writes through them later; the upload skipping of the
    drop-in layer must notice (content fingerprint), not hand the kernels a stale device copy.  A second locator
    object for the stimulus mask must get its own mask even if it reuses the id of a dead lambda."""
    from knpemi import _lib as L
    s = Setup("2d", 1)
    dp = s.a_emi.dp
    f = s.c_prev[0][0]
    view = f.x.array
    dp.push(L.F_C_PREV, 0, 0, f)
    view[:] = 7.25                       # no `.array` access after the upload
    dp.push(L.F_C_PREV, 0, 0, f)
    assert np.all(dp.pull_array(L.F_C_PREV, 0, 0, view.shape[0]) == 7.25)
    dp.push(L.F_C_PREV, 0, 0, f)         # unchanged: skipped (same stamp)
    assert dp._uploaded[(L.F_C_PREV, 0, 0)] == dp._stamp(f.x)
    ode = s.mem_models[0]['ode']
    from knpemi.utils import update_ode_variables
    update_ode_variables(ode, s.c_prev, s.phi_M_prev[1], s.ion_list, s.subdomain_list, s.mesh, s.ct, 1, 0)
    ode.step_lsoda(s.dt, s.stim_params['stimulus'], lambda x: x[0] < 20e-6)
    m1 = next(iter(ode._mask_cache.values())).copy()
    ode.step_lsoda(s.dt, s.stim_params['stimulus'], lambda x: x[0] > 40e-6)
    m2 = next(iter(ode._mask_cache.values()))
    assert m1.sum() > 0 and m2.sum() > 0 and not np.array_equal(m1, m2)


def test_trace_matches_oracle(hip_lib):
    from knpemi import interpolate_to_membrane
    s = Setup("2d", 1)
    s.perturb()
    o, P, params, ions = s.oracle()
    qe, qi = interpolate_to_membrane(s.phi[0], s.phi[1], s.phi_M_prev[1].function_space, s.mesh, s.ct,
                                     s.subdomain_list, 1)
    te, ti = P.trace(1, s.phi[0].x._a, s.phi[1].x._a)
    assert np.array_equal(qe.x._a, te) and np.array_equal(qi.x._a, ti)
    assert qe.name == s.phi[0].name


@pytest.mark.parametrize("g_syn", [0.0, 10.0])
def test_ode_sweep_matches_scipy_lsoda(hip_lib, g_syn):
    """HH sweep on the GPU vs ODEPACK LSODA (scipy) with the reference's side-effect semantic
    for the currents; tolerance 1e-6 relative (hard part 3)."""
    from knpemi.utils import update_ode_variables
    s = Setup("2d", 1, g_syn=g_syn)
    o, P, params, ions = s.oracle()
    ode = s.mem_models[0]['ode']
    ix = o.MODELS["hh_si"]["pidx"]
    mask = np.array([x[0] < 20e-6 for x in ode.dof_locations])
    rows = list(range(0, ode.nodes, 8))
    st_o, p_o = ode.states.copy(), ode.parameters.copy()
    t = 0.0
    for k in range(3):
        c_all, phi, phiM, mm = s.oracle_fields()
        update_ode_variables(ode, s.c_prev, s.phi_M_prev[1], s.ion_list, s.subdomain_list, s.mesh, s.ct, 1, k)
        ode.step_lsoda(s.dt, s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
        for name, kk in (("K", 0), ("Cl", 1), ("Na", 2)):
            te, ti = P.trace(1, c_all[0][kk], c_all[1][kk])
            p_o[:, ix[f"{name}_e"]] = te
            p_o[:, ix[f"{name}_i"]] = ti
        if k > 0:
            st_o[:, 3] = phiM[1]
        o.ode_sweep("hh_si", st_o, p_o, t, s.dt, mask, {ix["stim_amplitude"]: g_syn}, rows=rows)
        t += s.dt
        assert rel_err(ode.states[rows], st_o[rows]) < 1e-6
        ich = [ix["I_ch_Na"], ix["I_ch_K"], ix["I_ch_Cl"]]
        # currents cancel to ~1e-14 at rest: compare against the size of their terms (>= 1e-3 A/m^2)
        # (the evaluation point of the side-effect currents is reproducible to ~1e-7 dt only: tests/test_lsoda_host.py)
        dI = np.abs(ode.parameters[rows][:, ich] - p_o[rows][:, ich]).max()
        assert dI / max(np.abs(p_o[rows][:, ich]).max(), 1e-3) < 1e-5
        ode.get_membrane_potential(s.phi_M_prev[1])
        assert ode.last_stats["n_failed"] == 0 and ode.last_stats["n_rhs"] > 0
    assert abs(ode.time - 3 * s.dt) < 1e-15


def test_device_math_helpers(hip_lib):
    """The quotient, exponential and power the ODE sweep evaluates on the device (csrc/lsoda_core.h: kn_div = reciprocal
    estimate times the product form of the Newton series, kn_exp = two-constant reduction + degree-13 polynomial in
    Estrin's arrangement, kn_log = the classical f / (2 + f) reduction, kn_powr = exp(e log x)) against the C library:
    within 4 ulp (kn_div, kn_exp, kn_log), 16 ulp (kn_powr: the rounding of log x is amplified by e |log x|), exact
    limits at the ends of the range."""
    rng = np.random.default_rng(11)
    n = 200000

    def run(op, a, b):
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        out = np.empty_like(a)
        L.check(hip_lib.knpemi_debug_math(op, a.size, L.dptr(a), L.dptr(b), L.dptr(out)))
        return out

    def ulps(x, ref):
        return np.abs(x - ref) / np.spacing(np.abs(ref))

    a = rng.standard_normal(n) * 10.0 ** rng.uniform(-30, 30, n)
    b = rng.standard_normal(n) * 10.0 ** rng.uniform(-30, 30, n)
    assert ulps(run(0, a, b), a / b).max() <= 4.0
    assert ulps(run(0, np.ones(n), b), 1.0 / b).max() <= 4.0
    x = np.concatenate([rng.uniform(-700.0, 700.0, n // 2), rng.uniform(-5.0, 5.0, n // 2)])
    assert ulps(run(1, x, x), np.exp(x)).max() <= 4.0
    ends = np.array([0.0, -0.0, 710.0, 1e300, np.inf, -746.0, -1e300, -np.inf, 709.0, -744.0, -708.0])
    got = run(1, ends, ends)
    with np.errstate(over="ignore"):
        want = np.exp(ends)
    assert np.array_equal(got[:8], want[:8])
    assert ulps(got[8:], want[8:]).max() <= 4.0
    assert np.isnan(run(1, np.array([np.nan]), np.array([np.nan]))[0])
    pos = 10.0 ** rng.uniform(-300, 300, n)
    pos[: n // 4] = rng.uniform(0.5, 2.0, n // 4)
    assert ulps(run(3, pos, pos), np.log(pos)).max() <= 4.0
    ends = np.array([0.0, np.inf, 1.0, 5e-324, 1e-310])
    with np.errstate(divide="ignore"):
        assert np.array_equal(run(3, ends, ends)[:3], np.log(ends[:3]))
        assert ulps(run(3, ends, ends)[3:], np.log(ends[3:])).max() <= 4.0
    assert np.isnan(run(3, np.array([-1.0, np.nan]), np.array([1.0, 1.0]))).all()
    base = 10.0 ** rng.uniform(-12, 3, n)
    ex = 1.0 / rng.integers(2, 14, n)
    assert ulps(run(2, base, ex), base ** ex).max() <= 16.0
    assert run(2, np.array([0.0]), np.array([0.5]))[0] == 0.0


def test_lsoda_failure_is_reported(hip_lib):
    """`assert success` after every LSODA call (odeSolver.py:121): a dof whose state is NaN cannot be integrated; the
    sweep must say so (KNPEMI_EODE -> AssertionError, failure count) instead of returning silently, and the healthy
    dofs of the same launch are still integrated."""
    from knpemi import update_ode_variables
    s = Setup("2d", 1, g_syn=10.0)
    ode = s.mem_models[0]['ode']
    update_ode_variables(ode, s.c_prev, s.phi_M_prev[1], s.ion_list, s.subdomain_list, s.mesh, s.ct, 1, 0)
    good = ode.states.copy()
    ode.states[5, 3] = np.nan
    with pytest.raises(AssertionError, match="LSODA failed"):
        ode.step_lsoda(s.dt, s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
    assert ode.last_stats["n_failed"] == 1
    ok = np.arange(ode.nodes) != 5
    assert np.all(np.isfinite(ode.states[ok])) and np.all((ode.states[ok] != good[ok]).any(axis=1))


def test_ode_sweep_is_bit_reproducible(hip_lib):
    from knpemi.utils import update_ode_variables
    out = []
    for _ in range(2):
        s = Setup("2d", 1, g_syn=10.0)
        ode = s.mem_models[0]['ode']
        for k in range(2):
            update_ode_variables(ode, s.c_prev, s.phi_M_prev[1], s.ion_list, s.subdomain_list, s.mesh, s.ct, 1, k)
            ode.step_lsoda(s.dt, s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
            ode.get_membrane_potential(s.phi_M_prev[1])
        out.append((ode.states.copy(), ode.parameters.copy()))
    assert np.array_equal(out[0][0].view(np.uint64), out[1][0].view(np.uint64))
    assert np.array_equal(out[0][1].view(np.uint64), out[1][1].view(np.uint64))


def test_abi_error_paths(hip_lib):
    import ctypes as C
    from knpemi import _lib as L
    s = Setup("2d", 1)
    dp = s.a_emi.dp
    bad = np.zeros(3)
    rc = hip_lib.knpemi_set_field(dp.h, L.F_PHI, 0, 0, L.dptr(bad), 3)
    assert rc == L.EINVAL and b"length" in hip_lib.knpemi_last_error()
    assert hip_lib.knpemi_set_field(dp.h, 99, 0, 0, L.dptr(bad), 3) == L.EINVAL
    assert hip_lib.knpemi_assemble_emi(None, 0) == L.EINVAL
    n, nnz = C.c_int64(), C.c_int64()
    assert hip_lib.knpemi_csr_dims(dp.h, 7, C.byref(n), C.byref(nnz)) == L.EINVAL
    # solver entry points
    assert hip_lib.knpemi_solver_setup(dp.h, 9, L.PC_AMG, 0.0) == L.EINVAL
    assert hip_lib.knpemi_solver_setup(dp.h, L.B_EMI, 5, 0.0) == L.EINVAL
    assert hip_lib.knpemi_solver_setup(None, L.B_EMI, L.PC_AMG, 0.0) == L.EINVAL
    it, rr = C.c_int(), C.c_double()
    assert hip_lib.knpemi_solve_emi(dp.h, -1.0, 0.0, 10, C.byref(it), C.byref(rr)) == L.EINVAL
    assert hip_lib.knpemi_solve_knp(dp.h, 1e-5, 0.0, -3, C.byref(it), C.byref(rr)) == L.EINVAL
    lev, b = C.c_int(), C.c_int()
    assert hip_lib.knpemi_solver_info(dp.h, L.B_KNP, C.byref(lev), C.byref(rr), C.byref(b)) == L.OK
    assert lev.value == 0 and b.value == 0           # nothing built before the first solve


@pytest.mark.parametrize("kind,r", [("2d", 1), ("tet", 0), ("hex", 0)])
def test_assembly_matches_golden_fixtures(hip_lib, kind, r):
    """HIP path against the committed golden vectors (tests/golden/make_golden.py)."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"assembly_{kind}_r{r}.npz"))
    s = Setup(kind, r)
    s.perturb(12345)
    for split in (True, False):
        tag = "split" if split else "nosplit"
        _, (A, Pm, b, Ak, bk) = _assemble_both(s, split)
        v = np.random.default_rng(1).uniform(-1, 1, A.shape[0])
        vk = np.random.default_rng(2).uniform(-1, 1, Ak.shape[0])
        assert rel_err(b, g[f"{tag}_b_emi"]) < TOL and rel_err(bk, g[f"{tag}_b_knp"]) < TOL
        assert rel_err(A @ v, g[f"{tag}_A_emi_v"]) < TOL and rel_err(Pm @ v, g[f"{tag}_P_emi_v"]) < TOL
        assert rel_err(Ak @ vk, g[f"{tag}_A_knp_v"]) < TOL
        assert rel_err(A.diagonal(), g[f"{tag}_A_emi_diag"]) < TOL
        # structural sizes (scipy prunes exact zeros when it forms P = A + M, so P is not compared)
        assert (int(g[f"{tag}_nnz"][0]), int(g[f"{tag}_nnz"][2])) == (A.nnz, Ak.nnz)


@pytest.mark.parametrize("kind,r", [("2d", 1), ("tet", 0), ("hex", 0)])
def test_facet_integrals_formed_in_the_potential_write_back_launch(hip_lib, kind, r):
    """KNPEMI_OPT_FOLD_MEMBRANE: the launch that writes a potential back (here a pasted solution, as in bench.py's timed
    steps; knpemi_solve_emi's own write-back in the solver tests) also forms the membrane-facet integrals of b_knp
    (knpWeakForm.py:168-214).  b_knp equals the one assembled with the facet kernel as a launch of its own bit for bit and
    matches the oracle; the stored integrals are dropped as soon as one of their inputs changes (phi_M here)."""
    s = Setup(kind, r)
    s.perturb()
    check_facet_integrals_of_the_write_back_launch(s)


# The facet integrals formed by the write-back of the potential are reused only while none of their inputs has changed.
# The tests below run in a fresh process each: the KNPEMI_FUSED_* knobs are read once per process.  KNPEMI_FUSED_CHUNK=1
# gives every chunk of a solve after the first the same key, so that the later solves of a handle replay captured chunks
# throughout (the host code inside a chunk does not run on a replay).

def _in_child(call, env, timeout=600):
    """Run `call` (one of this module's functions, as source text) in a fresh process with `env` added."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = [os.path.join(root, p) for p in ("knp-emi-fenics-x_amd", "oracle", "examples/idealized_geometries", "tests")]
    code = "import sys\nsys.path[:0] = %r\nimport test_gpu_parity as t\nt.%s\n" % (paths, call)
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]


def _stepper(knp_method="bicgstab", fuse_update=None):
    """A DeviceStepper with the device solves (by default the end-of-step update fused into the KNP write-back) on the tet
    r=0 mesh."""
    from knpemi.stepper import DeviceStepper
    s = Setup("tet", 0, g_syn=10.0)
    for t in s.subdomain_list:
        for k in range(2):
            s.c[t][k].x.array[:] = s.c_prev[t][k].x._a
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev,
                       device_solves=(1e-9, 1e-10), overlap=False, knp_method=knp_method, fuse_update=fuse_update)
    st.add_membrane_model(s.mem_models[0]['ode'], s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
    return s, st


def _ode_step(st):
    m = st.models[0]
    L.check(st.lib.knpemi_ode_step(st.dp.h, m._sub, m._model, float(m.time), st.dt, m.rtol, m.atol,
                                   L.ODE_SET_TRACES | L.ODE_SET_V, L.iptr(m._ion_param), int(m.V_index)))
    m.time = m.time + st.dt


def _device_copy(a):
    """A device copy of the host array `a` (for knpemi_set_solution(..., on_device = 1)); freed at process exit."""
    hip = C.CDLL("libamdhip64.so")
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), C.c_size_t(a.nbytes)) == 0
    assert hip.hipMemcpy(dev, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
    return dev


def _knp_rhs_after_a_replayed_knp_solve(knp_method):
    s, st = _stepper(knp_method)
    o, P, params, ions = s.oracle()
    dp, h = st.dp, st.dp.h
    for _ in range(2):
        st.step()                                   # captures the chunks of both solves
    dp.solve(L.B_EMI, 1e-9, 1e-40)                  # the write-back forms the facet integrals ...
    L.check(dp.lib.knpemi_assemble_knp(h, st.flags_knp))   # ... and this assembly uses them
    dp.solve(L.B_KNP, 1e-10, 2e-40)                 # replayed; its write-back updates c_prev and phi_M
    L.check(dp.lib.knpemi_assemble_knp(h, st.flags_knp))
    b = dp.rhs(L.B_KNP)
    st.download()
    c_all, phi, phiM, mm = s.oracle_fields()
    _, bko = o.assemble_knp(P, params, ions, c_all, phi, phiM, mm, s.dt)
    assert rel_err(b, bko) < TOL, rel_err(b, bko)


@pytest.mark.parametrize("knp_method", ["bicgstab", "gmres"])
def test_folded_integrals_are_not_reused_after_a_replayed_knp_solve(hip_lib, knp_method):
    """EMI solve (folded write-back), KNP assembly, a KNP solve replayed from captured chunks with the end-of-step update in
    its write-back, KNP assembly again: the second b_knp is that of the updated fields (oracle), not one built from the
    facet integrals of the fields before the solve."""
    _in_child(f"_knp_rhs_after_a_replayed_knp_solve({knp_method!r})",
              {"KNPEMI_FUSED_GRAPH": "1", "KNPEMI_FUSED_CHUNK": "1"})


def _device_solve_run(emi_norm, fuse_update, out):
    """Six DeviceStepper steps with the device solves (EMI CG with the `emi_norm` test, KNP BiCGStab): the fields and the
    iteration count and relative residual of every solve into the file `out`."""
    from knpemi.pdeSolver import set_emi_solver_options
    s, st = _stepper("bicgstab", fuse_update=fuse_update)
    set_emi_solver_options(st.dp, emi_norm)
    for _ in range(6):
        st.step()
    st.download()
    fields = [s.phi[t].x._a for t in s.subdomain_list]
    fields += [d[t][k].x._a for d in (s.c, s.c_prev) for t in s.subdomain_list for k in range(2)]
    fields += [s.phi_M_prev[t].x._a for t in s.subdomain_list if t > 0]
    np.savez(out, fields=np.concatenate(fields), its=np.array([r[1] for r in st.iterations]),
             relres=np.array([r[2] for r in st.iterations]))


@pytest.mark.parametrize("emi_norm,fuse_update", [("true", True), ("true", False), ("preconditioned", True),
                                                  ("preconditioned", False)])
def test_replayed_solves_equal_direct_launches_bit_for_bit(hip_lib, tmp_path, emi_norm, fuse_update):
    """The same six steps with the chunks of the device solves launched directly and replayed from captured graphs (the
    fused loops with one iteration per chunk after the first, so that the later solves replay graphs of several chunks;
    the plain loops with their captured iteration bodies): the fields and every solve's iteration count and relative
    residual agree bit for bit."""
    pairs = [({"KNPEMI_FUSED_GRAPH": "0"}, {"KNPEMI_FUSED_GRAPH": "1", "KNPEMI_FUSED_CHUNK": "1"}),
             ({"KNPEMI_NO_FUSED": "1"}, {"KNPEMI_NO_FUSED": "1", "KNPEMI_NO_GRAPH": "1"})]
    for i, pair in enumerate(pairs):
        runs = []
        for j, env in enumerate(pair):
            out = str(tmp_path / f"run{i}{j}.npz")
            _in_child(f"_device_solve_run({emi_norm!r}, {fuse_update!r}, {out!r})", env)
            runs.append(np.load(out))
        a, b = runs
        assert len(a["its"]) == 12 and a["its"].sum() > 0, (pair, a["its"])
        for key in ("its", "relres", "fields"):
            assert np.array_equal(a[key], b[key]), (pair, key, a["its"], b["its"])


def _folded_and_fresh_knp_rhs_agree(n_calls=30, seed=34):
    """A seeded sequence of calls with a KNP assembly after each.  At random points of it (and at its end) that b_knp is
    compared with one assembled by the facet kernel as a launch of its own (KNPEMI_OPT_FOLD_MEMBRANE off and on again);
    in between, integrals formed by a write-back stay stored across the calls that follow it.  With this seed the
    sequence holds every kind of call, and an EMI solve followed by a replayed KNP solve with the update fused in
    (calls 5-6).  The two agree to rounding, not bit for bit: the write-back of the CG solve integrates with the solution
    before its mean is removed (a pasted solution has none, hence bit-identical there); stale integrals are off by 1e-9
    and more."""
    rng = np.random.default_rng(seed)
    ops = ["ode_step", "solve_emi", "solve_knp", "update_pde", "extrapolate_guess", "set_phi_M", "paste_phi",
           "fuse_membrane"]
    plan = [(ops[rng.integers(len(ops))], int(rng.integers(2)), bool(rng.random() < 0.5)) for _ in range(n_calls)]
    s, st = _stepper()
    dp, lib, h = st.dp, st.lib, st.dp.h
    st.step()                   # captures the chunks of both solves (KNP: with the update fused in)
    L.check(lib.knpemi_assemble_knp(h, st.flags_knp))
    phi0 = _device_copy(np.concatenate([s.phi[t].x._a for t in s.subdomain_list]))
    sub, nq = dp.sub_index[1], len(s.phi_M_prev[1].x._a)
    for i, (op, arg, check) in enumerate(plan):
        if op == "ode_step":
            _ode_step(st)
        elif op == "solve_emi":
            dp.solve(L.B_EMI, 1e-9, 1e-40)
        elif op == "solve_knp":
            L.check(lib.knpemi_set_option(h, L.OPT_FUSE_UPDATE, arg))
            dp.solve(L.B_KNP, 1e-10, 2e-40)
        elif op == "update_pde":
            L.check(lib.knpemi_update_pde(h))
        elif op == "extrapolate_guess":
            L.check(lib.knpemi_extrapolate_guess(h, arg))
        elif op == "set_phi_M":
            dp.push_array(L.F_PHI_M, sub, 0, dp.pull_array(L.F_PHI_M, sub, 0, nq) + 1e-4)
        elif op == "paste_phi":
            L.check(lib.knpemi_set_solution(h, L.B_EMI, phi0, 1))
        elif op == "fuse_membrane":
            L.check(lib.knpemi_set_option(h, L.OPT_FUSE_MEMBRANE, arg))
        L.check(lib.knpemi_assemble_knp(h, st.flags_knp))
        if check or i == n_calls - 1:
            b = dp.rhs(L.B_KNP)
            L.check(lib.knpemi_set_option(h, L.OPT_FOLD_MEMBRANE, 0))
            L.check(lib.knpemi_assemble_knp(h, st.flags_knp))
            L.check(lib.knpemi_set_option(h, L.OPT_FOLD_MEMBRANE, 1))
            assert rel_err(b, dp.rhs(L.B_KNP)) < 1e-12, (i, rel_err(b, dp.rhs(L.B_KNP)), plan[:i + 1])


def test_folded_integrals_match_a_fresh_facet_kernel_along_a_call_sequence(hip_lib):
    """30 calls that change inputs of the facet integrals, write the potential back or toggle the membrane options, in a
    fixed random order: b_knp agrees with b_knp from a fresh facet kernel to rounding wherever it is compared."""
    _in_child("_folded_and_fresh_knp_rhs_agree()",
              {"KNPEMI_FUSED_GRAPH": "1", "KNPEMI_FUSED_CHUNK": "1", "KNPEMI_BLOCK_CLASSIC": "1"})


def _facet_launches(st):
    """knp_membrane_kernel launches of one knpemi_assemble_knp."""
    k = L.KERNEL_NAMES.index("knp_membrane_kernel")
    n, ms = C.c_int64(), C.c_double()
    L.check(st.lib.knpemi_profile(st.dp.h, 1 << k))
    L.check(st.lib.knpemi_assemble_knp(st.dp.h, st.flags_knp))
    L.check(st.lib.knpemi_profile_read(st.dp.h, k, C.byref(n), C.byref(ms)))
    L.check(st.lib.knpemi_profile(st.dp.h, 0))
    return n.value


def _facet_kernel_skipped_after_a_write_back():
    s, st = _stepper()
    dp, lib, h = st.dp, st.lib, st.dp.h
    phi0 = _device_copy(np.concatenate([s.phi[t].x._a for t in s.subdomain_list]))
    for _ in range(2):          # bench.py's timed step: the potential pasted on the device
        _ode_step(st)
        L.check(lib.knpemi_assemble_emi(h, st.flags_emi))
        L.check(lib.knpemi_set_solution(h, L.B_EMI, phi0, 1))
        assert _facet_launches(st) == 0
        L.check(lib.knpemi_update_pde(h))
        assert _facet_launches(st) == 1
    for _ in range(2):          # DeviceStepper's step with the device solves, assemble_knp_twice
        _ode_step(st)
        L.check(lib.knpemi_assemble_emi(h, st.flags_emi))
        L.check(lib.knpemi_extrapolate_guess(h, L.B_EMI))
        dp.solve(L.B_EMI, 1e-9, 1e-40)
        assert _facet_launches(st) == 0 and _facet_launches(st) == 0
        L.check(lib.knpemi_extrapolate_guess(h, L.B_KNP))
        dp.solve(L.B_KNP, 1e-10, 2e-40)
        assert _facet_launches(st) == 1


def test_facet_kernel_is_skipped_after_a_write_back(hip_lib):
    """Where the write-back of the potential has formed the facet integrals -- a solution pasted on the device, as in
    bench.py's timed steps, or knpemi_solve_emi, as in DeviceStepper -- knpemi_assemble_knp launches no facet kernel, also
    when it assembles twice; after a change of the concentrations it does."""
    _in_child("_facet_kernel_skipped_after_a_write_back()", {"KNPEMI_FUSED_GRAPH": "0"})


def test_device_stepper_matches_dropin_path(hip_lib):
    """The device-resident step sequence (knpemi.stepper) leaves the same fields and ODE tables as the
    host-mirrored drop-in calls, bit for bit (no solves in between: c, phi held fixed)."""
    from knpemi import update_ode_variables, update_pde_variables
    from knpemi.pdeSolver import create_solver_emi, create_solver_knp
    from knpemi.stepper import DeviceStepper
    res = []
    for mode in ("dropin", "stepper", "stepper_ode_on_aux", "stepper_no_overlap"):
        s = Setup("tet", 0, g_syn=10.0)
        s.perturb()
        # physically sensible "solution" fields: c close to c_prev, phi_i - phi_e close to rest
        for t in s.subdomain_list:
            for k in range(2):
                s.c[t][k].x.array[:] = s.c_prev[t][k].x._a * 1.001
        s.phi[1].x.array[:] += -0.0744
        ode = s.mem_models[0]['ode']
        if mode.startswith("stepper"):
            st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi,
                               s.phi_M_prev, overlap=(mode != "stepper_no_overlap"))
            if mode == "stepper_ode_on_aux":
                st.ode_on_aux = True          # roles swapped: ODE sweep on the auxiliary stream, assembly on the main one
            st.add_membrane_model(ode, s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
            for _ in range(3):
                st.step()
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
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert np.array_equal(a, b)


def test_ten_time_steps_2d_match_oracle(hip_lib):
    """BASELINE configs[0]: 2D idealized mesh, 3 ions + HH, 10 time steps.  The whole loop of
    run_2D.py:341-372 through the knpemi API (GPU assembly + ODE sweep, direct host solves) against the
    oracle loop (oracle/driver.py)."""
    import adapters
    import driver
    from knpemi import update_ode_variables, update_pde_variables
    from knpemi.pdeSolver import create_solver_emi, create_solver_knp
    s = Setup("2d", 1, g_syn=10.0)
    o, P, params, ions = s.oracle()
    c_all, _, _, _ = s.oracle_fields()
    ode = s.mem_models[0]['ode']
    mask = np.array([x[0] < 20e-6 for x in ode.dof_locations])
    run = driver.OracleRun(P, params, ions, "hh_si", c_all, ode.states.copy(), ode.parameters.copy(),
                           ode.dof_locations, mask, {o.MODELS["hh_si"]["pidx"]["stim_amplitude"]: 10.0},
                           {'z': -1, 0: 0.0, 1: 0.0})
    emi = create_solver_emi(s.a_emi, s.L_emi, s.phi, s.entity_maps, s.subdomain_list, None, direct=True, p=s.p_emi)
    knp = create_solver_knp(s.a_knp, s.L_knp, s.c, s.entity_maps, s.subdomain_list, None, direct=True, p=s.p_knp)
    for k in range(10):
        update_ode_variables(ode, s.c_prev, s.phi_M_prev[1], s.ion_list, s.subdomain_list, s.mesh, s.ct, 1, k)
        ode.step_lsoda(s.dt, s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
        ode.get_membrane_potential(s.phi_M_prev[1])
        for ion, f in s.mem_models[0]['I_ch_k'].items():
            ode.get_parameter("I_ch_" + ion, f)
        emi.solve()
        knp.solve()
        update_pde_variables(s.c, s.c_prev, s.phi, s.phi_M_prev, s.physical_parameters, s.ion_list,
                             s.subdomain_list, s.mesh, s.ct)
        run.step()
    # potentials are defined up to a common constant: compare phi_M and the zero-mean potential
    assert rel_err(s.phi_M_prev[1].x._a, run.phiM[1]) < 1e-8
    x_gpu = np.concatenate([s.phi[0].x._a, s.phi[1].x._a])
    x_ref = np.concatenate([run.phi[0], run.phi[1]])
    assert rel_err(x_gpu - x_gpu.mean(), x_ref - x_ref.mean()) < 1e-8
    for t in (0, 1):
        for k in range(3):
            ref = run.c_all[t][k]
            got = s.c_prev[t][k].x._a if k < 2 else s.ion_list[-1][f'c_{t}'].x._a
            assert rel_err(got, ref) < 1e-10
    assert rel_err(ode.states, run.states) < 1e-8
    # physics sanity: the synaptic stimulus (x < 20 um) has depolarised the (electrotonically compact)
    # cell by more than 10 mV, slightly more at the stimulated end
    x = ode.dof_locations[:, 0]
    v = s.phi_M_prev[1].x._a
    assert v.mean() > -0.0744 + 0.010 and v[x < 15e-6].mean() > v[x > 40e-6].mean()


@pytest.mark.parametrize("sizes", [(16, 32, 64), (100, 200, 400)])
def test_mms_emi_convergence(hip_lib, sizes):
    """BASELINE configs[3]: manufactured solution of tests/run_mms_emi.py on the unit square with
    ICS = [0.25, 0.75]^2; GPU-assembled operator + diffusive RHS, L2 errors must converge at rate ~2
    (the reference only prints them).  (100, 200, 400) are the resolutions of the reference's
    tests/make_mesh_mms.py:96-98."""
    import contextlib
    import io
    from knpemi import create_functions_emi, create_functions_knp, emi_system, set_initial_conditions
    from knpemi.fem import Constant, extract_submesh, make_mesh_mms
    from knpemi.mms import l2_error
    from knpemi.pdeSolver import create_solver_emi
    from mms_problem import CONC, MMS, MMSMembraneModel
    errs = []
    for M in sizes:
        mesh, ct, ft = make_mesh_mms(M)
        s1, i2p, iv2p, _, _ = extract_submesh(mesh, ct, 1)
        s0, e2p, ev2p, _, _ = extract_submesh(mesh, ct, 0)
        g, g2p, gv2p, _, _ = extract_submesh(mesh, ft, 1)
        subs = {0: dict(name="ECS", mesh_sub=s0, sub_to_parent=e2p, sub_vertex_to_parent=ev2p),
                1: dict(name="neuron", mesh_sub=s1, sub_to_parent=i2p, sub_vertex_to_parent=iv2p, mesh_mem=g,
                        mem_to_parent=g2p)}
        one = lambda m: Constant(m, 1.0)
        pp = {'dt': one(mesh), 'F': one(mesh), 'psi': one(mesh), 'C_phi': one(mesh), 'C_M': one(mesh),
              'R': one(mesh), 'temperature': one(mesh), 'rho': {0: Constant(s0, 0.0), 1: Constant(s1, 0.0)}}
        ions = [dict(z=zz, name=n, D={0: one(s0), 1: one(s1)}) for n, zz in (("a", 1.0), ("b", -1.0), ("c", 1.0))]
        phi, phi_M_prev = create_functions_emi(subs, degree=1)
        c, c_prev = create_functions_knp(subs, ions, degree=1)
        for ion in ions:
            fe, fi = CONC[ion['name']]
            ion['c_init'] = {0: fe(s0.x.T), 1: fi(s1.x.T)}
        set_initial_conditions(ions, subs, c_prev)
        mm = MMSMembraneModel()
        mm.tag = 1
        subs[1]['mem_models'] = [{'ode': mm, 'I_ch_k': {'a': 0.0, 'b': 0.0, 'c': 0.0}}]
        a, p, Lf, dx, bc = emi_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c_prev, 1.0, mms=MMS)
        problem = create_solver_emi(a, Lf, phi, [g2p, e2p, i2p], subs, None, bcs=[bc])
        problem.solve()
        phi_e, phi_i = problem.u
        errs.append((l2_error(phi_i, MMS["phi_i_exact"]), l2_error(phi_e, MMS["phi_e_exact"])))
    errs = np.array(errs)
    rates = np.log2(errs[:-1] / errs[1:])
    print("MMS L2 errors (phi_i, phi_e):", errs, "rates:", rates)
    assert np.all(rates[-1] > 1.8) and np.all(errs[-1] < 5e-3)


@pytest.mark.parametrize("key", ["hh_si_stim0", "hh_si_stim10", "hh_mv_stim0", "hh_mv_stim1", "glial_stim0"])
def test_all_membrane_models_match_golden_trajectories(hip_lib, key):
    """Every device RHS (HH-SI, HH-mV, glial) integrated by the GPU LSODA against the committed ODEPACK
    trajectories (tests/golden/ode_models.npz): states to 1e-8, side-effect currents to 1e-5 (tests/test_lsoda_host.py)."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ode_models.npz"))
    model = key.rsplit("_stim", 1)[0]
    s = Setup("2d", 1, model=model)
    ode = s.mem_models[0]['ode']
    ode.states[:] = g[f"{key}_y0"]
    ode.parameters[:] = g[f"{key}_p0"]
    dt = float(g[f"{key}_dt"])
    ns = ode.states.shape[1]
    ich = [ode.ode.parameter_indices(f"I_ch_{n}") for n in ("Na", "K", "Cl")]
    for k in range(10):
        ode._pending_flags = 0          # parameters are used as they are (no trace refresh)
        ode.step_lsoda(dt, None)
        gold = g[f"{key}_traj"][k]
        assert np.abs(ode.states - gold[:ns]).max() <= 1e-8 * np.abs(gold[:ns]).max()
        assert np.abs(ode.parameters[:, ich] - gold[ns:]).max() <= 1e-5 * max(np.abs(gold[ns:]).max(), 1e-3)
    assert np.all(ode.states == ode.states[0])      # identical inputs -> identical bits on every dof


def test_two_waves_per_simd_ode_variant_is_bit_identical(hip_lib, monkeypatch):
    """Large sweeps (more waves than SIMDs) run a register-capped build of the ODE kernel so that two waves share a
    SIMD (KNPEMI_ODE_WAVES forces it here): spills change no arithmetic, so states, currents and counts are
    identical to the default build."""
    from knpemi.utils import update_ode_variables
    out = []
    for waves in ("1", "2"):
        monkeypatch.setenv("KNPEMI_ODE_WAVES", waves)
        s = Setup("2d", 2, g_syn=10.0)
        s.perturb()
        s.phi_M_prev[1].x.array[:] = -0.0744
        ode = s.mem_models[0]['ode']
        for k in range(3):
            update_ode_variables(ode, s.c_prev, s.phi_M_prev[1], s.ion_list, s.subdomain_list, s.mesh, s.ct, 1, k)
            ode.step_lsoda(s.dt, s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
            ode.get_membrane_potential(s.phi_M_prev[1])
        out.append((ode.states.copy(), ode.parameters.copy(), dict(ode.last_stats)))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert all(out[0][2][k] == out[1][2][k] for k in ("n_rhs", "n_steps"))


def _custom_problem(mesh, ct, ft, cell_specs, dt=1e-4):
    """Build functions/forms through the knpemi API for an arbitrary tagging.
    cell_specs = {cell tag: [(facet tag, model name), ...]} (ECS = tag 0 is implicit)."""
    import contextlib
    import io
    from helpers import C_M, FARADAY, PSI, load_model
    from knpemi import (create_functions_emi, create_functions_knp, emi_system, knp_system,
                        set_initial_conditions, setup_membrane_model)
    from knpemi.fem import Constant, extract_submesh
    tags = [0] + sorted(cell_specs)
    subs = {}
    for t in tags:
        sm, e2p, v2p, _, _ = extract_submesh(mesh, ct, t)
        subs[t] = dict(tag=t, name=f"sub{t}", mesh_sub=sm, sub_to_parent=e2p, sub_vertex_to_parent=v2p)
        if t > 0:
            mtags = [ftag for ftag, _ in cell_specs[t]]
            g, g2p, _, _, _ = extract_submesh(mesh, ft, mtags)
            subs[t].update(mesh_mem=g, mem_to_parent=g2p, membrane_tags=mtags,
                           ode_models={ftag: load_model(m) for ftag, m in cell_specs[t]})
    rho = {'z': -1, **{t: Constant(subs[t]['mesh_sub'], 0.1 * t) for t in tags}}
    pp = {'dt': Constant(mesh, dt), 'F': Constant(mesh, FARADAY), 'psi': Constant(mesh, PSI),
          'C_phi': Constant(mesh, C_M / dt), 'C_M': Constant(mesh, C_M), 'rho': rho}
    init = {"Na": (100.7, 12.8), "K": (3.3, 124.2), "Cl": (104.0, 137.0)}
    Dv = {"Na": 1.33e-9, "K": 1.96e-9, "Cl": 2.03e-9}
    ions = [dict(name=n, z=z, D={t: Constant(None, Dv[n] * (1 + 0.1 * t)) for t in tags},
                 c_init={t: Constant(None, init[n][0 if t == 0 else 1]) for t in tags})
            for n, z in (("K", 1.0), ("Cl", -1.0), ("Na", 1.0))]
    with contextlib.redirect_stdout(io.StringIO()):
        phi, phi_M_prev = create_functions_emi(subs, degree=1)
        c, c_prev = create_functions_knp(subs, ions, degree=1)
        set_initial_conditions(ions, subs, c_prev)
        for t in tags[1:]:
            subs[t]['mem_models'] = setup_membrane_model({'stimulus': {}, 'stimulus_locator': None}, pp,
                                                         subs[t]['ode_models'], ft, phi_M_prev[t].function_space, ions)
    a_emi, p_emi, L_emi = emi_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c_prev, dt)
    a_knp, p_knp, L_knp = knp_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c, c_prev, dt)
    ns = type("S", (), {})()
    ns.__dict__.update(mesh=mesh, ct=ct, ft=ft, subdomain_list=subs, ion_list=ions, physical_parameters=pp, dt=dt,
                       phi=phi, phi_M_prev=phi_M_prev, c=c, c_prev=c_prev, a_emi=a_emi, p_emi=p_emi, L_emi=L_emi,
                       a_knp=a_knp, p_knp=p_knp, L_knp=L_knp, entity_maps=[])
    # seeded, physically sensible perturbation
    rng = np.random.default_rng(7)
    for t in tags:
        for f in c_prev[t] + [ions[-1][f'c_{t}']]:
            f.x.array[:] *= 1.0 + 1e-3 * rng.uniform(-1, 1, f.x.array.shape[0])
        phi[t].x.array[:] = 1e-3 * rng.uniform(-1, 1, phi[t].x.array.shape[0])
        if t > 0:
            phi_M_prev[t].x.array[:] = -0.07 + 1e-3 * rng.uniform(-1, 1, phi_M_prev[t].x.array.shape[0])
            for mm in subs[t]['mem_models']:
                for f in mm['I_ch_k'].values():
                    f.x.array[:] = 1e-2 * rng.uniform(-1, 1, f.x.array.shape[0])
    return ns


def _compare_with_oracle(s, subdomains):
    import adapters
    from knpemi.pdeSolver import create_solver_emi, create_solver_knp
    o, P, params, ions = adapters.oracle_problem(s, subdomains)
    c_all, phi, phiM, mm = adapters.oracle_fields(s)
    emi = create_solver_emi(s.a_emi, s.L_emi, s.phi, [], s.subdomain_list, None, p=s.p_emi, direct=False)
    knp = create_solver_knp(s.a_knp, s.L_knp, s.c, [], s.subdomain_list, None, p=s.p_knp)
    A, b = emi.assemble()
    Ak, bk = knp.assemble()
    Ao, Po, bo = o.assemble_emi(P, params, ions, c_all, phiM, mm)
    Ako, bko = o.assemble_knp(P, params, ions, c_all, phi, phiM, mm, s.dt)
    return dict(A_emi=csr_rel_err(A, Ao), P_emi=csr_rel_err(emi.P, Po), b_emi=rel_err(b, bo),
                A_knp=csr_rel_err(Ak, Ako), b_knp=rel_err(bk, bko))


def test_three_subdomains_two_cell_types(hip_lib):
    """config-5 style tagging (local_astrocyte_depolarization/run_stim_duration.py:168-181): ECS + cell
    tag 1 (HH) + cell tag 2 (glial), each with its own membrane space and model; different D and rho per
    sub-domain; assembly and the end-of-step update against the oracle."""
    from knpemi import update_pde_variables
    from knpemi.fem import make_mesh_3D
    mesh, ct, ft = make_mesh_3D(0, "tetrahedron", axon_tags=(1, 1, 2, 2))
    s = _custom_problem(mesh, ct, ft, {1: [(1, "hh_si")], 2: [(2, "glial")]})
    errs = _compare_with_oracle(s, {0: [], 1: [1], 2: [2]})
    assert max(errs.values()) < TOL, errs
    import adapters
    o, P, params, ions = adapters.oracle_problem(s, {0: [], 1: [1], 2: [2]})
    c_all, phi, phiM, _ = adapters.oracle_fields(s)
    for t in s.subdomain_list:
        for k in range(2):
            s.c[t][k].x.array[:] = s.c_prev[t][k].x._a * 1.01
    c_new = {t: [f.x._a.copy() for f in s.c[t]] for t in s.subdomain_list}
    update_pde_variables(s.c, s.c_prev, s.phi, s.phi_M_prev, s.physical_parameters, s.ion_list,
                         s.subdomain_list, s.mesh, s.ct)
    o.update_pde_variables(P, ions, {'z': -1, 0: 0.0, 1: 0.1, 2: 0.2}, c_new, c_all, phi, phiM)
    for t in s.subdomain_list:
        assert rel_err(s.ion_list[-1][f'c_{t}'].x._a, c_all[t][2]) < 1e-14
        if t > 0:
            assert rel_err(s.phi_M_prev[t].x._a, phiM[t]) < 1e-14


def test_several_membrane_tags_on_one_cell(hip_lib):
    """benchmark/run_stim_duration.py:163-166 style: one cell whose membrane carries two facet tags, each
    with its own MembraneModel on the same Q; a third tag has no model and must not be integrated."""
    from knpemi.fem import make_mesh_2D, meshtags
    mesh, ct, ft = make_mesh_2D(1)
    vals = ft.values.copy()
    mem = np.flatnonzero(vals == 1)
    xm = mesh.x[mesh.facets[ft.indices[mem]]].mean(axis=1)[:, 0]
    vals[mem[xm > 20e-6]] = 6
    vals[mem[xm > 45e-6]] = 7          # tag 7: part of the membrane space, but no model -> not integrated
    ft2 = meshtags(mesh, 1, ft.indices, vals)
    s = _custom_problem(mesh, ct, ft2, {1: [(1, "hh_si"), (6, "hh_si")]})
    # the membrane space must contain the facets of all three tags
    s2 = None
    errs = _compare_with_oracle(s, {0: [], 1: [1, 6]})
    assert max(errs.values()) < TOL, errs


def test_empty_cell_subdomain(hip_lib):
    """make_mesh_2D(0): the ICS is empty; the library must accept a cellular
    sub-domain without cells, membrane or ODE points and still assemble the ECS blocks."""
    from knpemi.fem import make_mesh_2D
    mesh, ct, ft = make_mesh_2D(0)
    assert (ct.values == 1).sum() == 0
    s = _custom_problem(mesh, ct, ft, {1: [(1, "hh_si")]})
    errs = _compare_with_oracle(s, {0: [], 1: [1]})
    assert max(errs.values()) < TOL, errs
    ode = s.subdomain_list[1]['mem_models'][0]['ode']
    assert ode.nodes == 0
    ode.step_lsoda(1e-4, None)


def test_mms_knp_convergence(hip_lib):
    """Manufactured KNP problem of tests/mms_knp_problem.py through the knpemi API: GPU-assembled mass / dt +
    diffusion + drift operator and source right-hand side, device BiCGStab + AMG solve; second order in L2."""
    import contextlib
    import io
    import mms_knp_problem as K
    from knpemi import create_functions_emi, create_functions_knp, emi_system, knp_system, set_initial_conditions
    from knpemi.fem import Constant, Function, create_unit_square, extract_submesh, meshtags
    from knpemi.pdeSolver import create_solver_knp
    errs = []
    for M in (8, 16, 32):
        mesh = create_unit_square(None, M, M)
        ct = meshtags(mesh, 2, np.arange(mesh.num_cells), np.zeros(mesh.num_cells, np.int32))
        ft = meshtags(mesh, 1, np.zeros(0, np.int32), np.zeros(0, np.int32))
        subs = {}
        for t in (0, 1):
            sm, e2p, v2p, _, _ = extract_submesh(mesh, ct, t)
            subs[t] = dict(tag=t, name=f"sub{t}", mesh_sub=sm, sub_to_parent=e2p, sub_vertex_to_parent=v2p)
        g, g2p, _, _, _ = extract_submesh(mesh, ft, [1])
        subs[1].update(mesh_mem=g, mem_to_parent=g2p, membrane_tags=[1], mem_models=[])
        s0 = subs[0]['mesh_sub']
        cst = lambda v: {0: Constant(s0, v), 1: Constant(subs[1]['mesh_sub'], v)}
        pp = {'dt': Constant(mesh, K.DT), 'F': Constant(mesh, 1.0), 'psi': Constant(mesh, K.PSI),
              'C_phi': Constant(mesh, 1.0 / K.DT), 'C_M': Constant(mesh, 1.0), 'rho': {'z': -1, **cst(0.0)}}
        ions = [dict(name=n, z=z, D=cst(K.D), c_init=cst(1.0)) for n, z in zip("abc", K.Z)]
        with contextlib.redirect_stdout(io.StringIO()):
            phi, phi_M_prev = create_functions_emi(subs, degree=1)
            c, c_prev = create_functions_knp(subs, ions, degree=1)
            set_initial_conditions(ions, subs, c_prev)
        X0 = s0.x.T
        for k in range(2):
            c_prev[0][k].x.array[:] = K.C_EXACT[k](X0)
            c[0][k].x.array[:] = c_prev[0][k].x._a            # initial guess of the iterative solve
            f = Function(c_prev[0][k].function_space, name=f"f_{k}")
            f.x.array[:] = K.F_SOURCE[k](X0)
            ions[k]['f_source'] = f
        ions[2]['c_0'].x.array[:] = K.C_ELIM(X0)
        phi[0].x.array[:] = K.PHI(X0)
        emi_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c_prev, K.DT)
        a_knp, p_knp, L_knp = knp_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c, c_prev, K.DT)
        knp = create_solver_knp(a_knp, L_knp, c, [], subs, None, direct=False, p=p_knp, rtol=1e-12, atol=1e-40)
        knp.solve()
        errs.append([K.l2_error_p1(s0, c[0][k].x._a, K.C_EXACT[k]) for k in range(2)])
    errs = np.array(errs)
    rates = np.log2(errs[:-1] / errs[1:])
    print("KNP MMS L2 errors:", errs, "rates:", rates)
    assert np.all(rates > 1.9) and np.all(errs[-1] < 2e-2), (errs, rates)


@pytest.mark.parametrize("cell_type", ["tetrahedron", "hexahedron"])
def test_mms_knp_convergence_3d(hip_lib, cell_type):
    """The manufactured KNP steady state on the unit cube: an analytic check of the 3D row kernels (P1 tetrahedra,
    Q1 hexahedra) -- mass / dt, diffusion, drift, source -- with the device solve; second order."""
    import contextlib
    import io
    import mms_knp_problem as K
    from knpemi import create_functions_emi, create_functions_knp, emi_system, knp_system, set_initial_conditions
    from knpemi.fem import Constant, Function, create_box, extract_submesh, meshtags
    from knpemi.pdeSolver import create_solver_knp
    errs = []
    for M in (4, 8, 16):
        mesh = create_box(None, [np.zeros(3), np.ones(3)], (M, M, M), cell_type)
        ct = meshtags(mesh, 3, np.arange(mesh.num_cells), np.zeros(mesh.num_cells, np.int32))
        ft = meshtags(mesh, 2, np.zeros(0, np.int32), np.zeros(0, np.int32))
        subs = {}
        for t in (0, 1):
            sm, e2p, v2p, _, _ = extract_submesh(mesh, ct, t)
            subs[t] = dict(tag=t, name=f"sub{t}", mesh_sub=sm, sub_to_parent=e2p, sub_vertex_to_parent=v2p)
        g, g2p, _, _, _ = extract_submesh(mesh, ft, [1])
        subs[1].update(mesh_mem=g, mem_to_parent=g2p, membrane_tags=[1], mem_models=[])
        s0 = subs[0]['mesh_sub']
        cst = lambda v: {0: Constant(s0, v), 1: Constant(subs[1]['mesh_sub'], v)}
        pp = {'dt': Constant(mesh, K.DT), 'F': Constant(mesh, 1.0), 'psi': Constant(mesh, K.PSI),
              'C_phi': Constant(mesh, 1.0 / K.DT), 'C_M': Constant(mesh, 1.0), 'rho': {'z': -1, **cst(0.0)}}
        ions = [dict(name=n, z=z, D=cst(K.D), c_init=cst(1.0)) for n, z in zip("abc", K.Z)]
        with contextlib.redirect_stdout(io.StringIO()):
            phi, phi_M_prev = create_functions_emi(subs, degree=1)
            c, c_prev = create_functions_knp(subs, ions, degree=1)
            set_initial_conditions(ions, subs, c_prev)
        X0 = s0.x.T
        for k in range(2):
            c_prev[0][k].x.array[:] = K.C3_EXACT[k](X0)
            c[0][k].x.array[:] = c_prev[0][k].x._a
            f = Function(c_prev[0][k].function_space, name=f"f_{k}")
            f.x.array[:] = K.F3_SOURCE[k](X0)
            ions[k]['f_source'] = f
        ions[2]['c_0'].x.array[:] = K.C3_ELIM(X0)
        phi[0].x.array[:] = K.PHI3(X0)
        emi_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c_prev, K.DT)
        a_knp, p_knp, L_knp = knp_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c, c_prev, K.DT)
        knp = create_solver_knp(a_knp, L_knp, c, [], subs, None, direct=False, p=p_knp, rtol=1e-12, atol=1e-40)
        knp.solve()
        errs.append([K.nodal_rms_error(c[0][k].x._a, K.C3_EXACT[k](X0)) for k in range(2)])
    errs = np.array(errs)
    rates = np.log2(errs[:-1] / errs[1:])
    print("3D KNP MMS nodal errors:", errs, "rates:", rates)
    assert np.all(rates[-1] > 1.8) and np.all(errs[-1] < 5e-2), (errs, rates)


@pytest.mark.parametrize("cell_type", ["triangle", "tetrahedron", "hexahedron"])
def test_emi_volume_terms_recover_boltzmann_potential(hip_lib, cell_type):
    """Analytic check of the EMI volume kernels (kappa-stiffness and the all-ion diffusive right-hand side) in 2D and
    3D: concentrations in Boltzmann equilibrium with a given potential (tests/mms_knp_problem.py) make that potential
    the solution of the assembled system; device CG + AMG with the constant null space; second order."""
    import contextlib
    import io
    import mms_knp_problem as K
    from knpemi import create_functions_emi, create_functions_knp, emi_system, set_initial_conditions
    from knpemi.fem import Constant, create_box, create_unit_square, extract_submesh, meshtags
    from knpemi.pdeSolver import create_solver_emi
    errs = []
    for M in ((16, 32, 64) if cell_type == "triangle" else (4, 8, 16)):
        if cell_type == "triangle":
            mesh = create_unit_square(None, M, M)
        else:
            mesh = create_box(None, [np.zeros(3), np.ones(3)], (M, M, M), cell_type)
        ct = meshtags(mesh, mesh.tdim, np.arange(mesh.num_cells), np.zeros(mesh.num_cells, np.int32))
        ft = meshtags(mesh, mesh.tdim - 1, np.zeros(0, np.int32), np.zeros(0, np.int32))
        subs = {}
        for t in (0, 1):
            sm, e2p, v2p, _, _ = extract_submesh(mesh, ct, t)
            subs[t] = dict(tag=t, name=f"sub{t}", mesh_sub=sm, sub_to_parent=e2p, sub_vertex_to_parent=v2p)
        g, g2p, _, _, _ = extract_submesh(mesh, ft, [1])
        subs[1].update(mesh_mem=g, mem_to_parent=g2p, membrane_tags=[1], mem_models=[])
        s0 = subs[0]['mesh_sub']
        cst = lambda v: {0: Constant(s0, v), 1: Constant(subs[1]['mesh_sub'], v)}
        pp = {'dt': Constant(mesh, 1.0), 'F': Constant(mesh, 1.0), 'psi': Constant(mesh, K.PSI),
              'C_phi': Constant(mesh, 1.0), 'C_M': Constant(mesh, 1.0), 'rho': {'z': -1, **cst(0.0)}}
        ions = [dict(name=n, z=z, D=cst(K.D), c_init=cst(1.0)) for n, z in zip("abc", K.Z)]
        with contextlib.redirect_stdout(io.StringIO()):
            phi, phi_M_prev = create_functions_emi(subs, degree=1)
            c, c_prev = create_functions_knp(subs, ions, degree=1)
            set_initial_conditions(ions, subs, c_prev)
        ph, cs = K.emi_exact(s0.x.T)
        # ion order [a (z=+1), b (z=-1), c (z=+1, eliminated)]: the varying species must carry z = +1
        c_prev[0][0].x.array[:] = cs[0]
        c_prev[0][1].x.array[:] = cs[1]
        ions[2]['c_0'].x.array[:] = cs[2]
        a_emi, p_emi, L_emi = emi_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c_prev, 1.0)
        emi = create_solver_emi(a_emi, L_emi, phi, [], subs, None, direct=False, p=p_emi, rtol=1e-12, atol=1e-40)
        emi.solve()
        x = phi[0].x._a
        errs.append(K.nodal_rms_error(x - x.mean(), ph - ph.mean()))
    errs = np.array(errs)
    rates = np.log2(errs[:-1] / errs[1:])
    print(cell_type, "EMI Boltzmann check: errors", errs, "rates", rates)
    assert rates[-1] > 1.8 and errs[-1] < 2e-2, (errs, rates)


@pytest.mark.parametrize("splitting", [False, True])
def test_mms_knp_membrane_convergence(hip_lib, splitting):
    """Membrane variant of the manufactured KNP problem (tests/mms_knp_problem.py): the rational Robin terms of b_knp
    (alpha fractions, C, g, signs on both sides, with and without the splitting correction) assembled by
    knp_membrane_kernel + knp_rows and solved on the device; second order in L2 on both sub-domains."""
    import contextlib
    import io
    import mms_knp_problem as K
    from mms_problem import MMSMembraneModel
    from knpemi import create_functions_emi, create_functions_knp, emi_system, knp_system, set_initial_conditions
    from knpemi.fem import Constant, Function, extract_submesh, make_mesh_mms
    from knpemi.pdeSolver import create_solver_knp
    errs = []
    for M in (16, 32, 64):
        mesh, ct, ft = make_mesh_mms(M)
        s0, e2p, ev2p, _, _ = extract_submesh(mesh, ct, 0)
        s1, i2p, iv2p, _, _ = extract_submesh(mesh, ct, 1)
        g, g2p, _, _, _ = extract_submesh(mesh, ft, 1)
        subs = {0: dict(name="ECS", mesh_sub=s0, sub_to_parent=e2p, sub_vertex_to_parent=ev2p),
                1: dict(name="cell", mesh_sub=s1, sub_to_parent=i2p, sub_vertex_to_parent=iv2p, mesh_mem=g,
                        mem_to_parent=g2p)}
        cst = lambda v: {0: Constant(s0, v), 1: Constant(s1, v)}
        pp = {'dt': Constant(mesh, K.DT_M), 'F': Constant(mesh, K.F_CONST), 'psi': Constant(mesh, K.PSI),
              'C_phi': Constant(mesh, K.C_M / K.DT_M), 'C_M': Constant(mesh, K.C_M), 'rho': {'z': -1, **cst(0.0)}}
        ions = [dict(name=n, z=z, D=cst(K.D), c_init=cst(1.0)) for n, z in zip("abc", K.Z)]
        with contextlib.redirect_stdout(io.StringIO()):
            phi, phi_M_prev = create_functions_emi(subs, degree=1)
            c, c_prev = create_functions_knp(subs, ions, degree=1)
            set_initial_conditions(ions, subs, c_prev)
        Q = phi_M_prev[1].function_space
        XQ = g.x.T
        I = K.channel_currents(XQ)
        I_ch_k = {}
        for k, n in enumerate("abc"):
            I_ch_k[n] = Function(Q, name=f"I_ch_{n}")
            I_ch_k[n].x.array[:] = I[k]
        mm = MMSMembraneModel()
        mm.tag = 1
        subs[1]['mem_models'] = [{'ode': mm, 'I_ch_k': I_ch_k}]
        phi_M_prev[1].x.array[:] = K.membrane_potential_prev(XQ, splitting)
        for t, sm in ((0, s0), (1, s1)):
            X = sm.x.T
            for k in range(2):
                c_prev[t][k].x.array[:] = K.M_CPREV[k](X)
                c[t][k].x.array[:] = K.M_C[k](X) * 1.01          # initial guess, off the answer
            ions[2][f'c_{t}'].x.array[:] = K.M_C[2](X)
            phi[t].x.array[:] = K.M_PHI(X) - (K.PHI0 if t == 0 else 0.0)
        emi_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c_prev, K.DT_M)
        a_knp, p_knp, L_knp = knp_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c, c_prev, K.DT_M)
        for f in (a_knp, L_knp):
            f.shared['splitting_scheme'] = splitting
        knp = create_solver_knp(a_knp, L_knp, c, [], subs, None, direct=False, p=p_knp, rtol=1e-12, atol=1e-40)
        knp.solve()
        errs.append([K.l2_error_p1(sm, c[t][k].x._a, K.M_C[k]) for t, sm in ((0, s0), (1, s1)) for k in range(2)])
    errs = np.array(errs)
    rates = np.log2(errs[:-1] / errs[1:])
    print("KNP membrane MMS L2 errors:", errs, "rates:", rates)
    assert np.all(rates > 1.85) and np.all(errs[-1] < 1e-2), (errs, rates)


@pytest.mark.parametrize("cell_type", ["tetrahedron", "hexahedron"])
def test_mms_knp_membrane_convergence_3d(hip_lib, cell_type):
    """3D membrane variant of the manufactured KNP problem: the triangular (tetrahedra) and quadrilateral (hexahedra)
    membrane-facet kernels with their degree-6 rules, the 3D row kernels' membrane sums and the device solve; second
    order on both sub-domains (splitting scheme on)."""
    import contextlib
    import io
    import mms_knp_problem as K
    from mms_problem import MMSMembraneModel
    from knpemi import create_functions_emi, create_functions_knp, emi_system, knp_system, set_initial_conditions
    from knpemi.fem import Constant, Function, create_box, extract_submesh
    from knpemi.fem.idealized import _tag
    from knpemi.pdeSolver import create_solver_knp
    errs = []
    for M in (8, 16, 32) if cell_type == "hexahedron" else (8, 16):
        mesh = create_box(None, [np.zeros(3), np.ones(3)], (M, M, M), cell_type)
        ct, ft = _tag(mesh, [([0.25] * 3, [0.75] * 3)], [1], full_facet_tags=False)
        s0, e2p, ev2p, _, _ = extract_submesh(mesh, ct, 0)
        s1, i2p, iv2p, _, _ = extract_submesh(mesh, ct, 1)
        g, g2p, _, _, _ = extract_submesh(mesh, ft, 1)
        subs = {0: dict(name="ECS", mesh_sub=s0, sub_to_parent=e2p, sub_vertex_to_parent=ev2p),
                1: dict(name="cell", mesh_sub=s1, sub_to_parent=i2p, sub_vertex_to_parent=iv2p, mesh_mem=g,
                        mem_to_parent=g2p)}
        cst = lambda v: {0: Constant(s0, v), 1: Constant(s1, v)}
        pp = {'dt': Constant(mesh, K.DT_M3), 'F': Constant(mesh, K.F_CONST), 'psi': Constant(mesh, K.PSI),
              'C_phi': Constant(mesh, K.C_M / K.DT_M3), 'C_M': Constant(mesh, K.C_M), 'rho': {'z': -1, **cst(0.0)}}
        ions = [dict(name=n, z=z, D=cst(K.D), c_init=cst(1.0)) for n, z in zip("abc", K.Z)]
        with contextlib.redirect_stdout(io.StringIO()):
            phi, phi_M_prev = create_functions_emi(subs, degree=1)
            c, c_prev = create_functions_knp(subs, ions, degree=1)
            set_initial_conditions(ions, subs, c_prev)
        Q = phi_M_prev[1].function_space
        XQ = g.x.T
        I = K.channel_currents3(XQ)
        I_ch_k = {}
        for k, n in enumerate("abc"):
            I_ch_k[n] = Function(Q, name=f"I_ch_{n}")
            I_ch_k[n].x.array[:] = I[k]
        mm = MMSMembraneModel()
        mm.tag = 1
        subs[1]['mem_models'] = [{'ode': mm, 'I_ch_k': I_ch_k}]
        phi_M_prev[1].x.array[:] = K.membrane_potential_prev3(XQ, True)
        for t, sm in ((0, s0), (1, s1)):
            X = sm.x.T
            for k in range(2):
                c_prev[t][k].x.array[:] = K.M3_CPREV[k](X)
                c[t][k].x.array[:] = K.M3_C[k](X) * 1.01
            ions[2][f'c_{t}'].x.array[:] = K.M3_C[2](X)
            phi[t].x.array[:] = K.M3_PHI(X) - (K.PHI0 if t == 0 else 0.0)
        emi_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c_prev, K.DT_M3)
        a_knp, p_knp, L_knp = knp_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c, c_prev, K.DT_M3)
        knp = create_solver_knp(a_knp, L_knp, c, [], subs, None, direct=False, p=p_knp, rtol=1e-12, atol=1e-40)
        knp.solve()
        errs.append([K.nodal_rms_error(c[t][k].x._a, K.M3_C[k](sm.x.T)) for t, sm in ((0, s0), (1, s1)) for k in range(2)])
    errs = np.array(errs)
    rates = np.log2(errs[:-1] / errs[1:])
    print(cell_type, "3D KNP membrane MMS: errors", errs[-1], "rates", rates[-1])
    assert np.all(rates[-1] > 1.7) and np.all(errs[-1] < 1e-1), (errs, rates)


@pytest.mark.parametrize("splitting", [True, False])
@pytest.mark.parametrize("cell_type", ["triangle", "tetrahedron", "hexahedron"])
def test_emi_membrane_coupling_recovers_jump(hip_lib, cell_type, splitting):
    """Analytic check of the EMI membrane terms (coupling C_phi [u][v] with the facet mass of intervals, triangles and
    quadrilaterals, Robin right-hand side) in 2D and 3D: Boltzmann-equilibrium concentrations on both sides (zero
    total current) and phi_M_prev = PHI0 make phi_e = P u, phi_i = P u + PHI0 the solution; the jump across the membrane
    and both potentials come back at second order from the device CG + AMG solve."""
    import contextlib
    import io
    import mms_knp_problem as K
    from mms_problem import MMSMembraneModel
    from knpemi import create_functions_emi, create_functions_knp, emi_system, set_initial_conditions
    from knpemi.fem import Constant, Function, create_box, create_unit_square, extract_submesh
    from knpemi.fem.idealized import _tag
    from knpemi.pdeSolver import create_solver_emi
    errs = []
    d = 2 if cell_type == "triangle" else 3
    for M in ((16, 32, 64) if d == 2 else (8, 16)):
        mesh = create_unit_square(None, M, M) if d == 2 else create_box(None, [np.zeros(3), np.ones(3)], (M, M, M), cell_type)
        ct, ft = _tag(mesh, [([0.25] * d, [0.75] * d)], [1], full_facet_tags=False)
        s0, e2p, ev2p, _, _ = extract_submesh(mesh, ct, 0)
        s1, i2p, iv2p, _, _ = extract_submesh(mesh, ct, 1)
        g, g2p, _, _, _ = extract_submesh(mesh, ft, 1)
        subs = {0: dict(name="ECS", mesh_sub=s0, sub_to_parent=e2p, sub_vertex_to_parent=ev2p),
                1: dict(name="cell", mesh_sub=s1, sub_to_parent=i2p, sub_vertex_to_parent=iv2p, mesh_mem=g,
                        mem_to_parent=g2p)}
        cst = lambda v: {0: Constant(s0, v), 1: Constant(s1, v)}
        pp = {'dt': Constant(mesh, 1.0), 'F': Constant(mesh, 1.0), 'psi': Constant(mesh, K.PSI),
              'C_phi': Constant(mesh, 1.0), 'C_M': Constant(mesh, 1.0), 'rho': {'z': -1, **cst(0.0)}}
        ions = [dict(name=n, z=z, D=cst(K.D), c_init=cst(1.0)) for n, z in zip("abc", K.Z)]
        with contextlib.redirect_stdout(io.StringIO()):
            phi, phi_M_prev = create_functions_emi(subs, degree=1)
            c, c_prev = create_functions_knp(subs, ions, degree=1)
            set_initial_conditions(ions, subs, c_prev)
        Q = phi_M_prev[1].function_space
        zero = {}
        for n in "abc":
            zero[n] = Function(Q, name=f"I_ch_{n}")
        mm = MMSMembraneModel()
        mm.tag = 1
        subs[1]['mem_models'] = [{'ode': mm, 'I_ch_k': zero}]
        phi_M_prev[1].x.array[:] = K.PHI0
        if not splitting:
            # emiWeakForm.py:236: g = phi_M_prev - I_ch / C_phi; a non-zero channel current compensated in phi_M_prev
            # leaves the same solution and exercises that branch
            I_tot = 0.3 + 0.2 * np.cos(2 * np.pi * g.x[:, 0])
            zero["a"].x.array[:] = 0.7 * I_tot
            zero["c"].x.array[:] = 0.3 * I_tot
            phi_M_prev[1].x.array[:] = K.PHI0 + I_tot / 1.0
        exact = {}
        for t, sm in ((0, s0), (1, s1)):
            ph, cs = K.emi_exact(sm.x.T)
            exact[t] = ph + (K.PHI0 if t == 1 else 0.0)
            c_prev[t][0].x.array[:] = cs[0]
            c_prev[t][1].x.array[:] = cs[1]
            ions[2][f'c_{t}'].x.array[:] = cs[2]
        a_emi, p_emi, L_emi = emi_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c_prev, 1.0)
        a_emi.shared['splitting_scheme'] = splitting
        emi = create_solver_emi(a_emi, L_emi, phi, [], subs, None, direct=False, p=p_emi, rtol=1e-12, atol=1e-40)
        emi.solve()
        # P_emi - A_emi is the mass matrix of the cell (tabulated once at set-up): nothing on the ECS rows, entries
        # that sum to the volume of [0.25, 0.75]^d, symmetric
        A, _ = emi.assemble()
        Mm = (emi.P - A).tocsr()
        n0 = phi[0].x.array.shape[0]
        assert Mm[:n0].nnz == 0 or np.abs(Mm[:n0].data).max() == 0.0
        assert abs(Mm.sum() - 0.5 ** d) < 1e-10 and abs(Mm - Mm.T).max() < 1e-13
        x = np.concatenate([phi[0].x._a, phi[1].x._a])
        xe = np.concatenate([exact[0], exact[1]])
        shift = (x - xe).mean()                       # the system fixes the potentials up to one common constant
        jump = phi[1].x._a.mean() - exact[1].mean() - (phi[0].x._a.mean() - exact[0].mean())
        errs.append([K.nodal_rms_error(x - shift, xe), abs(jump)])
    errs = np.array(errs)
    rates = np.log2(errs[:-1] / errs[1:])
    print(cell_type, "EMI membrane check: errors", errs[-1], "rates", rates[-1])
    assert rates[-1][0] > 1.8 and errs[-1][0] < 2e-2 and errs[-1][1] < 5e-3, (errs, rates)


def test_vertex_valence_limit_is_reported(hip_lib):
    """Maximum sizes: CSR rows are addressed with one byte per slot (<= 255 entries).  A fan of 300 triangles around
    one vertex exceeds that and must be refused with a message, not assembled wrongly; 200 triangles pass."""
    from knpemi.fem import Mesh, meshtags
    from knpemi import _lib as L

    def fan(n):
        ang = 2 * np.pi * np.arange(n) / n
        x = np.vstack([[0.0, 0.0], np.c_[np.cos(ang), np.sin(ang)] * 1e-6])
        cells = np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], np.int32)
        mesh = Mesh(x, cells, "triangle")
        ct = meshtags(mesh, 2, np.arange(n), np.zeros(n, np.int32))
        ft = meshtags(mesh, 1, np.zeros(0, np.int32), np.zeros(0, np.int32))
        return mesh, ct, ft
    with pytest.raises(L.KnpemiError, match="255"):
        _custom_problem(*fan(300), {1: [(1, "hh_si")]})
    s = _custom_problem(*fan(200), {1: [(1, "hh_si")]})
    errs = _compare_with_oracle(s, {0: [], 1: [1]})
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("kind,r", [("2d", 1), ("tet", 0), ("hex", 0)])
def test_device_krylov_solves_match_direct_solves(hip_lib, kind, r):
    """`direct=False`: Jacobi-PCG (EMI, constant null space) and Jacobi-BiCGStab (KNP) on the device against
    SciPy sparse LU of the same GPU-assembled systems."""
    import scipy.sparse.linalg as spla
    import driver
    from knpemi.pdeSolver import create_solver_emi, create_solver_knp
    s = Setup(kind, r)
    s.perturb()
    s.phi[1].x.array[:] += -0.0744
    for t in s.subdomain_list:
        for k in range(2):
            s.c[t][k].x.array[:] = s.c_prev[t][k].x._a
    emi_d = create_solver_emi(s.a_emi, s.L_emi, s.phi, s.entity_maps, s.subdomain_list, None, direct=True, p=s.p_emi)
    A, b = emi_d.assemble()
    x_ref = driver.solve_singular(A, b)
    emi = create_solver_emi(s.a_emi, s.L_emi, s.phi, s.entity_maps, s.subdomain_list, None, direct=False, p=s.p_emi,
                            rtol=1e-12, atol=1e-40)
    emi.solve()
    x = np.concatenate([s.phi[0].x._a, s.phi[1].x._a])
    assert rel_err(x - x.mean(), x_ref - x_ref.mean()) < 1e-7
    assert 0 < emi.solver.getIterationNumber() <= 1000
    knp_d = create_solver_knp(s.a_knp, s.L_knp, s.c, s.entity_maps, s.subdomain_list, None, direct=True, p=s.p_knp)
    Ak, bk = knp_d.assemble()                      # uses the phi just solved for
    xk_ref = spla.splu(Ak.tocsc()).solve(bk)
    knp = create_solver_knp(s.a_knp, s.L_knp, s.c, s.entity_maps, s.subdomain_list, None, direct=False, p=s.p_knp,
                            rtol=1e-12, atol=1e-40)
    knp.solve()
    xk = np.concatenate([f.x._a for t in s.subdomain_list for f in s.c[t]])
    assert rel_err(xk, xk_ref) < 1e-9
    assert 0 < knp.solver.getIterationNumber() <= 1000
    info = emi.dp.solver_info(L.B_EMI)
    assert info["builds"] == 1 and info["levels"] >= (2 if len(x_ref) > 640 else 1) and info["op_complexity"] < 4
    # Jacobi preconditioning (selectable) reaches the same solutions with more iterations
    its_amg = emi.solver.getIterationNumber()
    emi.dp.solver_setup(L.B_EMI, L.PC_JACOBI)
    emi.dp.solver_setup(L.B_KNP, L.PC_JACOBI)
    for f in (s.phi[0], s.phi[1]):
        f.x.array[:] = 0.0
    emi.rtol = 1e-10
    emi.dp.push(L.F_PHI, 0, 0, s.phi[0])
    its, relres = (emi.dp.push(L.F_PHI, 1, 0, s.phi[1]), emi.dp.solve(L.B_EMI, 1e-10, 1e-40, 20000))[1]
    assert its > its_amg and relres <= 1e-10
    x = emi.dp.get_solution(L.B_EMI, len(x_ref))
    assert rel_err(x - x.mean(), x_ref - x_ref.mean()) < 1e-6
    with pytest.raises(L.KnpemiError):          # ksp_error_if_not_converged
        emi.dp.push(L.F_PHI, 0, 0, s.phi[0])
        emi.dp.solve(L.B_EMI, 1e-14, 1e-40, 3)


def test_device_resident_time_loop_matches_oracle(hip_lib):
    """Ten steps of the 2D problem entirely on the device (DeviceStepper with device Krylov solves, no host
    transfers inside the loop) against the oracle loop with direct solves."""
    import driver
    from knpemi.stepper import DeviceStepper
    s = Setup("2d", 1, g_syn=10.0)
    o, P, params, ions = s.oracle()
    c_all, _, _, _ = s.oracle_fields()
    ode = s.mem_models[0]['ode']
    mask = np.array([x[0] < 20e-6 for x in ode.dof_locations])
    run = driver.OracleRun(P, params, ions, "hh_si", c_all, ode.states.copy(), ode.parameters.copy(),
                           ode.dof_locations, mask, {o.MODELS["hh_si"]["pidx"]["stim_amplitude"]: 10.0},
                           {'z': -1, 0: 0.0, 1: 0.0})
    for t in s.subdomain_list:      # initial guess of the first KNP solve
        for k in range(2):
            s.c[t][k].x.array[:] = s.c_prev[t][k].x._a
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev,
                       device_solves=(1e-12, 1e-13))
    st.add_membrane_model(ode, s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
    for k in range(10):
        st.step()
        run.step()
    st.download()
    assert rel_err(s.phi_M_prev[1].x._a, run.phiM[1]) < 1e-6
    for t in (0, 1):
        for k in range(2):
            assert rel_err(s.c_prev[t][k].x._a, run.c_all[t][k]) < 1e-8
    assert rel_err(ode.states, run.states) < 1e-6
    assert all(it[1] <= 1000 for it in st.iterations)


def test_fused_update_and_overlap_variants_are_bit_identical(hip_lib, monkeypatch):
    """The stepper's launch-saving variants change no bit: update_pde_variables fused into the write-back kernel of the
    KNP solve (KNPEMI_OPT_FUSE_UPDATE) vs the separate launch; the EMI matrix assembled beside the ODE sweep (aux
    stream, separate Robin-term launch) vs after it (fused Robin term); the early part of the membrane-facet integrals
    beside the EMI solve (aux stream) vs in line -- fields, membrane potential, currents and ODE tables after six whole
    steps with the device solves.  The one-part forms of the membrane integrals (stand-alone facet kernel, or inside
    the KNP row kernel: KNPEMI_OPT_FUSE_MEMBRANE) agree with each other and with the two-part form to rounding (other
    summation orders)."""
    from knpemi.stepper import DeviceStepper
    out = []
    variants = ((True, True, 0.025, False, True), (False, True, 0.0, False, True), (False, False, 0.025, False, True),
                (False, False, 0.025, True, False), (True, True, 0.025, False, False))
    for fuse, overlap, thr, fuse_mem, early in variants:
        if fuse_mem:      # the in-row form needs row blocks of consecutive rows (one range of membrane entries per block)
            monkeypatch.setenv("KNPEMI_BLOCK_CLASSIC", "1")
        else:
            monkeypatch.delenv("KNPEMI_BLOCK_CLASSIC", raising=False)
        s = Setup("tet", 0, g_syn=10.0)
        for t in s.subdomain_list:
            for k in range(2):
                s.c[t][k].x.array[:] = s.c_prev[t][k].x._a
        st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi,
                           s.phi_M_prev, device_solves=(1e-9, 1e-10), fuse_update=fuse, overlap=overlap,
                           fuse_membrane=fuse_mem, early_membrane=early)
        st.overlap_threshold_ms = thr
        ode = s.mem_models[0]['ode']
        st.add_membrane_model(ode, s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
        for _ in range(6):
            st.step()
        st.download()
        out.append([s.phi[0].x._a.copy(), s.phi[1].x._a.copy(), s.phi_M_prev[1].x._a.copy(), ode.states.copy(),
                    ode.parameters.copy()] + [f.x._a.copy() for t in (0, 1) for f in s.c_prev[t]]
                   + [s.ion_list[-1][f'c_{t}'].x._a.copy() for t in (0, 1)])
    same = lambda x, y: all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(x, y))
    assert same(out[0], out[1]) and same(out[0], out[2])          # two-part form: fused update / overlap / in line
    for a, b in zip(out[3][2:4] + out[3][5:], out[4][2:4] + out[4][5:]):   # one-part forms: in-row vs facet kernel
        assert rel_err(b, a) < 1e-9                               # (the facet kernel sums its points lane-parallel)
    phi = lambda o: np.concatenate([o[0], o[1]])
    assert rel_err(phi(out[3]) - phi(out[3]).mean(), phi(out[0]) - phi(out[0]).mean()) < 1e-8   # solver tolerance 1e-9
    for a, b in zip(out[0][2:4] + out[0][5:], out[3][2:4] + out[3][5:]):
        assert rel_err(b, a) < 1e-9


def test_stepper_reports_lsoda_failures(hip_lib):
    """`assert success` (odeSolver.py:121) in the device-resident loop: a dof LSODA cannot integrate makes
    `download()` / `check_ode_failures()` raise instead of handing out fields fed by a wrong V / I_ch."""
    from knpemi import _lib as L
    from knpemi.stepper import DeviceStepper
    s = Setup("2d", 1, g_syn=10.0)
    ode = s.mem_models[0]['ode']
    ode.states[7, 3] = np.nan
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev)
    st.add_membrane_model(ode, s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
    st.step()
    with pytest.raises(L.KnpemiError, match="LSODA failed on 1 membrane dof"):
        st.download()


def _load_stim_driver():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "examples", "local_astrocyte_depolarization", "run_stim_duration.py")
    spec = importlib.util.spec_from_file_location("run_stim_duration", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_ecs_source_term_matches_oracle(hip_lib):
    """`ion['f_source']` on the ECS (knpWeakForm.py:164-166): b_knp with a nodal source field against the oracle."""
    import adapters
    from knpemi.fem import Function
    from knpemi.pdeSolver import create_solver_knp
    s = Setup("tet", 0)
    s.perturb()
    V0 = s.c_prev[0][0].function_space
    rng = np.random.default_rng(11)
    src = {}
    for k, ion in enumerate(s.ion_list[:-1]):
        f = Function(V0, name=f"f_source_{ion['name']}")
        f.x.array[:] = 50.0 * rng.uniform(-1, 1, f.x.array.shape[0])
        ion['f_source'] = f
        src[k] = f.x._a.copy()
    o, P, params, ions = adapters.oracle_problem(s)
    c_all, phi, phiM, mm = adapters.oracle_fields(s)
    knp = create_solver_knp(s.a_knp, s.L_knp, s.c, s.entity_maps, s.subdomain_list, None, p=s.p_knp)
    Ak, bk = knp.assemble()
    Ako, bko = o.assemble_knp(P, params, ions, c_all, phi, phiM, mm, s.dt, f_source=src)
    _, bko0 = o.assemble_knp(P, params, ions, c_all, phi, phiM, mm, s.dt)
    assert rel_err(bk, bko) < TOL and csr_rel_err(Ak, Ako) < TOL
    assert rel_err(bko, bko0) > 1e-6          # the source is visible in the right-hand side


def test_stim_duration_driver_device_resident_matches_dropin(hip_lib, tmp_path):
    """The YAML-configured three-sub-domain driver (neuron HH-mV + glia + pulsed ECS source): twelve
    steps through the drop-in API (host arrays authoritative, device Krylov solves) and through the device-resident
    stepper give the same fields; the source switches on and off inside the run and raises ECS K+ in its region."""
    drv = _load_stim_driver()
    cfg = drv.load_config("baseline")
    cfg.update(delay=0.2, period=0.6, pulse_width=0.3, end_time=5.0, save_frequency=1, f_value=97)
    pa, ha = drv.solve_system(dict(cfg), n_steps=12, device_resident=False, outdir=str(tmp_path / "a"), quiet=True)
    pb, hb = drv.solve_system(dict(cfg), n_steps=12, device_resident=True, outdir=str(tmp_path / "b"), quiet=True,
                              xdmf=True, extrapolate_guess=False)       # same initial guesses as the drop-in path
    # with the extrapolated initial guess (the default) the fields agree to the solver tolerance.  The extrapolation pays
    # while the fields move (the firing trajectory of bench.py: 5.3 against 5.85 CG iterations per step); around rest it
    # amplifies the solver-tolerance noise of the previous solutions (3 x_n - 3 x_(n-1) + x_(n-2): up to seven times) and the
    # concentration solves, which then need 0-3 iterations from the previous solution, take a few more: here, with
    # the source switching on and off, 76 + 44 against 80 + 35 iterations over the twelve steps -- never far apart
    pc, hc = drv.solve_system(dict(cfg), n_steps=12, device_resident=True, outdir=str(tmp_path / "c"), quiet=True)
    for tag in (0, 1, 2):
        for k in range(2):
            assert rel_err(pc.c_prev[tag][k].x._a, pa.c_prev[tag][k].x._a) < 1e-5
    assert sum(hc["its_emi"]) <= sum(hb["its_emi"])
    assert sum(hc["its_emi"]) + sum(hc["its_knp"]) <= 1.15 * (sum(hb["its_emi"]) + sum(hb["its_knp"]))
    assert ha["source"] == hb["source"] and 0.0 in ha["source"] and 97.0 in ha["source"]
    for tag in (0, 1, 2):
        assert rel_err(pb.phi[tag].x._a - pb.phi[tag].x._a.mean() * 0, pa.phi[tag].x._a) < 1e-5
        for k in range(2):
            assert rel_err(pb.c_prev[tag][k].x._a, pa.c_prev[tag][k].x._a) < 1e-8
    for tag in (1, 2):
        assert rel_err(pb.phi_M_prev[tag].x._a, pa.phi_M_prev[tag].x._a) < 1e-6
    # potassium accumulates where it is injected
    K0 = drv.INIT["K"][0]
    K = pa.c_prev[0][0].x._a
    assert K[pa.region].mean() > K0 + 1.0 and abs(K[~pa.region].min() - K0) < 1.0
    assert os.path.exists(tmp_path / "a" / "step_000011.npz") and os.path.exists(tmp_path / "b" / "step_000011.npz")
    # the XDMF time series holds the last saved membrane potential of the glial cell
    from knpemi.fem import hdf5
    with hdf5.File(str(tmp_path / "b" / "results_mem_2.h5"), "r") as h5:
        assert np.array_equal(h5.read("/Function/phi_M_2/11").ravel(), pb.phi_M_prev[2].x._a)
    assert all(0 <= i <= 1000 for i in ha["its_emi"] + ha["its_knp"] + hb["its_emi"] + hb["its_knp"])


@pytest.mark.parametrize("kind,r,label", [("tet", 1, "config 2: 124 416 tetrahedra"),
                                          ("hex", 2, "config 2h: 165 888 hexahedra"),
                                          ("tet", 2, "config 3 mesh: 995 328 tetrahedra")])
def test_full_size_properties(hip_lib, kind, r, label):
    """BASELINE-size meshes, checked through properties that need no oracle: sorted CSR rows,
    symmetry and constant null space of A_emi, P = A on the ECS rows, zero-sum
    membrane right-hand side, A_knp row sums = volume / dt at constant phi, linearity of A_emi in the concentrations,
    identical bits on re-assembly, and an ODE sweep whose equal inputs give equal outputs."""
    import hashlib
    from knpemi import update_ode_variables
    from knpemi.pdeSolver import create_solver_emi, create_solver_knp
    s = Setup(kind, r, g_syn=10.0)
    n0 = s.phi[0].x.array.shape[0]
    dt = s.dt
    emi = create_solver_emi(s.a_emi, s.L_emi, s.phi, s.entity_maps, s.subdomain_list, None, p=s.p_emi, direct=False)
    knp = create_solver_knp(s.a_knp, s.L_knp, s.c, s.entity_maps, s.subdomain_list, None, p=s.p_knp)
    # uniform concentrations (the initial state), constant potentials
    s.phi[0].x.array[:] = 0.0
    s.phi[1].x.array[:] = -0.0744
    s.phi_M_prev[1].x.array[:] = -0.0744
    A, b = emi.assemble()
    P = emi.P
    Ak, bk = knp.assemble()
    n = A.shape[0]
    scale = np.abs(A.data).max()
    # structure
    assert np.all(np.diff(A.indptr) > 0) and all(np.all(np.diff(A.indices[A.indptr[i]:A.indptr[i + 1]]) > 0)
                                                  for i in range(0, n, max(1, n // 2000)))
    # symmetry and the constant null space (pdeSolver.py:74-78)
    assert csr_rel_err(A, A.T.tocsr()) < 1e-13
    assert np.abs(A @ np.ones(n)).max() < 1e-11 * scale
    # P = A bit for bit on the ECS rows (on the cell rows P - A is the ICS mass, which in SI units sits at the
    # rounding level of A, ~1e-23 against ~1e-7, and cannot be recovered from the difference)
    M = (P - A).tocsr()
    assert M[:n0].nnz == 0 or np.abs(M[:n0].data).max() == 0.0
    # uniform concentrations: the volume part of b_emi vanishes, the membrane part (C_phi phi_M on both sides of every
    # facet with opposite signs) is there and sums to zero
    area = 4 * (4 * 22e-6 * 0.2e-6 + 2 * 0.2e-6 * 0.2e-6)
    assert abs(np.abs(b).sum() - 2 * (0.02 / dt) * 0.0744 * area) < 1e-9 * np.abs(b).sum()
    assert abs(b.sum()) < 1e-9 * np.abs(b).sum()
    # A_knp 1 at constant phi = lumped mass / dt: per ion the volume of the whole box
    vol = 32e-6 * 0.9e-6 * 0.9e-6
    rs = Ak @ np.ones(Ak.shape[0])
    assert abs(rs.sum() - 2 * vol / dt) < 1e-9 * (2 * vol / dt)
    # identical bits on re-assembly (checksum of checksums)
    def digest(*arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest())
        return h.hexdigest()
    d1 = digest(A.data, P.data, b, Ak.data, bk)
    A2, b2 = emi.assemble()
    Ak2, bk2 = knp.assemble()
    assert digest(A2.data, emi.P.data, b2, Ak2.data, bk2) == d1
    # linearity of A_emi in the concentrations: second difference of A(c), A(2c), A(3c) vanishes
    base = {(t, k): s.c_prev[t][k].x._a.copy() for t in s.subdomain_list for k in range(2)}
    elim = {t: s.ion_list[-1][f'c_{t}'].x._a.copy() for t in s.subdomain_list}
    mats = []
    for f in (1.0, 2.0, 3.0):
        for (t, k), v in base.items():
            s.c_prev[t][k].x.array[:] = f * v
        for t, v in elim.items():
            s.ion_list[-1][f'c_{t}'].x.array[:] = f * v
        mats.append(emi.assemble()[0].copy())
    assert np.abs(mats[2].data - 2.0 * mats[1].data + mats[0].data).max() < 1e-12 * np.abs(mats[2].data).max()
    for (t, k), v in base.items():
        s.c_prev[t][k].x.array[:] = v
    for t, v in elim.items():
        s.ion_list[-1][f'c_{t}'].x.array[:] = v
    # ODE sweep at full size: dofs with equal inputs (same stimulus flag, uniform traces) end in equal states
    ode = s.mem_models[0]['ode']
    s.phi_M_prev[1].x.array[:] = -0.0744
    for k in range(2):
        update_ode_variables(ode, s.c_prev, s.phi_M_prev[1], s.ion_list, s.subdomain_list, s.mesh, s.ct, 1, k)
        ode.step_lsoda(dt, s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
    stim = np.fromiter(map(s.stim_params['stimulus_locator'], ode.dof_locations), dtype=bool)
    for sel in (stim, ~stim):
        assert sel.any() and np.all(ode.states[sel] == ode.states[sel][0])
    assert not np.array_equal(ode.states[stim][0], ode.states[~stim][0])
    assert ode.last_stats["n_failed"] == 0


@pytest.mark.parametrize("kind,r,label", [("tet", 1, "config 2: 124 416 tetrahedra"),
                                          ("hex", 1, "hexahedral box r = 1: 20 736 hexahedra"),
                                          ("hex", 2, "config 2h: 165 888 hexahedra"),
                                          ("tet", 2, "config 3 mesh: 995 328 tetrahedra")])
def test_full_size_assembly_matches_oracle(hip_lib, kind, r, label):
    """The oracle on the BASELINE-size meshes (round-3 review: they were only property-checked, so the paths that only
    large meshes exercise -- the greedy chunk clustering with its tail cut, multi-slice pair lists, five row blocks per CU,
    the XCD remap -- had never met the oracle).  All five assembled objects (A_emi, P_emi, b_emi, A_knp, b_knp) of a
    perturbed state at 1e-10: with the splitting scheme against the numpy oracle (oracle/knpemi_oracle.py, FFCx-style
    quadrature + COO scatter), without it against the C++ port (oracle/knpemi_cpu.cpp, itself pinned to the numpy oracle
    by tests/test_cpu_port.py; its CSR patterns are the numpy oracle's) -- and the port against the numpy oracle on the
    way.  Forms: /root/reference/src/knpemi/emiWeakForm.py:138-241, knpWeakForm.py:123-216."""
    import scipy.sparse as sp
    import cpu_port
    from knpemi.pdeSolver import create_solver_emi, create_solver_knp
    s = Setup(kind, r)
    s.perturb()
    o, P, params, ions = s.oracle()
    c_all, phi, phiM, mm = s.oracle_fields()
    emi = create_solver_emi(s.a_emi, s.L_emi, s.phi, s.entity_maps, s.subdomain_list, None, p=s.p_emi, direct=False)
    knp = create_solver_knp(s.a_knp, s.L_knp, s.c, s.entity_maps, s.subdomain_list, None, p=s.p_knp)

    def device(splitting):
        for f in (s.a_emi, s.a_knp):
            f.shared['splitting_scheme'] = splitting
        A, b = emi.assemble()
        Ak, bk = knp.assemble()
        return A.copy(), emi.P.copy(), b.copy(), Ak.copy(), bk.copy()
    # -- with the splitting scheme: the numpy oracle
    A, Pm, b, Ak, bk = device(True)
    Ao, Po, bo = o.assemble_emi(P, params, ions, c_all, phiM, mm, splitting_scheme=True)
    Ako, bko = o.assemble_knp(P, params, ions, c_all, phi, phiM, mm, s.dt, splitting_scheme=True)
    errs = dict(A_emi=csr_rel_err(A, Ao), P_emi=csr_rel_err(Pm, Po), b_emi=rel_err(b, bo),
                A_knp=csr_rel_err(Ak, Ako), b_knp=rel_err(bk, bko))
    assert max(errs.values()) < TOL, (label, errs)
    # the patterns agree entry for entry (no structural zero on either side hides a missing contribution)
    Ao, Ako = Ao.tocsr(), Ako.tocsr()
    Ao.sort_indices()
    Ako.sort_indices()
    assert np.array_equal(A.indptr, Ao.indptr) and np.array_equal(A.indices, Ao.indices), label
    assert np.array_equal(Ak.indptr, Ako.indptr) and np.array_equal(Ak.indices, Ako.indices), label
    # -- the C++ port on the same state (the timed CPU baseline of bench.py): against the numpy oracle, then, without the
    # splitting scheme, as the checker of the device
    port = cpu_port.CpuPort(P, params, ions, Ao, Ako)
    Ich = np.stack([mm[1][0]["I_ch_k"][n] for n in ("K", "Cl", "Na")])
    a, pp, bb = port.assemble_emi(c_all, phiM, Ich, True)
    ak, bbk = port.assemble_knp(c_all, phi, phiM, Ich, True)
    assert rel_err(a, Ao.data) < 1e-12 and rel_err(bb, bo) < 1e-12 and rel_err(ak, Ako.data) < 1e-12 and rel_err(bbk, bko) < 1e-12
    A, Pm, b, Ak, bk = device(False)
    a, pp, bb = (x.copy() for x in port.assemble_emi(c_all, phiM, Ich, False))
    ak, bbk = (x.copy() for x in port.assemble_knp(c_all, phi, phiM, Ich, False))
    shape = Ao.shape
    errs = dict(A_emi=csr_rel_err(A, sp.csr_matrix((a, port.ci, port.rp), shape=shape)),
                P_emi=csr_rel_err(Pm, sp.csr_matrix((pp, port.ci, port.rp), shape=shape)), b_emi=rel_err(b, bb),
                A_knp=csr_rel_err(Ak, sp.csr_matrix((ak, port.kci, port.krp), shape=Ako.shape)), b_knp=rel_err(bk, bbk))
    assert max(errs.values()) < TOL, (label, "no splitting", errs)
    assert np.abs(b - bo).max() > 0 and np.abs(bk - bko).max() > 0      # the flag does change both right-hand sides


@pytest.mark.parametrize("workload,n_cells,n_steps", [("config5s", 995328, 6), ("config5s_r3", 7962624, 3)])
def test_config5_synthetic_full_size(hip_lib, workload, n_cells, n_steps):
    """BASELINE configs[4] stand-in at ~1e6 tetrahedra and at its stated size (`config5s_r3`: 7.96 M tetrahedra, 1.37 M
    vertices, 47 k membrane dofs; the reference-side anchor is
    /root/reference/examples/local_astrocyte_depolarization/run_stim_duration.py:150-211) (bench.py `config5s`: ECS + neuron cells 1,3 with the HH mV/ms
    model + glial cells 2,4 with the Kir4.1/pump model, pulsed ECS K+ source): properties that need no oracle --
    structure, symmetry and null space of A_emi, P = A on the ECS rows, A_knp row sums = volume / dt, identical bits on
    re-assembly, both ODE sweeps giving equal outputs for equal inputs -- and six whole device-resident time steps
    (device Krylov solves) during which the source raises K+ in its box, the glial membrane there depolarises, no
    concentration leaves its physical range and LSODA fails nowhere."""
    import hashlib
    import bench
    from knpemi import _lib as L
    from knpemi.pdeSolver import create_solver_emi, create_solver_knp
    from knpemi.stepper import DeviceStepper
    case = bench.Case(workload)
    p = case.s
    assert len(p.subdomain_list) == 3 and len(case.models) == 2
    assert sum(sd["mesh_sub"].num_cells for sd in p.subdomain_list.values()) == n_cells
    emi = create_solver_emi(p.a_emi, p.L_emi, p.phi, p.entity_maps, p.subdomain_list, None, p=p.p_emi, direct=False)
    knp = create_solver_knp(p.a_knp, p.L_knp, p.c, p.entity_maps, p.subdomain_list, None, p=p.p_knp)
    A, b = emi.assemble()
    P = emi.P
    Ak, bk = knp.assemble()
    n, n0 = A.shape[0], p.phi[0].x.array.shape[0]
    scale = np.abs(A.data).max()
    assert csr_rel_err(A, A.T.tocsr()) < 1e-13
    assert np.abs(A @ np.ones(n)).max() < 1e-11 * scale
    M = (P - A).tocsr()
    assert M[:n0].nnz == 0 or np.abs(M[:n0].data).max() == 0.0
    # P - A on the cell rows is the mass matrix of the two cellular sub-domains: its entries sum to their volume
    # (recovered from a difference of much larger numbers, hence only to ~1e-4)
    vol_cells = 4 * (22e-4 * 0.2e-4 * 0.2e-4)
    assert abs(M.sum() - vol_cells) < 1e-3 * vol_cells
    vol = 32e-4 * 0.9e-4 * 0.9e-4      # cm^3: every sub-domain's two ion blocks have row sums = lumped mass / dt
    rs = Ak @ np.ones(Ak.shape[0])
    assert abs(rs.sum() - 2 * vol / p.dt) < 1e-9 * (2 * vol / p.dt)

    def digest(*arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest())
        return h.hexdigest()
    d1 = digest(A.data, P.data, b, Ak.data, bk)
    A2, b2 = emi.assemble()
    Ak2, bk2 = knp.assemble()
    assert digest(A2.data, emi.P.data, b2, Ak2.data, bk2) == d1
    # equal inputs -> equal outputs, bit for bit, for both membrane models (uniform initial fields, no stimulus)
    from knpemi import update_ode_variables
    for (m, stim, loc), t in zip(case.models, (1, 2)):
        st0, pa0, t0 = m.states.copy(), m.parameters.copy(), m.time
        update_ode_variables(m, p.c_prev, p.phi_M_prev[t], p.ion_list, p.subdomain_list, p.mesh, p.ct, t, 0)
        m.step_lsoda(p.dt, stim, loc)
        assert m.last_stats["n_failed"] == 0 and m.last_stats["n_rhs"] > 2 * m.nodes
        assert np.all(m.states == m.states[0]) and not np.array_equal(m.states[0], st0[0])
        m.states[:], m.parameters[:], m.time = st0, pa0, t0
    # whole time steps on the device
    st = DeviceStepper((p.a_emi, p.p_emi, p.L_emi), (p.a_knp, p.p_knp, p.L_knp), p.c, p.c_prev, p.phi, p.phi_M_prev,
                       device_solves=case.solver_rtol)
    for m, stim, loc in case.models:
        st.add_membrane_model(m, stim, loc)
    st.set_source(0, case.source)
    k0 = p.c_prev[0][0].x._a.copy()
    vm0 = {t: p.phi_M_prev[t].x._a.copy() for t in (1, 2)}
    for _ in range(n_steps):
        st.step()
    st.download()           # raises if LSODA failed anywhere
    assert all(it[1] < 200 for it in st.iterations)
    k1 = p.c_prev[0][0].x._a
    inside = p.region
    assert inside.sum() > 10 and (k1[inside] - k0[inside]).min() > n_steps / 6.0    # mM; 0.6 ms of a 97 mM/ms source in 6 steps
    far = p.subdomain_list[0]["mesh_sub"].x[:, 0] < 4e-4
    assert np.abs(k1[far] - k0[far]).max() < 0.5
    for t in p.subdomain_list:
        for f in p.c_prev[t] + [p.ion_list[-1][f"c_{t}"]]:
            assert f.x._a.min() > 0.0 and np.all(np.isfinite(f.x._a))
    # glia near the source depolarises (K+ rises outside it), every membrane potential stays in a physical range
    xg = p.subdomain_list[2]["mesh_mem"].x
    near = np.abs(xg[:, 0] - 16e-4) < 2e-4
    dv = p.phi_M_prev[2].x._a - case.models[1][0].ode.init_state_values()[0]
    # (the whole glial membrane relaxes by ~0.5 mV from its tabulated initial state; the source adds to that locally)
    assert near.any() and dv[near].max() > dv[xg[:, 0] < 8e-4].max() + (0.2 if n_steps >= 6 else 0.0)
    for t in (1, 2):
        v = p.phi_M_prev[t].x._a
        assert -120.0 < v.min() and v.max() < 60.0


@pytest.mark.parametrize("kind,r", [("2d", 1), ("tet", 0), ("hex", 0)])
@pytest.mark.parametrize("n_ions", [2, 4])
def test_ion_counts_other_than_three_match_oracle(hip_lib, kind, r, n_ions):
    """The forms loop over an arbitrary `ion_list` (knpWeakForm.py:92,131, emiWeakForm.py:97); every reference driver
    uses three species.  K = 2 (one solved + one eliminated) and K = 4 (three solved, one of them divalent): operators,
    right-hand sides in both splitting modes, and the end-of-step update (eliminated ion from electroneutrality)
    against the oracle, which is generic in K."""
    from helpers import ion_count_problem, make_mesh
    from knpemi import update_pde_variables
    from knpemi.pdeSolver import create_solver_emi, create_solver_knp
    mesh_data = make_mesh(kind, r)
    for splitting in (True, False):
        s = ion_count_problem(mesh_data, n_ions, splitting)
        mesh, ct, subs, ions, pp, rho, dt = s.mesh, s.ct, s.subdomain_list, s.ion_list, s.physical_parameters, s.rho, s.dt
        phi, phi_M_prev, c, c_prev = s.phi, s.phi_M_prev, s.c, s.c_prev
        o, P, params, oions = s.oracle
        c_all, ophi, phiM, mm = s.oracle_fields
        emi = create_solver_emi(s.a_emi, s.L_emi, phi, [], subs, None, p=s.p_emi, direct=False)
        knp = create_solver_knp(s.a_knp, s.L_knp, c, [], subs, None, p=s.p_knp)
        A, b = emi.assemble()
        Ak, bk = knp.assemble()
        Ao, Po, bo = o.assemble_emi(P, params, oions, c_all, phiM, mm, splitting_scheme=splitting)
        Ako, bko = o.assemble_knp(P, params, oions, c_all, ophi, phiM, mm, dt, splitting_scheme=splitting)
        errs = dict(A_emi=csr_rel_err(A, Ao), P_emi=csr_rel_err(emi.P, Po), b_emi=rel_err(b, bo),
                    A_knp=csr_rel_err(Ak, Ako), b_knp=rel_err(bk, bko))
        assert Ak.shape[0] == (n_ions - 1) * A.shape[0]
        assert max(errs.values()) < 1e-10, (n_ions, splitting, errs)
        # end-of-step update: c_prev <- c, eliminated ion from electroneutrality with the background charge
        cnew = {t: [f.x._a.copy() for f in c[t]] for t in (0, 1)}
        update_pde_variables(c, c_prev, phi, phi_M_prev, pp, ions, subs, mesh, ct)
        zs = [i['z'] for i in ions]
        for t in (0, 1):
            for k in range(n_ions - 1):
                assert np.array_equal(c_prev[t][k].x._a, cnew[t][k])
            el = -(1.0 / zs[-1]) * (-1 * float(rho[t]) + sum(z * ck for z, ck in zip(zs[:-1], cnew[t])))
            assert rel_err(ions[-1][f'c_{t}'].x._a, el) < 1e-14


@pytest.mark.parametrize("r", [0, 1])
def test_lattice_tetrahedra_agree_with_the_general_tetrahedron_kernels(hip_lib, r, monkeypatch):
    """The box meshes of the reference's 3-D driver split into tetrahedra (make_mesh_3D.py:100-102): knpemi_create finds every
    cell to be a lattice tetrahedron of the uniform grid and the row kernels take gradient dot products and volumes from the
    shape table instead of staging coordinates (kernels_assemble.hip: tet_table_row0); KNPEMI_TET_NOT_UNIFORM=1 keeps the
    general kernels.  Both against the numpy oracle at 1e-10 and against each other to rounding, all five assembled objects,
    both splitting modes; the lattice path must actually have been taken (six shapes of the Kuhn split)."""
    from knpemi.pdeSolver import create_solver_emi, create_solver_knp
    out = {}
    for name in ("lattice", "general"):
        if name == "general":
            monkeypatch.setenv("KNPEMI_TET_NOT_UNIFORM", "1")
        else:
            monkeypatch.delenv("KNPEMI_TET_NOT_UNIFORM", raising=False)
        s = Setup("tet", r)
        s.perturb()
        emi = create_solver_emi(s.a_emi, s.L_emi, s.phi, s.entity_maps, s.subdomain_list, None, p=s.p_emi, direct=False)
        knp = create_solver_knp(s.a_knp, s.L_knp, s.c, s.entity_maps, s.subdomain_list, None, p=s.p_knp)
        o, P, params, ions = s.oracle()
        c_all, phi, phiM, mm = s.oracle_fields()
        for splitting in (True, False):
            for f in (s.a_emi, s.a_knp):
                f.shared['splitting_scheme'] = splitting
            A, b = emi.assemble()
            Ak, bk = knp.assemble()
            got = (A.copy(), emi.P.copy(), b.copy(), Ak.copy(), bk.copy())
            Ao, Po, bo = o.assemble_emi(P, params, ions, c_all, phiM, mm, splitting_scheme=splitting)
            Ako, bko = o.assemble_knp(P, params, ions, c_all, phi, phiM, mm, s.dt, splitting_scheme=splitting)
            errs = dict(A_emi=csr_rel_err(got[0], Ao), P_emi=csr_rel_err(got[1], Po), b_emi=rel_err(got[2], bo),
                        A_knp=csr_rel_err(got[3], Ako), b_knp=rel_err(got[4], bko))
            assert max(errs.values()) < TOL, (name, splitting, errs)
            out[name, splitting] = got
        import ctypes
        flags = ctypes.c_int(-1)
        L.check(emi.dp.lib.knpemi_debug_geometry(emi.dp.h, ctypes.byref(flags)))
        assert bool(flags.value & 1) == (name == "lattice"), (name, flags.value)
    for splitting in (True, False):
        for a, b in zip(out["lattice", splitting], out["general", splitting]):
            da, db = (a.data, b.data) if hasattr(a, "data") and hasattr(a, "indptr") else (a, b)
            assert np.abs(da - db).max() <= 1e-12 * np.abs(db).max()


def test_iteration_counts_on_the_hexahedral_box_stay_within_bounds(hip_lib):
    """Whole steps with the device solves on the hexahedral box at r = 1 (20 736 cells, stretched cells: 1.0 x 0.05 x 0.05 um
    -- the aggregation rule `aggregate_apart` of csrc/amg_host.h exists for them): the CG / BiCGStab iteration counts at the
    reference's tolerances (run_3D.py:296-305: 1e-5 / 1e-7) stay where round 4 measured them (config 2h: 7.4 + 2.9 per step;
    r = 1: ~6 + ~2.5), so that a regression of the aggregation or of the smoothing shows as a count, not only as a time.
    Solutions are checked by the residual of the reference's convergence test itself (KNPEMI_ESOLVE otherwise)."""
    from knpemi.stepper import DeviceStepper
    s = Setup("hex", 1, g_syn=10.0)
    for t in s.subdomain_list:
        for k in range(2):
            s.c[t][k].x.array[:] = s.c_prev[t][k].x._a
    ode = s.mem_models[0]['ode']
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev,
                       device_solves=(1e-5, 1e-7), knp_method="bicgstab")
    st.add_membrane_model(ode, s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
    for k in range(12):
        st.step()
    st.download()
    emi = [it[1] for it in st.iterations if it[0] == "emi"][2:]       # (the first solves start from the initial state)
    knp = [it[1] for it in st.iterations if it[0] == "knp"][2:]
    assert len(emi) == 10 and len(knp) == 10
    assert np.mean(emi) <= 10.0 and max(emi) <= 16, emi
    assert np.mean(knp) <= 4.0 and max(knp) <= 6, knp
    assert np.isfinite(s.phi_M_prev[1].x._a).all()
