"""The fixed-step membrane integrators (euler, rk4, rush_larsen: csrc/kernels_ode_fixed.hip) on the MI355X: against the
host build of the same header, run to run, on plug-in models, in coupled runs against LSODA, in the three-sub-domain
driver, and their failure report."""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np
import pytest

import fixed_step_host as fsh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "calibrate_initial_conditions"))
import run_calibration as rc  # noqa: E402

METHODS = ["euler", "rk4", "rush_larsen"]
SHIPPED = ["hh_si", "hh_mv", "glial"]
TOL = 1e-9     # device against host trajectories, as test_ode_standalone_gpu.py / test_gpu_parity.py (another exp)


def _membrane(name, n_cells=150):
    """Model `name` with its driver's parameters, V spread from node to node (151 dofs: two full waves and a part)."""
    module = rc.load_model(name)
    params, dt = rc.conditions(name)
    m = rc.make_membrane(module, n_cells, params)
    v = module.state_indices("V")
    m.states[:, v] += np.linspace(-2.0, 2.0, m.nodes) * (1e-3 if name == "hh_si" else 1.0)
    return module, m, dt


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHIPPED)
@pytest.mark.parametrize("method", METHODS)
def test_standalone_sweeps_match_the_host_build(hip_lib, method, name, monkeypatch):
    """knpemi_ode_create handles, n = 25: ten single launches == one advance of ten (bit for bit, also the records and
    counters) == a second run (bit for bit); states and currents against the host build of fixed_step.h to 1e-9."""
    monkeypatch.setenv("KNPEMI_ODE_ADVANCE_CHUNK", "4")      # launches of 4, 4, 2 steps
    module, a, dt = _membrane(name)
    _, b, _ = _membrane(name)
    _, c, _ = _membrane(name)
    stim = {"stim_amplitude": 10.0 if name == "hh_si" else 1.0}
    loc = lambda x: x[0] < 0.45          # noqa: E731
    mask = np.array([loc(x) for x in a.dof_locations])
    ref_y, ref_p = a.states.copy(), a.parameters.copy()
    for m in (a, b, c):
        m.set_integrator(method, 25)
    names = rc.state_names(module)
    sidx = {module.parameter_indices(k): v for k, v in stim.items()}
    n_rhs = 0
    traj = []
    for k in range(10):
        a.step(dt, stim, loc)
        c.step(dt, stim, loc)
        n_rhs += a.last_stats["n_rhs"]
        assert a.last_stats["n_steps"] == 25 * a.nodes and a.last_stats["n_failed"] == 0
        assert a.last_stats["n_rhs"] == ((100 if method == "rk4" else 25) + 1) * a.nodes
        traj.append(a.states.copy())
        assert fsh.sweep(name, method, ref_y, ref_p, k * dt, dt, 25, mask, sidx) == 0
        err_y, err_p = _rel(a.states, ref_y), _rel(a.parameters, ref_p)
        print(f"{name} {method} step {k}: states {err_y:.2e}, parameter rows {err_p:.2e} against the host build")
        assert err_y <= TOL and err_p <= TOL
    assert np.array_equal(a.states, c.states) and np.array_equal(a.parameters, c.parameters)
    hist = b.advance(dt, 10, stimulus=stim, stimulus_locator=loc, record=names, every=2)
    assert np.array_equal(a.states, b.states) and np.array_equal(a.parameters, b.parameters)
    assert a.time == b.time
    assert (b.last_stats["n_rhs"], b.last_stats["n_steps"], b.last_stats["n_failed"]) == (n_rhs, 250 * a.nodes, 0)
    for s in names:
        want = np.array([traj[2 * r + 1][:, module.state_indices(s)] for r in range(5)])
        assert np.array_equal(hist[s], want), s
    if name == "glial" and method == "rush_larsen":      # no gates: the Euler code
        _, e, _ = _membrane(name)
        e.set_integrator("euler", 25)
        e.advance(dt, 10, stimulus=stim, stimulus_locator=loc)
        assert np.array_equal(e.states, a.states) and np.array_equal(e.parameters, a.parameters)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHIPPED)
@pytest.mark.parametrize("method", METHODS)
def test_pde_bound_sweep_matches_the_host_build(hip_lib, method, name):
    """A PDE problem, SET_TRACES | SET_V and a stimulus mask: the trace columns against the oracle's traces, states /
    phi_M / I_ch fields against the host build from the same inputs (1e-9), a second run bit for bit."""
    from helpers import Setup
    from knpemi import _lib as L
    from knpemi.utils import update_ode_variables
    import knpemi_oracle as o
    out = []
    for run in range(2):
        s = Setup("2d", 1, model=name)
        s.perturb()
        ode = s.mem_models[0]['ode']
        mod = ode.ode
        v_ix = ode.V_index
        dt = s.dt if name == "hh_si" else 0.1
        ode.set_integrator(method, 25)
        v_in = ode.states[:, v_ix] * (1.0 + 0.01 * np.linspace(-1.0, 1.0, ode.nodes))
        s.phi_M_prev[1].x.array[:] = v_in
        st0, p0 = ode.states.copy(), ode.parameters.copy()
        update_ode_variables(ode, s.c_prev, s.phi_M_prev[1], s.ion_list, s.subdomain_list, s.mesh, s.ct, 1, 1)
        assert ode._pending_flags == L.ODE_SET_TRACES | L.ODE_SET_V
        stim = {"stim_amplitude": 10.0 if name == "hh_si" else 1.0}
        loc = s.stim_params['stimulus_locator']
        ode.step(dt, stim, loc)
        assert ode.last_stats["n_failed"] == 0
        dp, sub = ode._dp, ode._sub
        phi_m = dp.pull_array(L.F_PHI_M, sub, 0, ode.nodes)
        ich = [dp.pull_array(L.F_I_CH, sub, k, ode.nodes) for k in range(len(s.ion_list))]
        out.append((ode.states.copy(), ode.parameters.copy(), phi_m, ich))
        if run:
            continue
        # host reference from the same inputs
        _, P, _, _ = s.oracle()
        c_all, _, _, _ = s.oracle_fields()
        ref_y, ref_p = st0.copy(), p0.copy()
        for k, ion in enumerate(s.ion_list):
            te, ti = P.trace(1, c_all[0][k], c_all[1][k])
            ref_p[:, mod.parameter_indices(f"{ion['name']}_e")] = te
            ref_p[:, mod.parameter_indices(f"{ion['name']}_i")] = ti
        ref_y[:, v_ix] = v_in
        mask = np.array([bool(loc(x)) for x in ode.dof_locations])
        assert 0 < mask.sum() < ode.nodes
        assert fsh.sweep(name, method, ref_y, ref_p, 0.0, dt, 25, mask,
                         {mod.parameter_indices(k): v for k, v in stim.items()}) == 0
        err = dict(states=_rel(ode.states, ref_y), params=_rel(ode.parameters, ref_p),
                   phi_M=_rel(phi_m, ref_y[:, v_ix]))
        for k, ion in enumerate(s.ion_list):
            col = ref_p[:, mod.parameter_indices(f"I_ch_{ion['name']}")]
            err[f"I_ch_{ion['name']}"] = np.abs(ich[k] - col).max() / max(np.abs(ref_p[:, o._ich_slice(ref_p.shape[1])]).max(), 1e-300)
            assert np.array_equal(ich[k], ode.parameters[:, mod.parameter_indices(f"I_ch_{ion['name']}")])
        print(f"{name} {method}: against the host build {err}")
        assert max(err.values()) <= TOL, err
        assert np.array_equal(phi_m, ode.states[:, v_ix])
    for x, y in zip(out[0][:3], out[1][:3]):
        assert np.array_equal(x, y)
    for x, y in zip(out[0][3], out[1][3]):
        assert np.array_equal(x, y)


@pytest.mark.gpu
def test_method_entry_points_on_a_device_handle(hip_lib):
    import ctypes as C
    from knpemi import _lib as L
    _, m, dt = _membrane("hh_mv", 10)
    dp = m._device()
    meth, n = C.c_int(-1), C.c_int(-1)
    L.check(hip_lib.knpemi_ode_get_method(dp.h, 1, 0, C.byref(meth), C.byref(n)))
    assert (meth.value, n.value) == (L.ODE_LSODA, 0)
    for bad in (0, 10001, -1):
        assert hip_lib.knpemi_ode_set_method(dp.h, 1, 0, L.ODE_EULER, bad) == L.EINVAL
        assert b"1..10000" in hip_lib.knpemi_last_error()
    assert hip_lib.knpemi_ode_set_method(dp.h, 1, 0, 4, 25) == L.EINVAL
    assert hip_lib.knpemi_ode_set_method(dp.h, 1, 1, L.ODE_EULER, 25) == L.EINVAL     # no such model
    L.check(hip_lib.knpemi_ode_get_method(dp.h, 1, 0, C.byref(meth), C.byref(n)))
    assert (meth.value, n.value) == (L.ODE_LSODA, 0)
    L.check(hip_lib.knpemi_ode_set_method(dp.h, 1, 0, L.ODE_RUSH_LARSEN, 10000))
    L.check(hip_lib.knpemi_ode_get_method(dp.h, 1, 0, C.byref(meth), C.byref(n)))
    assert (meth.value, n.value) == (L.ODE_RUSH_LARSEN, 10000)
    # step_lsoda never switches methods silently; rtol / atol are ignored by a fixed-step method
    m.set_integrator("euler", 5)
    with pytest.raises(RuntimeError, match=r"call step\(\)"):
        m.step_lsoda(dt, None)
    m.rtol = m.atol = 0.0
    m.step(dt, None)
    m.set_integrator("lsoda")
    m.rtol, m.atol = 1e-8, 1e-10
    m.step_lsoda(dt, None)
    assert m.last_stats["n_failed"] == 0


@pytest.mark.gpu
def test_plugin_model_runs_euler_and_rk4_and_refuses_rush_larsen(hip_lib):
    """HH written as plug-in source (test_rtc_models.py) against the shipped ModelHHSI it restates, at that file's
    tolerances (states 1e-10, currents 1e-5); rush_larsen needs gate rates a plug-in does not bring."""
    from knpemi import _lib as L
    from knpemi.odeSolver import MembraneModel
    from test_rtc_models import HH_SI_SOURCE
    module, shipped, dt = _membrane("hh_si", 70)

    class _Plug:
        __name__ = "mm_hh_user"
        RHS_HIP = HH_SI_SOURCE
        init_state_values = staticmethod(module.init_state_values)
        init_parameter_values = staticmethod(module.init_parameter_values)
        state_indices = staticmethod(module.state_indices)
        parameter_indices = staticmethod(module.parameter_indices)

    class _Q:
        def tabulate_dof_coordinates(self):
            return shipped.dof_locations
    stim = {"stim_amplitude": 10.0}
    for method in ("euler", "rk4"):
        ref = _membrane("hh_si", 70)[1]
        user = MembraneModel(_Plug, None, 1, _Q())
        user.states[:], user.parameters[:] = ref.states, ref.parameters
        user2 = MembraneModel(_Plug, None, 1, _Q())
        user2.states[:], user2.parameters[:] = ref.states, ref.parameters
        for m in (ref, user, user2):
            m.set_integrator(method, 25)
        for _ in range(5):
            ref.step(dt, stim)
            user.step(dt, stim)
        user2.advance(dt, 5, stimulus=stim)
        assert user.last_stats["n_failed"] == 0 and user.last_stats["n_rhs"] == ref.last_stats["n_rhs"]
        assert np.array_equal(user.states, user2.states) and np.array_equal(user.parameters, user2.parameters)
        assert np.abs(user.states - ref.states).max() <= 1e-10 * np.abs(ref.states).max()
        cur = slice(15, 18)
        assert np.abs(user.parameters[:, cur] - ref.parameters[:, cur]).max() <= 1e-5 * np.abs(ref.parameters[:, cur]).max()
        assert not np.array_equal(ref.states, _membrane("hh_si", 70)[1].states)
    user = MembraneModel(_Plug, None, 1, _Q())
    user._device()
    with pytest.raises(L.KnpemiError, match="right-hand side only"):
        user.set_integrator("rush_larsen")
    assert user.method == "lsoda"
    user2 = MembraneModel(_Plug, None, 1, _Q())
    user2.set_integrator("rush_larsen")     # not bound yet: refused when it is, at the first step
    with pytest.raises(L.KnpemiError, match="right-hand side only"):
        user2.step(dt, stim)


def _coupled_run(n_steps, ode_method="lsoda", ode_substeps=None, tol=None):
    from helpers import Setup
    from knpemi.stepper import DeviceStepper
    s = Setup("2d", 1, g_syn=10.0)
    ode = s.mem_models[0]['ode']
    for t in s.subdomain_list:
        for k in range(2):
            s.c[t][k].x.array[:] = s.c_prev[t][k].x._a
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev,
                       device_solves=(1e-12, 1e-13), ode_method=ode_method, ode_substeps=ode_substeps)
    st.add_membrane_model(ode, s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
    if tol is not None:
        ode.rtol, ode.atol = tol
    for _ in range(n_steps):
        st.step()
    st.download()
    return s.phi_M_prev[1].x._a.copy(), ode.states.copy()


@pytest.mark.gpu
def test_coupled_run_against_lsoda(hip_lib):
    """The 2-D r = 1 set-up of test_ten_time_steps_2d_match_oracle, 40 steps, the stimulated cell fires.  Yardstick
    d0 = max |phi_M difference| between LSODA as shipped (rtol 1e-8 / atol 1e-10) and LSODA at 1e-10 / 1e-12: rk4 with
    25 sub-steps lies within 10 d0 of the tighter run; euler and rush_larsen halve their distance from it between 25
    and 50 sub-steps (factor in [1.6, 2.4]).
    Solves: the device Krylov solves at rtol 1e-12 / 1e-13, four orders below the looser ODE tolerance, so that d0
    measures the ODE tolerance and not the solver's."""
    n = 40
    loose, _ = _coupled_run(n)
    tight, states = _coupled_run(n, tol=(1e-10, 1e-12))
    d0 = np.abs(loose - tight).max()
    print(f"phi_M after {n} steps: {tight.min():.5f} .. {tight.max():.5f} V; d0 = {d0:.3e}")
    rk4, _ = _coupled_run(n, "rk4", 25)
    d_rk4 = np.abs(rk4 - tight).max()
    print(f"rk4 n=25: {d_rk4:.3e} = {d_rk4 / d0:.2f} d0")
    dist = {}
    for method in ("euler", "rush_larsen"):
        for sub in (25, 50):
            dist[method, sub] = np.abs(_coupled_run(n, method, sub)[0] - tight).max()
        print(f"{method}: n=25 {dist[method, 25]:.3e}, n=50 {dist[method, 50]:.3e}, "
              f"ratio {dist[method, 25] / dist[method, 50]:.3f}")
    assert tight.max() > -0.0744 + 0.030, "the cell has not fired"
    assert d_rk4 <= 10 * d0
    for method in ("euler", "rush_larsen"):
        assert 1.6 <= dist[method, 25] / dist[method, 50] <= 2.4


@pytest.mark.gpu
def test_three_subdomain_driver_with_rush_larsen(hip_lib, tmp_path):
    """run_stim_duration.py --device-resident --steps 20 --ode-method rush_larsen --series: neuron and glia sweeps on
    two streams, no failed dof (the downloads would refuse), the series written."""
    spec = importlib.util.spec_from_file_location(
        "run_stim_duration", os.path.join(ROOT, "examples", "local_astrocyte_depolarization", "run_stim_duration.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    cfg = drv.load_config("baseline")
    path = tmp_path / "s.npz"
    with contextlib.redirect_stdout(io.StringIO()):
        p, hist = drv.solve_system(cfg, n_steps=20, device_resident=True, outdir=str(tmp_path), quiet=True,
                                   series=str(path), ode_method="rush_larsen")
    for tag in (1, 2):
        for mm in p.subdomain_list[tag]["mem_models"]:
            assert (mm["ode"].method, mm["ode"].substeps) == ("rush_larsen", 25)
            assert np.isfinite(mm["ode"].states).all()
    ser = np.load(path)
    assert ser["t"].shape == (20,)
    for key in ("phi_M_neuron", "phi_M_glia", "K_ecs_max"):
        assert np.isfinite(ser[key]).all(), key
    # the same 20 steps with LSODA: first-order sub-steps of 4 us stay close to it
    with contextlib.redirect_stdout(io.StringIO()):
        _, ref = drv.solve_system(cfg, n_steps=20, device_resident=True, outdir=str(tmp_path), quiet=True)
    assert abs(hist["phi_M_neuron"][-1] - ref["phi_M_neuron"][-1]) < 0.5      # mV
    assert abs(hist["phi_M_glia"][-1] - ref["phi_M_glia"][-1]) < 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_nonfinite_state_is_refused_like_an_lsoda_failure(hip_lib, method):
    from helpers import Setup
    from knpemi import _lib as L
    from knpemi.stepper import DeviceStepper
    s = Setup("2d", 1, g_syn=10.0)
    ode = s.mem_models[0]['ode']
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev,
                       ode_method=method)
    ode.states[7, 0] = np.nan       # one row of the state table (gate m of dof 7)
    st.add_membrane_model(ode, s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
    st.step()
    with pytest.raises(L.KnpemiError, match="1 membrane dof") as e:
        st.check_ode_failures()
    assert e.value.code == L.EODE
    st.step()
    with pytest.raises(L.KnpemiError) as e:
        st.download()
    assert e.value.code == L.EODE
    # the same through MembraneModel.advance: the dof is frozen with its last good state and named
    _, m, dt = _membrane("hh_mv", 20)
    m.set_integrator(method, 25)
    m.states[3, 1] = np.inf
    with pytest.raises(RuntimeError, match=r"failed on 1 membrane dof\(s\): dofs \[3\] at steps \[0\]"):
        m.advance(dt, 6)
    assert m.last_stats["n_failed"] == 1 and np.isinf(m.states[3, 1]) and np.isfinite(np.delete(m.states, 3, 0)).all()
