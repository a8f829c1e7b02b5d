"""Membrane models on their own (knpemi_ode_create) and many steps per launch (ode_advance_kernel) on the MI355X."""
import os
import sys

import numpy as np
import pytest

from ode_steady import steady_steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "calibrate_initial_conditions"))
import run_calibration as rc  # noqa: E402

MODELS = ["hh_mv", "glial", "glial_benchmark"]   # two shipped right-hand sides and the hipRTC plug-in


def _membrane(name, n_cells=10, seed=0):
    """Model `name` on an interval mesh with its driver's parameters, states spread a little from node to node."""
    module = rc.load_model(name)
    params, dt = rc.conditions(name)
    m = rc.make_membrane(module, n_cells, params)
    v = module.state_indices("V")
    m.states[:, v] += np.linspace(-2.0, 2.0, m.nodes) * (1e-3 if name == "hh_si" else 1.0)
    return module, m, dt


def _host_rhs(name, module):
    if name == "glial_benchmark":
        return lambda y, t, p: module.rhs(t, y, np.zeros(len(y)), p)
    import knpemi_oracle as o
    return o.MODELS[name]["rhs"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_standalone_step_matches_odepack_and_a_pde_bound_model(hip_lib, name):
    from scipy.integrate import odeint
    from helpers import Setup
    from knpemi.odeSolver import MembraneModel
    module, alone, dt = _membrane(name)
    # the same model bound to the 2-D r = 1 problem, on the same number of dofs
    s = Setup("2d", 1, model="hh_mv" if name == "hh_mv" else "glial", build_forms=False)
    Q = s.phi_M_prev[1].function_space
    bound = MembraneModel(module, s.ft, 1, Q)
    free = MembraneModel(module, s.ft, 1, Q)
    s.subdomain_list[1]['mem_models'] = [{'ode': bound, 'I_ch_k': s.mem_models[0]['I_ch_k']}]
    s.mem_models = s.subdomain_list[1]['mem_models']
    s.build_forms()
    assert bound._dp is not None and free._dp is None
    rows = np.arange(free.nodes) % alone.nodes
    for m in (bound, free):
        m.states[:], m.parameters[:] = alone.states[rows], alone.parameters[rows]
    ref_y, ref_p = alone.states.copy(), alone.parameters.copy()
    f = _host_rhs(name, module)
    for k in range(3):
        alone.step_lsoda(dt, None)
        bound._pending_flags = 0
        bound.step_lsoda(dt, None)
        free.step_lsoda(dt, None)
        for i in range(alone.nodes):
            ref_y[i] = odeint(f, ref_y[i], [k * dt, (k + 1) * dt], args=(ref_p[i],), rtol=1e-8, atol=1e-10)[-1]
        assert np.abs(alone.states - ref_y).max() <= 1e-8 * np.abs(ref_y).max()
        assert np.array_equal(free.states, bound.states) and np.array_equal(free.parameters, bound.parameters)
        assert np.array_equal(free.states[:alone.nodes], alone.states)
    assert alone.last_stats["n_failed"] == 0 and alone.last_stats["n_rhs"] > alone.nodes


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_advance_equals_repeated_steps_bit_for_bit(hip_lib, name, monkeypatch):
    monkeypatch.setenv("KNPEMI_ODE_ADVANCE_CHUNK", "8")
    n, every = 37, 3                     # five launches of 8 steps, the last one short
    module, a, dt = _membrane(name)
    _, b, _ = _membrane(name)
    stim = {"stim_amplitude": 1.0 if name != "hh_si" else 10.0}
    loc = lambda x: x[0] < 0.45          # noqa: E731
    names = rc.state_names(module)
    traj, n_rhs, n_st = [], 0, 0
    for _ in range(n):
        a.step_lsoda(dt, stim, loc)
        traj.append(a.states.copy())
        n_rhs += a.last_stats["n_rhs"]
        n_st += a.last_stats["n_steps"]
    hist = b.advance(dt, n, stimulus=stim, stimulus_locator=loc, record=names, every=every)
    assert hip_lib.knpemi_ode_advance_chunk(b._dp.h, b._sub, b._model) == 8
    assert np.array_equal(a.states, b.states)
    assert np.array_equal(a.parameters, b.parameters)
    assert a.time == b.time
    assert (b.last_stats["n_rhs"], b.last_stats["n_steps"], b.last_stats["n_failed"]) == (n_rhs, n_st, 0)
    for i, s in enumerate(names):
        want = np.array([traj[r * every + every - 1][:, module.state_indices(s)] for r in range(n // every)])
        assert hist[s].shape == (n // every, a.nodes) and np.array_equal(hist[s], want), s
    # the host picks the launch length itself when not forced
    monkeypatch.delenv("KNPEMI_ODE_ADVANCE_CHUNK")
    b.advance(dt, 5)
    assert 1 <= hip_lib.knpemi_ode_advance_chunk(b._dp.h, b._sub, b._model) <= 2048


@pytest.mark.gpu
def test_steady_state_of_hh_mv(hip_lib):
    module, m, dt = _membrane("hh_mv")
    names = rc.state_names(module)
    y0 = m.states.copy()
    rtol, atol, window = 1e-10, 1e-12, 20
    steps, hist = m.steady_state(dt, 20000, rtol=rtol, atol=atol, window=window, record=names)
    traj = np.concatenate([y0[None], np.stack([hist[s] for s in names], axis=2)])
    assert (steps > 0).all()
    assert np.array_equal(steps, steady_steps(traj, rtol, atol, window))
    for q in range(m.nodes):        # frozen after the step on which it became steady
        assert (traj[steps[q]:, q] == m.states[q]).all()
    assert abs(m.time - steps.max() * dt) < 1e-9 * steps.max()
    # a fixed point: another 500 plain steps barely move it
    y = m.states.copy()
    m.advance(dt, 500)
    assert np.abs(m.states - y).max() < 1e-6
    # The example's initial values were calibrated with the whole neuron + glia + ECS system, whose concentrations move;
    # the membrane alone at the driver's fixed concentrations rests 0.84 mV below (measured): within 1.5 mV, gates 0.03.
    rest = module.init_state_values()
    assert (np.abs(m.states[:, 3] - rest[3]) < 1.5).all() and (np.abs(m.states[:, :3] - rest[:3]) < 0.03).all()


@pytest.mark.gpu
def test_parameter_sweep_equals_single_runs(hip_lib):
    module = rc.load_model("hh_mv")
    params, dt = rc.conditions("hh_mv")
    values = np.linspace(2.0, 8.0, 4096)
    m = rc.make_membrane(module, len(values) - 1, params)
    kix = module.parameter_indices("K_e")
    m.parameters[:, kix] = values
    steps = m.steady_state(dt, 3000, rtol=1e-8, atol=1e-10, window=10)
    assert (steps > 0).sum() > 0
    for q in (0, 1, 1000, 2047, 4095):
        one = rc.make_membrane(module, 1, params)
        one.parameters[:, kix] = values[q]
        s1 = one.steady_state(dt, 3000, rtol=1e-8, atol=1e-10, window=10)
        assert s1[0] == steps[q]
        assert np.array_equal(one.states[0], m.states[q]) and np.array_equal(one.parameters[0], m.parameters[q])


@pytest.mark.gpu
def test_calibrate_then_run_matches_oracle_step(hip_lib):
    import driver
    from helpers import Setup, rel_err
    from knpemi.stepper import DeviceStepper
    s = Setup("2d", 1, g_syn=10.0, build_forms=False)
    ode = s.mem_models[0]['ode']
    params, dt = rc.conditions("hh_si")
    for key, value in params.items():
        ode.parameters[:, ode.ode.parameter_indices(key)] = value
    before = ode.states.copy()
    ode.advance(dt, 200)                     # standalone: no PDE problem yet
    assert ode._standalone is not None and not np.array_equal(before, ode.states)
    ode.time = 0
    s.build_forms()                          # moves to the PDE problem with its tables
    assert ode._standalone is None
    o, P, prm, ions = s.oracle()
    c_all, _, _, _ = s.oracle_fields()
    mask = np.array([x[0] < 20e-6 for x in ode.dof_locations])
    run = driver.OracleRun(P, prm, ions, "hh_si", c_all, ode.states.copy(), ode.parameters.copy(),
                           ode.dof_locations, mask, {o.MODELS["hh_si"]["pidx"]["stim_amplitude"]: 10.0},
                           {'z': -1, 0: 0.0, 1: 0.0})
    for t in s.subdomain_list:
        for k in range(2):
            s.c[t][k].x.array[:] = s.c_prev[t][k].x._a
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev,
                       device_solves=(1e-12, 1e-13))
    st.add_membrane_model(ode, s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
    st.step()
    run.step()
    st.download()
    assert rel_err(s.phi_M_prev[1].x._a, run.phiM[1]) < 1e-6
    for t in (0, 1):
        for k in range(2):
            assert rel_err(s.c_prev[t][k].x._a, run.c_all[t][k]) < 1e-8
    assert rel_err(ode.states, run.states) < 1e-6
