"""What a membrane sweep reads and writes around the integrator (csrc/ode_kernel.h: head and tail of ode_step_body), on the
MI355X: the flags-0 sweep against the one-step advance kernel, the device's own trace / V / stimulus writes against the same
values written by the host, and the statistics slots over two sweeps.  Everything is compared bit for bit: the head and
tail move values, they compute nothing.

Sizes: hh_si runs 4 lanes per dof, so 16 dofs fill a wave -- 1, 15, 16, 17, 33 dofs are a single dof, a partial wave, a
full one, one dof in a second wave (whose other lanes repeat it) and two waves and a part; glial runs one lane per dof:
1, 64, 65."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "calibrate_initial_conditions"))
import run_calibration as rc  # noqa: E402

SIZES = [("hh_si", n) for n in (1, 15, 16, 17, 33)] + [("glial", n) for n in (1, 64, 65)]


class _Dofs:
    """The only thing MembraneModel asks of a function space: where its dofs are (no mesh needed for n dofs)."""

    def __init__(self, n):
        self.x = np.zeros((n, 3))
        self.x[:, 0] = np.linspace(0.0, 1.0, n) if n > 1 else 0.0

    def tabulate_dof_coordinates(self):
        return self.x


def _membrane(name, nq):
    """Model `name` on nq dofs with its driver's parameters; states and two parameters differ from dof to dof, so a row or
    a state that ends up at the wrong dof shows."""
    from knpemi.odeSolver import MembraneModel
    module = rc.load_model(name)
    params, dt = rc.conditions(name)
    m = MembraneModel(module, None, 1, _Dofs(nq))
    for key, value in params.items():
        m.parameters[:, module.parameter_indices(key)] = value
    spread = np.linspace(-1.0, 1.0, nq) if nq > 1 else np.zeros(1)
    m.states[:, module.state_indices("V")] += 2.0 * spread * (1e-3 if name == "hh_si" else 1.0)
    for key in ("K_e", "Na_i"):
        m.parameters[:, module.parameter_indices(key)] *= 1.0 + 0.05 * spread
    return module, m, dt


def _stim(name):
    return {"stim_amplitude": 10.0 if name == "hh_si" else 1.0}


def _loc(x):
    return x[0] < 0.45


@pytest.mark.gpu
@pytest.mark.parametrize("name,nq", SIZES)
def test_flags0_sweep_equals_one_step_of_advance(hip_lib, name, nq):
    _, a, dt = _membrane(name, nq)
    _, b, _ = _membrane(name, nq)
    for k in range(2):      # the second step starts from rows that hold the first one's currents
        a.step_lsoda(dt, _stim(name), _loc)
        b.advance(dt, 1, stimulus=_stim(name), stimulus_locator=_loc)
        assert np.array_equal(a.states, b.states), k
        assert np.array_equal(a.parameters, b.parameters), k
        sa, sb = a.last_stats, b.last_stats
        assert (sa["n_rhs"], sa["n_steps"], sa["n_failed"]) == (sb["n_rhs"], sb["n_steps"], sb["n_failed"]), k
        assert sa["n_failed"] == 0 and sa["n_steps"] >= nq and sa["n_rhs"] > sa["n_steps"]


@pytest.mark.gpu
@pytest.mark.parametrize("name,nq", SIZES)
def test_two_sweeps_accumulate_statistics(hip_lib, name, nq):
    from knpemi import _lib as L
    _, a, dt = _membrane(name, nq)
    _, b, _ = _membrane(name, nq)
    want = dict(n_rhs=0, n_steps=0, n_failed=0)
    for _ in range(2):
        a.step_lsoda(dt, _stim(name), _loc)
        for key in want:
            want[key] += a.last_stats[key]
    # the same two sweeps without reading the counters in between
    dp = b._device()
    b._set_stimulus(_stim(name), _loc)
    states, params = b.states.copy(), b.parameters.copy()
    L.check(hip_lib.knpemi_ode_set_tables(dp.h, b._sub, b._model, L.dptr(states), L.dptr(params)))
    t = 0
    for _ in range(2):
        L.check(hip_lib.knpemi_ode_step(dp.h, b._sub, b._model, float(t), float(dt), b.rtol, b.atol, 0,
                                        L.iptr(b._ion_param), int(b.V_index)))
        t = t + dt
    assert b._read_stats(0.0) == L.OK
    assert {k: b.last_stats[k] for k in want} == want
    L.check(hip_lib.knpemi_ode_get_tables(dp.h, b._sub, b._model, L.dptr(states), L.dptr(params)))
    assert np.array_equal(states, a.states) and np.array_equal(params, a.parameters)
    # read and reset
    assert b._read_stats(0.0) == L.OK
    assert {k: b.last_stats[k] for k in want} == dict(n_rhs=0, n_steps=0, n_failed=0)


def _pde_sweep(name, device_writes, inputs=None):
    """One sweep of the model bound to the 2-D r = 1 problem.  device_writes: SET_TRACES | SET_V and a masked stimulus;
    otherwise flags 0 on tables into which the host has written `inputs` = (trace columns, V, stimulus rows)."""
    from helpers import Setup
    from knpemi import _lib as L
    from knpemi.utils import update_ode_variables
    s = Setup("2d", 1, model=name)
    s.perturb()
    ode = s.mem_models[0]['ode']
    mod = ode.ode
    v_ix = ode.V_index
    dt = s.dt if name == "hh_si" else 0.1
    v_in = ode.states[:, v_ix] * (1.0 + 0.01 * np.linspace(-1.0, 1.0, ode.nodes))
    loc = s.stim_params['stimulus_locator']
    mask = np.array([bool(loc(x)) for x in ode.dof_locations])
    assert 0 < mask.sum() < ode.nodes
    sidx = mod.parameter_indices("stim_amplitude")
    trace_cols = [mod.parameter_indices(f"{ion['name']}_{side}") for ion in s.ion_list for side in "ei"]
    ich_cols = [mod.parameter_indices(f"I_ch_{ion['name']}") for ion in s.ion_list]
    p_before = ode.parameters.copy()
    if device_writes:
        s.phi_M_prev[1].x.array[:] = v_in
        update_ode_variables(ode, s.c_prev, s.phi_M_prev[1], s.ion_list, s.subdomain_list, s.mesh, s.ct, 1, 1)
        assert ode._pending_flags == L.ODE_SET_TRACES | L.ODE_SET_V
        ode.step_lsoda(dt, _stim(name), loc)
    else:
        traces, v, amplitude = inputs
        ode.parameters[:, trace_cols] = traces
        ode.states[:, v_ix] = v
        ode.parameters[mask, sidx] = amplitude
        ode._pending_flags = 0
        ode.step_lsoda(dt, None)
    assert ode.last_stats["n_failed"] == 0
    dp, sub = ode._dp, ode._sub
    phi_m = dp.pull_array(L.F_PHI_M, sub, 0, ode.nodes)
    ich = np.stack([dp.pull_array(L.F_I_CH, sub, k, ode.nodes) for k in range(len(s.ion_list))], axis=1)
    # what the sweep was given, from the host side: the oracle's nodal traces of the same concentration fields
    _, P, _, _ = s.oracle()
    c_all, _, _, _ = s.oracle_fields()
    host_traces = np.stack([t for k in range(len(s.ion_list)) for t in P.trace(1, c_all[0][k], c_all[1][k])], axis=1)
    return dict(states=ode.states.copy(), params=ode.parameters.copy(), phi_M=phi_m, I_ch=ich, stats=dict(ode.last_stats),
                v_in=v_in, mask=mask, sidx=sidx, trace_cols=trace_cols, ich_cols=ich_cols, v_ix=v_ix,
                host_traces=host_traces, p_before=p_before, amplitude=_stim(name)["stim_amplitude"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hh_si", "glial"])
def test_device_written_inputs_equal_host_written_inputs(hip_lib, name):
    A = _pde_sweep(name, True)
    # the rows hold what the device wrote into them: the traces -- nodal values of the concentration fields, the oracle's
    # up to the rounding of the eliminated ion's concentration (a sum of two products, formed on the device and on the host:
    # a few ulp of its largest term; 1e-14 of the column's largest value is ~45 ulp) --, the stimulus under the mask only ...
    dev_traces = A["params"][:, A["trace_cols"]]
    assert (np.abs(dev_traces - A["host_traces"]).max(axis=0) <= 1e-14 * np.abs(A["host_traces"]).max(axis=0)).all()
    assert not np.array_equal(dev_traces, A["p_before"][:, A["trace_cols"]])
    assert (A["params"][A["mask"], A["sidx"]] == A["amplitude"]).all()
    assert np.array_equal(A["params"][~A["mask"], A["sidx"]], A["p_before"][~A["mask"], A["sidx"]])
    # ... and the currents of the last right-hand side call, which are also the I_ch fields; phi_M is the new V
    assert np.array_equal(A["params"][:, A["ich_cols"]], A["I_ch"])
    assert np.array_equal(A["phi_M"], A["states"][:, A["v_ix"]])
    assert np.abs(A["I_ch"]).max() > 0.0
    untouched = [j for j in range(A["params"].shape[1]) if j not in A["trace_cols"] + A["ich_cols"] + [A["sidx"]]]
    assert np.array_equal(A["params"][:, untouched], A["p_before"][:, untouched])
    B = _pde_sweep(name, False, (dev_traces, A["v_in"], A["amplitude"]))
    for key in ("states", "phi_M", "I_ch", "params"):
        assert np.array_equal(A[key], B[key]), key
    for key in ("n_rhs", "n_steps", "n_failed"):
        assert A["stats"][key] == B["stats"][key], key
