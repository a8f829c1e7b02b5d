"""Times the membrane sweep per integrator (lsoda, euler, rk4, rush_larsen) on the GPU; not part of any test.

  1. config 2 (idealized 3-D geometry, tetrahedra, resolution 1: 2 952 membrane dofs of hh_si): the ODE tables at the
     start of every step of the trajectory window the bench times by default (steps [5, 25) of a run from t = 0 with
     device solves, LSODA as shipped) are recorded once; every method then sweeps exactly those 20 tables (uploaded
     again before each launch, plain sweep without the PDE head), timed by the events around the kernel
     (knpemi_profile).  Per configuration: median over the repeats of the mean sweep time of the window, and the
     min .. max of the repeats as the spread.
  2. 10^5 dofs of hh_mv on a handle of its own, one step from a state on the upstroke, timed by knpemi_timer_*.
  3. Whole time steps of DeviceStepper with device solves, lsoda against rk4 with 25 sub-steps, wall clock between
     synchronisations over the same window.

Prints one JSON line.
"""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("knp-emi-fenics-x_amd", os.path.join("examples", "idealized_geometries"),
          os.path.join("examples", "calibrate_initial_conditions")):
    sys.path.insert(0, os.path.join(ROOT, p))

WARMUP, STEPS = 5, 20
CONFIGS = [("lsoda", None)] + [(m, n) for m in ("euler", "rush_larsen", "rk4") for n in (5, 10, 25, 50)]


def stats(values):
    v = sorted(values)
    return dict(median=float(np.median(v)), min=v[0], max=v[-1])


def make_stepper(ode_method="lsoda", ode_substeps=None):
    from knpemi.stepper import DeviceStepper
    from setup_problem import Setup
    s = Setup("tet", 1, g_syn=10.0)
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev,
                       device_solves=(1e-5, 1e-7), ode_method=ode_method, ode_substeps=ode_substeps)
    ode = s.subdomain_list[1]['mem_models'][0]['ode']
    st.add_membrane_model(ode, s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
    return s, st, ode


def tables(ode):
    from knpemi import _lib as L
    st, pa = np.empty_like(ode.states), np.empty_like(ode.parameters)
    L.check(ode._dp.lib.knpemi_ode_get_tables(ode._dp.h, ode._sub, ode._model, L.dptr(st), L.dptr(pa)))
    return st, pa


def window_sweeps(repeats):
    from knpemi import _lib as L
    s, st, ode = make_stepper()
    for _ in range(WARMUP):
        st.step()
    snaps = []
    for _ in range(STEPS):
        snaps.append((float(ode.time),) + tables(ode))
        st.step()
    st.check_ode_failures()
    dp, lib = ode._dp, ode._dp.lib
    kid = L.KERNEL_NAMES.index("ode_step_kernel")
    out = {"dofs": int(ode.nodes)}
    for method, n in CONFIGS:
        ode.set_integrator(method, n)
        per_sweep = []
        for rep in range(repeats + 1):         # the first pass warms up
            L.check(lib.knpemi_profile(dp.h, 1 << kid))
            for t, y, p in snaps:
                L.check(lib.knpemi_ode_set_tables(dp.h, ode._sub, ode._model, L.dptr(y), L.dptr(p)))
                L.check(lib.knpemi_ode_step(dp.h, ode._sub, ode._model, t, st.dt, ode.rtol, ode.atol, 0,
                                            L.iptr(ode._ion_param), int(ode.V_index)))
            cnt, ms = C.c_int64(), C.c_double()
            L.check(lib.knpemi_profile_read(dp.h, kid, C.byref(cnt), C.byref(ms)))
            L.check(lib.knpemi_profile(dp.h, 0))
            if rep:
                per_sweep.append(ms.value * 1e3 / max(cnt.value, 1))
        st.check_ode_failures()
        out[method if n is None else f"{method}_{n}"] = stats(per_sweep)
    return out


def big_sweep(nd, repeats):
    import run_calibration as rc
    module = rc.load_model("hh_mv")
    params, dt = rc.conditions("hh_mv")
    m = rc.make_membrane(module, nd - 1, params)
    m.parameters[:, module.parameter_indices("K_e")] = np.linspace(2.0, 8.0, nd)
    stim = {"stim_amplitude": 1.0}
    m.advance(dt, 5, stimulus=stim)          # onto the upstroke, LSODA
    y0, p0, t0 = m.states.copy(), m.parameters.copy(), m.time
    out = {"dofs": nd}
    for method, n in CONFIGS:
        m.set_integrator(method, n)
        us = []
        for rep in range(repeats + 1):
            m.states[:], m.parameters[:], m.time = y0, p0, t0
            m.step(dt, stim)
            if rep:
                us.append(m.last_stats["ms"] * 1e3)
        out[method if n is None else f"{method}_{n}"] = stats(us)
    return out


def whole_steps(repeats):
    out = {}
    for method, n in (("lsoda", None), ("rk4", 25)):
        s, st, ode = make_stepper(method, n)
        ms = []
        for rep in range(repeats + 1):
            st.reset()
            for _ in range(WARMUP):
                st.step()
            st.dp.sync()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                st.step()
            st.dp.sync()
            if rep:
                ms.append((time.perf_counter() - t0) * 1e3 / STEPS)
        st.check_ode_failures()
        out[method if n is None else f"{method}_{n}"] = stats(ms)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--dofs", type=int, default=100000)
    ap.add_argument("--skip", nargs="*", default=[], choices=["window", "big", "steps"])
    a = ap.parse_args()
    out = {"window": [WARMUP, WARMUP + STEPS], "repeats": a.repeats}
    with contextlib.redirect_stdout(io.StringIO()):
        if "window" not in a.skip:
            out["config2_sweep_us"] = window_sweeps(a.repeats)
        if "big" not in a.skip:
            out["big_sweep_us"] = big_sweep(a.dofs, a.repeats)
        if "steps" not in a.skip:
            out["config2_step_ms"] = whole_steps(max(3, a.repeats // 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
