"""CPU tests of the fixed-step membrane integrators (csrc/fixed_step.h + membrane_models.h, host build in tests/native):
the three schemes against a numpy restatement with the oracle's right-hand sides, their orders and stiffness limits
against ODEPACK at tight tolerances, and the Python / ABI surface that needs no device."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.integrate import odeint

import fixed_step_host as fsh
import knpemi_oracle as o

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ["hh_si_stim0", "hh_si_stim10", "hh_mv_stim0", "hh_mv_stim1", "glial_stim0"]
GATES = {"hh_si": (0, 1, 2), "hh_mv": (0, 1, 2), "glial": ()}


def golden():
    return np.load(os.path.join(HERE, "golden", "ode_models.npz"))


def model_of(key):
    return key.rsplit("_stim", 1)[0]


# ---- the restatement: the three formulas of the issue / fixed_step.h, with the oracle's right-hand side -------------
def f(rhs, t, y, p):
    return np.array(rhs(list(y), t, p.copy()), dtype=np.float64)


def gate_rates(rhs, t, y, p, gates):
    """a_i, b_i of dy_i/dt = a_i (1 - y_i) - b_i y_i: the right-hand side at y_i = 0 is a_i, at y_i = 1 it is -b_i."""
    y0, y1 = np.array(y), np.array(y)
    y0[list(gates)], y1[list(gates)] = 0.0, 1.0
    return f(rhs, t, y0, p), -f(rhs, t, y1, p)


def restated_interval(rhs, method, y, p, t0, dt, n, gates):
    h = dt / n
    y = np.array(y, dtype=np.float64)
    for j in range(n):
        t = t0 + j * h
        if method == "euler":
            y = y + h * f(rhs, t, y, p)
        elif method == "rk4":
            k1 = f(rhs, t, y, p)
            k2 = f(rhs, t + h / 2, y + h / 2 * k1, p)
            k3 = f(rhs, t + h / 2, y + h / 2 * k2, p)
            k4 = f(rhs, t + h, y + h * k3, p)
            y = y + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        else:
            new = y + h * f(rhs, t, y, p)
            if gates:
                a, b = gate_rates(rhs, t, y, p, gates)
                for i in gates:
                    y_inf = a[i] / (a[i] + b[i])
                    new[i] = y_inf + (y[i] - y_inf) * math.exp(-(a[i] + b[i]) * h)
            y = new
    return y


@pytest.mark.parametrize("n", [1, 5, 25])
@pytest.mark.parametrize("method", ["euler", "rk4", "rush_larsen"])
@pytest.mark.parametrize("key", KEYS)
def test_host_build_matches_restatement(key, method, n):
    """10 intervals from the golden start states: states agree to 1e-12 relative per right-hand-side evaluation (the
    bound test_lsoda_host.py puts on one evaluation, accumulated), and the currents in the parameter row are the
    right-hand side's at the final state of every interval.  Where a sub-step of the key's dt is past the scheme's
    stability limit and the restatement stops being finite (rk4, n = 1 on the spike of hh_mv_stim1), the host build
    has to agree up to that interval and report it as failed."""
    g = golden()
    model = model_of(key)
    rhs = o.MODELS[model]["rhs"]
    y, p = g[f"{key}_y0"].copy(), g[f"{key}_p0"].copy()
    dt = float(g[f"{key}_dt"])
    ref = y.copy()
    evals = 0
    sl = o._ich_slice(len(p))
    for k in range(10):
        rc, nfe, nst = fsh.step(model, method, y, p, k * dt, dt, n)
        assert nst == n and nfe == (4 * n if method == "rk4" else n) + 1
        try:
            ref = restated_interval(rhs, method, ref, g[f"{key}_p0"], k * dt, dt, n, GATES[model])
        except OverflowError:
            ref = np.full_like(ref, np.nan)
        if not np.isfinite(ref).all():
            # past the scheme's stability limit (h = 0.1 ms on the spike of hh_mv_stim1): the restatement overflows,
            # and the host build must report the same interval as failed
            print(f"{key} {method} n={n} interval {k}: restatement not finite, host build rc = {rc}")
            assert rc == 1
            return
        assert rc == 0
        evals += nfe
        err = np.abs(y - ref).max()
        print(f"{key} {method} n={n} interval {k}: |y - restatement| = {err:.3e} (max |y| {np.abs(ref).max():.3e})")
        assert err <= 1e-12 * evals * np.abs(ref).max()
        pr = g[f"{key}_p0"].copy()
        rhs(list(y), (k * dt) + dt, pr)
        assert np.abs(p[sl] - pr[sl]).max() <= 1e-12 * max(np.abs(pr[sl]).max(), 1e-300)
        # nothing but the currents changes in the row
        keep = np.ones(len(p), bool)
        keep[sl] = False
        assert np.array_equal(p[keep], g[f"{key}_p0"][keep])


def run_host(key, method, dt, n, n_intervals):
    """States after every interval, [n_intervals][n_states] (rows after a failure are NaN)."""
    g = golden()
    model = model_of(key)
    y, p = g[f"{key}_y0"].copy(), g[f"{key}_p0"].copy()
    out = np.full((n_intervals, len(y)), np.nan)
    for k in range(n_intervals):
        if fsh.step(model, method, y, p, k * dt, dt, n)[0] != 0:
            break
        out[k] = y
    return out


def run_odeint(key, dt, n_intervals):
    g = golden()
    rhs = o.MODELS[model_of(key)]["rhs"]
    times = dt * np.arange(n_intervals + 1)
    # the interval ends as output times: with [0, T] alone ODEPACK stops with "excess work" on the spike
    return odeint(rhs, g[f"{key}_y0"].copy(), times, args=(g[f"{key}_p0"].copy(),), rtol=1e-12, atol=1e-13)[1:]


@pytest.mark.parametrize("key", ["hh_mv_stim1", "hh_si_stim10"])
def test_orders_of_convergence(key):
    """100 intervals of the key's dt across an action potential; error = max over the states at the end against ODEPACK
    at rtol 1e-12.  Euler and Rush-Larsen: observed order within 0.3 of 1 from n = 25, 50, 100.  RK4: order above 3.5
    from n = 2, 4, 8 (the slope of log error over log h across the three)."""
    dt = float(golden()[f"{key}_dt"])
    ref = run_odeint(key, dt, 100)
    err = {}
    for method, ns in (("euler", (25, 50, 100)), ("rush_larsen", (25, 50, 100)), ("rk4", (2, 4, 8))):
        for n in ns:
            err[method, n] = np.abs(run_host(key, method, dt, n, 100)[-1] - ref[-1]).max()
            print(f"{key} {method} n={n}: error at the end {err[method, n]:.4e}")
    for method in ("euler", "rush_larsen"):
        for n in (25, 50):
            order = math.log2(err[method, n] / err[method, 2 * n])
            print(f"{key} {method} order from n={n},{2 * n}: {order:.3f}")
            assert abs(order - 1.0) <= 0.3
    order = math.log2(err["rk4", 2] / err["rk4", 8]) / 2
    print(f"{key} rk4 order from n=2,4,8: {order:.3f}")
    assert order > 3.5


def test_rush_larsen_outlasts_euler_on_the_spike():
    """h = 0.045 ms on the firing HH cell, as 224 intervals of one sub-step so that every sub-step is seen (Euler's
    overshoot sits on single sub-steps: sampled at every second one, its peak reads 54.5 mV): Rush-Larsen follows
    the spike (peak V within 2 mV of ODEPACK's) with every gate in [0, 1]; Euler overshoots it by more than 50 mV or
    blows up."""
    key, dt, n_int = "hh_mv_stim1", 0.045, 224
    ref = run_odeint(key, dt, n_int)
    rl = run_host(key, "rush_larsen", dt, 1, n_int)
    eu = run_host(key, "euler", dt, 1, n_int)
    peak_ref, peak_rl = ref[:, 3].max(), rl[:, 3].max()
    print(f"peak V: odeint {peak_ref:.3f}, rush_larsen {peak_rl:.3f}, euler {np.nanmax(eu[:, 3]):.3f} "
          f"(finite: {np.isfinite(eu).all()})")
    assert np.isfinite(rl).all()
    assert abs(peak_rl - peak_ref) <= 2.0
    assert rl[:, :3].min() >= 0.0 and rl[:, :3].max() <= 1.0
    assert (not np.isfinite(eu).all()) or eu[:, 3].max() > peak_ref + 50.0


def test_rush_larsen_is_euler_on_a_model_without_gates():
    g = golden()
    for n in (1, 5, 25):
        ya, pa = g["glial_stim0_y0"].copy(), g["glial_stim0_p0"].copy()
        yb, pb = ya.copy(), pa.copy()
        dt = float(g["glial_stim0_dt"])
        for k in range(10):
            assert fsh.step("glial", "euler", ya, pa, k * dt, dt, n)[0] == 0
            assert fsh.step("glial", "rush_larsen", yb, pb, k * dt, dt, n)[0] == 0
            assert np.array_equal(ya.view(np.uint64), yb.view(np.uint64))
            assert np.array_equal(pa.view(np.uint64), pb.view(np.uint64))


def test_gate_masks_and_rates():
    """The models' gate declarations: m, h, n of the HH models with the rates of their right-hand sides, none for glia."""
    g = golden()
    for key in ("hh_si_stim10", "hh_mv_stim1", "glial_stim0"):
        model = model_of(key)
        y, p = g[f"{key}_y0"].copy(), g[f"{key}_p0"].copy()
        a, b = np.zeros(len(y)), np.zeros(len(y))
        mask = fsh.load().fixed_step_host_rates(fsh.MODEL_ID[model], 0.0, fsh._ptr(y), fsh._ptr(p), fsh._ptr(a), fsh._ptr(b))
        assert mask == sum(1 << i for i in GATES[model])
        if GATES[model]:
            ar, br = gate_rates(o.MODELS[model]["rhs"], 0.0, y, p, GATES[model])
            for i in GATES[model]:
                assert abs(a[i] - ar[i]) <= 1e-12 * abs(ar[i]) and abs(b[i] - br[i]) <= 1e-12 * abs(br[i])


def test_nonfinite_state_is_reported():
    g = golden()
    y, p = g["hh_mv_stim1_y0"].copy(), g["hh_mv_stim1_p0"].copy()
    y[3] = np.nan
    for method in ("euler", "rk4", "rush_larsen"):
        assert fsh.step("hh_mv", method, y.copy(), p.copy(), 0.0, 0.1, 25)[0] == 1


def test_substep_count_is_checked_without_a_device():
    """0 and 10001 sub-steps are refused before anything reaches the device; the ABI refuses a null handle."""
    from knpemi import _lib as L
    from knpemi.odeSolver import MembraneModel

    class Q:
        def tabulate_dof_coordinates(self):
            return np.zeros((3, 2))
    import mm_hh
    m = MembraneModel(mm_hh, None, 1, Q())
    for bad in (0, 10001, -3):
        for method in ("euler", "rk4", "rush_larsen"):
            with pytest.raises(ValueError, match="1..10000"):
                m.set_integrator(method, bad)
    with pytest.raises(ValueError, match="unknown integrator"):
        m.set_integrator("heun")
    assert (m.method, m.substeps) == ("lsoda", None)
    m.set_integrator("rk4")
    assert (m.method, m.substeps) == ("rk4", 25)       # the reference drivers' n_steps_ODE
    with pytest.raises(RuntimeError, match=r"call step\(\)"):
        m.step_lsoda(1e-4, None)
    m.set_integrator("lsoda", 7)
    assert (m.method, m.substeps) == ("lsoda", None)
    assert fsh.load().fixed_step_host(0, 1, None, None, 0.0, 1.0, 0, None) == -100
    assert (L.ODE_LSODA, L.ODE_EULER, L.ODE_RK4, L.ODE_RUSH_LARSEN) == (0, 1, 2, 3)


def test_abi_exports_the_method_entry_points(hip_lib):
    from knpemi import _lib as L
    header = open(os.path.join(os.path.dirname(HERE), "include", "knpemi_hip.h")).read()
    for name, value in (("LSODA", 0), ("EULER", 1), ("RK4", 2), ("RUSH_LARSEN", 3)):
        assert f"#define KNPEMI_ODE_{name} {value}\n" in header
    assert "n_steps_ODE" in header
    for name in ("knpemi_ode_set_method", "knpemi_ode_get_method"):
        assert hasattr(hip_lib, name) and name in L.SIGNATURES
    if shutil.which("nm"):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
        assert " T knpemi_ode_set_method" in syms and " T knpemi_ode_get_method" in syms
    assert hip_lib.knpemi_ode_set_method(None, 1, 0, L.ODE_RK4, 25) == L.EINVAL
    assert hip_lib.knpemi_ode_get_method(None, 1, 0, None, None) == L.EINVAL
