"""CPU tests of the membrane events' host side (knpemi.events): `record_host` against a scalar restatement of the
rules, interpolated crossing times against an analytic signal, the ring of crossing times, the conduction velocity,
and the five knpemi_events_* symbols of the C ABI."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from knpemi.events import MembraneEvents, conduction_velocity, ring_to_times

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


class ScalarDof:
    """One membrane dof, written from the rules one record at a time in plain Python floats."""

    def __init__(self, threshold, reset, keep):
        self.thr, self.rst, self.keep = threshold, reset, keep
        self.first = True
        self.v_prev, self.armed, self.count = NAN, False, 0
        self.t_first = self.t_last = self.v_peak = self.t_peak = NAN
        self.ring = [NAN] * keep
        self.t_prev = None

    def record(self, t, v):
        if self.first:
            self.v_prev, self.armed, self.v_peak, self.t_peak = v, v < self.thr, v, t
            self.first = False
        elif not math.isfinite(v):
            self.v_prev = v
        else:
            if not self.armed and v < self.rst:
                self.armed = True
            if self.armed and v >= self.thr:
                tc = self.t_prev + (t - self.t_prev) * ((self.thr - self.v_prev) / (v - self.v_prev))
                self.count += 1
                self.t_last = tc
                if self.count == 1:
                    self.t_first = tc
                if self.keep:
                    self.ring[(self.count - 1) % self.keep] = tc
                self.armed = False
            if v > self.v_peak:
                self.v_peak, self.t_peak = v, t
            self.v_prev = v
        self.t_prev = t

    def times(self):
        m = min(self.count, self.keep)
        return [self.ring[(n - 1) % self.keep] for n in range(self.count - m + 1, self.count + 1)] + [NAN] * (self.keep - m)


def _same(a, b):
    """Equal bit for bit, NaN in the same places."""
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def _piecewise(rng, n_t, n_q, thr, rst):
    """Random piecewise-linear sequences that wander across [rst - 1, thr + 1], with the planted special dofs."""
    knots = rng.uniform(rst - 1.0, thr + 1.0, (n_t // 4 + 2, n_q))
    s = np.arange(n_t) / 4.0
    i = s.astype(int)
    v = knots[i] + (s - i)[:, None] * (knots[i + 1] - knots[i])
    v[0, :10] = thr + rng.uniform(0.1, 1.0, 10)          # start above the threshold
    v[:, 10] = thr                                       # sits exactly on it from the first record on
    v[:, 11] = thr - 0.5
    v[20:, 11] = thr                                     # reaches it exactly, once, and stays
    v[7, 12] = np.nan                                    # one NaN sample
    v[:, 13] = rst - 0.5                                 # one crossing, then a dip that does not reach reset
    v[10:, 13] = thr + 0.5
    v[20:30, 13] = 0.5 * (thr + rst)
    v[30:, 13] = thr + 0.25
    v[:, 14] = rst - 1.0                                 # never reaches the threshold
    v[5, 15] = np.inf                                    # an infinite sample
    return v


@pytest.mark.parametrize("thr,rst,keep", [(-0.02, -0.04, 3), (0.1, 0.1, 0), (0.0, -0.3, 8)])
def test_record_host_equals_scalar_restatement(thr, rst, keep):
    rng = np.random.default_rng(11)
    n_t, n_q = 60, 97
    v = _piecewise(rng, n_t, n_q, thr, rst)
    t = np.cumsum(rng.uniform(0.5e-3, 2e-3, n_t))        # non-uniform times
    ev = MembraneEvents({1: n_q})
    ev.watch(1, thr, rst, keep=keep)
    dofs = [ScalarDof(thr, rst, keep) for _ in range(n_q)]
    for k in range(n_t):
        ev.record_host(t[k], {1: v[k]})
        for q in range(n_q):
            dofs[q].record(float(t[k]), float(v[k, q]))
    m = ev.maps(1)
    assert np.array_equal(m["count"], [d.count for d in dofs])
    for key in ("t_first", "t_last", "v_peak", "t_peak"):
        assert _same(m[key], [getattr(d, key) for d in dofs]), key
    assert m["times"].shape == (n_q, keep) and _same(m["times"], np.array([d.times() for d in dofs]).reshape(n_q, keep))
    # the planted dofs did what they were planted for
    assert m["count"][10] == 0 and m["count"][14] == 0 and m["count"][11] == 1 and m["count"][13] == 1
    assert m["t_first"][11] == t[20] and m["v_peak"][13] == thr + 0.5
    assert (m["count"][:10] >= 0).all() and m["count"].max() > 1
    assert np.array_equal(ev.fired(1), m["count"] > 0)
    with pytest.raises(ValueError, match="greater than the previous"):
        ev.record_host(t[-1], {1: v[-1]})


@pytest.mark.parametrize("thr", [0.0, 0.3])
def test_crossing_times_of_a_sine_within_the_interpolation_bound(thr):
    f, dt, n = 5.0, 0.97e-3, 1000
    t = np.arange(n) * dt
    om = 2.0 * math.pi * f
    ev = MembraneEvents({1: 1})
    ev.watch(1, thr, -0.5, keep=8)
    for k in range(n):
        ev.record_host(t[k], {1: np.array([math.sin(om * t[k])])})
    # upward crossings of sin(om t) = thr at t0 + k / f; the first record (t = 0) cannot count one
    t0 = math.asin(thr) / om
    exact = np.array([t0 + k / f for k in range(0 if thr > 0.0 else 1, 10) if t0 + k / f < t[-1]])
    m = ev.maps(1)
    assert m["count"][0] == len(exact) and len(exact) >= 4
    # linear interpolation: |v - chord| <= dt^2 max|v''| / 8 on an interval, and the chord rises at least as fast as
    # the smallest |v'| on it, |v'(t*)| - dt max|v''|
    v2 = om * om
    slope = om * math.sqrt(1.0 - thr * thr) - dt * v2
    bound = dt * dt * v2 / (8.0 * slope)
    err = np.abs(m["times"][0, :len(exact)] - exact)
    assert err.max() <= bound, (err.max(), bound)
    assert abs(m["t_first"][0] - exact[0]) <= bound and abs(m["t_last"][0] - exact[-1]) <= bound
    assert m["v_peak"][0] <= 1.0 and m["v_peak"][0] >= 1.0 - 0.5 * (om * dt) ** 2
    periods = (m["t_peak"][0] - 0.25 / f) * f            # the sample nearest to a maximum, of whichever period
    assert abs(periods - round(periods)) / f <= dt
    rate = ev.firing_rate(1, 0.0, t[-1])
    assert rate[0] == len(exact) / t[-1]


def test_ring_keeps_the_latest_crossings_oldest_first():
    f, dt = 10.0, 1.03e-3
    om = 2.0 * math.pi * f
    t = np.arange(int(7.5 / f / dt)) * dt             # 7.5 periods: the crossings of periods 0 .. 7
    all_of, some = MembraneEvents({1: 1}), MembraneEvents({1: 1})
    all_of.watch(1, 0.25, -0.25, keep=16)
    some.watch(1, 0.25, -0.25, keep=3)
    for tk in t:
        for ev in (all_of, some):
            ev.record_host(tk, {1: np.array([math.sin(om * tk)])})
    a, s = all_of.maps(1), some.maps(1)
    assert a["count"][0] == 8 and s["count"][0] == 8
    assert np.array_equal(s["times"][0], a["times"][0, 5:8])            # crossings 6, 7, 8, oldest first
    assert np.isnan(a["times"][0, 8:]).all() and np.all(np.diff(a["times"][0, :8]) > 0)
    assert s["t_first"][0] == a["times"][0, 0] and s["t_last"][0] == a["times"][0, 7]
    # what `keep` limits: a window that begins before the oldest remembered crossing and does not cover them all
    assert np.isnan(some.firing_rate(1, 0.5 * (a["times"][0, 1] + a["times"][0, 2]), t[-1])[0])
    assert np.isnan(some.firing_rate(1, a["times"][0, 5] - 1e-6, t[-1])[0])
    assert some.firing_rate(1, a["times"][0, 5], t[-1])[0] == 3 / (t[-1] - a["times"][0, 5])
    assert some.firing_rate(1, a["times"][0, 5] + 1e-6, t[-1])[0] == 2 / (t[-1] - (a["times"][0, 5] + 1e-6))
    assert some.firing_rate(1, 0.0, t[-1])[0] == 8 / t[-1]
    # the slot arithmetic on its own: crossing n in slot (n - 1) % keep
    ring = np.array([[7.0], [8.0], [6.0]])
    assert np.array_equal(ring_to_times(ring, np.array([8])), [[6.0, 7.0, 8.0]])
    assert _same(ring_to_times(np.array([[1.0], [2.0], [NAN]]), np.array([2])), [[1.0, 2.0, NAN]])


def _membrane_2d():
    from knpemi.fem import extract_submesh, make_mesh_2D
    mesh, ct, ft = make_mesh_2D(1)
    mem = extract_submesh(mesh, ft, [1])[0]
    return {0: dict(tag=0), 1: dict(tag=1, mesh_mem=mem)}, mem


def test_conduction_velocity_recovers_the_speed():
    subs, mem = _membrane_2d()
    ev = MembraneEvents(subs)
    ev.watch(1, -20e-3, -40e-3, keep=2)
    x = ev.locations(1)
    assert x.shape == (mem.num_vertices, 2) and np.array_equal(x, mem.x)
    x0 = np.array([x[:, 0].min(), x[x[:, 0].argmin(), 1]])
    c = 0.73
    t_first = np.linalg.norm(x - x0, axis=1) / c
    speed, rms, n = ev.conduction_velocity(1, x0, maps=dict(t_first=t_first, locations=x))
    assert n == x.shape[0] and abs(speed - c) <= 1e-12 * c and rms <= 1e-12 * np.ptp(x[:, 0])
    # only the fired dofs count, and an offset of the activation times does not change the slope
    t2 = t_first + 3.0e-3
    t2[::3] = np.nan
    speed2, _, n2 = conduction_velocity(x, t2, x0)
    assert n2 == int(np.isfinite(t2).sum()) and abs(speed2 - c) <= 1e-12 * c
    # through the object's own state: nothing fired yet
    with pytest.raises(ValueError, match="at least 3"):
        ev.conduction_velocity(1, x0)
    t3 = np.full(x.shape[0], np.nan)
    t3[:2] = t_first[:2]
    with pytest.raises(ValueError, match="at least 3"):
        conduction_velocity(x, t3, x0)


def test_watch_and_save(tmp_path):
    subs, mem = _membrane_2d()
    ev = MembraneEvents(subs)
    with pytest.raises(ValueError, match="no cell"):
        ev.watch(0, 0.0)
    with pytest.raises(ValueError, match="reset"):
        ev.watch(1, 0.0, reset=0.1)
    with pytest.raises(ValueError, match="keep"):
        ev.watch(1, 0.0, keep=65)
    ev.watch(1, 0.0, keep=2)
    with pytest.raises(ValueError, match="watched already"):
        ev.watch(1, 0.0, keep=2)
    n = mem.num_vertices
    ev.record_host(0.0, {1: np.full(n, -1.0)})
    ev.record_host(1.0, {1: np.linspace(-1.0, 1.0, n)})
    path = tmp_path / "ev.npz"
    ev.save(path)
    z = np.load(path)
    assert set(z.files) == {f"1/{k}" for k in ("count", "t_first", "t_last", "v_peak", "t_peak", "times", "locations")}
    assert np.array_equal(z["1/count"], (np.linspace(-1.0, 1.0, n) >= 0.0).astype(np.int32))
    assert "fired" in ev.summary(1, origin=mem.x[0])
    ev.reset_host()
    assert ev.maps(1)["count"].sum() == 0


NAMES = ("knpemi_events_set", "knpemi_events_record", "knpemi_events_read", "knpemi_events_reset", "knpemi_events_clear")


def test_events_abi_is_declared_exported_and_bound(hip_lib):
    from knpemi import _lib as L
    header = open(os.path.join(ROOT, "include", "knpemi_hip.h")).read()
    ctype_of = {"knpemi_handle*": C.c_void_p, "int": C.c_int, "double": C.c_double, "const int32_t*": L.c_int_p,
                "int32_t*": L.c_int_p, "const double*": L.c_dbl_p, "double*": L.c_dbl_p}
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in knpemi_hip.h"
        params = [" ".join(p.split()[:-1]) for p in m.group(1).replace("\n", " ").split(",")]
        assert hasattr(hip_lib, name), f"{name} is not exported"
        res, args = L.SIGNATURES[name]
        assert res is C.c_int and args == [ctype_of[p] for p in params], (name, params)
        fn = getattr(hip_lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args
    assert int(re.search(r"#define\s+KNPEMI_EVENTS_MAX_KEEP\s+(\d+)", header).group(1)) == L.EVENTS_MAX_KEEP
    # a null handle is refused before anything touches a device
    assert hip_lib.knpemi_events_record(None, 0.0) == L.EINVAL
    assert hip_lib.knpemi_events_set(None, 0, None, None, None, 0) == L.EINVAL
    assert hip_lib.knpemi_events_read(None, 1, None, None, None, None, None, None) == L.EINVAL
    assert hip_lib.knpemi_events_reset(None) == L.EINVAL and hip_lib.knpemi_events_clear(None) == L.EINVAL
