"""GPU tests of the membrane events (knpemi_events_*, DeviceStepper.detect, MembraneModel.detect) against the numpy
restatement `MembraneEvents.record_host`: counts, peaks and the NaN pattern of every time exactly; interpolated
crossing times within 8 eps max(|t|, |t - t_prev|) -- the formula t_prev + (t - t_prev) * ((thr - v_prev) / (v - v_prev))
has four roundings in front of the last add, and the compiler may contract the last multiply-add."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

from knpemi import _lib as L
from knpemi.events import MembraneEvents

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
KEEP = 3


def _time_tol(ref, t):
    """8 eps max(|t_k|, t_k - t_(k-1)) for every crossing time in `ref`, t_k being the record that found it (the first
    record at or after it)."""
    t = np.asarray(t)
    k = np.clip(np.searchsorted(t, np.nan_to_num(ref, nan=t[0])), 1, len(t) - 1)
    return 8.0 * EPS * np.maximum(np.abs(t[k]), t[k] - t[k - 1])


def _compare(dev, ref, t):
    assert np.array_equal(dev["count"], ref["count"])
    for key in ("v_peak", "t_peak"):
        assert np.array_equal(dev[key], ref[key], equal_nan=True), key
    worst = 0.0
    for key in ("t_first", "t_last", "times"):
        assert dev[key].shape == ref[key].shape and np.array_equal(np.isnan(dev[key]), np.isnan(ref[key])), key
        err = np.abs(dev[key] - ref[key])
        ok = ~np.isnan(ref[key])
        assert (err[ok] <= _time_tol(ref[key], t)[ok]).all(), (key, np.nanmax(err))
        worst = max(worst, float(np.nanmax(err / np.maximum(np.abs(ref[key]), 1e-300), initial=0.0)))
    return worst


def _problem(kind):
    """(set-up, device problem) of the three handles of the kernel test."""
    from helpers import Setup
    if kind == "three":
        from test_observables_gpu import _problem as three
        s = three("three", 0)[0]
    else:
        with contextlib.redirect_stdout(io.StringIO()):
            s = Setup("2d", 1) if kind == "2d" else Setup("tet", 0)
    return s, s.a_emi.dp


def _samples(rng, n_q, t, thr, rst):
    """A_q sin(2 pi f_q t_k + phi_q) with the planted dofs: [n_t][n_q]."""
    A = rng.uniform(0.5, 1.5, n_q)
    f = rng.uniform(50.0, 400.0, n_q)
    ph = rng.uniform(0.0, 2.0 * np.pi, n_q)
    v = A[None, :] * np.sin(2.0 * np.pi * f[None, :] * t[:, None] + ph[None, :])
    assert n_q >= 8
    v[:, 0] = thr                              # constant exactly at the threshold
    v[:, 1] = thr - 0.3
    v[17, 1] = thr                             # touches the threshold exactly once
    v[:, 2] = rst - 0.2                        # a crossing, a dip between reset and threshold, above again
    v[8:, 2] = thr + 0.4
    v[15:25, 2] = 0.5 * (thr + rst)
    v[25:, 2] = thr + 0.2
    v[11, 3] = np.nan                          # one NaN sample
    v[:, 4] = 0.1 * np.sin(2.0 * np.pi * f[4] * t + ph[4]) + thr - 0.2      # never reaches the threshold
    return v


CASES = [("2d", (1,)), ("tet", (1,)), ("three", (2,)), ("three", (1, 2))]


@pytest.mark.parametrize("kind,tags", CASES, ids=[f"{k}-{'+'.join(map(str, t))}" for k, t in CASES])
def test_kernel_matches_the_restatement_on_synthetic_samples(hip_lib, kind, tags):
    s, dp = _problem(kind)
    lib = dp.lib
    rng = np.random.default_rng(5)
    t = np.cumsum(rng.uniform(0.4e-3, 1.6e-3, 40))                 # non-uniform record times
    level = {1: (0.2, -0.1), 2: (-0.05, -0.3)}
    dev, host = MembraneEvents(s.subdomain_list), MembraneEvents(s.subdomain_list)
    for ev in (dev, host):
        for tag in tags:
            ev.watch(tag, *level[tag], keep=KEEP)
    v = {tag: _samples(rng, dev.n_q[tag], t, *level[tag]) for tag in s.subdomain_list if tag > 0}
    dev._attach(lib, dp.h, dp.sub_index)

    def play(n):
        for k in range(n):
            for tag in v:                      # unwatched cells are written too: their dofs are not in the grid
                dp.push_array(L.F_PHI_M, dp.sub_index[tag], 0, v[tag][k])
            L.check(lib.knpemi_events_record(dp.h, float(t[k])))
            host.record_host(t[k], {tag: v[tag][k] for tag in tags})

    play(len(t))
    for tag in tags:
        ref = host.maps(tag)
        # the condition of the test, on the host reference
        assert (ref["count"] > KEEP).mean() >= 0.25 and (ref["count"] == 0).any()
        assert ref["count"][0] == 0 and ref["count"][1] == 1 and ref["count"][2] == 1 and ref["count"][4] == 0
        assert ref["t_first"][1] == t[17]
        worst = _compare(dev.maps(tag), ref, t)
        print(f"{kind} cell {tag}: {dev.n_q[tag]} dofs, {int(ref['count'].sum())} crossings, largest relative "
              f"difference of a crossing time {worst:.2e}")
    # stale state is gone after a reset
    L.check(lib.knpemi_events_reset(dp.h))
    host.reset_host()
    for tag in tags:
        m = dev.maps(tag)
        assert m["count"].sum() == 0 and np.isnan(m["t_first"]).all() and np.isnan(m["times"]).all()
        assert np.isnan(m["v_peak"]).all() and np.isnan(m["t_peak"]).all()
    play(5)
    for tag in tags:
        _compare(dev.maps(tag), host.maps(tag), t)
    # arguments
    n_sub = len(s.subdomain_list)
    one, thr, rst = np.array([1], np.int32), np.array([0.0]), np.array([-1.0])

    def set_(sub, thr=thr, rst=rst, keep=KEEP):
        sub = np.asarray(sub, np.int32)
        rst = L.dptr(rst) if rst is not None else None
        return lib.knpemi_events_set(dp.h, len(sub), L.iptr(sub), L.dptr(thr), rst, keep)
    assert lib.knpemi_events_record(dp.h, float(t[4])) == L.EINVAL           # not greater than the previous record's
    assert lib.knpemi_events_record(dp.h, float("nan")) == L.EINVAL
    assert set_([0]) == L.EINVAL and set_([n_sub]) == L.EINVAL and set_([-1]) == L.EINVAL
    assert set_([1, 1], np.zeros(2), np.zeros(2)) == L.EINVAL and b"twice" in lib.knpemi_last_error()
    assert set_(one, rst=np.array([0.5])) == L.EINVAL                         # reset > threshold
    assert set_(one, keep=-1) == L.EINVAL and set_(one, keep=L.EVENTS_MAX_KEEP + 1) == L.EINVAL
    # a refused table leaves the previous one in place
    L.check(lib.knpemi_events_record(dp.h, float(t[5])))
    if len(tags) == 1 and n_sub > 2:                                          # the other cell is not watched
        other = 3 - tags[0]
        assert lib.knpemi_events_read(dp.h, dp.sub_index[other], None, None, None, None, None, None) == L.EINVAL
    assert lib.knpemi_events_read(dp.h, 0, None, None, None, None, None, None) == L.EINVAL
    assert set_(one, rst=None, keep=L.EVENTS_MAX_KEEP) == L.OK                # reset defaults to the threshold
    L.check(lib.knpemi_events_clear(dp.h))
    assert lib.knpemi_events_record(dp.h, 1.0) == L.EINVAL
    assert lib.knpemi_events_read(dp.h, 1, None, None, None, None, None, None) == L.EINVAL
    assert lib.knpemi_events_reset(dp.h) == L.EINVAL


# ---- through the stepper -------------------------------------------------------------------------------------------
STEPS = 20


def _stepper(observe=False, **kw):
    from knpemi.stepper import DeviceStepper
    from test_observables_gpu import _observables, _problem as obs_problem
    s, models, cells = obs_problem("2d", 1)
    kw.setdefault("device_solves", (1e-9, 1e-10))
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev, **kw)
    for m, stim, loc in models:
        st.add_membrane_model(m, stim, loc)
    obs = None
    if observe:
        obs = _observables(s, cells)
        st.observe(obs)
    return s, st, obs


def _steps(st, n, after=None):
    with contextlib.redirect_stdout(io.StringIO()):
        for k in range(n):
            st.step()
            if after is not None:
                after(k + 1)


@pytest.fixture(scope="module")
def threshold(hip_lib):
    """(threshold, the largest phi_M of every dof) from one preliminary run of the same steps.

    The threshold is the midpoint between the smallest and the largest of the dofs' peaks, so that it separates dofs
    that reach it from dofs that do not.  The midpoint between the smallest initial phi_M and the largest phi_M of the
    run cannot do that on this mesh: the 60 um cell is nearly isopotential.  In the oracle time loop (oracle/driver.py,
    direct solves, on the CPU) the dofs' peaks after 20 steps lie in [-50.525, -50.242] mV with the membrane at rest at
    -72.66 mV after the first step (and the phi_M function zero before it), and they stay within 0.5 mV of each other
    up to the overshoot of the action potential at step 27: with that midpoint every dof fires or none does, for every
    number of steps."""
    s, st, _ = _stepper()
    top = np.full(s.phi_M_prev[1].x._a.shape, -np.inf)

    def after(k):
        st.download()
        np.maximum(top, s.phi_M_prev[1].x._a, out=top)
    _steps(st, STEPS, after)
    return 0.5 * (float(top.min()) + float(top.max())), top


def _detect_run(threshold, every, **kw):
    """(stepper, device events, host events fed from a download after every recorded step, record times)."""
    s, st, _ = _stepper(**kw)
    dev, host = MembraneEvents(s.subdomain_list), MembraneEvents(s.subdomain_list)
    for ev in (dev, host):
        ev.watch(1, threshold, keep=KEEP)
    st.detect(dev, every=every)
    times = []

    def after(k):
        if k % every == 0:
            st.download()
            times.append(k * st.dt)
            host.record_host(times[-1], s.phi_M_prev)
    return s, st, dev, host, times, after


@pytest.mark.parametrize("every", [1, 3])
def test_stepper_maps_match_downloads(hip_lib, threshold, every):
    thr, top = threshold
    s, st, dev, host, times, after = _detect_run(thr, every)
    _steps(st, STEPS, after)
    ref = host.maps(1)
    if every == 1:      # the condition of the test: a dof that fires and one that does not, within the steps run
        assert (top >= thr).any() and (top < thr).any()
        assert (ref["count"] > 0).any() and (ref["count"] == 0).any()
    assert len(times) == STEPS // every
    _compare(dev.maps(1), ref, times)
    assert np.array_equal(dev.fired(1), ref["count"] > 0)
    with pytest.raises(RuntimeError, match="already"):
        st.detect(MembraneEvents(s.subdomain_list))


def test_reset_gives_bit_identical_maps(hip_lib, threshold):
    """reset() and the same steps again: every map bit for bit, so no state of the first run is left.  The solves
    start from the previous solution here (extrapolate_guess=False): the extrapolated guess carries the solutions of
    the last steps across reset(), which moves the iterates of the first solves within their tolerance.  No download
    in between: it would move the host objects, which reset() goes back to, on to the end of the run."""
    s, st, dev, host, times, after = _detect_run(threshold[0], 1, extrapolate_guess=False)
    _steps(st, STEPS)
    a = dev.maps(1)
    assert (a["count"] > 0).any() and (a["count"] == 0).any()
    st.reset()
    _steps(st, STEPS)
    b = dev.maps(1)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_observables_and_events_together(hip_lib, threshold):
    thr = threshold[0]
    s0, st0, obs0 = _stepper(observe=True)                      # observables alone
    _steps(st0, STEPS)
    alone = obs0.series()
    s1, st1, dev1, _, _, _ = _detect_run(thr, 1)                # events alone
    _steps(st1, STEPS)
    only = dev1.maps(1)
    s2, st2, obs2 = _stepper(observe=True)                      # both
    dev2 = MembraneEvents(s2.subdomain_list)
    dev2.watch(1, thr, keep=KEEP)
    st2.detect(dev2)
    _steps(st2, STEPS)
    both = obs2.series()
    assert alone.keys() == both.keys() and alone["t"].shape == (STEPS,)
    for k in alone:
        assert np.array_equal(alone[k], both[k]), k
    m = dev2.maps(1)
    assert (m["count"] > 0).any()
    for k in only:
        assert np.array_equal(only[k], m[k], equal_nan=True), k


# ---- stand-alone membrane models -------------------------------------------------------------------------------------
def test_standalone_membrane_model_records_firing(hip_lib):
    """65 dofs of hh_mv with a tonic drive that rises from dof to dof (the calibration example's parameter sweep, here of
    the sodium leak conductance): the first dofs stay silent, the last ones fire three times in 20 ms."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "examples", "calibrate_initial_conditions"))
    import run_calibration as rc
    module = rc.load_model("hh_mv")
    params, _ = rc.conditions("hh_mv")
    with contextlib.redirect_stdout(io.StringIO()):
        m = rc.make_membrane(module, 64, params)
    assert m.nodes == 65
    m.parameters[:, module.parameter_indices("g_leak_Na")] = np.linspace(0.1, 1.0, m.nodes)
    m.set_integrator("rush_larsen", 25)
    dev, host = MembraneEvents({m.tag: m.nodes}), MembraneEvents({m.tag: m.nodes})
    for ev in (dev, host):
        ev.watch(m.tag, -20.0, -40.0, keep=KEEP)
    m.detect(dev)
    with pytest.raises(RuntimeError, match="already"):
        m.detect(MembraneEvents({m.tag: m.nodes}))
    iv = module.state_indices("V")
    times = []
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(400):
            m.step(0.05, None)
            times.append(float(m.time))
            host.record_host(m.time, {m.tag: np.ascontiguousarray(m.states[:, iv])})
    got, ref = dev.maps(m.tag), host.maps(m.tag)
    _compare(got, ref, times)
    count = got["count"]
    assert count[0] == 0 and count[-1] >= 2 and (count == 0).sum() >= 2 and (count >= 2).sum() >= 2
    assert (np.maximum.accumulate(count) - count <= 1).all()            # non-decreasing along the ramp, within one
    assert np.array_equal(dev.locations(m.tag), m.dof_locations)
    # advance / steady_state run inside one launch and do not write the samples: the maps stay as they are
    with contextlib.redirect_stdout(io.StringIO()):
        m.advance(0.05, 40)
    after = dev.maps(m.tag)
    for k in got:
        assert np.array_equal(got[k], after[k], equal_nan=True), k
