"""GPU tests of the field maps (knpemi_maps_*, DeviceStepper.track) against the numpy restatement
`FieldMaps.record_host`, with the tolerances maps_cases.py derives from the formulas: counts, peaks, troughs and the NaN
pattern exactly, arrival times within 8 eps max(|t|, D), the accumulated statistics within (8 + n) eps of the sum of
their |increments|, the series' n exactly and its measure within the bound of a changed order of summation."""
import ctypes as C

import numpy as np
import pytest

import maps_cases as mc
from knpemi import _lib as L
from knpemi.maps import FieldMaps, STAT_MAPS

pytestmark = pytest.mark.gpu

_PROBLEMS = {}


def _problem(kind):
    """(set-up, device problem) of the three handles of the kernel test, built once each."""
    if kind not in _PROBLEMS:
        from helpers import Setup
        if kind == "three":
            from test_observables_gpu import _problem as three
            s = three("three", 0)[0]
        else:
            with mc.quiet():
                s = Setup("2d", 1) if kind == "2d" else Setup("tet", 0)
        _PROBLEMS[kind] = (s, s.a_emi.dp)
    return _PROBLEMS[kind]


def _series(lib, dp, n_cols, n_rows=64, reset=0):
    buf = np.full((n_rows, max(n_cols, 1)), np.nan)
    rows, over = C.c_int64(), C.c_int64()
    L.check(lib.knpemi_maps_series_read(dp.h, n_rows, L.dptr(buf), C.byref(rows), C.byref(over), reset))
    return buf[:min(rows.value, n_rows), :n_cols], rows.value, over.value


def _initial(m):
    for key, a in m.items():
        if key != "locations":
            assert np.isnan(a).all() if key in ("v_max", "t_max", "v_min", "t_min", "t_arrival") else not a.any(), key


CASES = [(kind, name, cells) for kind, cells in (("2d", (1,)), ("tet", (1,)), ("three", (2,)))
         for name in ("one_c", "four", "phi_M", "bulk_and_membrane")] + [("three", "phi_M", (1, 2))]


@pytest.mark.parametrize("kind,name,cells", CASES, ids=[f"{k}-{n}-{'+'.join(map(str, c))}" for k, n, c in CASES])
def test_kernel_matches_the_restatement_on_synthetic_samples(hip_lib, kind, name, cells):
    s, dp = _problem(kind)
    lib = dp.lib
    watches = mc.config(name, cells)
    dev, host = mc.field_maps(s, watches), mc.field_maps(s, watches)
    rng = np.random.default_rng(5)
    t = mc.record_times(rng)
    play = mc.Play(host, rng, t)
    capacity = 16 if name == "four" else 64          # once below the number of records: rows are dropped and counted
    dev._attach(dp, capacity)
    n_cols = dev.n_cols
    assert n_cols == 2 * min(2, sum(w[4].get("series", False) for w in watches)) > 0

    def run(ks):
        rows = []
        for k in ks:
            play.push(dp, k)
            L.check(lib.knpemi_maps_record(dp.h, float(t[k])))
            rows.append(host.record_host(t[k], *play.host(k)))
        return np.array(rows)

    def check(n_rec):
        worst = 0.0
        for wname in host.watches:
            worst = max(worst, mc.compare(dev.maps(wname), host.maps(wname), host.increment_sums(wname), t, n_rec))
        return worst

    ref = run(range(len(t)))
    mc.check_conditions(host, play, ref)              # the conditions of the test, on the host reference
    worst = check(len(t))
    got, n_rows, dropped = _series(lib, dp, n_cols)
    kept = min(capacity, len(t))
    assert (n_rows, dropped) == (kept, len(t) - kept)
    mc.compare_series(host, got, ref[:kept], [mc.series_terms(host, play, k) for k in range(kept)])
    print(f"{kind} {name}: {[w.n for w in host.watches.values()]} items, largest difference of an accumulated statistic "
          f"{worst:.2e} of its increments, {n_rows} rows kept, {dropped} dropped")
    # stale state is gone after a reset
    L.check(lib.knpemi_maps_reset(dp.h))
    host.reset_host()
    for wname in dev.watches:
        _initial(dev.maps(wname))
    assert _series(lib, dp, n_cols)[1:] == (0, 0)
    ref = run(range(5))
    check(5)
    got, n_rows, dropped = _series(lib, dp, n_cols)
    assert (n_rows, dropped) == (5, 0)
    mc.compare_series(host, got, ref, [mc.series_terms(host, play, k) for k in range(5)])

    # arguments: every refused table leaves the previous one in place
    n_sub, K = len(s.subdomain_list), len(s.ion_list)
    ALLB = L.MAPS_PEAK | L.MAPS_TROUGH | L.MAPS_INTEGRAL | L.MAPS_THRESHOLD
    wt = np.ones(sum(w.n for w in host.watches.values()) + dp.n_vert[0])

    def set_(spec, thr=(0.0,), weight=wt, cap=8, h=dp.h):
        spec = np.ascontiguousarray(spec, np.int32).reshape(-1, 4)
        thr = np.resize(np.asarray(thr, np.float64), spec.shape[0]) if thr is not None else None
        return lib.knpemi_maps_set(h, spec.shape[0], L.iptr(spec.ravel()), L.dptr(thr) if thr is not None else None,
                                   L.dptr(weight) if weight is not None else None, cap)
    ok = [L.F_C, 0, 0, ALLB]
    assert lib.knpemi_maps_set(dp.h, 1, None, None, None, 8) == L.EINVAL and set_(ok, thr=None) == L.EINVAL
    assert set_(np.zeros((0, 4))) == L.EINVAL and set_([ok] * (L.MAPS_MAX_WATCH + 1), thr=np.arange(33.0)) == L.EINVAL
    assert set_([L.F_I_CH, 1, 0, ALLB]) == L.EINVAL and set_([L.F_C_PREV, 0, 0, ALLB]) == L.EINVAL and set_([99, 0, 0, ALLB]) == L.EINVAL
    assert set_([L.F_PHI, n_sub, 0, ALLB]) == L.EINVAL and set_([L.F_PHI, -1, 0, ALLB]) == L.EINVAL
    assert set_([L.F_C, 0, K - 1, ALLB]) == L.EINVAL and set_([L.F_C, 0, -1, ALLB]) == L.EINVAL
    assert set_([L.F_PHI_M, 0, 0, ALLB]) == L.EINVAL and b"membrane" in lib.knpemi_last_error()
    assert set_([ok, ok]) == L.EINVAL and b"twice" in lib.knpemi_last_error()
    assert set_([L.F_C, 0, 0, L.MAPS_PEAK | L.MAPS_SERIES]) == L.EINVAL and set_([L.F_C, 0, 0, L.MAPS_PEAK | L.MAPS_BELOW]) == L.EINVAL
    assert set_([L.F_C, 0, 0, 0]) == L.EINVAL and set_([L.F_C, 0, 0, ALLB | 64]) == L.EINVAL
    assert set_(ok, thr=(np.nan,)) == L.EINVAL and set_(ok, thr=(np.inf,)) == L.EINVAL
    assert set_([L.F_C, 0, 0, ALLB | L.MAPS_SERIES], cap=0) == L.EINVAL and set_([L.F_C, 0, 0, ALLB | L.MAPS_SERIES], weight=None) == L.EINVAL
    nine = [[L.F_PHI, 0, 0, ALLB]] * (L.MAPS_MAX_PER_SPACE + 1)
    assert set_(nine, thr=np.arange(9.0)) == L.EINVAL and b"PER_SPACE" in lib.knpemi_last_error()
    assert lib.knpemi_maps_record(dp.h, float(t[4])) == L.EINVAL           # not greater than the previous record's
    assert lib.knpemi_maps_record(dp.h, float("nan")) == L.EINVAL
    nq = np.array([8], np.int32)
    ode = C.c_void_p()
    L.check(lib.knpemi_ode_create(dp.device, 1, L.iptr(nq), C.byref(ode)))
    assert set_(ok, h=ode) == L.EINVAL and b"has no fields" in lib.knpemi_last_error()
    lib.knpemi_destroy(ode)
    first = next(iter(host.watches.values()))
    buf = np.empty(first.n + 1)
    read = lambda j, which, n: lib.knpemi_maps_read(dp.h, j, which, buf.ctypes.data_as(C.c_void_p), n)      # noqa: E731
    have = {which for st in first.stats for _, which in STAT_MAPS[st]}
    for which in range(9):
        assert read(0, which, first.n) == (L.OK if which in have else L.EINVAL), which
    assert read(0, 9, first.n) == L.EINVAL and read(0, -1, first.n) == L.EINVAL
    assert read(len(watches), min(have), first.n) == L.EINVAL and read(-1, min(have), first.n) == L.EINVAL
    assert read(0, min(have), first.n + 1) == L.EINVAL and lib.knpemi_maps_read(dp.h, 0, min(have), None, first.n) == L.EINVAL
    # ... so a further record still matches
    ref = np.vstack([ref, run([5])])
    check(6)
    got, n_rows, dropped = _series(lib, dp, n_cols, reset=1)
    assert (n_rows, dropped) == (6, 0) and _series(lib, dp, n_cols)[1:] == (0, 0)
    mc.compare_series(host, got, ref, [mc.series_terms(host, play, k) for k in range(6)])
    # a table without a series has no buffer; a table of every statistic on eight watches of one space is accepted
    assert set_([L.F_PHI, 0, 0, L.MAPS_PEAK], thr=None, weight=None, cap=0) == L.OK
    assert lib.knpemi_maps_series_read(dp.h, 0, None, None, None, 0) == L.EINVAL and b"series" in lib.knpemi_last_error()
    L.check(lib.knpemi_maps_record(dp.h, 0.5))
    assert set_(nine[:8], thr=np.arange(8.0)) == L.OK
    L.check(lib.knpemi_maps_clear(dp.h))
    assert lib.knpemi_maps_record(dp.h, 1.0) == L.EINVAL and lib.knpemi_maps_reset(dp.h) == L.EINVAL
    assert read(0, 0, first.n) == L.EINVAL and lib.knpemi_maps_series_read(dp.h, 0, None, None, None, 0) == L.EINVAL


@pytest.mark.parametrize("kind", ["2d", "three"])
def test_unselected_statistics_are_not_touched(hip_lib, kind):
    """A watch with the peak only has no other array to read, and leaves the arrays of its neighbour in the space alone:
    the neighbour's maps equal, bit for bit, those of a run with the neighbour alone."""
    s, dp = _problem(kind)
    lib = dp.lib
    rng = np.random.default_rng(9)
    t, n = mc.record_times(rng), 12          # the first 12 of the 40 records the samples are planted for
    neighbour = ("Cl_all", "c", 0, "Cl", dict(threshold=mc.LEVEL, stats=mc.ALL, series=True))
    lean = ("K_peak", "c", 0, "K", dict(stats=("peak",)))
    out = {}
    for label, watches in (("both", [lean, neighbour]), ("alone", [neighbour])):
        fm = mc.field_maps(s, watches)
        play = mc.Play(mc.field_maps(s, [lean, neighbour]), np.random.default_rng(9), t)
        fm._attach(dp, 16)
        for k in range(n):
            play.push(dp, k)
            L.check(lib.knpemi_maps_record(dp.h, float(t[k])))
        out[label] = (fm.maps("Cl_all"), _series(lib, dp, 2)[0])
        if label == "both":
            m = fm.maps("K_peak")
            v = play.v[("c", 0, "K")][:n]
            assert set(m) == {"v_max", "t_max", "locations"} and np.array_equal(m["v_max"], np.nanmax(v, axis=0))
            assert np.array_equal(m["t_max"], t[:n][np.nanargmax(v, axis=0)])
            buf = np.empty(fm.watches["K_peak"].n)
            for which in range(2, 9):
                assert lib.knpemi_maps_read(dp.h, 0, which, buf.ctypes.data_as(C.c_void_p), buf.size) == L.EINVAL
        L.check(lib.knpemi_maps_clear(dp.h))
        fm._detach()
    assert out["both"][0]["count"].any() and out["both"][0]["excess"].any()
    for key, a in out["alone"][0].items():
        assert np.array_equal(a, out["both"][0][key], equal_nan=True), key
    assert out["alone"][1].shape == (n, 2) and np.array_equal(out["alone"][1], out["both"][1])


# ---- through the stepper -------------------------------------------------------------------------------------------
STEPS = 20


def _stepper(**kw):
    from test_events_gpu import _stepper as stepper
    s, st, _ = stepper(**kw)
    return s, st


def _steps(st, n, after=None):
    with mc.quiet():
        for k in range(n):
            st.step()
            if after is not None:
                after(k + 1)


@pytest.fixture(scope="module")
def level(hip_lib):
    """The level of ECS K+: the midpoint between the smallest and the largest per-vertex peak of one preliminary run of
    the same steps, as the events tests choose theirs.  In the oracle time loop (oracle/driver.py, direct solves, on the
    CPU) the per-vertex peaks of ECS K+ on this mesh after 20 steps differ: see the docstring of
    test_stepper_maps_match_downloads."""
    s, st = _stepper()
    top = np.full(s.c[0][0].x._a.shape, -np.inf)

    def after(k):
        st.download()
        np.maximum(top, s.c[0][0].x._a, out=top)
    _steps(st, STEPS, after)
    return 0.5 * (float(top.min()) + float(top.max())), top


def _watch(fm, thr):
    fm.watch("K_ecs", "c", tag=0, ion="K", threshold=thr, stats=mc.ALL, series=True)
    fm.watch("phi_M_1", "phi_M", tag=1, stats=("peak", "trough", "integral"))
    return fm


def _track_run(thr, every, **kw):
    """(set-up, stepper, device maps, host maps fed from a download after every recorded step, record times, series terms)."""
    s, st = _stepper(**kw)
    dev, host = _watch(FieldMaps(s.subdomain_list, s.ion_list), thr), _watch(FieldMaps(s.subdomain_list, s.ion_list), thr)
    st.track(dev, every=every, capacity=8)           # drained into the host series more than once at every=1
    times, terms = [], []

    def after(k):
        if k % every == 0:
            st.download()
            times.append(k * st.dt)
            host.record_host(times[-1], s.phi, s.c, s.phi_M_prev)
            beyond = s.c[0][0].x._a >= thr
            terms.append([(int(beyond.sum()), float(host.watches["K_ecs"].w[beyond].sum()))])
    return s, st, dev, host, times, terms, after


@pytest.mark.parametrize("every", [1, 3])
def test_stepper_maps_match_downloads(hip_lib, level, every):
    """20 steps of the 2d r = 1 problem with device solves.  The stimulated end of the cell releases K+ into the ECS next
    to it, so the per-vertex peaks of ECS K+ differ over the mesh within these steps: in the oracle time loop on the CPU
    (oracle/driver.py, direct solves) they lie in [3.32434, 3.32608] mM after 20 steps, from 3.32370 mM everywhere at
    the start, and 153 of the 256 ECS vertices reach their midpoint 3.32521 mM.  With the midpoint of the peaks as the
    level, some vertices are reached and some are not."""
    thr, top = level
    s, st, dev, host, times, terms, after = _track_run(thr, every)
    _steps(st, STEPS, after)
    ref = host.maps("K_ecs")
    if every == 1:      # the condition of the test: a vertex that is reached and one that is not, within the steps run
        assert (top >= thr).any() and (top < thr).any()
        assert (ref["count"] > 0).any() and (ref["count"] == 0).any()
    assert len(times) == STEPS // every
    for name in ("K_ecs", "phi_M_1"):
        mc.compare(dev.maps(name), host.maps(name), host.increment_sums(name), times)
    assert np.ptp(host.maps("phi_M_1")["v_max"]) > 0 or np.ptp(host.maps("phi_M_1")["integral"]) > 0
    got, want = dev.series(), host.series()
    assert list(got) == ["t", "K_ecs/measure", "K_ecs/n"] and got["t"].shape == (STEPS // every,)
    assert np.array_equal(got["t"], times)
    rows = lambda ser: np.stack([ser["K_ecs/measure"], ser["K_ecs/n"]], axis=1)      # noqa: E731
    mc.compare_series(host, rows(got), rows(want), terms)
    with pytest.raises(RuntimeError, match="already"):
        st.track(_watch(FieldMaps(s.subdomain_list, s.ion_list), thr))
    with pytest.raises(RuntimeError, match="attached"):
        dev.watch("late", "phi", tag=0)


def test_reset_gives_bit_identical_maps_and_series(hip_lib, level):
    """reset() and the same steps again: every map and the series bit for bit, so no state of the first run is left
    (extrapolate_guess=False: the extrapolated guess carries the solutions of the last steps across reset(), as
    test_events_gpu.test_reset_gives_bit_identical_maps explains)."""
    s, st, dev, host, times, terms, after = _track_run(level[0], 1, extrapolate_guess=False)
    _steps(st, STEPS)
    a = {name: dev.maps(name) for name in dev.watches}
    sa = dev.series()
    assert (a["K_ecs"]["count"] > 0).any() and (a["K_ecs"]["count"] == 0).any() and sa["t"].shape == (STEPS,)
    st.reset()
    _steps(st, STEPS)
    sb = dev.series()
    for name in a:
        b = dev.maps(name)
        for k in a[name]:
            assert np.array_equal(a[name][k], b[k], equal_nan=True), (name, k)
    for k in sa:
        assert sb[k].shape == (STEPS,) and np.array_equal(sa[k], sb[k]), k


def test_every_recorder_together_equals_each_alone(hip_lib, level):
    """observe, detect, fluxes, exchange and track on one stepper: the output of each equals its output when it is the
    only recorder attached, bit for bit."""
    from knpemi import IonFluxes, MembraneEvents, MembraneExchange
    from test_observables_gpu import _observables

    def attach(s, st, which):
        out = {}
        if "observe" in which:
            out["observe"] = _observables(s, (1,))
            st.observe(out["observe"])
        if "detect" in which:
            out["detect"] = MembraneEvents(s.subdomain_list)
            out["detect"].watch(1, -0.06, keep=2)
            st.detect(out["detect"])
        if "fluxes" in which:
            out["fluxes"] = IonFluxes(s.subdomain_list, s.ion_list, s.physical_parameters)
            for tag in s.subdomain_list:
                out["fluxes"].watch(tag)
            st.fluxes(out["fluxes"])
        if "exchange" in which:
            out["exchange"] = MembraneExchange(s.subdomain_list, s.ion_list, s.physical_parameters, ft=s.ft)
            out["exchange"].watch(1)
            st.exchange(out["exchange"])
        if "track" in which:
            out["track"] = _watch(FieldMaps(s.subdomain_list, s.ion_list), level[0])
            st.track(out["track"])
        return out

    def results(rec):
        out = {}
        for name, r in rec.items():
            if name == "detect":
                out[name] = r.maps(1)
            elif name == "track":
                out[name] = {f"{w}/{k}": v for w in r.watches for k, v in r.maps(w).items()}
                out[name].update(r.series())
            else:
                out[name] = r.series()
        return out

    names = ("observe", "detect", "fluxes", "exchange", "track")
    steps = 10
    alone = {}
    for name in names:
        s, st = _stepper()
        rec = attach(s, st, (name,))
        _steps(st, steps)
        alone[name] = results(rec)[name]
    s, st = _stepper()
    rec = attach(s, st, names)
    _steps(st, steps)
    both = results(rec)
    assert (both["track"]["K_ecs/v_max"] > s.c_prev[0][0].x._a.min()).any() and both["track"]["t"].shape == (steps,)
    for name in names:
        assert alone[name].keys() == both[name].keys(), name
        for k, v in alone[name].items():
            assert np.array_equal(v, both[name][k], equal_nan=v.dtype.kind == "f"), (name, k)
