"""GPU tests of the DG recorders (knpemi_dg_observe_*, knpemi_dg_events_*, dg_jump_kernel; DGProblem.observe / detect /
record) against the numpy restatements of knpemi.dg_recording.

Tolerances are the project's: linear functionals and extrema 1e-13 of the column's largest magnitude (what
tests/test_observables_gpu.py holds device rows to); jump seminorms 1e-10 S, S the same sum with [u]^2 replaced by
u_T^2 + u_N^2 (the DG kernels' standing tolerance against the restatement: fast_rcp / fast_rsqrt are in play)."""
import ctypes as C

import numpy as np
import pytest

import dg_record_cases as R

pytestmark = pytest.mark.gpu

ZS = [1.0, -1.0, 2.0, -1.0]
PARAMS = dict(dt=0.05, F=1.3, psi=0.8, C_M=0.7)


def _ions(K):
    return [dict(name=f"i{k}", z=ZS[k], D=[1.0 + 0.3 * k, 0.6 + 0.2 * k]) for k in range(K)]


def _problem(kind, M, K=3):
    from knpemi.dg import DGProblem
    obs, (m, ct, ft) = R.observables(kind, M, K)
    dp = DGProblem(m, ct, ft, [0, 1], [1], n_ions=K)
    dp.set_params(PARAMS, _ions(K))
    return dp, obs


def _push_and_update(dp, K, seed):
    """A new random state on the device, then the end-of-step update; returns the fields the device then holds."""
    from test_dg_gpu import _random_state
    c_all, phi, phi_M, I_ch, _ = _random_state(dp, K, seed)
    for k, c in enumerate(c_all):
        dp.set_concentration(k, c)
    dp.set_potential(phi)
    dp.set_membrane_potential(phi_M)
    dp.update(np.stack([c.ravel() for c in c_all[:K - 1]]))
    return [dp.get_concentration(k) for k in range(K)], dp.get_potential(), dp.get_membrane_potential()


def _run_records(kind, M, K, seeds):
    dp, obs = _problem(kind, M, K)
    R.define_all(obs)
    dp.observe(obs)
    fields = []
    for j, seed in enumerate(seeds):
        fields.append(_push_and_update(dp, K, seed))
        dp.record(0.1 * (j + 1))
    ser = obs.series()
    rows = np.stack([ser[k] for k in obs.keys], axis=1)
    return dp, obs, ser, rows, fields


def _check_rows(obs, rows, fields):
    ref = np.stack([obs.evaluate_host(*f) for f in fields])
    tol = R.row_tolerances(obs, ref, fields)
    err = np.abs(rows - ref)
    for j, key in enumerate(obs.keys):
        print(f"{key:16s} |dev - host| {err[:, j].max():.3e}  tol {tol[j]:.3e}")
    bad = [(k, err[:, j].max(), tol[j]) for j, k in enumerate(obs.keys) if not (err[:, j] <= tol[j]).all()]
    assert not bad, bad


@pytest.mark.parametrize("K", [3, 4])
@pytest.mark.parametrize("kind,M,general", [("2d", 8, False), ("tet", 4, False), ("hex", 4, False), ("hex", 4, True),
                                            ("hex_jittered", 4, False)])
def test_rows_match_evaluate_host(hip_lib, kind, M, general, K, monkeypatch):
    """Three records with a new random state pushed and updated between them, every kind of observable defined, the jump
    seminorms of phi and of the eliminated ion in both sub-domains included."""
    if general:
        monkeypatch.setenv("KNPEMI_DG_HEX_GENERAL", "1")
    else:
        monkeypatch.delenv("KNPEMI_DG_HEX_GENERAL", raising=False)
    dp, obs, ser, rows, fields = _run_records(kind, M, K, (1, 2, 3))
    assert np.array_equal(ser["t"], [0.1 * (j + 1) for j in range(3)]) and rows.shape == (3, len(obs.keys))
    _check_rows(obs, rows, fields)
    for key in R.jump_keys(obs):
        assert (ser[key] > 0).all(), key


def test_multi_workgroup_folds_are_exact_and_reproducible(hip_lib):
    """Tetrahedra M = 8: 3072 cells -- the ECS reductions span more than four observe chunks with a remainder, the jump
    kernel runs 48 workgroups, the events 576 membrane nodes.  Rows and maps match the host; two identical runs are
    bit-identical."""
    from knpemi.dg_recording import DGMembraneEvents
    from test_events_gpu import _compare
    out = []
    for rep in range(2):
        dp, obs = _problem("tet", 8)
        R.define_all(obs)
        ev = DGMembraneEvents(obs.mesh, R.facet_marker(obs), [1])
        ev.watch(0.0, reset=-0.005, keep=2)               # phi_M = phi_i - phi_e of the random states: +-0.02
        ref = DGMembraneEvents(obs.mesh, R.facet_marker(obs), [1])
        ref.watch(0.0, reset=-0.005, keep=2)
        dp.observe(obs)
        dp.detect(ev)
        fields, ts = [], []
        for j, seed in enumerate((1, 2, 3, 4)):
            fields.append(_push_and_update(dp, 3, seed))
            ts.append(0.1 * (j + 1))
            dp.record(ts[-1])
            ref.record_host(ts[-1], fields[-1][2])
        ser = obs.series()
        rows = np.stack([ser[k] for k in obs.keys], axis=1)
        maps = ev.maps()
        if rep == 0:
            chunk = 256 * 8                              # OBS_CHUNK of csrc/kernels_observe.hip: entries per workgroup
            n_ecs = int((obs.cell_sub == 0).sum()) * obs.nv
            assert obs.n_cells == 3072 and n_ecs > 4 * chunk and n_ecs % chunk and obs.nq == 576
            _check_rows(obs, rows, fields)
            _compare(maps, ref.maps(), ts)
            assert maps["count"].shape == (192, 3) and maps["count"].max() >= 1
        out.append((rows, maps))
    assert np.array_equal(out[0][0], out[1][0])
    for k in ("count", "t_first", "t_last", "v_peak", "t_peak", "times"):
        assert np.array_equal(out[0][1][k], out[1][1][k], equal_nan=True), k


@pytest.mark.parametrize("kind,M", [("2d", 8), ("hex_jittered", 4)])
def test_penalty_identity_ties_the_jump_to_the_assembled_operator(hip_lib, kind, M):
    """With concentrations constant per sub-domain kappa_s is constant, so the potential matrices assembled at gamma = 20
    and gamma = 10 differ by 10 sum_s kappa_s times the bilinear form of J_s: u^T (A_20 - A_10) u = 10 sum_s kappa_s
    J_s(u) for any broken u, with the membrane present.  1e-10 relative."""
    dp, obs = _problem(kind, M)
    ions = _ions(3)
    conc = [[2.0, 1.5], [3.0, 0.7], [1.2, 2.4]]
    for k in range(3):
        dp.set_concentration(k, np.where(dp.cell_sub[:, None] > 0, conc[k][1], conc[k][0]) * np.ones((1, dp.nv)))
    rng = np.random.default_rng(7)
    dp.set_membrane_potential(0.2 + 0.1 * rng.random((dp.nmf, dp.nf)))
    u = rng.standard_normal((dp.n_cells, dp.nv))
    dp.set_potential(u)
    A = {}
    for gamma in (10.0, 20.0):
        dp.set_params(PARAMS, ions, gamma=gamma)
        dp.assemble_emi()
        A[gamma] = dp.matrix(0)
    for tag in (0, 1):
        obs.jump(f"J{tag}", "phi", tag)
    dp.observe(obs)
    dp.record(1.0)
    ser = obs.series()
    kappa = [PARAMS["F"] * PARAMS["psi"] * sum(i["z"] ** 2 * i["D"][s] * conc[k][s] for k, i in enumerate(ions)) for s in (0, 1)]
    lhs = float(u.ravel() @ ((A[20.0] - A[10.0]) @ u.ravel()))
    rhs = 10.0 * sum(kappa[s] * ser[f"J{s}"][0] for s in (0, 1))
    print(f"{kind}: u^T (A_20 - A_10) u = {lhs:.15e}, 10 sum kappa J = {rhs:.15e}, relative difference {abs(lhs - rhs) / abs(rhs):.3e}")
    assert abs(lhs - rhs) <= 1e-10 * abs(rhs)


def test_events_on_the_device_follow_record_host(hip_lib):
    """A synthetic phi_M sequence through set_membrane_potential + record(t): counts, peaks and the NaN pattern exactly,
    crossing times within the bound of tests/test_events_gpu.py; reset restores the first-record state."""
    from knpemi.dg_recording import DGMembraneEvents
    from test_events_gpu import _compare
    dp, obs = _problem("tet", 4)
    ev = DGMembraneEvents(obs.mesh, R.facet_marker(obs), [1])
    ref = DGMembraneEvents(obs.mesh, R.facet_marker(obs), [1])
    for e in (ev, ref):
        e.watch(0.3, reset=-0.2, keep=3)
    dp.detect(ev)
    with pytest.raises(RuntimeError, match="already"):
        dp.detect(DGMembraneEvents(obs.mesh, R.facet_marker(obs), [1]))
    rng = np.random.default_rng(3)
    shape = (dp.nmf, dp.nf)
    A, f, ph = rng.uniform(0.5, 1.5, shape), rng.uniform(50.0, 400.0, shape), rng.uniform(0.0, 2 * np.pi, shape)
    ts = [1e-3 * (k + 1) for k in range(14)]
    for k, t in enumerate(ts):
        v = A * np.sin(2 * np.pi * f * t + ph)
        if k == 6:
            v[::5, 0] = np.nan
        dp.set_membrane_potential(v)
        dp.record(t)
        ref.record_host(t, v)
    got, want = ev.maps(), ref.maps()
    assert got["count"].shape == shape and got["count"].max() >= 2 and got["times"].shape == shape + (3,)
    _compare(got, want, ts)
    assert np.array_equal(ev.fired(), want["count"] > 0)
    from knpemi import _lib as L
    with pytest.raises(L.KnpemiError, match="greater than the previous"):
        L.check(dp.lib.knpemi_dg_events_record(dp.h, ts[-1]))
    with pytest.raises(L.KnpemiError, match="must be finite"):
        L.check(dp.lib.knpemi_dg_events_record(dp.h, float("nan")))
    dp.reset_recorders()
    fresh = ev.maps()
    assert (fresh["count"] == 0).all() and np.isnan(fresh["v_peak"]).all() and np.isnan(fresh["times"]).all()
    ref.reset_host()
    v = A * np.sin(ph)
    dp.set_membrane_potential(v)
    dp.record(ts[0])                                     # an earlier time is a first record again
    ref.record_host(ts[0], v)
    _compare(ev.maps(), ref.maps(), ts[:2])


def test_series_mechanics_and_refusals(hip_lib):
    """Capacity and dropped rows, rewind by read(reset=1), refused sets that leave the previous recorder recording, record
    before set / before set_params, destroy with recorders attached."""
    from knpemi import _lib as L
    from knpemi.dg import DGProblem
    dp, obs = _problem("2d", 8)
    lib, h = dp.lib, dp.h
    assert lib.knpemi_dg_observe_record(h) == L.EINVAL and b"no observables set" in lib.knpemi_last_error()
    assert lib.knpemi_dg_events_record(h, 0.0) == L.EINVAL and b"no events set" in lib.knpemi_last_error()
    obs.point("p", [0.1, 0.1], tag=0)
    obs.reduce("m", "phi", 1, "max")
    obs.jump("J", "phi", 0)
    obs.upload(dp, 4)
    fields = _push_and_update(dp, 3, 1)
    want = obs.evaluate_host(*fields)
    for _ in range(6):
        L.check(lib.knpemi_dg_observe_record(h))

    def read(n, reset):
        buf, rows, over = np.zeros((max(n, 1), obs.n_cols)), C.c_int64(), C.c_int64()
        L.check(lib.knpemi_dg_observe_read(h, n, L.dptr(buf), C.byref(rows), C.byref(over), reset))
        return buf[:min(n, rows.value)], rows.value, over.value

    def tol(want, fields):                               # one row: 1e-13 of the value, 1e-10 S for the jump
        return np.where(np.array(obs.keys) == "J", 1e-10 * obs.jump_host(fields[1], 0, squares=True), 1e-13 * np.abs(want))
    buf, rows, over = read(6, 1)
    assert (rows, over) == (4, 2) and buf.shape[0] == 4 and all(np.array_equal(buf[0], r) for r in buf)
    assert (np.abs(buf[0] - want) <= tol(want, fields)).all()
    assert read(6, 0)[1:] == (0, 0)
    # refused sets: the name in the message, the previous recorder still records the next row
    spec, ptr, idx, w, denom = obs.table()
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    bad_idx = idx.copy()
    bad_idx[0] = dp.n
    assert lib.knpemi_dg_observe_set(h, len(obs.items), L.iptr(spec.ravel()), p64(ptr), L.iptr(bad_idx), L.dptr(w),
                                     L.dptr(denom), 4) == L.EINVAL
    assert b"knpemi_dg_observe_set" in lib.knpemi_last_error() and b"index out of range" in lib.knpemi_last_error()
    bad_w = w.copy()
    bad_w[1] = np.nan
    assert lib.knpemi_dg_observe_set(h, len(obs.items), L.iptr(spec.ravel()), p64(ptr), L.iptr(idx), L.dptr(bad_w),
                                     L.dptr(denom), 4) == L.EINVAL
    assert b"knpemi_dg_observe_set" in lib.knpemi_last_error() and b"not finite" in lib.knpemi_last_error()
    bad_spec = spec.copy()
    bad_spec[0, 3] = 7
    assert lib.knpemi_dg_observe_set(h, len(obs.items), L.iptr(bad_spec.ravel()), p64(ptr), L.iptr(idx), L.dptr(w),
                                     L.dptr(denom), 4) == L.EINVAL and b"unknown op" in lib.knpemi_last_error()
    fields = _push_and_update(dp, 3, 2)
    L.check(lib.knpemi_dg_observe_record(h))
    buf, rows, over = read(1, 1)
    want = obs.evaluate_host(*fields)
    assert (rows, over) == (1, 0) and (np.abs(buf[0] - want) <= tol(want, fields)).all()
    L.check(lib.knpemi_dg_observe_clear(h))
    assert lib.knpemi_dg_observe_record(h) == L.EINVAL and b"no observables set" in lib.knpemi_last_error()
    # the handle stays usable; a second attachment is refused by name
    dp.observe(obs, capacity=4)
    with pytest.raises(RuntimeError, match="already"):
        dp.observe(obs)
    for j in range(6):                                   # the tap drains a full buffer: nothing is dropped
        dp.record(float(j + 1))
    assert obs.series()["t"].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    # before knpemi_dg_set_params
    m, ct, ft = R.mesh("2d", 4)
    raw = DGProblem(m, ct, ft, [0, 1], [1])
    o2 = R.observables("2d", 4)[0]
    o2.reduce("m", "phi", 0, "min")
    o2.upload(raw, 2)
    assert lib.knpemi_dg_observe_record(raw.h) == L.EINVAL and b"knpemi_dg_set_params" in lib.knpemi_last_error()
    # destroy with recorders attached
    del raw, dp


def test_driver_series_and_events(hip_lib, tmp_path, resolution=1):
    """DGRun with --series and --events: 5 steps, 5 rows, finite values, t as stepped, and the membrane point's phi_M equal
    to the facet-node values the driver downloads at the last step.  (Resolution 1: the mesh of resolution 0 does not
    resolve the cell, it has no intracellular point and no membrane.)"""
    import run_2D_dg as D
    spath, epath = str(tmp_path / "s.npz"), str(tmp_path / "e.npz")
    run = D.DGRun(resolution, series=spath, events=epath)
    ts = []
    for _ in range(5):
        run.step()
        ts.append(run.time)
    run.save()
    s, e = np.load(spath), np.load(epath)
    assert np.array_equal(s["t"], ts)
    for key in s.files:
        assert s[key].shape == (5,) and np.isfinite(s[key]).all(), key
    for key in ("ECS/phi", "ICS/K", "mem/phi_M", "mem/Na_e", "K_ecs_max", "K_ecs_avg", "J_phi_ecs", "J_K_ics"):
        assert key in s.files, key
    f, w = run.obs.membrane_weights(D.FIGURE_POINTS["mem"], 1)
    v = float(np.dot(w, run.dp.get_membrane_potential()[f]))
    assert abs(s["mem/phi_M"][-1] - v) <= 1e-13 * abs(v)
    assert e["count"].shape == (run.dp.nmf, run.dp.nf) and e["times"].shape == (run.dp.nmf, run.dp.nf, 8)
