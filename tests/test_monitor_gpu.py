"""GPU tests of the membrane monitors (knpemi_monitor_*, csrc/kernels_monitor.hip, DeviceStepper.monitor,
MembraneModel.monitor) against the host build of csrc/membrane_monitors.h (tests/native) and the numpy restatement
MembraneMonitor.compute_host, which tests/test_monitor_host.py pins to that host build.  TOL is relative to the sum of
the absolute values of a quantity's terms (test_monitor_host.restated), carried through the weights of a column."""
import contextlib
import functools
import io
import os
import sys

import numpy as np
import pytest

import exchange_cases as xc
import monitor_host as mh
from test_monitor_host import restated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "calibrate_initial_conditions"))
import run_calibration as rc  # noqa: E402

pytestmark = pytest.mark.gpu

MODELS = ["hh_si", "hh_mv", "glial"]
TOL = 1e-9       # device against host for another exp (tests/test_fixed_step_gpu.py:21)
OPS = ("average", "integral", "min", "max")
STEPS = 5


def _sizes():
    from knpemi import monitor
    d = monitor.fold_depth()
    return [1, 63, 64, 65, 257, d * 256, d * 256 + 5]


def _membrane(name, n):
    """Model `name` over n dofs with the sample tables of the host tests (rest, upstroke, peak, a seeded spread)."""
    module = rc.load_model(name)
    with contextlib.redirect_stdout(io.StringIO()):
        m = rc.make_membrane(module, n - 1, {}) if n > 1 else rc.make_membrane(module, 1, {})
    if n == 1:      # an interval mesh has two dofs at least: keep the first
        m.nodes, m.indices, m.dof_locations = 1, m.indices[:1], m.dof_locations[:1]
    y, p = mh.sample_tables(name, n, seed=n)
    m.states, m.parameters = y.copy(), p.copy()
    return module, m


def _scaled_err(model, t, y, p, dev):
    """Largest error of dev[(quantity, dof)] against the host build, relative to the terms' scale."""
    names = mh.names(model)
    ref = mh.evaluate(model, t, y, p)
    sc = restated(model, t, y, p)
    worst, bits = 0.0, True
    for i, n in enumerate(names):
        err = np.abs(dev[n] - ref[i]) / np.where(sc[n][1] > 0, sc[n][1], 1.0)
        worst = max(worst, float(err.max()))
        bits = bits and np.array_equal(dev[n], ref[i])
    return worst, bits


@pytest.mark.parametrize("name", MODELS)
def test_standalone_eval_matches_the_host_build(hip_lib, name):
    """knpemi_ode_create handles at the sizes that cover one lane, the wave and workgroup edges and many workgroups with a
    partly filled last one: MembraneModel.monitor against the host build per dof.  (knpemi_monitor_eval writes per-dof
    values only: the fold of the partials at these sizes is test_fold_of_the_partials_at_and_beyond_its_depth.)"""
    worst = 0.0
    for n in _sizes():
        _, m = _membrane(name, n)
        for t in mh.sample_times(name)[1:3]:
            dev = m.monitor(t=t)
            assert list(dev) == mh.names(name) and all(v.shape == (n,) for v in dev.values())
            err, _ = _scaled_err(name, t, m.states, m.parameters, dev)
            worst = max(worst, err)
            assert err <= TOL, (name, n, t, err)
    print(f"{name}: MembraneModel.monitor against the host build, worst {worst:.2e} of the terms' scale")
    # a selection keeps the caller's order, and the tables are not touched
    _, m = _membrane(name, 65)
    y0, p0 = m.states.copy(), m.parameters.copy()
    sel = m.monitor(names=["I_K", "E_K"], t=0.0)
    full = m.monitor(t=0.0)
    assert list(sel) == ["I_K", "E_K"] and all(np.array_equal(sel[k], full[k]) for k in sel)
    assert np.array_equal(m.states, y0) and np.array_equal(m.parameters, p0)
    with pytest.raises(ValueError, match="unknown quantity"):
        m.monitor(names=["E_Ca"])


@pytest.mark.parametrize("name", MODELS)
def test_totals_are_the_currents_handed_to_the_pdes(hip_lib, name):
    """After one euler step the fixed-step kernel has evaluated rhs at the end state and stored its currents: the
    monitor's totals at t0 + dt from the tables it left are those currents."""
    module, m = _membrane(name, 257)
    _, dt = rc.conditions(name)
    m.set_integrator("euler", 25)
    with contextlib.redirect_stdout(io.StringIO()):
        m.step(dt, {})
    dev = m.monitor(t=m.time)
    sc = restated(name, m.time, m.states, m.parameters)
    for ion in ("Na", "K", "Cl"):
        col = m.parameters[:, module.parameter_indices(f"I_ch_{ion}")]
        if f"I_{ion}" not in dev:
            assert (col == 0.0).all()
            continue
        err = float((np.abs(dev[f"I_{ion}"] - col) / sc[f"I_{ion}"][1]).max())
        print(f"{name} I_{ion}: {err:.2e} of the terms' scale; bits agree: {np.array_equal(dev[f'I_{ion}'], col)}")
        assert err <= TOL


# ---- PDE handles -----------------------------------------------------------------------------------------------------
def _stepper(s):
    from knpemi.stepper import DeviceStepper
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev)
    for tag in list(s.subdomain_list)[1:]:
        for mm in s.subdomain_list[tag]["mem_models"]:
            st.add_membrane_model(mm["ode"], {}, None)
    return st


def _monitor(s):
    """Every model of every cell watched, two points per watch, every reduction of every quantity."""
    from knpemi import MembraneMonitor
    mon = MembraneMonitor(s.subdomain_list, s.ion_list, ft=s.ft)
    for tag in list(s.subdomain_list)[1:]:
        mon.watch(tag)
        mem = s.subdomain_list[tag]["mesh_mem"]
        cells = np.asarray(mem.cells)
        for j, name in ((0, f"a{tag}"), (cells.shape[0] // 2, f"b{tag}")):
            X = np.asarray(mem.x)[cells[j]]
            w = np.array([0.5, 0.3, 0.15, 0.05])[:X.shape[0]]
            mon.point(name, tag, (w / w.sum()) @ X)
        for op in OPS:
            mon.reduce(f"{op}{tag}", tag, op=op)
    return mon


def _state(s):
    hs = xc.host_state(s)
    tables = {(tag, j): (mm["ode"].states.copy(), mm["ode"].parameters.copy())
              for tag in list(s.subdomain_list)[1:] for j, mm in enumerate(s.subdomain_list[tag]["mem_models"])}
    return dict(c=hs["c_prev"], phi_M=hs["phi_M_prev"], tables=tables), hs


def _everything(s):
    """Every field, phi_M, I_ch, state and parameter table of the downloaded problem, flat."""
    st, hs = _state(s)
    out = [hs["phi"][t] for t in hs["phi"]] + [a for t in hs["c_prev"] for a in hs["c_prev"][t]]
    out += [hs["phi_M_prev"][t] for t in hs["phi_M_prev"]]
    out += [a for t in hs["I_ch"] for mm in hs["I_ch"][t] for a in mm.values()]
    out += [a for k in st["tables"] for a in st["tables"][k]]
    out += [f.x._a.copy() for t in s.subdomain_list for f in s.c[t]]
    return out


@functools.lru_cache(maxsize=None)
def _run(name, attach=True, every=1, capacity=1024, second=False):
    """STEPS steps of the set-up `name` with the monitor attached (fields on); after every step the fields are downloaded
    and compute_host evaluates them.  Returns (set-up, monitor, series, [(t, values, row, state)], device values of the
    last record, everything downloaded at the end, series of a second run after reset())."""
    s = xc.build(name)
    for t in s.subdomain_list:          # the end-of-step update copies c into c_prev: start from c = c_prev, not from
        for k in range(len(s.c[t])):    # the random c of the perturbed set-ups (no physical state for a membrane model)
            s.c[t][k].x.array[:] = s.c_prev[t][k].x._a
    st = _stepper(s)
    mon = None
    if attach:
        mon = _monitor(s)
        st.monitor(mon, every=every, capacity=capacity, fields=True)
    seen, again = [], None
    collect = attach and every == 1 and capacity > STEPS and not second
    with contextlib.redirect_stdout(io.StringIO()):
        for k in range(STEPS):
            st.step()
            if collect:
                st.download()
                state, _ = _state(s)
                t = (k + 1) * float(s.dt)
                seen.append((t,) + mon.compute_host(t, state) + (state,))
        ser = mon.series() if attach else None
        dev_values = {key: mon.values(*key) for key in mon.watched} if attach else None
        if second:      # from the host objects, which nothing has downloaded into: the same start
            st.reset()
            for k in range(STEPS):
                st.step()
            again = mon.series()
        st.download()
    final = _everything(s)
    return s, mon, ser, seen, dev_values, final, again


def _column_scale(mon, ckey, kind, key, i, p, scales, w):
    from knpemi import _lib as L
    sc = scales[key][mon.names(*key)[i]]
    if kind == L.MON_POINT:
        _, _, q, pw = mon._points[p]
        return float(np.abs(pw) @ sc[q])
    on = w[key] > 0
    if kind == L.MON_INTEGRAL:
        return float(w[key][on] @ sc[on])
    if kind == L.MON_AVERAGE:
        return float(w[key][on] @ sc[on]) / float(w[key].sum())
    return float(sc[on].max())


@pytest.mark.parametrize("name", ["2d", "tet", "hex", "three"])
def test_series_and_values_match_the_restatement(hip_lib, name):
    s, mon, ser, seen, dev_values, _, _ = _run(name)
    n_watch = len(mon.watched)
    assert mon.n_cols == sum((2 + len(OPS)) * len(idx) for idx in mon.watched.values())
    if name == "three":
        assert n_watch == 2 and mon.n_cols > 64      # the last workgroup's fold spans more than one wave
    assert ser["t"].shape == (STEPS,) and np.allclose(ser["t"], [t for t, *_ in seen], rtol=1e-14, atol=0)
    w = {key: mon.weights(*key) for key in mon.watched}
    worst = 0.0
    for r, (t, values, row, state) in enumerate(seen):
        scales = {}
        for key in mon.watched:
            y, p = mon.rows_host(*key, state)
            scales[key] = {n: v[1] for n, v in restated(mon.model_id(*key), t, y, p).items()}
        for ckey, kind, key, i, p in mon._cols:
            # (a quantity whose terms are all zero -- g_stim without a stimulus -- has scale 0: any difference is an error)
            err = abs(ser[ckey][r] - row[ckey]) / (_column_scale(mon, ckey, kind, key, i, p, scales, w) or 1e-300)
            worst = max(worst, err)
            assert err <= TOL, (name, ckey, r, err)
    # the per-dof arrays of the latest record
    t, values, _, _ = seen[-1]
    for key in mon.watched:
        assert set(dev_values[key]) == set(values[key])
        for n, v in values[key].items():
            err = float((np.abs(dev_values[key][n] - v) / np.where(scales[key][n] > 0, scales[key][n], 1.0)).max())
            worst = max(worst, err)
            assert err <= TOL, (name, key, n, err)
    # the states moved: the series is not a constant
    assert any(np.ptp(ser[k]) > 0 for k, _ in mon.columns())
    print(f"{name}: series and values against compute_host, worst {worst:.2e} of the terms' scale")


@pytest.mark.parametrize("name", ["2d", "three"])
def test_the_monitor_changes_nothing(hip_lib, name):
    """The same steps with and without the monitor attached leave every field, phi_M, I_ch, state and parameter table
    bit-identical."""
    with_mon, without = _run(name)[5], _run(name, attach=False)[5]
    assert len(with_mon) == len(without)
    for a, b in zip(with_mon, without):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_series_buffer(hip_lib):
    """A second run after reset() repeats the series bit for bit; a capacity below the number of records drains with no
    row lost; every=2 halves the rows and carries the right times."""
    s, mon, ser, _, _, _, again = _run("2d", second=True)
    assert set(again) == set(ser)
    for k in ser:
        assert np.array_equal(ser[k].view(np.uint64), again[k].view(np.uint64)), k
    small = _run("2d", capacity=2)[2]
    for k in ser:
        assert np.array_equal(ser[k].view(np.uint64), small[k].view(np.uint64)), k
    half = _run("2d", every=2)[2]
    dt = float(s.dt)
    assert half["t"].shape == (STEPS // 2,) and np.allclose(half["t"], [2 * dt, 4 * dt], rtol=1e-14, atol=0)
    for k in ser:
        assert np.array_equal(half[k].view(np.uint64), ser[k][1::2][:STEPS // 2].view(np.uint64)), k


def test_refusals(hip_lib):
    import ctypes as C
    from knpemi import _lib as L
    s, mon, *_ = _run("2d")
    st = _stepper(xc.build("2d"))
    m2 = _monitor(xc.build("2d"))
    with pytest.raises(L.KnpemiError, match="no monitors set"):
        L.check(st.lib.knpemi_monitor_record(st.dp.h, 0.0, 0))
    # a refused set leaves the previous table alone
    st2 = _stepper(s)      # the problem of _run: its handle holds the monitor's table
    h, lib = st2.dp.h, st2.lib
    spec, ionp = np.array([1, 0, 1 << 25, 3], np.int32), np.zeros(6, np.int32)
    wts = np.ones(mon.n_dofs(1))
    for bad_spec, match in ((spec, "beyond the model's count"), (np.array([0, 0, 1, 3], np.int32), "ECS"),
                            (np.array([1, 3, 1, 3], np.int32), "out of range"), (np.array([1, 0, 0, 3], np.int32), "empty")):
        with pytest.raises(L.KnpemiError, match=match):
            L.check(lib.knpemi_monitor_set(h, 1, L.iptr(bad_spec), L.iptr(ionp), L.dptr(wts), 0, None, 0, None, None, None, 4))
    twice = np.array([1, 0, 1, 3, 1, 0, 2, 3], np.int32)
    ion2 = np.array([9, 10, 11, 12, 13, 14] * 2, np.int32)
    with pytest.raises(L.KnpemiError, match="listed twice"):
        L.check(lib.knpemi_monitor_set(h, 2, L.iptr(twice), L.iptr(ion2), L.dptr(np.concatenate([wts, wts])), 0, None, 0,
                                       None, None, None, 4))
    with pytest.raises(L.KnpemiError, match="finite"):
        L.check(lib.knpemi_monitor_record(h, float("nan"), 0))
    L.check(lib.knpemi_monitor_record(h, 1.0, 0))      # the table of _run is still there
    rows, over = C.c_int64(), C.c_int64()
    L.check(lib.knpemi_monitor_read(h, 0, None, C.byref(rows), C.byref(over), 1))
    assert rows.value == 1 and over.value == 0
    # partitioned steps are refused, naming the monitor
    st.monitor(m2)
    with pytest.raises(NotImplementedError, match="monitors"):
        st.step(halo=object())
    with pytest.raises(RuntimeError, match="already"):
        st.monitor(_monitor(xc.build("2d")))


def _plug_in_without_monitor():
    """examples/benchmark/mm_glial.py as a module that brings its right-hand side only."""
    import types
    full = rc.load_model("glial_benchmark")
    bare = types.ModuleType("mm_glial_bare")
    for k, v in vars(full).items():
        if k not in ("MONITOR_NAMES", "monitor", "monitor_indices") and not k.startswith("__"):
            setattr(bare, k, v)
    return bare


def test_a_slot_bound_from_source_has_no_monitor(hip_lib):
    """A plug-in that brings its own right-hand side and no monitor: names() is empty, monitor raises, and the library
    refuses the slot."""
    from knpemi import _lib as L
    module = _plug_in_without_monitor()
    with contextlib.redirect_stdout(io.StringIO()):
        m = rc.make_membrane(module, 4, rc.conditions("glial_benchmark")[0])
    assert m.monitor_names() == []
    with pytest.raises(ValueError, match="brings no monitor"):
        m.monitor()
    dp = m._device()
    out = np.zeros(m.nodes)
    with pytest.raises(L.KnpemiError, match="bound from source has no monitor"):
        L.check(dp.lib.knpemi_monitor_eval(dp.h, m._sub, m._model, 0.0, 1, None, None, None, 0, L.dptr(out), out.size))
    # a shipped model brings its monitor: no second one
    _, g = _membrane("glial", 5)
    gp = g._device()
    with pytest.raises(L.KnpemiError, match="not bound from source"):
        L.check(gp.lib.knpemi_monitor_bind_source(gp.h, g._sub, g._model, 1, b"x"))


def _benchmark_glial(n):
    """examples/benchmark/mm_glial.py (its own right-hand side and monitor through hipRTC) and the shipped glial model
    over n dofs with the same membrane potentials, concentrations, conductances and pump constants."""
    conds, _ = rc.conditions("glial_benchmark")
    plug, ship = rc.load_model("glial_benchmark"), rc.load_model("glial")
    with contextlib.redirect_stdout(io.StringIO()):
        a, b = rc.make_membrane(plug, n - 1, conds), rc.make_membrane(ship, n - 1, conds)
    rng = np.random.default_rng(11)
    V = rng.uniform(-95.0, -40.0, n)
    a.states[:, 0], b.states[:, 0] = V, V
    for name in ("K_e", "K_i", "Na_e", "Na_i", "Cl_e", "Cl_i"):
        f = rng.uniform(0.9, 1.1, n)
        a.parameters[:, plug.parameter_indices(name)] *= f
        b.parameters[:, ship.parameter_indices(name)] *= f
    return plug, a, b


def test_plug_in_monitor_through_hiprtc(hip_lib):
    """mm_glial.py: its Python `monitor`, translated by rhs_codegen and compiled as a program of its own, under the record
    kernel's body.  Per dof (knpemi_monitor_eval) it equals the module's own Python monitor in every quantity, and the
    shipped glial monitor where the two models coincide (the Nernst potentials, the pump and the leak currents, I_Na and
    I_Cl; the Kir factor has other constants).  Watched through knpemi_monitor_set on 700 dofs -- three workgroups of the
    plug-in's kernel -- the series row (a point, integral, average, min, max) equals numpy on those values and repeats."""
    import ctypes as C
    from knpemi import _lib as L
    n = 700
    plug, a, b = _benchmark_glial(n)
    names = a.monitor_names()
    assert names == plug.MONITOR_NAMES == mh.names("glial")
    dev, shipped = a.monitor(t=0.0), b.monitor(t=0.0)
    host = np.zeros((len(names), n))
    for q in range(n):
        plug.monitor(a.states[q], 0.0, a.parameters[q], host[:, q])
    sc = {k: v[1] for k, v in restated("glial", 0.0, b.states, b.parameters).items()}
    worst = 0.0
    for i, k in enumerate(names):
        err = float((np.abs(dev[k] - host[i]) / sc[k]).max())
        worst = max(worst, err)
        assert err <= TOL, (k, err)
    for k in ("E_Na", "E_K", "E_Cl", "i_pump", "i_Na_leak", "i_Cl_leak", "I_Na", "I_Cl"):
        err = float((np.abs(dev[k] - shipped[k]) / sc[k]).max())
        worst = max(worst, err)
        assert err <= TOL, (k, err)
    assert (np.abs(dev["g_Kir"] - shipped["g_Kir"]) > 1e-6 * np.abs(shipped["g_Kir"])).any()      # another model there
    print(f"mm_glial.py through hipRTC: worst {worst:.2e} of the terms' scale")
    # the series row of the plug-in's program
    dp = a._device()
    lib, h = dp.lib, dp.h
    L.check(lib.knpemi_ode_set_tables(h, a._sub, a._model, L.dptr(np.ascontiguousarray(a.states)),
                                      L.dptr(np.ascontiguousarray(a.parameters))))
    nq = len(names)
    w = np.where(np.arange(n) % 7 == 0, 0.0, 1.0 + 0.001 * np.arange(n))
    pt_q, pt_w = np.array([[3, 300, 699, -1]], np.int32), np.array([[0.5, 0.25, 0.25, 0.0]])
    cols = [(L.MON_POINT, 0, i, 0) for i in range(nq)]
    cols += [(kind, 0, i, 0) for kind in (L.MON_INTEGRAL, L.MON_AVERAGE, L.MON_MIN, L.MON_MAX_OP) for i in range(nq)]
    spec, col_spec = np.array([a._sub, a._model, (1 << nq) - 1, 0], np.int32), np.array(cols, np.int32)
    L.check(lib.knpemi_monitor_set(h, 1, L.iptr(spec), None, L.dptr(w), len(cols), L.iptr(col_spec), 1,
                                   L.iptr(np.zeros(1, np.int32)), L.iptr(pt_q), L.dptr(pt_w), 4))
    L.check(lib.knpemi_monitor_record(h, 0.0, 0))
    L.check(lib.knpemi_monitor_record(h, 0.0, 1))
    rows = np.full((2, len(cols)), np.nan)
    got, over = C.c_int64(), C.c_int64()
    L.check(lib.knpemi_monitor_read(h, 2, L.dptr(rows), C.byref(got), C.byref(over), 1))
    assert got.value == 2 and over.value == 0 and np.array_equal(rows[0].view(np.uint64), rows[1].view(np.uint64))
    on = w > 0
    for c, (kind, _, i, _) in enumerate(cols):
        v, s = host[i], sc[names[i]]
        if kind == L.MON_POINT:
            want, scale = float(pt_w[0, :3] @ v[pt_q[0, :3]]), float(pt_w[0, :3] @ s[pt_q[0, :3]])
        elif kind in (L.MON_INTEGRAL, L.MON_AVERAGE):
            d = float(w.sum()) if kind == L.MON_AVERAGE else 1.0
            want, scale = float(w[on] @ v[on]) / d, float(w[on] @ s[on]) / d
        else:
            want, scale = float(v[on].min() if kind == L.MON_MIN else v[on].max()), float(s[on].max())
        assert abs(rows[0, c] - want) <= TOL * scale, (c, kind, i)
    out = np.empty(n)
    L.check(lib.knpemi_monitor_fields(h, 0, 5, L.dptr(out), n))
    assert (np.abs(out - host[5]) <= TOL * sc["i_Kir"]).all()


# ---- the series row on stand-alone handles: the fold of the partials at and beyond its depth -------------------------
def _standalone_series(name, n, records=2):
    """knpemi_monitor_set on a handle of knpemi_ode_create: every quantity of the model over n dofs with seeded dof weights
    (a fifth of them zero), integral / average / min / max of each and two points.  Returns (column specs, point table,
    weights, sample tables, t, rows of `records` identical records, per-dof fields of the last one)."""
    import ctypes as C
    from knpemi import _lib as L
    module, m = _membrane(name, n)
    dp = m._device()
    lib, h = dp.lib, dp.h
    L.check(lib.knpemi_ode_set_tables(h, m._sub, m._model, L.dptr(m.states), L.dptr(m.parameters)))
    nq = len(mh.names(name))
    rng = np.random.default_rng(100 + n)
    w = np.where(rng.random(n) < 0.2, 0.0, rng.uniform(0.5, 1.5, n))
    pt_q = np.array([[0, n // 3, n // 2, n - 1], [n - 1, n // 5, -1, -1]], np.int32)
    pt_w = np.array([[0.4, 0.3, 0.2, 0.1], [0.75, 0.25, 0.0, 0.0]])
    pt_watch = np.zeros(2, np.int32)
    cols = [(L.MON_POINT, 0, i, p) for p in range(2) for i in range(nq)]
    cols += [(kind, 0, i, 0) for kind in (L.MON_INTEGRAL, L.MON_AVERAGE, L.MON_MIN, L.MON_MAX_OP) for i in range(nq)]
    spec = np.array([m._sub, m._model, (1 << nq) - 1, int(m.V_index)], np.int32)
    col_spec = np.array(cols, np.int32)
    L.check(lib.knpemi_monitor_set(h, 1, L.iptr(spec), None, L.dptr(w), len(cols), L.iptr(col_spec), 2, L.iptr(pt_watch),
                                   L.iptr(pt_q), L.dptr(pt_w), 8))
    t = mh.sample_times(name)[1]
    for r in range(records):
        L.check(lib.knpemi_monitor_record(h, t, 1 if r == records - 1 else 0))
    rows = np.full((records, len(cols)), np.nan)
    got, over = C.c_int64(), C.c_int64()
    L.check(lib.knpemi_monitor_read(h, records, L.dptr(rows), C.byref(got), C.byref(over), 1))
    assert got.value == records and over.value == 0
    fields = np.empty((nq, n))
    for i in range(nq):
        L.check(lib.knpemi_monitor_fields(h, 0, i, L.dptr(fields[i]), n))
    return cols, (pt_q, pt_w), w, m, t, rows, fields


@pytest.mark.parametrize("name", MODELS)
def test_fold_of_the_partials_at_and_beyond_its_depth(hip_lib, name):
    """n_q = D 256 (exactly `depth` workgroup partials: one full batch of the fold) and D 256 + 5 (a batch and a
    remainder): integral, average, minimum and maximum of every quantity and two points against numpy on the host
    build's per-dof values; a second record repeats the row bit for bit; the row does not depend on `fields`."""
    from knpemi import _lib as L
    from knpemi import monitor
    d = monitor.fold_depth()
    for n in (d * 256, d * 256 + 5):
        assert -(-n // 256) >= d
        cols, (pt_q, pt_w), w, m, t, rows, fields = _standalone_series(name, n)
        assert np.array_equal(rows[0].view(np.uint64), rows[1].view(np.uint64))
        ref = mh.evaluate(name, t, m.states, m.parameters)
        sc = [v[1] for v in (restated(name, t, m.states, m.parameters)[q] for q in mh.names(name))]
        on = w > 0
        worst = 0.0
        for i in range(len(ref)):
            scale = np.where(sc[i] > 0, sc[i], 1.0)
            assert (np.abs(fields[i] - ref[i]) <= TOL * scale).all()
        for c, (kind, _, i, p) in enumerate(cols):
            v, s = ref[i], sc[i]
            if kind == L.MON_POINT:
                q = pt_q[p][pt_q[p] >= 0]
                want, scale = float(pt_w[p][:len(q)] @ v[q]), float(np.abs(pt_w[p][:len(q)]) @ s[q])
            elif kind == L.MON_INTEGRAL:
                want, scale = float(w[on] @ v[on]), float(w[on] @ s[on])
            elif kind == L.MON_AVERAGE:
                want, scale = float(w[on] @ v[on]) / float(w.sum()), float(w[on] @ s[on]) / float(w.sum())
            else:
                want, scale = float(v[on].min() if kind == L.MON_MIN else v[on].max()), float(s[on].max())
            err = abs(rows[0, c] - want) / (scale or 1e-300)
            worst = max(worst, err)
            assert err <= TOL, (name, n, c, kind, i, err)
        print(f"{name} n_q = {n}: row against numpy on the host build, worst {worst:.2e} of the terms' scale")


def test_set_and_fields_refusals(hip_lib):
    """knpemi_monitor_set refuses an unbound model slot and a sub-domain without membrane dofs; knpemi_monitor_fields
    refuses a call before a record with fields, a quantity the watch does not select and a wrong length."""
    from knpemi import _lib as L
    from knpemi.odeSolver import OdeProblem
    spec, w = np.array([1, 0, 1, 0], np.int32), np.ones(4)
    unbound = OdeProblem([4])
    with pytest.raises(L.KnpemiError, match="not bound"):
        L.check(unbound.lib.knpemi_monitor_set(unbound.h, 1, L.iptr(spec), None, L.dptr(w), 0, None, 0, None, None, None, 4))
    empty = OdeProblem([0])
    L.check(empty.lib.knpemi_ode_bind(empty.h, 1, 0, L.MODEL_GLIAL, 1, 23))
    with pytest.raises(L.KnpemiError, match="no membrane dofs"):
        L.check(empty.lib.knpemi_monitor_set(empty.h, 1, L.iptr(spec), None, L.dptr(w), 0, None, 0, None, None, None, 4))
    _, m = _membrane("glial", 65)
    dp = m._device()
    lib, h = dp.lib, dp.h
    L.check(lib.knpemi_ode_set_tables(h, m._sub, m._model, L.dptr(m.states), L.dptr(m.parameters)))
    out = np.zeros(65)
    with pytest.raises(L.KnpemiError, match="no monitors set"):
        L.check(lib.knpemi_monitor_fields(h, 0, 1, L.dptr(out), 65))
    sel = np.array([m._sub, m._model, 0b110, 0], np.int32)      # E_K and E_Cl
    L.check(lib.knpemi_monitor_set(h, 1, L.iptr(sel), None, L.dptr(np.ones(65)), 0, None, 0, None, None, None, 4))
    L.check(lib.knpemi_monitor_record(h, 0.0, 0))
    with pytest.raises(L.KnpemiError, match="no record with fields yet"):
        L.check(lib.knpemi_monitor_fields(h, 0, 1, L.dptr(out), 65))
    L.check(lib.knpemi_monitor_record(h, 0.0, 1))
    with pytest.raises(L.KnpemiError, match="not selected"):
        L.check(lib.knpemi_monitor_fields(h, 0, 0, L.dptr(out), 65))
    with pytest.raises(L.KnpemiError, match="length"):
        L.check(lib.knpemi_monitor_fields(h, 0, 1, L.dptr(out[:64].copy()), 64))
    with pytest.raises(L.KnpemiError, match="bad watch"):
        L.check(lib.knpemi_monitor_fields(h, 1, 1, L.dptr(out), 65))
    L.check(lib.knpemi_monitor_fields(h, 0, 2, L.dptr(out), 65))
    ref = mh.evaluate("glial", 0.0, m.states, m.parameters)
    assert (np.abs(out - ref[2]) <= TOL * np.abs(ref[2])).all()
    L.check(lib.knpemi_monitor_reset(h))
    with pytest.raises(L.KnpemiError, match="no record with fields yet"):
        L.check(lib.knpemi_monitor_fields(h, 0, 1, L.dptr(out), 65))
    L.check(lib.knpemi_monitor_clear(h))
    with pytest.raises(L.KnpemiError, match="no monitors set"):
        L.check(lib.knpemi_monitor_record(h, 0.0, 0))


def test_shipped_and_plug_in_watches_in_one_record(hip_lib):
    """One handle, three slots -- shipped glial, mm_glial.py from source, shipped hh_mv -- watched in this order: a record
    is three launches (library, plug-in program, library) that share the partials, the ticket and the tail.  Every column
    equals the one the slot gives when it is watched alone, bit for bit, and a second record repeats the row."""
    import ctypes as C
    from knpemi import _lib as L
    from knpemi.odeSolver import OdeProblem
    from knpemi.rhs_codegen import hip_monitor_from_module, hip_source_from_module
    n = (300, 700, 257)
    plug, a, b = _benchmark_glial(n[1])
    tables = [mh.sample_tables("glial", n[0], seed=1), (np.ascontiguousarray(a.states), np.ascontiguousarray(a.parameters)),
              mh.sample_tables("hh_mv", n[2], seed=2)]
    counts = (11, 11, 19)

    def problem():
        dp = OdeProblem(list(n))
        L.check(dp.lib.knpemi_ode_bind(dp.h, 1, 0, L.MODEL_GLIAL, 1, 23))
        L.check(dp.lib.knpemi_ode_bind_source(dp.h, 2, 0, 1, 21, (plug.RHS_HIP or hip_source_from_module(plug)).encode()))
        L.check(dp.lib.knpemi_monitor_bind_source(dp.h, 2, 0, 11, hip_monitor_from_module(plug).encode()))
        L.check(dp.lib.knpemi_ode_bind(dp.h, 3, 0, L.MODEL_HH_MV, 4, 22))
        for s, (y, p) in enumerate(tables):
            L.check(dp.lib.knpemi_ode_set_tables(dp.h, 1 + s, 0, L.dptr(y), L.dptr(p)))
        return dp

    def rows_of(dp, watched, records=1):
        spec, wts, cols = [], [], []
        for k, s in enumerate(watched):
            spec += [1 + s, 0, (1 << counts[s]) - 1, 3 if s == 2 else 0]
            wts.append(1.0 + 0.01 * (np.arange(n[s]) % 13))
            cols += [(L.MON_POINT, k, i, k) for i in range(counts[s])]
            cols += [(kind, k, i, 0) for kind in (L.MON_INTEGRAL, L.MON_MIN, L.MON_MAX_OP) for i in range(counts[s])]
        spec, col_spec = np.array(spec, np.int32), np.array(cols, np.int32)
        pt_watch = np.arange(len(watched), dtype=np.int32)
        pt_q = np.array([[0, n[s] - 1, n[s] // 2, -1] for s in watched], np.int32)
        pt_w = np.tile([0.2, 0.3, 0.5, 0.0], (len(watched), 1))
        L.check(dp.lib.knpemi_monitor_set(dp.h, len(watched), L.iptr(spec), None, L.dptr(np.concatenate(wts)), len(cols),
                                          L.iptr(col_spec), len(watched), L.iptr(pt_watch), L.iptr(pt_q), L.dptr(pt_w), 4))
        for r in range(records):
            L.check(dp.lib.knpemi_monitor_record(dp.h, 0.7, r % 2))
        rows = np.full((records, len(cols)), np.nan)
        got, over = C.c_int64(), C.c_int64()
        L.check(dp.lib.knpemi_monitor_read(dp.h, records, L.dptr(rows), C.byref(got), C.byref(over), 1))
        assert got.value == records and over.value == 0
        return rows

    dp = problem()
    mixed = rows_of(dp, (0, 1, 2), records=2)
    assert np.isfinite(mixed).all() and np.array_equal(mixed[0].view(np.uint64), mixed[1].view(np.uint64))
    alone = np.concatenate([rows_of(dp, (s,))[0] for s in (0, 1, 2)])
    assert np.array_equal(mixed[0].view(np.uint64), alone.view(np.uint64))
