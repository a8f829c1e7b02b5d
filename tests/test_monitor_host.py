"""CPU tests of the membrane monitors: the host build of csrc/membrane_monitors.h (tests/native) against a numpy
restatement written here from membrane_models.h, its totals against the models' own right-hand sides bit for bit, the
identities between the mechanisms and the totals, the gates against `rates`; and the Python layer of knpemi.monitor that
needs no device."""
import numpy as np
import pytest

import exchange_cases as xc
import fixed_step_host as fsh
import monitor_host as mh

MODELS = ["hh_si", "hh_mv", "glial"]
TOL = 1e-12      # relative to the sum of the absolute values of a quantity's terms (test_fixed_step_host.py:196)
N_ROWS = 96


# ---- the restatement: name -> (value, scale), scale = the sum of the absolute values of the quantity's terms ----------
def restated(model, t, y, p):
    a = np.abs
    out = {}
    if model in ("hh_si", "hh_mv"):
        si = model == "hh_si"
        m, h, n, V = y.T
        gNa, gK, glNa, glK, stim = p[:, 0], p[:, 1], p[:, 2], p[:, 3], p[:, 8]
        E_Na = np.log(p[:, 11] / p[:, 12]) / (p[:, 21] * p[:, 19])
        E_K = np.log(p[:, 9] / p[:, 10]) / (p[:, 21] * p[:, 19])
        i_pump = p[:, 6] / ((1 + p[:, 4] / p[:, 9]) ** 2 * (1 + p[:, 5] / p[:, 12]) ** 3)
        period, tau, t_end = (0.03, 0.002, 0.125) if si else (30.0, 2.0, 125.0)
        g_Na, g_K = gNa * h * m ** 3, gK * n ** 4
        g_stim = stim * np.exp(-np.fmod(t, period) / tau) * float(t < t_end)
        k = 1e3 if si else 1.0
        u = k * (V + 65.0 / k)
        am, bm = k * 0.1 * (25. - u) / (np.exp((25. - u) / 10.) - 1), k * 4. * np.exp(-u / 18.)
        ah, bh = k * 0.07 * np.exp(-u / 20.), k / (np.exp((30. - u) / 10.) + 1)
        an, bn = k * 0.01 * (10. - u) / (np.exp((10. - u) / 10.) - 1.), k * 0.125 * np.exp(-u / 80.)
        dNa, dK = a(V) + a(E_Na), a(V) + a(E_K)
        out.update(E_Na=(E_Na, a(E_Na)), E_K=(E_K, a(E_K)), i_pump=(i_pump, a(i_pump)), g_Na=(g_Na, a(g_Na)),
                   g_K=(g_K, a(g_K)), g_stim=(g_stim, a(g_stim)),
                   i_Na_leak=(glNa * (V - E_Na), glNa * dNa), i_Na_gated=(g_Na * (V - E_Na), g_Na * dNa),
                   i_stim=(g_stim * (V - E_Na), g_stim * dNa), i_K_leak=(glK * (V - E_K), glK * dK),
                   i_K_gated=(g_K * (V - E_K), g_K * dK),
                   I_Na=((glNa + g_Na + g_stim) * (V - E_Na) + 3 * i_pump, (glNa + g_Na + g_stim) * dNa + 3 * a(i_pump)),
                   I_K=((glK + g_K) * (V - E_K) - 2 * i_pump, (glK + g_K) * dK + 2 * a(i_pump)))
        for g, al, be in (("m", am, bm), ("h", ah, bh), ("n", an, bn)):
            out[f"{g}_inf"] = (al / (al + be), a(al / (al + be)))
            out[f"tau_{g}"] = (1.0 / (al + be), a(1.0 / (al + be)))
        return out
    V = y[:, 0]
    glCl, glNa, glK = p[:, 0], p[:, 1], p[:, 2]
    E_Na = np.log(p[:, 15] / p[:, 16]) / (p[:, 22] * p[:, 20])
    E_K = np.log(p[:, 13] / p[:, 14]) / (p[:, 22] * p[:, 20])
    E_Cl = np.log(p[:, 17] / p[:, 18]) / (p[:, 22] * p[:, 21])
    i_pump = p[:, 10] * (p[:, 13] / (p[:, 13] + p[:, 8])) * (p[:, 16] ** 1.5 / (p[:, 16] ** 1.5 + p[:, 9] ** 1.5))
    E_K_init = 8.315e3 * 307e3 / 96500e3 * np.log(p[:, 11] / p[:, 12])
    gfac = np.sqrt(p[:, 13] / p[:, 11]) * (1 + np.exp(18.5 / 42.4)) * (1 + np.exp(-(118.6 + E_K_init) / 44.1))
    g_Kir = gfac / ((1 + np.exp((V - E_K + 18.5) / 42.4)) * (1 + np.exp(-(118.6 + V) / 44.1)))
    i_Kir = glK * g_Kir * (V - E_K)
    dNa, dK, dCl = a(V) + a(E_Na), a(V) + a(E_K), a(V) + a(E_Cl)
    out.update(E_Na=(E_Na, a(E_Na)), E_K=(E_K, a(E_K)), E_Cl=(E_Cl, a(E_Cl)), i_pump=(i_pump, a(i_pump)),
               g_Kir=(g_Kir, a(g_Kir)), i_Kir=(i_Kir, glK * g_Kir * dK), i_Na_leak=(glNa * (V - E_Na), glNa * dNa),
               i_Cl_leak=(glCl * (V - E_Cl), glCl * dCl), I_Na=(glNa * (V - E_Na) + 3 * i_pump, glNa * dNa + 3 * a(i_pump)),
               I_K=(i_Kir - 2 * i_pump, glK * g_Kir * dK + 2 * a(i_pump)), I_Cl=(glCl * (V - E_Cl), glCl * dCl))
    return out


@pytest.fixture(scope="module", params=MODELS)
def case(request):
    """(model, names, [(t, states, params, host values, restatement)]) -- computed once per model."""
    model = request.param
    y, p = mh.sample_tables(model, N_ROWS)
    runs = [(t, y, p, mh.evaluate(model, t, y, p), restated(model, t, y, p)) for t in mh.sample_times(model)]
    return model, mh.names(model), runs


def test_counts_and_names(case):
    model, names, _ = case
    assert len(names) == {"hh_si": 19, "hh_mv": 19, "glial": 11}[model] and len(set(names)) == len(names)
    assert len(names) <= 32


def test_host_build_matches_numpy(case):
    model, names, runs = case
    worst = 0.0
    for t, y, p, v, ref in runs:
        assert set(ref) == set(names)
        for i, name in enumerate(names):
            want, scale = ref[name]
            assert np.isfinite(v[i]).all()
            err = np.abs(v[i] - want) / np.where(scale > 0, scale, 1.0)
            worst = max(worst, float(err.max()))
            assert err.max() <= TOL, (model, name, t, float(err.max()))
    print(f"{model}: host build against numpy, worst {worst:.2e} of the terms' scale")


def test_the_samples_cover_rest_upstroke_and_peak(case):
    model, _, runs = case
    V = runs[0][1][:, -1] / mh.UNITS[model][1]
    assert V.min() < -60.0 and V.max() > 20.0 and ((V > -50.0) & (V < 0.0)).any()


def test_totals_are_the_currents_of_rhs_bit_for_bit(case):
    model, names, runs = case
    for t, y, p, v, _ in runs:
        cur = mh.currents(model, t, y, p)
        for j, name in enumerate(("I_Na", "I_K", "I_Cl")):
            if name in names:
                assert np.array_equal(v[names.index(name)].view(np.uint64), cur[j].view(np.uint64)), (model, name, t)
            else:
                assert model != "glial" and np.all(cur[j] == 0.0)


def test_mechanisms_add_up_to_the_totals(case):
    model, names, runs = case
    for t, y, p, v, ref in runs:
        q = dict(zip(names, v))
        if model == "glial":
            sums = {"I_Na": q["i_Na_leak"] + 3 * q["i_pump"], "I_K": q["i_Kir"] - 2 * q["i_pump"], "I_Cl": q["i_Cl_leak"]}
        else:
            sums = {"I_Na": q["i_Na_leak"] + q["i_Na_gated"] + q["i_stim"] + 3 * q["i_pump"],
                    "I_K": q["i_K_leak"] + q["i_K_gated"] - 2 * q["i_pump"]}
        for name, s in sums.items():
            assert (np.abs(s - q[name]) <= TOL * ref[name][1]).all(), (model, name, t)


def test_gates_against_rates(case):
    model, names, runs = case
    if model == "glial":
        assert not any(n.endswith("_inf") or n.startswith("tau_") for n in names)
        return
    t, y, p, v, _ = runs[1]
    q = dict(zip(names, v))
    lib = fsh.load()
    for r in range(y.shape[0]):
        a, b = np.zeros(4), np.zeros(4)
        lib.fixed_step_host_rates(fsh.MODEL_ID[model], t, fsh._ptr(y[r].copy()), fsh._ptr(p[r].copy()), fsh._ptr(a), fsh._ptr(b))
        for i, g in enumerate("mhn"):
            assert q[f"{g}_inf"][r] == a[i] / (a[i] + b[i]) and q[f"tau_{g}"][r] == 1.0 / (a[i] + b[i])
    assert (q["m_inf"] > 0).all() and (q["m_inf"] < 1).all()


# ---- the Python layer ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three():
    return xc.build("three", forms=False)


def _monitor(s):
    from knpemi import MembraneMonitor
    return MembraneMonitor(s.subdomain_list, s.ion_list, ft=s.ft)


def _membrane_point(s, tag, j):
    mem = s.subdomain_list[tag]["mesh_mem"]
    X = np.asarray(mem.x)[np.asarray(mem.cells)[j]]
    w = np.array([0.5, 0.3, 0.2, 0.0])[:X.shape[0]]
    return (w / w.sum()) @ X


def test_catalogue_comes_from_the_library(hip_lib, three):
    from knpemi import monitor as km
    for model in MODELS:
        names = km.catalogue(model)
        assert names == mh.names(model)
        assert hip_lib.knpemi_monitor_count(mh.MODEL_ID[model]) == len(names)
        assert hip_lib.knpemi_monitor_name(mh.MODEL_ID[model], len(names)) is None
    assert hip_lib.knpemi_monitor_count(7) == 0 and km.catalogue("other") == [] and km.catalogue(None) == []
    mon = _monitor(three)
    assert mon.names(1) == mh.names("hh_si") and mon.names(2) == mh.names("glial")
    assert not hasattr(km, "NAMES")      # no second copy of the names in Python


def test_validation(hip_lib, three):
    mon = _monitor(three)
    with pytest.raises(ValueError, match="ECS"):
        mon.watch(0)
    with pytest.raises(ValueError, match="no sub-domain"):
        mon.watch(9)
    with pytest.raises(ValueError, match="no membrane model"):
        mon.watch(1, model=1)
    with pytest.raises(ValueError, match="unknown quantity"):
        mon.watch(1, quantities=("E_Cl",))      # the HH model has no chloride
    with pytest.raises(ValueError, match="not watched"):
        mon.point("p", 1, _membrane_point(three, 1, 0))
    mon.watch(1, quantities=("E_K", "I_Na"))
    with pytest.raises(ValueError, match="watched already"):
        mon.watch(1)
    with pytest.raises(ValueError, match="does not watch"):
        mon.reduce("r", 1, quantities=("E_Na",))
    with pytest.raises(ValueError, match="unknown op"):
        mon.reduce("r", 1, op="median")
    mon.reduce("r", 1)
    with pytest.raises(ValueError, match="taken"):
        mon.reduce("r", 1, op="max")
    with pytest.raises(ValueError, match="not in"):
        mon.point("far", 1, np.array([1.0, 1.0, 1.0]))
    with pytest.raises(RuntimeError, match="not attached"):
        mon.values(1)
    mon._dev = (None, None)      # as after DeviceStepper.monitor
    for define in (lambda: mon.watch(2), lambda: mon.reduce("s", 1), lambda: mon.point("p", 1, _membrane_point(three, 1, 0))):
        with pytest.raises(RuntimeError, match="attached"):
            define()


def test_a_model_without_a_monitor_cannot_be_watched(hip_lib, three, monkeypatch):
    """A plug-in that brings its own right-hand side (no MODEL_ID of a shipped model) has no monitor: names() is empty
    and watch raises."""
    mm = three.subdomain_list[2]["mem_models"][0]["ode"]
    plug_in = type("PlugIn", (), {"RHS_HIP": "...", "parameter_indices": staticmethod(mm.ode.parameter_indices)})
    monkeypatch.setattr(mm, "ode", plug_in)
    monkeypatch.setattr(mm, "_monitor_cache", None)      # (the names are cached per model)
    mon = _monitor(three)
    assert mon.names(2) == [] and mon.model_id(2) is None and mon.names(1)
    with pytest.raises(ValueError, match="brings no monitor"):
        mon.watch(2)


def test_column_order(hip_lib, three):
    mon = _monitor(three)
    mon.watch(2, quantities=("i_pump", "E_K", "i_Kir"))      # kept in the catalogue's order
    mon.watch(1)
    mon.point("glia", 2, _membrane_point(three, 2, 3))
    mon.reduce("mean", 2, op="average", quantities=("i_pump", "E_K"))
    mon.reduce("top", 1, op="max", quantities=("I_K",))
    assert [k for k, w in mon.columns()] == ["glia/E_K", "glia/i_pump", "glia/i_Kir", "mean/E_K", "mean/i_pump", "top/I_K"]
    assert all(w == 1 for _, w in mon.columns()) and mon.n_cols == 6
    assert mon.mask(2) == (1 << 1) | (1 << 3) | (1 << 5) and mon.mask(1) == (1 << 19) - 1


def _state(s):
    hs = xc.host_state(s)
    return dict(c=hs["c_prev"], phi_M=hs["phi_M_prev"])


def test_record_host_against_a_per_dof_evaluation(hip_lib, three):
    """compute_host on the "three" set-up (hh_si on cell 1, glial on cell 2): per-dof values against the host build fed
    with rows built here by the rule (traces into the ion columns, V = phi_M), points and reductions from those."""
    s = three
    mon = _monitor(s)
    pts = {}
    for tag in (1, 2):
        mon.watch(tag)
        for j, name in ((0, f"a{tag}"), (5, f"b{tag}")):
            pts[name] = (tag, _membrane_point(s, tag, j))
            mon.point(name, tag, pts[name][1])
        for op in ("average", "integral", "min", "max"):
            mon.reduce(f"{op}{tag}", tag, op=op)
    assert mon.n_cols == 6 * (19 + 11) and mon.n_cols > 64
    st = _state(s)
    # a stimulus amplitude in the neuron's table and times inside the first period and in a later one: g_stim, i_stim and
    # the totals are pinned at non-zero values
    mm1 = s.subdomain_list[1]["mem_models"][0]["ode"]
    p1 = mm1.parameters.copy()
    p1[:, mm1.ode.parameter_indices("stim_amplitude")] = np.linspace(5.0, 15.0, mm1.nodes)
    st["tables"] = {(1, 0): (mm1.states.copy(), p1)}
    for t in (0.3e-3, 61.7e-3):
        _check_record_host(s, mon, pts, st, t, {1: p1})


def _check_record_host(s, mon, pts, st, t, params_of):
    values, row = mon.compute_host(t, st)
    ecs = s.subdomain_list[0]["mesh_sub"]
    for tag, model in ((1, "hh_si"), (2, "glial")):
        mm = s.subdomain_list[tag]["mem_models"][0]["ode"]
        mem, ics = s.subdomain_list[tag]["mesh_mem"], s.subdomain_list[tag]["mesh_sub"]
        y, p = mm.states.copy(), params_of.get(tag, mm.parameters).copy()
        for q in range(mm.nodes):
            ve = int(np.flatnonzero(ecs.parent_vertices == mem.parent_vertices[q])[0])
            vi = int(np.flatnonzero(ics.parent_vertices == mem.parent_vertices[q])[0])
            for k, ion in enumerate(s.ion_list):
                p[q, mm.ode.parameter_indices(f"{ion['name']}_e")] = st["c"][0][k][ve]
                p[q, mm.ode.parameter_indices(f"{ion['name']}_i")] = st["c"][tag][k][vi]
            y[q, mm.V_index] = st["phi_M"][tag][q]
        ref = dict(zip(mh.names(model), mh.evaluate(model, t, y, p)))
        scale = {n: v[1] for n, v in restated(model, t, y, p).items()}
        assert set(values[(tag, 0)]) == set(ref)
        for n in ref:
            assert (np.abs(values[(tag, 0)][n] - ref[n]) <= TOL * scale[n]).all(), (tag, n)
        w = mon.weights(tag)
        area = float(w.sum())
        assert area > 0 and (w > 0).all()
        for n in ref:
            big = float(scale[n].max())
            assert abs(row[f"integral{tag}/{n}"] - float(w @ ref[n])) <= 1e-11 * area * big
            assert abs(row[f"average{tag}/{n}"] - float(w @ ref[n]) / area) <= 1e-11 * big
            assert row[f"min{tag}/{n}"] == ref[n].min() and row[f"max{tag}/{n}"] == ref[n].max()
    # point weights sum to one and reproduce the coordinates of the point
    for name, key, q, w in mon._points:
        assert abs(w.sum() - 1.0) < 1e-12 and len(q) == 3
        X = np.asarray(s.subdomain_list[key[0]]["mesh_mem"].x)[q]
        assert np.allclose(w @ X, pts[name][1], atol=1e-12 * np.abs(X).max())
    assert (values[(1, 0)]["g_stim"] > 0).all() and (values[(1, 0)]["i_stim"] != 0).all()
    # the series of record_host carries the row
    mon.clear()
    mon.record_host(t, st)
    ser = mon.series()
    assert ser["t"].tolist() == [t] and ser["a2/E_K"][0] == row["a2/E_K"]


def test_average_of_a_constant_field_is_the_constant(hip_lib, three):
    """Every dof the same row and state: every quantity is constant over the membrane, and so are its average, minimum,
    maximum and point values."""
    s = three
    mon = _monitor(s)
    mon.watch(2)
    mon.point("p", 2, _membrane_point(s, 2, 2))
    for op in ("average", "min", "max"):
        mon.reduce(op, 2, op=op)
    mm = s.subdomain_list[2]["mem_models"][0]["ode"]
    y0, p0 = mh.sample_tables("glial", 1)
    y, p = np.tile(y0, (mm.nodes, 1)), np.tile(p0, (mm.nodes, 1))
    values, row = mon.compute_host(0.0, {"tables": {(2, 0): (y, p)}})
    for n, v in values[(2, 0)].items():
        c = v[0]
        assert (v == c).all()
        for col in ("average", "p"):
            assert abs(row[f"{col}/{n}"] - c) <= 1e-12 * abs(c)
        assert row[f"min/{n}"] == c and row[f"max/{n}"] == c


def test_integral_weights_use_only_the_models_facets(hip_lib, three):
    from knpemi.fem.probe import integral_weights
    s = three
    mon = _monitor(s)
    mem = s.subdomain_list[1]["mesh_mem"]
    ftag = s.ft.dense()[mem.parent_entities]
    tag_of_model = int(s.subdomain_list[1]["mem_models"][0]["ode"].tag)
    assert np.array_equal(mon._geometry(1, 0)[2], ftag == tag_of_model)
    # half of the facets taken away from the model: the weights are those of the other half alone
    mask = mon._geometry(1, 0)[2].copy()
    mask[::2] = False
    mon._geo[(1, 0)] = mon._geo[(1, 0)][:2] + (mask,)
    w = mon.weights(1)
    assert np.array_equal(w, integral_weights(mem, cell_mask=mask))
    touched = np.zeros(mem.x.shape[0], bool)
    touched[np.asarray(mem.cells)[mask].ravel()] = True
    assert (w[~touched] == 0).all() and (w[touched] > 0).all() and 0 < w.sum() < integral_weights(mem).sum()
    # a point on a facet that no longer carries the model is refused
    mon.watch(1)
    with pytest.raises(ValueError, match="not in"):
        mon.point("gone", 1, _membrane_point(s, 1, 0))
    mon.point("kept", 1, _membrane_point(s, 1, 1))


def test_entry_points_refuse_a_null_handle(hip_lib):
    from knpemi import _lib as L
    assert hip_lib.knpemi_monitor_record(None, 0.0, 0) == L.EINVAL
    assert hip_lib.knpemi_monitor_reset(None) == L.EINVAL and hip_lib.knpemi_monitor_clear(None) == L.EINVAL
    assert hip_lib.knpemi_monitor_read(None, 0, None, None, None, 0) == L.EINVAL


# ---- plug-in monitors ----------------------------------------------------------------------------------------------------
SYNTHETIC_MONITOR = """
def monitor(states, t, parameters, monitored):
    (m, V) = states
    g, E, tau = parameters[0], parameters[1], parameters[3]
    i_gated = g * m ** 3 * (V - E)
    monitored[0] = i_gated
    monitored[1] = math.exp(-np.fmod(t, 30.0) / tau) * (t < 125)
    monitored[1 + 1] = 1.0 / (1.0 + math.exp(-(V + 40.0) / 5.0)) if V > -90 else 0.0
    return monitored
"""


def test_codegen_translates_a_monitor_and_it_compiles(hip_lib):
    import ctypes as C
    from knpemi import _lib as L
    from knpemi import rhs_codegen as cg
    src = cg.hip_monitor_from_python(SYNTHETIC_MONITOR, n_states=2, n_params=4, n_monitored=3)
    assert "__device__ inline void monitor(double t, const double* states, const double* parameters, double* monitored)" in src
    assert "monitored[0] = v_i_gated;" in src and "monitored[2] = " in src and "values[" not in src
    log = C.create_string_buffer(8192)
    rc = hip_lib.knpemi_monitor_compile_source(2, 4, 3, src.encode(), log, len(log))
    assert rc == L.OK, log.value.decode()
    # a source that does not compile, and sizes out of range
    assert hip_lib.knpemi_monitor_compile_source(2, 4, 3, b"__device__ void monitor(int nonsense) {}", log, len(log)) == L.EINVAL
    assert b"monitor" in log.value
    assert hip_lib.knpemi_monitor_compile_source(2, 4, 33, src.encode(), None, 0) == L.EINVAL
    assert hip_lib.knpemi_monitor_compile_source(2, 4, 3, None, None, 0) == L.EINVAL


@pytest.mark.parametrize("body,what", [
    ("parameters[0] = 1.0", r"store into `parameters\[0\]`"),
    ("states[0] = 1.0", r"store into `states\[0\]`"),
    ("monitored[i] = 1.0", "literal index"),
    ("monitored[3] = 1.0", "index 3 of `monitored` is out of range"),
    ("for k in range(3):\n        monitored[0] = 1.0", "statement `For`"),
    ("monitored[0] = scipy.special.erf(t)", "call of `scipy.special.erf`"),
    ("monitored[0] = math.gamma(t)", "`math.gamma` has no device counterpart"),
    ("monitored[0] = undefined_name", "`undefined_name` is read before it is assigned"),
])
def test_codegen_refuses_what_a_monitor_may_not_do_by_name(body, what):
    from knpemi import rhs_codegen as cg
    src = f"def monitor(states, t, parameters, monitored):\n    i = 0\n    {body}\n"
    with pytest.raises(NotImplementedError, match=what):
        cg.hip_monitor_from_python(src, n_states=2, n_params=4, n_monitored=3)
    with pytest.raises(NotImplementedError, match="signature"):
        cg.hip_monitor_from_python("def monitor(states, t, parameters):\n    pass\n")


def test_benchmark_glial_brings_a_monitor(hip_lib):
    """examples/benchmark/mm_glial.py: names, indices, a Python monitor whose totals are the currents its own `rhs`
    stores, and a translation that compiles."""
    import ctypes as C
    import importlib.util
    import os
    from knpemi import _lib as L
    from knpemi import rhs_codegen as cg
    path = os.path.join(os.path.dirname(mh.HERE), "examples", "benchmark", "mm_glial.py")
    spec = importlib.util.spec_from_file_location("mm_glial_benchmark", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert cg.monitor_names_of(mod) == mh.names("glial") and mod.monitor_indices("E_K", "I_Cl") == [1, 10]
    p = mod.init_parameter_values(psi=96500e3 / (8.315e3 * 307e3), z_Na=1.0, z_K=1.0, z_Cl=-1.0, Cm=1.0, K_e=3.1, K_i=99.3,
                                  Na_e=144.6, Na_i=15.8, Cl_e=133.6, Cl_i=5.2)
    y, m = mod.init_state_values(), np.zeros(11)
    mod.monitor(y, 0.0, p, m)
    mod.rhs(0.0, y, np.zeros(1), p)
    assert m[8] == p[mod.parameter_indices("I_ch_Na")] and m[9] == p[mod.parameter_indices("I_ch_K")]
    assert m[10] == p[mod.parameter_indices("I_ch_Cl")]
    src = cg.hip_monitor_from_module(mod)
    log = C.create_string_buffer(8192)
    assert hip_lib.knpemi_monitor_compile_source(1, 21, 11, src.encode(), log, len(log)) == L.OK, log.value.decode()


def test_an_untranslatable_monitor_leaves_the_model_without_one(tmp_path):
    """A plug-in whose Python `monitor` holds a construct the translation refuses: the model has no monitor and says why
    (its right-hand side is not affected); the translation of a good one runs once per model."""
    import importlib.util
    from knpemi import rhs_codegen as cg
    from knpemi.odeSolver import MembraneModel

    def module(name, body):
        path = tmp_path / f"{name}.py"
        path.write_text("import numpy as np\nMONITOR_NAMES = ['a']\n"
                        "def init_state_values():\n    return np.zeros(1)\n"
                        "def init_parameter_values():\n    return np.zeros(2)\n"
                        f"def monitor(states, t, parameters, monitored):\n{body}\n")
        spec = importlib.util.spec_from_file_location(name, str(path))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    class Q:
        def tabulate_dof_coordinates(self):
            return np.zeros((3, 2))
    bad = MembraneModel(module("mm_bad", "    for k in range(2):\n        monitored[0] = states[0]"), None, 1, Q())
    assert bad.monitor_names() == [] and "statement `For`" in bad.monitor_refused
    assert bad._plug_in_monitor() == ([], None)
    good = MembraneModel(module("mm_good", "    monitored[0] = states[0] * parameters[1]"), None, 1, Q())
    calls = []
    real = cg.hip_monitor_from_module
    cg.hip_monitor_from_module = lambda ode: calls.append(1) or real(ode)
    try:
        for _ in range(5):
            assert good.monitor_names() == ["a"]
        names, src = good._plug_in_monitor()
    finally:
        cg.hip_monitor_from_module = real
    assert len(calls) == 1 and good.monitor_refused is None and "monitored[0] = (states[0] * parameters[1]);" in src
