"""GPU tests of the observables: the device rows (knpemi_observe_*, DeviceStepper.observe) against the host evaluation
of the same functionals (Observables.evaluate_host) on fields downloaded after every step."""
import contextlib
import ctypes as C
import io
import os

import numpy as np
import pytest

from helpers import Setup
from knpemi import _lib as L

pytestmark = pytest.mark.gpu

# points inside each mesh: ECS, ICS and membrane of cell 1 (2D: ICS = [1,61] x [1,3] um, membrane y = 3 um, the
# reference's make_figures.py:250-257; 3D: axon 1 = [5,27] x [0.2,0.4] x [0.2,0.4] um, make_mesh_3D.py:12-24)
POINTS = {
    2: dict(ECS=[25e-6, 3.5e-6], ICS=[25e-6, 2e-6], mem=[25.3e-6, 3e-6]),
    3: dict(ECS=[16.1e-6, 0.45e-6, 0.13e-6], ICS=[16.1e-6, 0.31e-6, 0.27e-6], mem=[16.1e-6, 0.4e-6, 0.33e-6]),
}


def _observables(s, cells=(1,)):
    from knpemi import Observables
    obs = Observables(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list)
    P = POINTS[s.mesh.gdim]
    obs.point("ECS", tag=0, x=P["ECS"])
    obs.point("ICS", tag=1, x=P["ICS"])
    obs.membrane_point("mem", tag=1, x=P["mem"])
    obs.reduce("K_ecs_max", "c", ion="K", tag=0, op="max")
    obs.reduce("Na_ecs_min", "c", ion="Na", tag=0, op="min")
    obs.reduce("phi_ecs_int", "phi", tag=0, op="integral")
    obs.reduce("K_ics_avg", "c", ion="K", tag=1, op="average")
    for t in cells:
        obs.reduce(f"phi_M_{t}", "phi_M", tag=t, op="nodal_mean")
        obs.reduce(f"phi_M_{t}_max", "phi_M", tag=t, op="max")
        obs.reduce(f"phi_M_{t}_int", "phi_M", tag=t, op="integral")
    if 2 in cells:
        obs.point("ICS2", tag=2, x=[16.1e-6, 0.61e-6, 0.27e-6])
        obs.membrane_point("mem2", tag=2, x=[16.1e-6, 0.5e-6, 0.33e-6])
    return obs


def _problem(kind, r):
    with contextlib.redirect_stdout(io.StringIO()):
        if kind == "three":
            from knpemi.fem import make_mesh_3D
            from test_gpu_parity import _custom_problem
            mesh, ct, ft = make_mesh_3D(0, "tetrahedron", axon_tags=(1, 1, 2, 2))
            s = _custom_problem(mesh, ct, ft, {1: [(1, "hh_si")], 2: [(2, "glial")]})
            models = [(mm["ode"], {}, None) for t in (1, 2) for mm in s.subdomain_list[t]["mem_models"]]
            cells = (1, 2)
        else:
            s = Setup(kind, r, g_syn=10.0)
            models = [(s.mem_models[0]["ode"], s.stim_params["stimulus"], s.stim_params["stimulus_locator"])]
            cells = (1,)
    for t in s.subdomain_list:          # the solves start from c = c_prev
        for k in range(2):
            s.c[t][k].x.array[:] = s.c_prev[t][k].x._a
    return s, models, cells


def _run(kind, r, every, device_solves=(1e-9, 1e-10), fuse_update=None, steps=20, capacity=1024, reference=True):
    """(observables, device series, host rows evaluated from downloads after every recorded step, their scales)."""
    from knpemi.stepper import DeviceStepper
    s, models, cells = _problem(kind, r)
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev,
                       device_solves=device_solves, fuse_update=fuse_update)
    for m, stim, loc in models:
        st.add_membrane_model(m, stim, loc)
    obs = _observables(s, cells)
    st.observe(obs, every=every, capacity=capacity)
    ref, scale = [], []
    with contextlib.redirect_stdout(io.StringIO()):
        for k in range(steps):
            st.step()
            if reference and (k + 1) % every == 0:
                st.download()
                ref.append(obs.evaluate_host(s.phi, s.c, s.phi_M_prev))
                scale.append(_abs_scale(obs, s))
    obs.dt = float(s.dt)
    return obs, obs.series(), np.array(ref), np.array(scale)


def _abs_scale(obs, s):
    """sum |w u| / denom of every sum: the size of the rounding the order of summation may change."""
    row = np.empty(len(obs.items))
    for j, o in enumerate(obs.items):
        u = {L.F_PHI: lambda: s.phi[o.tag].x._a, L.F_C: lambda: s.c[o.tag][o.idx].x._a,
             L.F_C_ELIM: lambda: s.ion_list[-1][f"c_{o.tag}"].x._a, L.F_PHI_M: lambda: s.phi_M_prev[o.tag].x._a}[o.field]()
        row[j] = np.abs(o.w * u[o.ids]).sum() / abs(o.denom)
    return row


def _check(obs, ser, ref, scale, every, steps=20, moving=True):
    n = steps // every
    assert ser["t"].shape == (n,) and ref.shape == (n, len(obs.items))
    assert np.allclose(ser["t"], np.arange(1, n + 1) * every * obs.dt, rtol=1e-12)
    for j, o in enumerate(obs.items):
        dev = ser[o.key]
        if o.op in (L.OBS_MIN, L.OBS_MAX):
            assert np.array_equal(dev, ref[:, j]), o.key
        else:
            err = np.abs(dev - ref[:, j]) / np.maximum(scale[:, j], 1e-300)
            assert err.max() <= 1e-13, (o.key, err.max())
    if moving:      # the fields move: the series is not a constant
        assert np.ptp(ser["mem/phi_M"]) > 0


@pytest.mark.parametrize("kind,r", [("2d", 1), ("tet", 0), ("hex", 0)])
@pytest.mark.parametrize("every", [1, 3])
def test_device_rows_match_host_evaluation(hip_lib, kind, r, every):
    """Device solves, end-of-step update as a launch of its own (update_pde_kernel)."""
    obs, ser, ref, scale = _run(kind, r, every, fuse_update=False)
    _check(obs, ser, ref, scale, every)


@pytest.mark.parametrize("every", [1, 3])
def test_device_rows_with_device_solves(hip_lib, every):
    """Fused update: the rows follow the KNP write-back that also performs update_pde_variables."""
    obs, ser, ref, scale = _run("2d", 1, every, device_solves=(1e-6, 1e-7))
    _check(obs, ser, ref, scale, every)


def _fused_graph_case():
    obs, ser, ref, scale = _run("tet", 0, 1, device_solves=(1e-6, 1e-7))
    _check(obs, ser, ref, scale, 1)


def test_device_rows_with_fused_graph(hip_lib):
    """The same with the chunks of the fused solver loops replayed as captured graphs (KNPEMI_FUSED_GRAPH=1)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = [os.path.join(root, p) for p in ("knp-emi-fenics-x_amd", "oracle", "examples/idealized_geometries", "tests")]
    code = "import sys\nsys.path[:0] = %r\nimport test_observables_gpu as t\nt._fused_graph_case()\n" % (paths,)
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, KNPEMI_FUSED_GRAPH="1"),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]


def test_three_subdomains(hip_lib):
    """Two cells: the second cell's ODE sweep runs on the second auxiliary stream.  Without solves (this perturbed
    set-up of test_gpu_parity is an assembly case, not a state the solves can start from); the same two-cell schedule
    with the device solves runs in test_stim_driver_series_matches_history."""
    obs, ser, ref, scale = _run("three", 0, 1, device_solves=None)
    _check(obs, ser, ref, scale, 1, moving=False)


def test_two_runs_are_bit_identical(hip_lib):
    a = _run("tet", 0, 1, device_solves=(1e-6, 1e-7), reference=False)[1]
    b = _run("tet", 0, 1, device_solves=(1e-6, 1e-7), reference=False)[1]
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_capacity_drains_in_order(hip_lib):
    obs, ser, ref, scale = _run("2d", 1, 1, fuse_update=False, steps=10, capacity=4)
    _check(obs, ser, ref, scale, 1, steps=10)


def test_raw_records_past_capacity(hip_lib):
    from knpemi.stepper import DeviceStepper
    s, models, cells = _problem("2d", 1)
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev)
    for m, stim, loc in models:
        st.add_membrane_model(m, stim, loc)
    obs = _observables(s)
    dp, lib = st.dp, st.lib
    obs.upload(dp, 3)
    n = len(obs.items)
    rows, over = C.c_int64(), C.c_int64()

    def read(k):
        buf = np.full((k, n), np.nan)
        L.check(lib.knpemi_observe_read(dp.h, k, L.dptr(buf), C.byref(rows), C.byref(over), 0))
        return buf
    for _ in range(2):
        with contextlib.redirect_stdout(io.StringIO()):
            st.step()
        L.check(lib.knpemi_observe_record(dp.h))
    first = read(2)
    assert rows.value == 2 and over.value == 0 and np.isfinite(first).all()
    with contextlib.redirect_stdout(io.StringIO()):
        st.step()
    for _ in range(5):
        L.check(lib.knpemi_observe_record(dp.h))
    after = read(3)
    assert rows.value == 3 and over.value == 4
    assert np.array_equal(after[:2], first)
    st.download()
    assert np.allclose(after[2], obs.evaluate_host(s.phi, s.c, s.phi_M_prev), rtol=1e-12, atol=1e-300)
    L.check(lib.knpemi_observe_read(dp.h, 0, None, C.byref(rows), C.byref(over), 1))
    L.check(lib.knpemi_observe_read(dp.h, 0, None, C.byref(rows), C.byref(over), 0))
    assert rows.value == 0 and over.value == 0
    L.check(lib.knpemi_observe_clear(dp.h))
    assert lib.knpemi_observe_record(dp.h) == L.EINVAL
    # an index outside the field is refused before anything runs
    spec, ptr, idx, w, denom = obs.table(dp.sub_index)
    idx = idx.copy()
    idx[0] = 1 << 30
    rc = lib.knpemi_observe_set(dp.h, n, L.iptr(spec.ravel()), ptr.ctypes.data_as(C.POINTER(C.c_int64)), L.iptr(idx),
                                L.dptr(w), L.dptr(denom), 4)
    assert rc == L.EINVAL and b"out of range" in lib.knpemi_last_error()


def test_partitioned_step_is_refused(hip_lib):
    from knpemi.stepper import DeviceStepper
    s, models, cells = _problem("2d", 1)
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev)
    st.observe(_observables(s))
    with pytest.raises(NotImplementedError, match="partitioned"):
        st.step(halo=object())


def test_stim_driver_series_matches_history(hip_lib, tmp_path):
    """run_stim_duration.py --device-resident --steps 50 --series: one row per step; at the save_frequency steps the
    rows equal the driver's own history (computed from full downloads)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "run_stim_duration", os.path.join(root, "examples", "local_astrocyte_depolarization", "run_stim_duration.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    cfg = drv.load_config("baseline")
    path = tmp_path / "s.npz"
    with contextlib.redirect_stdout(io.StringIO()):
        _, hist = drv.solve_system(cfg, n_steps=50, device_resident=True, outdir=str(tmp_path), quiet=True,
                                   series=str(path))
    ser = np.load(path)
    assert ser["t"].shape == (50,)
    for key in ("ECS/phi", "ECS/K", "neuron/Na", "neuron_mem/phi_M", "neuron_mem/K_e", "neuron_mem/K_i"):
        assert np.isfinite(ser[key]).all(), key
    saved = [k for k in range(50) if k % cfg["save_frequency"] == 0 or k == 49]
    assert np.allclose(ser["t"][saved], hist["t"], rtol=1e-12, atol=0)
    assert np.array_equal(ser["K_ecs_max"][saved], np.array(hist["K_ecs_max"]))
    for key in ("phi_M_neuron", "phi_M_glia"):
        h = np.array(hist[key])
        assert np.abs(ser[key][saved] - h).max() <= 1e-13 * np.abs(h).max(), key
