"""Host side of the standalone membrane models: the interval mesh of the calibration set-up, the new ABI entries, the
plug-in's multi-step kernel entry and the steady-state criterion (no device needed)."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np

from ode_steady import steady_steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_create_interval_mesh_tags_and_space():
    from knpemi.fem import GhostMode, create_interval, functionspace, meshtags
    omega = create_interval(None, 10, (0, 1), ghost_mode=GhostMode.shared_facet)
    assert omega.num_vertices == 11 and omega.num_cells == 10 and omega.cell_type == "interval"
    assert np.allclose(omega.x[:, 0], np.linspace(0.0, 1.0, 11))
    assert (omega.cells == np.stack([np.arange(10), np.arange(1, 11)], 1)).all()
    n = omega.topology.index_map(omega.topology.dim).size_local
    assert n == 10 and omega.topology.index_map(omega.topology.dim).num_ghosts == 0
    ct = meshtags(omega, omega.topology.dim, np.arange(n, dtype=np.int32), np.full(n, 1, np.int32))
    assert (ct.find(1) == np.arange(10)).all()
    x = functionspace(omega, ("CG", 1)).tabulate_dof_coordinates()
    assert x.shape == (11, 3) and np.allclose(x[:, 0], np.linspace(0, 1, 11)) and not x[:, 1:].any()
    assert create_interval(None, 4, (-2.0, 2.0), ghost_mode=GhostMode.none).x[1, 0] == -1.0


def test_new_ode_entries_declared_exported_and_bound(hip_lib):
    from knpemi import _lib as L
    header = open(os.path.join(ROOT, "include", "knpemi_hip.h")).read()
    for name in ("knpemi_ode_create", "knpemi_ode_advance", "knpemi_ode_advance_chunk"):
        assert re.search(rf"\b{name}\s*\(", header) and hasattr(hip_lib, name) and name in L.SIGNATURES
    struct = re.search(r"typedef struct knpemi_ode_ss \{(.*?)\} knpemi_ode_ss;", header, re.S).group(1)
    assert [f for f, _ in L.OdeSS._fields_] == re.findall(r"(\w+)[,;]", struct.replace("double", "").replace("int32_t", ""))
    assert C.sizeof(L.OdeSS) == 24
    consts = dict(re.findall(r"#define\s+KNPEMI_([A-Z_0-9]+)\s+\(?(-?\d+)\)?", header))
    for name in ("EODE", "EINVAL", "MAX_SUB", "ODE_SET_V", "ODE_SET_TRACES"):
        assert int(consts[name]) == getattr(L, name)


def test_no_device_standalone_handle_fails_loudly(hip_lib):
    from knpemi import _lib as L
    if hip_lib.knpemi_device_count() > 0:
        return
    h = C.c_void_p()
    nq = np.array([11], np.int32)
    assert hip_lib.knpemi_ode_create(0, 1, L.iptr(nq), C.byref(h)) == L.EHIP and not h.value
    assert hip_lib.knpemi_ode_create(0, 0, L.iptr(nq), C.byref(h)) == L.EINVAL
    assert hip_lib.knpemi_ode_advance(None, 1, 0, 0.0, 0.1, 1, 1e-8, 1e-10, None, 0, 1, None, None, None,
                                      None) == L.EINVAL


def test_plugin_compiles_with_the_advance_entry(hip_lib):
    spec = importlib.util.spec_from_file_location("mm_glial_bench", os.path.join(ROOT, "examples", "benchmark",
                                                                                 "mm_glial.py"))
    mm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mm)
    log = C.create_string_buffer(1 << 16)
    assert hip_lib.knpemi_ode_compile_source(1, 21, mm.RHS_HIP.encode(), log, len(log)) == 0, log.value.decode()
    src = open(os.path.join(ROOT, "knp-emi-fenics-x_amd", "csrc", "kernels_rtc.hip")).read()
    assert "ode_user_advance_kernel" in src and "ode_advance_body<ModelUser" in src


def test_steady_state_criterion():
    n_steps, nodes = 60, 5
    decay = np.array([0.5, 0.7, 0.9, 0.95, 1.0])        # the last node never settles
    k = np.arange(n_steps + 1)[:, None]
    traj = np.stack([-70.0 + 5.0 * decay[None, :] ** k, 0.1 + 0.01 * decay[None, :] ** k], axis=2)
    traj[:, 4, 0] += 0.1 * np.sin(k[:, 0])
    window = 4
    got = steady_steps(traj, 1e-9, 1e-12, window)
    for q in range(nodes):
        d = np.abs(np.diff(traj[:, q, :], axis=0))
        still = (d <= 1e-12 + 1e-9 * np.abs(traj[1:, q, :])).all(axis=1)
        want = -1
        for s in range(window - 1, n_steps):
            if still[s - window + 1:s + 1].all():
                want = s + 1
                break
        assert got[q] == want
    assert 0 < got[0] < got[1] and got[4] == -1
    # a still spell shorter than the window does not count; a frozen tail stays steady
    flat = np.zeros((10, 1, 1))
    flat[5] = 1.0
    assert steady_steps(flat, 0.0, 0.0, 3).tolist() == [3]
    flat[2] = 1.0
    assert steady_steps(flat, 0.0, 0.0, 3).tolist() == [9]
