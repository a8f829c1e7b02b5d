"""Host build of the product's membrane monitors (tests/native/monitor_host_check.cpp), shared by the CPU and the GPU
tests of the monitors."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL_ID = {"hh_si": 0, "hh_mv": 1, "glial": 2}
_lib = None


def load():
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "native", "_build", "libmonitor_host.so")
        src = os.path.join(HERE, "native", "monitor_host_check.cpp")
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
        lib = C.CDLL(so)
        dp = C.POINTER(C.c_double)
        lib.monitor_host_name.restype = C.c_char_p
        lib.monitor_host_name.argtypes = [C.c_int, C.c_int]
        lib.monitor_host.argtypes = [C.c_int, C.c_double, dp, dp, dp]
        lib.monitor_host_currents.argtypes = [C.c_int, C.c_double, dp, dp, dp]
        _lib = lib
    return _lib


def _ptr(a):
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_double))


def names(model):
    lib = load()
    return [lib.monitor_host_name(MODEL_ID[model], i).decode() for i in range(lib.monitor_host_count(MODEL_ID[model]))]


def evaluate(model, t, states, params):
    """(quantities, rows): the host build's monitor of every row of the tables."""
    lib, mid = load(), MODEL_ID[model]
    states, params = np.ascontiguousarray(states, np.float64), np.ascontiguousarray(params, np.float64)
    out = np.empty((states.shape[0], lib.monitor_host_count(mid)))
    for r in range(states.shape[0]):
        assert lib.monitor_host(mid, float(t), _ptr(states[r]), _ptr(params[r]), _ptr(out[r])) == out.shape[1]
    return out.T.copy()


def currents(model, t, states, params):
    """(3, rows): I_Na, I_K, I_Cl as Model::rhs leaves them in the parameter row (host build)."""
    lib, mid = load(), MODEL_ID[model]
    states, params = np.ascontiguousarray(states, np.float64), np.ascontiguousarray(params, np.float64)
    out = np.empty((states.shape[0], 3))
    for r in range(states.shape[0]):
        assert lib.monitor_host_currents(mid, float(t), _ptr(states[r]), _ptr(params[r]), _ptr(out[r])) == 0
    return out.T.copy()


def golden():
    return np.load(os.path.join(HERE, "golden", "ode_models.npz"))


GOLDEN_KEYS = {"hh_si": ("hh_si_stim0", "hh_si_stim10"), "hh_mv": ("hh_mv_stim0", "hh_mv_stim1"), "glial": ("glial_stim0",)}
# what one unit of time and of potential is in the model's own units (hh_si: s and V; the others ms and mV)
UNITS = {"hh_si": (1e-3, 1e-3), "hh_mv": (1.0, 1.0), "glial": (1.0, 1.0)}


def sample_tables(model, n, seed=0):
    """(states (n, NS), params (n, NP)) that cover rest, upstroke and peak: first the golden start state and the states of
    the golden trajectories (rest, and the first steps under a stimulus), then a seeded spread around them -- V between
    -90 and +45 mV, gates over (0.02, 0.98), every concentration within 10 % of the golden row's, a stimulus amplitude
    in half of the rows."""
    g = golden()
    ys, ps = [], []
    for key in GOLDEN_KEYS[model]:
        y0, p0 = g[f"{key}_y0"], g[f"{key}_p0"]
        ys.append(y0)
        ps.append(p0)
        for r in g[f"{key}_traj"]:
            ys.append(r[:len(y0)])
            ps.append(p0)
    ys, ps = np.array(ys)[:n], np.array(ps)[:n]
    rng = np.random.default_rng(seed)
    m = n - len(ys)
    if m > 0:
        p0 = g[f"{GOLDEN_KEYS[model][-1]}_p0"]
        ns = len(g[f"{GOLDEN_KEYS[model][0]}_y0"])
        y = rng.uniform(0.02, 0.98, (m, ns))
        y[:, -1] = rng.uniform(-90.0, 45.0, m) * UNITS[model][1]
        p = np.tile(p0, (m, 1))
        conc = slice(9, 13) if model != "glial" else slice(13, 19)
        p[:, conc] *= rng.uniform(0.9, 1.1, (m, conc.stop - conc.start))
        if model != "glial":
            p[:, 8] = np.where(rng.random(m) < 0.5, 0.0, p0[0] * rng.uniform(0.01, 0.5, m))
        ys, ps = np.concatenate([ys, y]), np.concatenate([ps, p])
    return np.ascontiguousarray(ys), np.ascontiguousarray(ps)


def sample_times(model):
    """Inside the first stimulus period, in a later one, and past the stimulus' end."""
    u = UNITS[model][0]
    return [0.0, 0.7 * u, 41.3 * u, 130.0 * u]
