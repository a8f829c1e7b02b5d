"""Host build of the product's fixed-step integrators (tests/native/fixed_step_host_check.cpp), shared by the CPU and
the GPU tests of the fixed-step methods."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL_ID = {"hh_si": 0, "hh_mv": 1, "glial": 2}
METHOD_ID = {"euler": 1, "rk4": 2, "rush_larsen": 3}
_lib = None


def load():
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "native", "_build", "libfixed_step_host.so")
        src = os.path.join(HERE, "native", "fixed_step_host_check.cpp")
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
        lib = C.CDLL(so)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        lib.fixed_step_host.argtypes = [C.c_int, C.c_int, dp, dp, C.c_double, C.c_double, C.c_int, ip]
        lib.fixed_step_host_rates.argtypes = [C.c_int, C.c_double, dp, dp, dp, dp]
        lib.fixed_step_host_rates.restype = C.c_uint
        _lib = lib
    return _lib


def _ptr(a):
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_double))


def step(model, method, y, p, t0, dt, n):
    """One interval in place on the state y and the parameter row p; returns (rc, n_rhs, n_substeps)."""
    stats = (C.c_int * 2)()
    rc = load().fixed_step_host(MODEL_ID[model], METHOD_ID[method], _ptr(y), _ptr(p), float(t0), float(dt), int(n), stats)
    return rc, stats[0], stats[1]


def sweep(model, method, states, params, t0, dt, n, mask=None, stimulus=None):
    """MembraneModel.step over the rows of the tables, in place: stimulus pairs {column: value} into the masked rows,
    then one interval per row.  Returns the number of rows left with a non-finite state."""
    bad = 0
    for r in range(states.shape[0]):
        if stimulus and (mask is None or mask[r]):
            for idx, val in stimulus.items():
                params[r, idx] = val
        y, p = states[r].copy(), params[r].copy()
        bad += step(model, method, y, p, t0, dt, n)[0] != 0
        states[r], params[r] = y, p
    return bad
