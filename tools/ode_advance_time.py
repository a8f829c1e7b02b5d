"""Times the multi-step membrane ODE launch (knpemi_ode_advance / ode_advance_kernel) on the GPU; not part of any test.

  1. advance(10 000) against 10 000 step_lsoda calls, 11 dofs of hh_mv (the calibration set-up);
  2. a 10^5-dof parameter sweep of hh_mv (K_e) to steady state;
  3. the steps per launch the host chose in each.

Prints one JSON line.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "calibrate_initial_conditions"))
import run_calibration as rc  # noqa: E402


def main():
    import contextlib
    import io
    module = rc.load_model("hh_mv")
    params, dt = rc.conditions("hh_mv")
    n = int(os.environ.get("ODE_ADVANCE_STEPS", "10000"))
    out = {}
    with contextlib.redirect_stdout(io.StringIO()):
        a = rc.make_membrane(module, 10, params)
        b = rc.make_membrane(module, 10, params)
        a.step_lsoda(dt, None)     # bind + warm up both handles
        b.advance(dt, 1)
        t0 = time.perf_counter()
        for _ in range(n):
            a.step_lsoda(dt, None)
        out["step_lsoda_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        b.advance(dt, n)
        out["advance_s"] = time.perf_counter() - t0
    out["advance_chunk"] = b._dp.lib.knpemi_ode_advance_chunk(b._dp.h, b._sub, b._model)
    out["bit_identical"] = bool(np.array_equal(a.states, b.states))
    nd = int(os.environ.get("ODE_SWEEP_DOFS", "100000"))
    with contextlib.redirect_stdout(io.StringIO()):
        s = rc.make_membrane(module, nd - 1, params)
        s.parameters[:, module.parameter_indices("K_e")] = np.linspace(2.0, 8.0, nd)
        t0 = time.perf_counter()
        steps = s.steady_state(dt, 20000, rtol=1e-8, atol=1e-10, window=10)
        out["sweep_s"] = time.perf_counter() - t0
    out["sweep_dofs"] = nd
    out["sweep_steady"] = int((steps >= 0).sum())
    out["sweep_max_steps"] = int(steps.max())
    out["sweep_chunk"] = s._dp.lib.knpemi_ode_advance_chunk(s._dp.h, s._sub, s._model)
    out["sweep_gpu_ms"] = s.last_stats["ms"]
    out["steps"] = n
    print(json.dumps(out))


if __name__ == "__main__":
    main()
