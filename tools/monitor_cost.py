"""Cost of recording membrane monitors in the device-resident loop (knpemi.monitor, DeviceStepper.monitor).

Config 2 (tet r=1) with the device solves: ms per whole step with nothing attached, with the monitors of cell 1 (every
quantity of the model at two membrane points, and its average, minimum and maximum over the membrane) recorded every
step, and with the per-dof fields written as well.  All legs start from the same state (DeviceStepper.reset), so they run
the same solver iterations; the legs alternate and the median of the windows is printed as one JSON line.  For the
kernel's own time run this under `rocprofv3 --kernel-trace --stats` and read monitor_kernel in the statistics.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("knp-emi-fenics-x_amd", "examples/idealized_geometries", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    from setup_problem import Setup
    from knpemi import MembraneMonitor
    from knpemi.stepper import DeviceStepper
    with contextlib.redirect_stdout(io.StringIO()):
        s = Setup("tet", 1, g_syn=10.0)
    for t in s.subdomain_list:
        for k in range(2):
            s.c[t][k].x.array[:] = s.c_prev[t][k].x._a
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev,
                       device_solves=(1e-6, 1e-7))
    st.add_membrane_model(s.mem_models[0]["ode"], s.stim_params["stimulus"], s.stim_params["stimulus_locator"])
    mon = MembraneMonitor(s.subdomain_list, s.ion_list, ft=s.ft)
    mon.watch(1)
    mem = s.subdomain_list[1]["mesh_mem"]
    cells = np.asarray(mem.cells)
    for j, name in ((0, "first"), (cells.shape[0] // 2, "middle")):
        mon.point(name, 1, np.asarray(mem.x)[cells[j]].mean(axis=0))
    for op in ("average", "min", "max"):
        mon.reduce(op, 1, op=op)

    def leg():
        st.reset()
        with contextlib.redirect_stdout(io.StringIO()):
            for _ in range(args.warmup):
                st.step()
            st.dp.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                st.step()
            st.dp.sync()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    # a first, untimed pass of every leg: AMG set-up, solver mode choice, the ODE/assembly overlap decision
    leg()
    st.monitor(mon, every=1, capacity=4096, fields=True)
    leg()
    legs = dict(plain=(False, False), series=(True, False), series_fields=(True, True))
    ms = {k: [] for k in legs}
    tap = st.taps["monitor"]
    for _ in range(args.repeats):
        for name, (on, fields) in legs.items():       # switch off what the leg does not record (the table stays on the device)
            tap.enabled, tap.fields = on, fields
            ms[name].append(leg())
    tap.enabled = True
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print(json.dumps(dict(workload="config2", steps=args.steps, windows=args.repeats, membrane_dofs=mon.n_dofs(1),
                          columns=mon.n_cols, quantities=len(mon.watched[(1, 0)]),
                          ms_per_step_plain=med["plain"], ms_per_step_series=med["series"],
                          ms_per_step_series_fields=med["series_fields"],
                          us_per_step_series=float(np.median(np.array(ms["series"]) - np.array(ms["plain"])) * 1e3),
                          us_per_step_series_fields=float(np.median(np.array(ms["series_fields"]) - np.array(ms["plain"])) * 1e3),
                          windows_ms=ms)))


if __name__ == "__main__":
    main()
