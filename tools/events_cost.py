"""Cost of recording membrane events in the device-resident loop (knpemi.events, DeviceStepper.detect).

Config 2 (tet r=1) with the device solves: ms per whole step with nothing attached, with the events of cell 1 recorded
every step, and with the events and the ten observables of tools/observe_cost.py recorded every step.  All legs start
from the same state (DeviceStepper.reset), so they run the same solver iterations; the legs alternate and the median of
the windows (7, as `bench.py --full` times) is printed as one JSON line.  For the kernel's own time run this under
`rocprofv3 --kernel-trace --stats` and read events_record_kernel in the statistics.
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
    ap.add_argument("--threshold", type=float, default=-20e-3)
    args = ap.parse_args()
    from setup_problem import Setup
    from knpemi import MembraneEvents, Observables
    from knpemi.stepper import DeviceStepper
    with contextlib.redirect_stdout(io.StringIO()):
        s = Setup("tet", 1, g_syn=10.0)
    for t in s.subdomain_list:
        for k in range(2):
            s.c[t][k].x.array[:] = s.c_prev[t][k].x._a
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev,
                       device_solves=(1e-6, 1e-7))
    st.add_membrane_model(s.mem_models[0]["ode"], s.stim_params["stimulus"], s.stim_params["stimulus_locator"])
    obs = Observables(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list)
    obs.point("ECS", 0, [16.1e-6, 0.45e-6, 0.13e-6])
    obs.point("ICS", 1, [16.1e-6, 0.31e-6, 0.27e-6])
    obs.reduce("phi_M_neuron", "phi_M", tag=1, op="nodal_mean")
    obs.reduce("K_ecs_max", "c", ion="K", tag=0, op="max")
    ev = MembraneEvents(s.subdomain_list)
    ev.watch(1, args.threshold, reset=args.threshold - 20e-3, keep=8)

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
    st.detect(ev)
    st.observe(obs, every=1, capacity=4096)
    leg()
    fired = int(ev.fired(1).sum())
    attached = dict(plain=(False, False), events=(True, False), events_observed=(True, True))
    ms = {k: [] for k in attached}
    for _ in range(args.repeats):
        for name, (e, o) in attached.items():       # switch off what the leg does not record (the tables stay on the device)
            st.taps["detect"].enabled, st.taps["observe"].enabled = e, o
            ms[name].append(leg())
    st.taps["detect"].enabled = st.taps["observe"].enabled = True
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print(json.dumps(dict(workload="config2", steps=args.steps, windows=args.repeats, membrane_dofs=int(ev.n_q[1]),
                          fired_dofs=fired, observables=len(obs.items),
                          ms_per_step_plain=med["plain"], ms_per_step_events=med["events"],
                          ms_per_step_events_observed=med["events_observed"],
                          us_per_step_events=float(np.median(np.array(ms["events"]) - np.array(ms["plain"])) * 1e3),
                          windows_ms=ms)))


if __name__ == "__main__":
    main()
