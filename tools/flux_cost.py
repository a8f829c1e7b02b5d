"""Cost of recording ion fluxes in the device-resident loop (knpemi.fluxes, DeviceStepper.fluxes).

Config 2 (tet r=1) or the 995 328-tet mesh (`--workload config3`) with the device solves: ms per whole step with nothing
attached, with the series row of every ion and the current in every sub-domain recorded every step, and with the
per-cell fields written as well.  All legs start from the same state (DeviceStepper.reset), so they run the same solver
iterations; the legs alternate and the median of the windows is printed as one JSON line, together with the bytes one
launch must move by the algorithm (cell indices + one 64-byte record per cell vertex + bytes written).  For the
kernel's own time run this under `rocprofv3 --kernel-trace --stats` and pass the statistics file of that run to a
second, unprofiled call with `--stats`: it adds the average duration of flux_kernel and the fraction of the HBM peak
those bytes make of it.
"""
import argparse
import contextlib
import csv
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("knp-emi-fenics-x_amd", "examples/idealized_geometries", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12       # bytes per second (MI355X)


def kernel_stats(path):
    """{"series": (calls, average us), "fields": ...} of flux_kernel<kind, fields> from a rocprofv3 statistics CSV."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if "flux_kernel" not in name:
                continue
            leg = "fields" if ("true" in name or "Lb1" in name or ", 1>" in name) else "series"
            out[leg] = (int(row["Calls"]), float(row["AverageNs"]) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["config2", "config3"], default="config2")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel statistics (.csv) of a profiled run of this tool")
    args = ap.parse_args()
    from setup_problem import Setup
    from knpemi import IonFluxes
    from knpemi.stepper import DeviceStepper
    with contextlib.redirect_stdout(io.StringIO()):
        s = Setup("tet", 1 if args.workload == "config2" else 2, g_syn=10.0)
    for t in s.subdomain_list:
        for k in range(2):
            s.c[t][k].x.array[:] = s.c_prev[t][k].x._a
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev,
                       device_solves=(1e-6, 1e-7))
    st.add_membrane_model(s.mem_models[0]["ode"], s.stim_params["stimulus"], s.stim_params["stimulus_locator"])
    fl = IonFluxes(s.subdomain_list, s.ion_list, s.physical_parameters)
    for tag in s.subdomain_list:
        fl.watch(tag)

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

    # a first, untimed pass of every leg: AMG set-up, solver mode choice, the ODE/assembly overlap decision, the
    # allocation of the field buffers
    leg()
    st.fluxes(fl, every=1, capacity=4096)
    tap = st.taps["fluxes"]
    modes = dict(plain=None, series=False, fields=True)
    for m in (False, True):
        tap.fields = m
        leg()
    ms = {k: [] for k in modes}
    for _ in range(args.repeats):
        for name, m in modes.items():       # switched off for the plain leg (the table stays on the device)
            tap.enabled, tap.fields = m is not None, bool(m)
            ms[name].append(leg())
    tap.enabled = True
    med = {k: float(np.median(v)) for k, v in ms.items()}
    n_cells = sum(fl.n_cells(t) for t in fl.watched)
    nv, g = 4, 3
    read = n_cells * nv * (4 + 64)
    written = dict(series=0, fields=n_cells * (len(s.ion_list) + 1) * 2 * g * 8)
    out = dict(workload=args.workload, steps=args.steps, windows=args.repeats, cells=n_cells, columns=fl.n_cols,
               ms_per_step_plain=med["plain"], ms_per_step_series=med["series"], ms_per_step_fields=med["fields"],
               us_per_step_series=float(np.median(np.array(ms["series"]) - np.array(ms["plain"])) * 1e3),
               us_per_step_fields=float(np.median(np.array(ms["fields"]) - np.array(ms["plain"])) * 1e3),
               algorithmic_bytes=dict(series=read, fields=read + written["fields"]),
               yardsticks=dict(events_us_per_step=3.0, events_kernel_us=4.1), windows_ms=ms)
    if args.stats:
        for name, (calls, us) in kernel_stats(args.stats).items():
            b = out["algorithmic_bytes"][name]
            out[f"kernel_{name}"] = dict(calls=calls, average_us=us, hbm_fraction=b / (us * 1e-6) / HBM_PEAK)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
