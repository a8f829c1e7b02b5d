"""Cost of one on-device recorder in the device-resident loop: `--recorder observe | events | fluxes | exchange | maps |
monitor` (knpemi.observables, .events, .fluxes, .exchange, .maps, .monitor and the DeviceStepper method that attaches each).

Config 2 (tet r=1) or the 995 328-tet mesh (`--workload config3`) with the device solves: ms per whole step with nothing
recorded (the leg `plain`: the tap switched off, the table stays on the device) and with the recorder's other legs, every
step.  All legs start from the same state (DeviceStepper.reset), so they run the same solver iterations; the legs
alternate and the median of the windows is printed as one JSON line: `ms_per_step_<leg>`, `us_per_step_<leg>` (the median
of the windows' differences to `plain`), `windows_ms`, and what RECORDERS holds for the recorder.  For the kernel's own
time run this under `rocprofv3 --kernel-trace --stats` and pass the statistics file of that run to a second, unprofiled
call with `--stats`: it adds the average duration of the recorder's kernel (`kernel_series`, `kernel_fields`) and, where
the recorder counts the bytes one launch must move by the algorithm, the fraction of the HBM peak they make of it.

The recorders:
  observe   ten observables: two points (eight functionals), the nodal mean of phi_M and the ECS maximum of K;
  events    the events of cell 1, keep = 8; the leg `events_observed` records the ten observables as well;
  fluxes    every ion and the current in every sub-domain: the series row, and with the per-cell fields; bytes: cell
            indices + one 64-byte record per cell vertex + bytes written;
  exchange  every ion and the currents of cell 1: the series row, and with the per-facet means.  The launch sits between
            the KNP assembly and the KNP solve; the membrane is a 2-D set, so its cost is a launch's latency;
  maps      tables on the ECS vertices: `one` (K+, every statistic), `peak` (K+, the peak only), `four` (phi and the three
            ions, every statistic).  Also the record launch on its own for these and `one_series` (`one` with the series
            tail): `--records` launches back to back between two device events, on the fields the run has left, as us per
            launch (launch gaps included), with the bytes one launch moves per item by the algorithm -- the sample (8 bytes
            of a dense array, or the 48 bytes of a vertex record once per space), v_prev read and written with the
            integral or the threshold, the integral read and written, exposure and excess read and written (counted for
            every item: an upper bound), v_max / v_min read, the weight of a series watch -- and the rate they make;
  monitor   cell 1: every quantity of the model at two membrane points, and its average, minimum and maximum over the
            membrane: the series row, and with the per-dof fields.
"""
import argparse
import contextlib
import csv
import ctypes as C
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


def ten_observables(s):
    from knpemi import Observables
    obs = Observables(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list)
    obs.point("ECS", 0, [16.1e-6, 0.45e-6, 0.13e-6])
    obs.point("ICS", 1, [16.1e-6, 0.31e-6, 0.27e-6])
    obs.reduce("phi_M_neuron", "phi_M", tag=1, op="nodal_mean")
    obs.reduce("K_ecs_max", "c", ion="K", tag=0, op="max")
    return obs


def tap_legs(st, legs):
    """switch(leg) for legs {leg: {tap name: None (off) or the tap's `fields`}}."""
    def switch(leg):
        for name, fields in legs[leg].items():
            st.taps[name].enabled, st.taps[name].fields = fields is not None, bool(fields)
    return list(legs), switch


# Per recorder: build(s, st, args) attaches it and returns (legs, switch, extra): the legs' names, `plain` first;
# switch(leg) prepares a leg; extra(ms) -> the recorder's own JSON keys from the windows {leg: [ms]}, called after the last
# window.  KERNEL: the kernel-name match of --stats.
def build_observe(s, st, args):
    obs = ten_observables(s)
    st.observe(obs, every=1, capacity=4096)
    legs, switch = tap_legs(st, dict(plain=dict(observe=None), observed=dict(observe=False)))
    return legs, switch, lambda ms: dict(
        observables=len(obs.items), entries=int(sum(o.ids.shape[0] for o in obs.items)), plain=ms["plain"],
        observed=ms["observed"], us_per_recorded_step=float(np.median(np.array(ms["observed"]) - np.array(ms["plain"])) * 1e3))


def build_events(s, st, args):
    from knpemi import MembraneEvents
    ev, obs = MembraneEvents(s.subdomain_list), ten_observables(s)
    ev.watch(1, args.threshold, reset=args.threshold - 20e-3, keep=8)
    st.detect(ev)
    st.observe(obs, every=1, capacity=4096)
    legs, switch = tap_legs(st, dict(plain=dict(detect=None, observe=None), events=dict(detect=False, observe=None),
                                     events_observed=dict(detect=False, observe=False)))
    return legs, switch, lambda ms: dict(membrane_dofs=int(ev.n_q[1]), fired_dofs=int(ev.fired(1).sum()),
                                         observables=len(obs.items))


def build_fluxes(s, st, args):
    from knpemi import IonFluxes
    fl = IonFluxes(s.subdomain_list, s.ion_list, s.physical_parameters)
    for tag in s.subdomain_list:
        fl.watch(tag)
    st.fluxes(fl, every=1, capacity=4096)
    n_cells = sum(fl.n_cells(t) for t in fl.watched)
    read = n_cells * 4 * (4 + 64)
    legs, switch = tap_legs(st, dict(plain=dict(fluxes=None), series=dict(fluxes=False), fields=dict(fluxes=True)))
    return legs, switch, lambda ms: dict(
        cells=n_cells, columns=fl.n_cols, yardsticks=dict(events_us_per_step=3.0, events_kernel_us=4.1),
        algorithmic_bytes=dict(series=read, fields=read + n_cells * (len(s.ion_list) + 1) * 2 * 3 * 8))


def build_exchange(s, st, args):
    from knpemi import MembraneExchange
    ex = MembraneExchange(s.subdomain_list, s.ion_list, s.physical_parameters)
    ex.watch(1)
    st.exchange(ex, every=1, capacity=4096)
    legs, switch = tap_legs(st, dict(plain=dict(exchange=None), series=dict(exchange=False), fields=dict(exchange=True)))
    return legs, switch, lambda ms: dict(facets=ex.n_facets(1), columns=ex.n_cols)


def build_monitor(s, st, args):
    from knpemi import MembraneMonitor
    mon = MembraneMonitor(s.subdomain_list, s.ion_list, ft=s.ft)
    mon.watch(1)
    mem = s.subdomain_list[1]["mesh_mem"]
    cells = np.asarray(mem.cells)
    for j, name in ((0, "first"), (cells.shape[0] // 2, "middle")):
        mon.point(name, 1, np.asarray(mem.x)[cells[j]].mean(axis=0))
    for op in ("average", "min", "max"):
        mon.reduce(op, 1, op=op)
    st.monitor(mon, every=1, capacity=4096, fields=True)
    legs, switch = tap_legs(st, dict(plain=dict(monitor=None), series=dict(monitor=False), series_fields=dict(monitor=True)))
    return legs, switch, lambda ms: dict(membrane_dofs=mon.n_dofs(1), columns=mon.n_cols,
                                         quantities=len(mon.watched[(1, 0)]))


def map_bytes_per_item(fm):
    """Bytes one record of the field maps moves per item of the space, by the algorithm (module docstring)."""
    total, record = 0, False
    for w in fm.watches.values():
        in_record = w.quantity == "phi" or (w.quantity == "c" and w.ion == fm.ion_names[-1])
        record |= in_record
        total += 0 if in_record else 8
        if "integral" in w.stats or "threshold" in w.stats:
            total += 16
        total += 16 * ("integral" in w.stats) + 32 * ("threshold" in w.stats) + 8 * ("peak" in w.stats) + 8 * ("trough" in w.stats)
        total += 8 * w.series
    return total + (48 if record else 0)


def build_maps(s, st, args):
    from knpemi import FieldMaps
    from knpemi import _lib as L
    dp, lib = st.dp, st.lib
    level = float(s.c_prev[0][0].x._a.max()) + 1e-3          # ECS K+ passes it where the cell releases K+
    stats = ("peak", "trough", "integral", "threshold")

    def make(watches):
        fm = FieldMaps(s.subdomain_list, s.ion_list)
        for name, quantity, ion, kw in watches:
            fm.watch(name, quantity, tag=0, ion=ion, **kw)
        return fm
    every = dict(threshold=level, stats=stats)
    tabs = dict(
        one=make([("K", "c", "K", every)]),
        peak=make([("K", "c", "K", dict(stats=("peak",)))]),
        four=make([("phi", "phi", None, dict(threshold=0.0, stats=stats)), ("K", "c", "K", every),
                   ("Cl", "c", "Cl", dict(threshold=100.0, stats=stats)), ("Na", "c", "Na", dict(threshold=100.0, stats=stats))]),
        one_series=make([("K", "c", "K", dict(series=True, **every))]))
    st.track(tabs["one"], every=1)
    tap = st.taps["track"]
    names = ("one", "peak", "four")

    def use(name):
        """Replace the device table by that of `name`; the tap's record launch does not depend on the table."""
        tabs[name]._dev = None
        tabs[name]._attach(dp, 4096)

    def switch(leg):
        tap.enabled = leg != "plain"
        if tap.enabled:
            use(leg)
            tap.reset()

    def extra(ms):
        # the record launch on its own, on the fields the last leg has left
        n_items = int(s.subdomain_list[0]["mesh_sub"].num_vertices)
        clock, launch = [1.0e3], {}

        def burst(n):
            for _ in range(n):
                clock[0] += 1.0e-4
                L.check(lib.knpemi_maps_record(dp.h, clock[0]))
        for name in names + ("one_series",):
            use(name)
            burst(20)
            us = []
            for _ in range(args.repeats):
                L.check(lib.knpemi_maps_reset(dp.h))
                burst(2)
                dp.sync()
                L.check(lib.knpemi_timer_start(dp.h))
                burst(args.records)
                out = C.c_double()
                L.check(lib.knpemi_timer_stop_ms(dp.h, C.byref(out)))
                us.append(out.value * 1e3 / args.records)
            b = map_bytes_per_item(tabs[name])
            launch[name] = dict(us_per_launch=float(np.median(us)), bytes_per_item=b,
                                gbytes_per_s=b * n_items / (float(np.median(us)) * 1e-6) / 1e9, windows_us=us)
        return dict(items=n_items, launch=launch, ms_per_step={k: float(np.median(v)) for k, v in ms.items()},
                    us_per_step={k: float(np.median(np.array(ms[k]) - np.array(ms["plain"])) * 1e3) for k in names})
    return ("plain",) + names, switch, extra


RECORDERS = dict(observe=build_observe, events=build_events, fluxes=build_fluxes, exchange=build_exchange, maps=build_maps,
                 monitor=build_monitor)
KERNEL = dict(observe="observe_kernel", events="events_record_kernel", fluxes="flux_kernel", exchange="exchange_kernel",
              maps="maps_record_kernel", monitor="monitor_kernel")


def kernel_stats(path, match):
    """{"series": (calls, average us), "fields": ...} of the kernel `match`<..., fields> from a rocprofv3 statistics CSV."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if match not in name:
                continue
            leg = "fields" if ("true" in name or "Lb1" in name or ", 1>" in name) else "series"
            out[leg] = (int(row["Calls"]), float(row["AverageNs"]) / 1e3)
    return out


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--recorder", choices=list(RECORDERS), required=True)
    ap.add_argument("--workload", choices=["config2", "config3"], default="config2")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel statistics (.csv) of a profiled run of this tool")
    ap.add_argument("--threshold", type=float, default=-20e-3, help="events: the firing threshold")
    ap.add_argument("--records", type=int, default=400, help="maps: record launches per timed burst")
    return ap


def main():
    args = parser().parse_args()
    from setup_problem import Setup
    from knpemi.stepper import DeviceStepper
    with contextlib.redirect_stdout(io.StringIO()):
        s = Setup("tet", 1 if args.workload == "config2" else 2, g_syn=10.0)
    for t in s.subdomain_list:
        for k in range(2):
            s.c[t][k].x.array[:] = s.c_prev[t][k].x._a
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev,
                       device_solves=(1e-6, 1e-7))
    st.add_membrane_model(s.mem_models[0]["ode"], s.stim_params["stimulus"], s.stim_params["stimulus_locator"])

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
    legs, switch, extra = RECORDERS[args.recorder](s, st, args)
    for name in legs[1:]:
        switch(name)
        leg()
    ms = {name: [] for name in legs}
    for _ in range(args.repeats):
        for name in legs:
            switch(name)
            ms[name].append(leg())
    switch(legs[-1])
    out = dict(recorder=args.recorder, workload=args.workload, steps=args.steps, windows=args.repeats)
    for name in legs:
        out[f"ms_per_step_{name}"] = float(np.median(ms[name]))
    for name in legs[1:]:
        out[f"us_per_step_{name}"] = float(np.median(np.array(ms[name]) - np.array(ms["plain"])) * 1e3)
    out.update(extra(ms), windows_ms=ms)
    if args.stats:
        for name, (calls, us) in kernel_stats(args.stats, KERNEL[args.recorder]).items():
            out[f"kernel_{name}"] = dict(calls=calls, average_us=us)
            if name in out.get("algorithmic_bytes", {}):
                out[f"kernel_{name}"]["hbm_fraction"] = out["algorithmic_bytes"][name] / (us * 1e-6) / HBM_PEAK
    print(json.dumps(out))


if __name__ == "__main__":
    main()
