"""Cost of one on-device recorder in the device-resident loop: `--recorder observe | events | fluxes | exchange | maps |
monitor | snapshot` (knpemi.observables, .events, .fluxes, .exchange, .maps, .monitor, .snapshots and the DeviceStepper
method that attaches each).

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
  snapshot  `Snapshots.watch_results()` as doubles (`f8`) and as floats (`f4`), every step, depth 4, into a sink that drops
            the frames: pack launch, copy to pinned memory and the take on the host.  Also the pack launch on its own,
            with streaming and with plain stores: `--records` launches back to back between two device events as us per
            launch (launch gaps included), the kernel's own time from the library's event profile (KNPEMI_K_SNAPSHOT), and
            the bytes one launch must move by the algorithm (kn_snapshot_bytes) as a fraction of the HBM peak.

`--save-path` instead compares two ways of saving a run: the three-sub-domain problem of the stim driver
(examples/local_astrocyte_depolarization, `--resolution`) with the device solves, `--steps` steps saving every
`--save-every`-th: `download` (DeviceStepper.download + the driver's write_results, on the stepping thread), `snapshots`
(Snapshots.watch_results + NpzSink, flushed at the end of the window) and `plain` (nothing saved); the legs alternate in
one process and the median of the windows is printed.
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


def build_snapshot(s, st, args):
    from knpemi import _lib as L
    from knpemi.snapshots import Snapshots
    dp, lib = st.dp, st.lib
    lib.kn_snapshot_bytes.restype, lib.kn_snapshot_bytes.argtypes = C.c_longlong, [C.c_void_p]
    lib.kn_snapshot_pack_only.restype, lib.kn_snapshot_pack_only.argtypes = C.c_int, [C.c_void_p, C.c_int]
    lib.kn_snapshot_stream_stores.restype, lib.kn_snapshot_stream_stores.argtypes = C.c_int, [C.c_int]
    count = [0]

    def drop(t, k, frame):
        count[0] += 1
    tabs = {}
    for name in ("f8", "f4"):
        tabs[name] = Snapshots(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list, sink=drop)
        tabs[name].watch_results(dtype=name)
    st.snapshot(tabs["f8"], every=1, depth=4)
    tap = st.taps["snapshot"]
    current = ["f8"]
    stalls = dict(f8=0, f4=0)

    def use(name):
        """Replace the device table by that of `name`; the tap records into whichever is current."""
        old = tabs[current[0]]
        old.flush()
        stalls[current[0]] += old.stalls
        old._detach()
        tabs[name]._attach(dp, 4)
        tap.target = tabs[name]
        current[0] = name

    def record(t, f):
        L.check(tabs[current[0]]._tick(t, st.k))

    def rewind():      # every window starts with DeviceStepper.reset, which restarts the counters
        stalls[current[0]] += tabs[current[0]].stalls
        tabs[current[0]]._rewind()
    tap.record, tap.rewind = record, rewind

    def switch(leg):
        tap.enabled = leg != "plain"
        if tap.enabled and leg != current[0]:
            use(leg)

    def extra(ms):
        launch = {}
        default = lib.kn_snapshot_stream_stores(-1)
        for name in ("f8", "f4"):
            use(name)
            b = int(lib.kn_snapshot_bytes(dp.h))
            launch[name] = dict(algorithmic_bytes=b, frame_bytes=tabs[name]._layout[1])
            for mode, label in ((1, "stream"), (0, "plain")):
                lib.kn_snapshot_stream_stores(mode)
                L.check(lib.kn_snapshot_pack_only(dp.h, 20))
                us = []
                for _ in range(args.repeats):
                    dp.sync()
                    L.check(lib.knpemi_timer_start(dp.h))
                    L.check(lib.kn_snapshot_pack_only(dp.h, args.records))
                    out = C.c_double()
                    L.check(lib.knpemi_timer_stop_ms(dp.h, C.byref(out)))
                    us.append(out.value * 1e3 / args.records)
                # the kernel's own time: an event pair around every launch
                L.check(lib.knpemi_profile(dp.h, 1 << L.K_SNAPSHOT))
                L.check(lib.kn_snapshot_pack_only(dp.h, 50))
                n, tot = C.c_int64(), C.c_double()
                L.check(lib.knpemi_profile_read(dp.h, L.K_SNAPSHOT, C.byref(n), C.byref(tot)))
                L.check(lib.knpemi_profile(dp.h, 0))
                med, kern = float(np.median(us)), tot.value * 1e3 / max(n.value, 1)
                launch[name][label] = dict(us_per_launch=med, windows_us=us, kernel_us_event_pair=kern,
                                           gbytes_per_s=b / (med * 1e-6) / 1e9, hbm_fraction=b / (med * 1e-6) / HBM_PEAK,
                                           hbm_fraction_event_pair=b / (kern * 1e-6) / HBM_PEAK)
            lib.kn_snapshot_stream_stores(default)
        return dict(watches=len(tabs["f8"].watches), frames_dropped_into_the_sink=count[0], stalls=stalls, launch=launch,
                    default_stores="stream" if default else "plain",
                    algorithmic_bytes=dict(f8=launch["f8"]["algorithmic_bytes"], f4=launch["f4"]["algorithmic_bytes"]))
    return ("plain", "f8", "f4"), switch, extra


def save_path(args):
    """The --save-path comparison (module docstring); prints one JSON line."""
    import importlib.util
    import shutil
    import tempfile
    from knpemi.snapshots import NpzSink, Snapshots
    from knpemi.stepper import DeviceStepper
    spec = importlib.util.spec_from_file_location("run_stim_duration", os.path.join(
        ROOT, "examples", "local_astrocyte_depolarization", "run_stim_duration.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    cfg = drv.load_config("baseline")
    cfg["mesh"]["resolution_factor"] = args.resolution
    with contextlib.redirect_stdout(io.StringIO()):
        p = drv.Problem(cfg)
    st = DeviceStepper((p.a_emi, p.p_emi, p.L_emi), (p.a_knp, p.p_knp, p.L_knp), p.c, p.c_prev, p.phi, p.phi_M_prev,
                       device_solves=(1e-6, 1e-7))
    for tag in (1, 2):
        for mm in p.subdomain_list[tag]["mem_models"]:
            st.add_membrane_model(mm["ode"], p.stim_params["stimulus"], p.stim_params["stimulus_locator"])
    st.set_source(0, p.f_source_K.x._a)
    outdir = tempfile.mkdtemp(prefix="knpemi_save_path_")
    compressed = not args.uncompressed
    snap = Snapshots(p.mesh, p.ct, p.ft, p.subdomain_list, p.ion_list, sink=NpzSink(outdir, compressed=compressed, k_offset=-1))
    snap.watch_results()
    st.snapshot(snap, every=args.save_every, depth=args.depth)
    tap = st.taps["snapshot"]
    if compressed:
        write = drv.write_results
    else:
        def write(p, outdir, k, t):      # the arrays of write_results, without the compression
            fields = {}
            for tag in p.subdomain_list:
                fields[f"phi_{tag}"] = p.phi[tag].x._a
                for ion, f in zip(p.ion_list[:-1], p.c[tag]):
                    fields[f"{ion['name']}_{tag}"] = f.x._a
                fields[f"{p.ion_list[-1]['name']}_{tag}"] = p.ion_list[-1][f"c_{tag}"].x._a
                if tag > 0:
                    fields[f"phi_M_{tag}"] = p.phi_M_prev[tag].x._a
            np.savez(os.path.join(outdir, f"step_{k:06d}.npz"), t=t, **fields)
    legs = ("plain", "download", "snapshots") if args.save_path == "both" else ("plain", args.save_path)
    stalls, waits = [], []

    def leg(which):
        st.reset()
        tap.enabled = which == "snapshots"
        with contextlib.redirect_stdout(io.StringIO()):
            for _ in range(args.warmup):
                st.step()
            snap.flush()
            st.dp.sync()
            before, waited = snap.stalls, snap.waits
            t0 = time.perf_counter()
            for _ in range(args.steps):
                st.step()
                if which == "download" and st.k % args.save_every == 0:
                    st.download()
                    write(p, outdir, st.k - 1, st.k * st.dt)
            if which == "snapshots":
                snap.flush()
            st.dp.sync()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        if which == "snapshots":
            stalls.append(snap.stalls - before)
            waits.append(snap.waits - waited)
        return ms
    try:
        for name in legs:
            leg(name)
        ms = {name: [] for name in legs}
        for _ in range(args.repeats):
            for name in legs:
                ms[name].append(leg(name))
        files = len(os.listdir(outdir))
    finally:
        snap.close()
        shutil.rmtree(outdir, ignore_errors=True)
    out = dict(save_path=args.save_path, resolution=args.resolution, steps=args.steps, save_every=args.save_every,
               depth=args.depth, compressed=compressed, windows=args.repeats, frame_bytes=snap._layout[1] if snap._layout else None,
               vertices={t: int(sd["mesh_sub"].num_vertices) for t, sd in p.subdomain_list.items()}, files=files,
               stalls_per_window=stalls, writer_queue_full_per_window=waits)
    for name in legs:
        out[f"ms_per_step_{name}"] = float(np.median(ms[name]))
    for name in legs[1:]:
        out[f"us_per_step_{name}"] = float(np.median(np.array(ms[name]) - np.array(ms["plain"])) * 1e3)
    out["windows_ms"] = ms
    print(json.dumps(out))


RECORDERS = dict(observe=build_observe, events=build_events, fluxes=build_fluxes, exchange=build_exchange, maps=build_maps,
                 monitor=build_monitor)
KERNEL = dict(observe="observe_kernel", events="events_record_kernel", fluxes="flux_kernel", exchange="exchange_kernel",
              maps="maps_record_kernel", monitor="monitor_kernel")
# The snapshots are not a series recorder -- frames through a ring instead of rows in a buffer -- and are kept beside the six
FRAME_RECORDERS = dict(snapshot=build_snapshot)
FRAME_KERNEL = dict(snapshot="snapshot_pack_kernel")


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
    ap.add_argument("--recorder", choices=list(RECORDERS) + list(FRAME_RECORDERS), default=None)
    ap.add_argument("--save-path", choices=["download", "snapshots", "both"], default=None,
                    help="compare the ways of saving a run instead (module docstring); both: the two, alternating")
    ap.add_argument("--save-every", type=int, default=5, help="--save-path: save every n-th step (the driver's save_frequency)")
    ap.add_argument("--depth", type=int, default=4, help="--save-path: slots of the snapshot ring")
    ap.add_argument("--resolution", type=int, default=1, help="--save-path: resolution_factor of the driver's mesh")
    ap.add_argument("--uncompressed", action="store_true", help="--save-path: .npz without compression, both ways")
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
    if args.save_path:
        return save_path(args)
    if not args.recorder:
        raise SystemExit("give --recorder or --save-path")
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
    legs, switch, extra = {**RECORDERS, **FRAME_RECORDERS}[args.recorder](s, st, args)
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
        for name, (calls, us) in kernel_stats(args.stats, {**KERNEL, **FRAME_KERNEL}[args.recorder]).items():
            if args.recorder in FRAME_RECORDERS:      # the template argument of the pack kernel is the kind of store
                name = dict(fields="stream", series="plain")[name]
            out[f"kernel_{name}"] = dict(calls=calls, average_us=us)
            if name in out.get("algorithmic_bytes", {}):
                out[f"kernel_{name}"]["hbm_fraction"] = out["algorithmic_bytes"][name] / (us * 1e-6) / HBM_PEAK
    print(json.dumps(out))


if __name__ == "__main__":
    main()
