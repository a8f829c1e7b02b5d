"""Times the field snapshots of a DG run (knpemi.dg_snapshots, csrc/kernels_dg_snapshot.hip).

Pack launch: on the idealized 3D meshes of tools/dg_time.py (r = 1, l = 2: 124 416 tetrahedra, 20 736 hexahedra), per form,
the watches of `watch_results` (phi and the three ions of both sub-domains, phi_M), `--reps` launches back to back behind one
synchronisation, the median and the range of five such windows; with the bytes one launch moves by the algorithm
(kn_dg_snapshot_bytes).  The launches re-read the same records, which the last-level cache holds at these sizes: the rate is
one over cache-resident data, not a share of the HBM peak.

Step with saving: the 2D driver (examples/idealized_geometries/run_2D_dg.py, device solves) saving every fifth step, three
ways, the legs alternating window by window in one process:
    none      nothing saved;
    download  one blocking get_* per field and np.savez of the arrays -- what a DG run could do before;
    snapshot  DGSnapshots + NpzSink (uncompressed, as the download leg), per form, timed until flush() returns.
Reports per leg the median and the range of the microseconds per step over the windows, the stalls at depth 4, and whether
the snapshot leg was at most as slow as the download leg in every window.  One JSON object; --out writes it to a file.

    python tools/dg_snapshot_time.py [-r 1] [-l 2] [--reps 2000] [--resolution 4] [--windows 9] [--steps 20] [--out profiles/dg_snapshot.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("knp-emi-fenics-x_amd", "examples/idealized_geometries", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))

FORMS = ("broken", "cell_mean", "vertex")


def pack_times(cell, r, l, reps):
    from dg_time import init_fields
    from knpemi import _lib as L
    from knpemi.dg import DGProblem
    from knpemi.dg_snapshots import DGSnapshots
    from knpemi.fem.idealized import make_mesh_3D
    mesh, ct, ft = make_mesh_3D(r, cell, l=l)
    out = dict(cell=cell)
    for form in FORMS:
        dp = init_fields(DGProblem(mesh, ct, ft, [0, 1], [1]))      # a fresh handle per form: one snapshot tap each
        lib = dp.lib
        lib.kn_dg_snapshot_bytes.restype, lib.kn_dg_snapshot_bytes.argtypes = C.c_longlong, [C.c_void_p]
        lib.kn_dg_snapshot_pack_only.restype, lib.kn_dg_snapshot_pack_only.argtypes = C.c_int, [C.c_void_p, C.c_int]
        snap = DGSnapshots(mesh, ct, ft, [0, 1], [1], ["Na", "K", "Cl"], writer="inline")
        snap.watch_results(form=form)
        dp.snapshot(snap, depth=2)
        L.check(lib.kn_dg_snapshot_pack_only(dp.h, 20))
        dp.sync()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            L.check(lib.kn_dg_snapshot_pack_only(dp.h, reps))
            dp.sync()
            ts.append((time.perf_counter() - t0) / reps * 1e6)
        us = statistics.median(ts)
        nbytes = int(lib.kn_dg_snapshot_bytes(dp.h))
        out.update(cells=dp.n_cells, dofs=dp.n, membrane_nodes=dp.nmf * dp.nf)
        out[form] = dict(pack_us=us, pack_us_min=min(ts), pack_us_max=max(ts), bytes=nbytes, GBps=nbytes / us / 1e3, frame_bytes=snap._layout[1],
                         items={n: c for n, _, _, c in snap._layout[0] if n in ("phi_0", "phi_1", "phi_M_1")})
        snap.close()
        del dp
    return out


def step_times(resolution, windows, steps, every, forms):
    import numpy as np
    import run_2D_dg
    from knpemi.dg_snapshots import NpzSink
    tmp = tempfile.TemporaryDirectory()
    legs = {"none": run_2D_dg.DGRun(resolution), "download": run_2D_dg.DGRun(resolution)}
    for form in forms:
        sink = NpzSink(os.path.join(tmp.name, form), compressed=False)
        legs["snapshot_" + form] = run_2D_dg.DGRun(resolution, snapshots=True, save_every=every, snapshot_form=form, sinks=[sink])
    os.makedirs(os.path.join(tmp.name, "download"))

    def window(name, run):
        dp = run.dp
        dp.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            run.step()
            if name == "download" and run.k % every == 0:
                arrays = {f"c{k}": dp.get_concentration(k) for k in range(dp.K)}
                np.savez(os.path.join(tmp.name, "download", f"step_{run.k:06d}.npz"), t=run.time, phi=dp.get_potential(),
                         phi_M=dp.get_membrane_potential(), **arrays)
        if run.snap is not None:
            run.snap.flush()
        dp.sync()
        return (time.perf_counter() - t0) / steps * 1e6
    for name, run in legs.items():                         # warm-up: the solver set-up, the first files
        window(name, run)
    times = {name: [] for name in legs}
    for _ in range(windows):
        for name, run in legs.items():
            times[name].append(window(name, run))
    dp = legs["none"].dp
    out = dict(resolution=resolution, cells=dp.n_cells, dofs=dp.n, membrane_nodes=dp.nmf * dp.nf, windows=windows,
               steps_per_window=steps, save_every=every)
    for name, ts in times.items():
        out[name] = dict(median_us=statistics.median(ts), min_us=min(ts), max_us=max(ts), windows_us=ts)
    for form in forms:
        leg = "snapshot_" + form
        snap = legs[leg].snap
        out[leg].update(depth=snap.depth, stalls=snap.stalls, writer_waits=snap.waits, frame_bytes=snap._layout[1],
                        not_slower_than_download_in_every_window=all(s <= d for s, d in zip(times[leg], times["download"])),
                        ranges_overlap_download=min(times["download"]) <= max(times[leg]))
        snap.close()
    tmp.cleanup()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("-r", type=int, default=1)
    ap.add_argument("-l", type=int, default=2)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--resolution", type=int, default=4)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--save-every", type=int, default=5)
    ap.add_argument("--forms", default="broken,vertex")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.windows < 7:
        ap.error("at least 7 windows")
    import torch  # noqa: F401  (before the library is loaded, as bench.py does: the process then has one HIP runtime)
    result = dict(pack=[pack_times(cell, a.r, a.l, a.reps) for cell in ("tetrahedron", "hexahedron")],
                  step=step_times(a.resolution, a.windows, a.steps, a.save_every, a.forms.split(",")))
    text = json.dumps(result, indent=1)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
