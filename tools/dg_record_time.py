"""Times one record of the DG recorders on the idealized 3D meshes of tools/dg_time.py: the observe launch alone (points,
reductions over both sub-domains, a membrane point), the jump launch (dg_jump_kernel: every sub-domain, all K + 1 fields) and
the events launch, beside the two assembly kernels of a DG step measured in the same process, and the bytes the jump kernel
must move; and the two launches of the per-cell ion balance (knpemi.dg_balance): the membrane launch alone, the pair of a
record, the bytes each must move, and a step of the device's own work (both assemblies, the update) with and without them.
Prints one JSON line per mesh; --out appends them to a file.

    python tools/dg_record_time.py [-r 1] [-l 2] [--reps 50] [--out profiles/dg_record.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("knp-emi-fenics-x_amd", "examples/idealized_geometries", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))


def jump_bytes(dp):
    """HBM bytes one jump launch must move: every dof record once (neighbour records are re-reads of the same array), the
    neighbour and facet tables, the cells' sub-domains, and the workgroup partials it writes."""
    nfc = 6 if dp.nv == 8 else dp.nv
    tasks = dp.n_cells * nfc
    return dp.n * 64 + tasks * 8 + dp.n_cells + (tasks + 255) // 256 * dp.n_sub * 5 * 8


def balance_bytes(dp, which):
    """HBM bytes one launch of the ion balance must move (which = 0: membrane launch, 1: flux launch): every dof record
    once, the facet tables, the cells' sub-domains, and its columns of the cell table (64 bytes per cell and ion: the
    membrane launch writes 3 of the 8 doubles, the flux launch reads those and writes the other 5)."""
    nfc = 6 if dp.nv == 8 else dp.nv
    tasks = dp.n_cells * nfc
    if which == 0:
        return dp.n * 64 + tasks * 4 + dp.nmf * 2 * 8 + dp.n_cells + dp.n_cells * dp.K * 24 + dp.nmf * dp.nf * (dp.K + 1) * 8
    return dp.n * 64 + tasks * 8 + dp.n_cells + dp.n_cells * dp.K * 64 + (dp.n_cells * 24 if dp.nv == 8 else 0)


def balance_times(dp, mesh, ct, ft, reps):
    """Microseconds of the membrane launch alone, of the pair of a record, and of a step of the device's own work without
    the solves (both assemblies, the end-of-step update on a device buffer) with and without the two launches in it."""
    import numpy as np
    import torch
    from knpemi import _lib as L
    from knpemi.dg_balance import DGIonBalance
    bal = DGIonBalance(mesh, ct, ft, [0, 1], [1], ["Na", "K", "Cl"])
    dp.balance(bal, capacity=4 * reps + 8)
    c = torch.tensor(np.stack([dp.get_concentration(k).ravel() for k in range(dp.K - 1)]), device=f"cuda:{dp.device}")
    torch.cuda.synchronize()

    def timed(body):
        body(0)
        dp.sync()
        t0 = time.perf_counter()
        for k in range(reps):
            body(1 + k)
        dp.sync()
        return (time.perf_counter() - t0) / reps * 1e6

    def membrane(k):
        L.check(dp.lib.knpemi_dg_balance_record_membrane(dp.h))

    def pair(k):
        dp.record_membrane()
        dp.record(float(k))

    def step(recorded):
        def body(k):
            dp.assemble_emi()
            dp.assemble_knp()
            if recorded:
                dp.record_membrane()
            dp.update_device(c.data_ptr())
            if recorded:
                dp.record(float(k))
        return body
    out = dict(balance_membrane_us=timed(membrane))
    dp.reset_recorders()
    out["balance_pair_us"] = timed(pair)
    dp.reset_recorders()
    # alternate the two versions of the step, twice: the spread between equal runs is part of the result
    plain, recorded = [], []
    for _ in range(2):
        plain.append(timed(step(False)))
        dp.reset_recorders()
        recorded.append(timed(step(True)))
        dp.reset_recorders()
    out.update(step_us=plain, step_recorded_us=recorded)
    return out


def per_record_us(dp, reps):
    """Microseconds per dp.record(t) of `reps` records enqueued back to back behind one synchronisation."""
    dp.record(0.0)
    dp.sync()
    t0 = time.perf_counter()
    for k in range(reps):
        dp.record(1.0 + k)
    dp.sync()
    return (time.perf_counter() - t0) / reps * 1e6


def measure(cell, general, r, l, reps):
    from dg_time import init_fields
    from knpemi.dg import DGProblem
    from knpemi.dg_recording import DGMembraneEvents, DGObservables
    from knpemi.fem.idealized import make_mesh_3D
    if general:
        os.environ["KNPEMI_DG_HEX_GENERAL"] = "1"
    else:
        os.environ.pop("KNPEMI_DG_HEX_GENERAL", None)
    out = dict(cell=cell, kernels="general" if general else ("box" if cell == "hexahedron" else "simplex"))
    times = {}
    mesh, ct, ft = make_mesh_3D(r, cell, l=l)
    for what in ("observe", "observe+jump", "events"):
        dp = init_fields(DGProblem(mesh, ct, ft, [0, 1], [1]))      # a fresh handle per recorder: one tap each
        if what == "events":
            ev = DGMembraneEvents(mesh, ft, [1])
            ev.watch(-20e-3, keep=8)
            dp.detect(ev)
        else:
            obs = DGObservables(mesh, ct, ft, [0, 1], [1], ["Na", "K", "Cl"])
            c = dp.X[dp.cell_sub == 0][0].mean(axis=0)
            obs.point("p", c, tag=0)
            obs.membrane_point("m", dp.XM[0].mean(axis=0), 1)
            for tag in (0, 1):
                obs.reduce(f"max{tag}", "c", tag, "max", ion="K")
                obs.reduce(f"avg{tag}", "phi", tag, "average")
                if what == "observe+jump":
                    obs.jump(f"Jphi{tag}", "phi", tag)
                    obs.jump(f"JK{tag}", "c", tag, ion="K")
            dp.observe(obs, capacity=4 * reps)
        times[what] = per_record_us(dp, reps)
        if what == "observe":
            out.update(cells=dp.n_cells, dofs=dp.n, membrane_nodes=dp.nmf * dp.nf,
                       emi_kernel_us=dp.time_kernel(0, 20) * 1e3, knp_kernel_us=dp.time_kernel(1, 20) * 1e3,
                       jump_bytes=jump_bytes(dp))
        del dp
    dp = init_fields(DGProblem(mesh, ct, ft, [0, 1], [1]))
    out.update(balance_times(dp, mesh, ct, ft, reps))
    out.update(balance_membrane_bytes=balance_bytes(dp, 0), balance_flux_bytes=balance_bytes(dp, 1))
    out["balance_flux_us"] = out["balance_pair_us"] - out["balance_membrane_us"]
    del dp
    out.update(observe_us=times["observe"], jump_us=times["observe+jump"] - times["observe"], events_us=times["events"])
    out["jump_GBps"] = out["jump_bytes"] / max(out["jump_us"], 1e-9) / 1e3
    out["jump_over_assembly"] = out["jump_us"] / (out["emi_kernel_us"] + out["knp_kernel_us"])
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("-r", type=int, default=1)
    ap.add_argument("-l", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (before the library is loaded, as bench.py does: the process then has one HIP runtime)
    for cell, general in (("tetrahedron", False), ("hexahedron", False), ("hexahedron", True)):
        line = json.dumps(measure(cell, general, a.r, a.l, a.reps))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
