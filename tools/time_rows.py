#!/usr/bin/env python3
"""Row kernels by themselves: `reps` back-to-back launches of the EMI and KNP assemblies on one workload's mesh (fields at
the perturbed initial state), each bracketed by HIP events.  usage: tools/time_rows.py [workload] [reps]

    tools/time_rows.py --mesh 2d --res 6 --cell-type quadrilateral --cell-type triangle [--repeats 7] [--json PATH]

times the row kernels of the 2-D rectangle (make_mesh_2D) instead of a bench workload.  Quadrilaterals are timed with 2 and
with 4 lanes per row, with the closed forms (GEO 1) and with the quadrature forced (KNPEMI_QUAD_GENERAL=1, GEO 0);
triangles as knpemi_create sets them up.  Every variant is a handle of its own in this one process; after a warm-up the
variants take turns, `repeats` times, `reps` launches each, and the figure of a variant is the median of its per-launch
times over the turns, with their range.  The share of the HBM peak is from the algorithmic bytes of bench.py."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (sets the package paths)
from knpemi import _lib as L  # noqa: E402

KERNELS = ("emi_rows_kernel", "knp_rows_kernel")


def time_launches(dp, fn, flags, name, reps):
    """us per launch of `reps` launches of the row kernel `name` through the assembly call `fn`."""
    lib = dp.lib
    kid = L.KERNEL_NAMES.index(name)
    L.check(lib.knpemi_profile(dp.h, 1 << kid))
    for _ in range(reps):
        L.check(fn(dp.h, flags))
    n, ms = C.c_int64(), C.c_double()
    L.check(lib.knpemi_profile_read(dp.h, kid, C.byref(n), C.byref(ms)))
    L.check(lib.knpemi_profile(dp.h, 0))
    return ms.value / max(1, n.value) * 1e3


def workload_main(workload, reps):
    import argparse
    args = argparse.Namespace(scaling="weak", knp_twice=False, no_overlap=True, frozen_state=True)
    case, stepper, _ = bench.build_problem(workload, args, 0, 1)
    dp, lib = stepper.dp, stepper.dp.lib
    case.s.perturb()
    stepper.reset()
    out = {}
    for name, fn, flags in ((KERNELS[0], lib.knpemi_assemble_emi, stepper.flags_emi),
                            (KERNELS[1], lib.knpemi_assemble_knp, stepper.flags_knp)):
        for _ in range(3):
            L.check(fn(dp.h, flags))
        dp.sync()
        out[name] = time_launches(dp, fn, flags, name, reps)
    survey, design, sizes = bench.algorithmic_bytes(case, dp)
    print(workload, {k: (round(v, 2), round(survey[k] / (v * 1e-6) / 1e9 / bench.HBM_PEAK_GBS, 3)) for k, v in out.items()},
          "(us, fraction of 8 TB/s by the SURVEY accounting)")


def mesh_variants(cell_types):
    """(label, cell type, environment of knpemi_create)"""
    out = []
    for ct in cell_types:
        if ct == "quadrilateral":
            for geo, env in ((1, {}), (0, {"KNPEMI_QUAD_GENERAL": "1"})):
                for lpr in (2, 4):
                    out.append((f"quadrilateral/lpr{lpr}/geo{geo}", ct, dict(env, KNPEMI_LPR=str(lpr))))
        else:
            out.append((ct, ct, {}))
    return out


def mesh_main(a):
    import contextlib
    import io
    import json
    import types
    import numpy as np
    from knpemi.fem import make_mesh_2D
    from knpemi.pdeSolver import create_solver_emi, create_solver_knp
    from setup_problem import Setup
    built = []
    for label, ct, env in mesh_variants(a.cell_type):
        for k in ("KNPEMI_LPR", "KNPEMI_QUAD_GENERAL"):
            os.environ.pop(k, None)
        os.environ.update(env)
        with contextlib.redirect_stdout(io.StringIO()):
            s = Setup("2d", a.res, mesh_data=make_mesh_2D(a.res, cell_type=ct))
            s.perturb()
            emi = create_solver_emi(s.a_emi, s.L_emi, s.phi, s.entity_maps, s.subdomain_list, None, p=s.p_emi, direct=False)
            knp = create_solver_knp(s.a_knp, s.L_knp, s.c, s.entity_maps, s.subdomain_list, None, p=s.p_knp)
            emi.assemble()                 # pushes every field
            knp.assemble()
        dp = knp.dp
        lay, flags = (C.c_int * 9)(), C.c_int(0)
        L.check(dp.lib.knpemi_debug_layout(dp.h, lay, 9))
        L.check(dp.lib.knpemi_debug_geometry(dp.h, C.byref(flags)))
        survey, _, sizes = bench.algorithmic_bytes(types.SimpleNamespace(s=s, models=[]), dp)
        calls = ((KERNELS[0], dp.lib.knpemi_assemble_emi, L.WANT_P), (KERNELS[1], dp.lib.knpemi_assemble_knp, 0))
        built.append(dict(label=label, dp=dp, keep=(s, emi, knp), calls=calls, survey=survey,
                          info=dict(cells=sizes["nc"], rows=sizes["N"], lanes_per_row=lay[1], row_blocks=lay[8],
                                    geometry_flags=flags.value, lds_emi=lay[5], lds_knp=lay[6])))
        print(label, built[-1]["info"], flush=True)
    for b in built:                        # warm-up
        for name, fn, flags in b["calls"]:
            for _ in range(3):
                L.check(fn(b["dp"].h, flags))
        b["dp"].sync()
        b["us"] = {k: [] for k in KERNELS}
    for _ in range(a.repeats):             # the variants take turns
        for b in built:
            for name, fn, flags in b["calls"]:
                b["us"][name].append(time_launches(b["dp"], fn, flags, name, a.reps))
    result = dict(mesh=f"make_mesh_2D({a.res})", reps=a.reps, repeats=a.repeats, hbm_peak_GBs=bench.HBM_PEAK_GBS, variants={})
    for b in built:
        row = dict(b["info"])
        for k in KERNELS:
            v = np.array(b["us"][k])
            med = float(np.median(v))
            row[k] = dict(median_us=round(med, 2), min_us=round(float(v.min()), 2), max_us=round(float(v.max()), 2),
                          algorithmic_bytes=int(b["survey"][k]),
                          hbm_fraction=round(b["survey"][k] / (med * 1e-6) / 1e9 / bench.HBM_PEAK_GBS, 4))
        result["variants"][b["label"]] = row
        print(b["label"], {k: row[k] for k in KERNELS}, flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="config3")
    ap.add_argument("reps", nargs="?", type=int, default=20)
    ap.add_argument("--mesh", choices=["2d"], default=None, help="time the 2-D rectangle instead of a bench workload")
    ap.add_argument("--res", type=int, default=6)
    ap.add_argument("--cell-type", action="append", choices=["triangle", "quadrilateral"], default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.mesh is None:
        return workload_main(a.workload, a.reps)
    a.cell_type = a.cell_type or ["quadrilateral", "triangle"]
    mesh_main(a)


if __name__ == "__main__":
    main()
