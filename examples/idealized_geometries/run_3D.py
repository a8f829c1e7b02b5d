#!/usr/bin/env python3
"""3D idealized run (four axons in a box) on the MI355X hot path: the reference's
`examples/idealized_geometries/run_3D.py` (hexahedral mesh, `make_mesh_3D.py:100-102`; g_syn = 0,
Tstop = 2e-3, `run_3D.py:176-177,265`), or the 6-tet split of BASELINE configs 2/3 with `--tets`.

    python run_3D.py [--res 0] [--steps 20] [--tets] [--iterative]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from run_2D import solve_system  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--tets", action="store_true")
    ap.add_argument("--iterative", action="store_true")
    ap.add_argument("--mesh-file", default=None, help="XDMF mesh written by make_mesh_3D.py (default: generate)")
    ap.add_argument("--series", metavar="PATH", default=None, help="time series at the figures' points (.npz)")
    ap.add_argument("--events", metavar="PATH", default=None, help="membrane events of cell 1 per dof (.npz)")
    ap.add_argument("--event-threshold", type=float, default=-20e-3, metavar="V", help="crossing level of --events (V)")
    ap.add_argument("--fluxes", metavar="PATH", default=None, help="series of the ion fluxes of every sub-domain (.npz)")
    ap.add_argument("--exchange", metavar="PATH", default=None,
                    help="series of what every ion carries across the membrane of cell 1 (.npz)")
    ap.add_argument("--ode-method", choices=["lsoda", "euler", "rk4", "rush_larsen"], default="lsoda")
    ap.add_argument("--ode-substeps", type=int, default=None, help="sub-steps per time step of a fixed-step method (25)")
    a = ap.parse_args()
    s, it_emi, it_knp = solve_system("tet" if a.tets else "hex", a.res, a.steps, direct=not a.iterative,
                                     g_syn=0.0, mesh_file=a.mesh_file, out=os.path.join(HERE, "results", f"3D_{a.res}.npz"),
                                     series=a.series, ode_method=a.ode_method, ode_substeps=a.ode_substeps, events=a.events,
                                     event_threshold=a.event_threshold, fluxes=a.fluxes, exchange=a.exchange)
    v = s.phi_M_prev[1].x._a
    print(f"phi_M after {a.steps} steps: min {v.min():.6f} V, max {v.max():.6f} V")
    print(it_emi)
    print(it_knp)
