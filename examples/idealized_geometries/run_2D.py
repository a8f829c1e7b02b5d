#!/usr/bin/env python3
"""2D idealized neuron-in-ECS run on the MI355X hot path.

Same structure as the reference's `examples/idealized_geometries/run_2D.py` (`solve_odes` :80-111,
time loop :341-372): per step the membrane ODEs, the EMI solve, the KNP solve and the end-of-step
update, through the knpemi API.  The mesh comes from the in-memory generator or from the XDMF file `make_mesh_2D.py` writes (`--mesh-file`);
ADIOS2 checkpoints are replaced by a compressed `.npz` of the final fields (I/O is outside the hot path).

    python run_2D.py [--res 1] [--steps 10] [--iterative] [--cell-type quadrilateral]

`--cell-type quadrilateral` runs the same rectangle on Q1 squares (one keyword of `dolfinx.mesh.create_rectangle` in the
reference's mesh script); a mesh file with a `Quadrilateral` topology works through `--mesh-file`.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "knp-emi-fenics-x_amd"))
sys.path.insert(0, HERE)

from knpemi import (create_solver_emi, create_solver_knp, update_ode_variables,  # noqa: E402
                    update_pde_variables)
from setup_problem import Setup  # noqa: E402


def solve_odes(s, k, ode_method="lsoda", ode_substeps=None):
    """ Solve ODEs (membrane models) for each membrane tag in each subdomain """
    for tag, subdomain in s.subdomain_list.items():
        if tag == 0:
            continue
        phi_M_prev_sub = s.phi_M_prev[tag]
        for mem_model in subdomain['mem_models']:
            ode_model = mem_model['ode']
            update_ode_variables(ode_model, s.c_prev, phi_M_prev_sub, s.ion_list, s.subdomain_list,
                                 s.mesh, s.ct, tag, k)
            if k == 0:
                ode_model.set_integrator(ode_method, ode_substeps)
            # step_lsoda of the reference; `step` is the same call with the integrator of --ode-method
            ode_model.step(dt=s.dt, stimulus=s.stim_params['stimulus'],
                           stimulus_locator=s.stim_params['stimulus_locator'])
            ode_model.get_membrane_potential(phi_M_prev_sub)
            for ion, I_ch_k in mem_model['I_ch_k'].items():
                ode_model.get_parameter("I_ch_" + ion, I_ch_k)


def read_mesh(mesh_file):
    """run_2D.py:114-134 of the reference, through knpemi.fem.XDMFFile."""
    from knpemi.fem import XDMFFile
    with XDMFFile(None, mesh_file, 'r') as xdmf:
        mesh = xdmf.read_mesh(ghost_mode=None)
        ct = xdmf.read_meshtags(mesh, name='cell_marker')
        ft = xdmf.read_meshtags(mesh, name='facet_marker')
    xdmf.close()
    return mesh, ct, ft


# The points of the reference's figures (make_figures.py:250-257 in 2D, :267-273 in 3D; um).  2D: ECS above the cell,
# ICS inside [1,61] x [1,3], membrane on its upper side y = 3.  3D: the ECS between axons 1 and 2 (y in (0.4, 0.5)),
# inside axon 1 ([5,27] x [0.2,0.4] x [0.2,0.4]), and on its upper face z = 0.4.
FIGURE_POINTS = {2: dict(ECS=(25.0, 3.5), ICS=(25.0, 2.0), mem=(25.0, 3.0)),
                 3: dict(ECS=(25.0, 0.45, 0.65), ICS=(25.0, 0.3, 0.3), mem=(25.6, 0.34, 0.4))}


def figure_observables(s):
    """phi and the ions at the figures' ECS / ICS points, phi_M and the traces at their membrane point."""
    from knpemi import Observables
    obs = Observables(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list)
    P = {k: np.array(v) * 1e-6 for k, v in FIGURE_POINTS[s.mesh.gdim].items()}
    obs.point("ECS", 0, P["ECS"])
    obs.point("ICS", 1, P["ICS"])
    obs.membrane_point("mem", 1, P["mem"])
    return obs


def membrane_events(s, threshold):
    """Upward crossings of `threshold` on the membrane of cell 1, re-armed 20 mV below it, the latest 8 times kept."""
    from knpemi import MembraneEvents
    ev = MembraneEvents(s.subdomain_list)
    ev.watch(1, threshold, reset=threshold - 20e-3, keep=8)
    return ev


def ion_fluxes(s):
    """Fluxes of every ion and the current density in every sub-domain."""
    from knpemi import IonFluxes
    fl = IonFluxes(s.subdomain_list, s.ion_list, s.physical_parameters)
    for tag in s.subdomain_list:
        fl.watch(tag)
    return fl


def membrane_exchange(s):
    """What every ion carries across the membrane of cell 1, the capacitive and the channel current."""
    from knpemi import MembraneExchange
    ex = MembraneExchange(s.subdomain_list, s.ion_list, s.physical_parameters, ft=s.ft)
    ex.watch(1)
    return ex


def field_maps(s, threshold):
    """Per-vertex maps of ECS K+ (peak, time integral, arrival at `threshold`, exposure and excess over it, and the ECS
    volume beyond it as a series) and peak / trough of phi_M on every cell."""
    from knpemi import FieldMaps
    fm = FieldMaps(s.subdomain_list, s.ion_list)
    fm.watch("K_ecs", "c", tag=0, ion="K", threshold=threshold, stats=("peak", "integral", "threshold"), series=True)
    for tag in list(s.subdomain_list)[1:]:
        fm.watch(f"phi_M_{tag}", "phi_M", tag=tag, stats=("peak", "trough"))
    return fm


def membrane_monitors(s):
    """The monitored quantities of the membrane model of cell 1 (Nernst potentials, conductances, currents by mechanism,
    gates) at the figures' membrane point -- make_figures.py:146-149 of the reference re-derives E_Na and E_K there from
    checkpoints -- and their average, minimum and maximum over the membrane."""
    from knpemi import MembraneMonitor
    mon = MembraneMonitor(s.subdomain_list, s.ion_list, ft=s.ft)
    mon.watch(1)
    mon.point("mem", 1, np.array(FIGURE_POINTS[s.mesh.gdim]["mem"]) * 1e-6)
    for op in ("average", "min", "max"):
        mon.reduce(op, 1, op=op)
    return mon


def monitor_state(s):
    """What MembraneMonitor.record_host takes at the end of a step: the concentrations the next sweep's traces are taken
    from, and phi_M; the tables are the models' own."""
    return dict(c={t: list(s.c_prev[t]) + [s.ion_list[-1][f"c_{t}"]] for t in s.subdomain_list},
                phi_M={t: s.phi_M_prev[t] for t in list(s.subdomain_list)[1:]})


def solve_system(kind, res, n_steps, direct=True, g_syn=10.0, out=None, mesh_file=None, series=None,
                 ode_method="lsoda", ode_substeps=None, events=None, event_threshold=-20e-3, fluxes=None, exchange=None,
                 maps=None, maps_threshold=None, monitor=None, cell_type=None):
    """cell_type: "quadrilateral" generates the 2-D mesh on quadrilaterals (None: the kind's default cells; a mesh file
    brings its own).
    series: path of a .npz with the time series at the figures' points (figure_observables), or None.
    ode_method / ode_substeps: the membrane integrator (MembraneModel.set_integrator); the reference's drivers name the
    sub-step count `n_steps_ODE` (run_2D.py:176).
    events: path of a .npz with the membrane events of cell 1 (knpemi.MembraneEvents: upward crossings of
    event_threshold per membrane dof, activation times, peaks), or None.
    fluxes: path of a .npz with the series of the ion fluxes and the current density of every sub-domain
    (knpemi.IonFluxes: integrals of the diffusive and the drift part, largest magnitude), or None.
    exchange: path of a .npz with the series of the membrane exchange of cell 1 (knpemi.MembraneExchange: molar flux of
    every ion out of the cell and into the ECS, capacitive and channel current, per step), or None.
    maps: path of a .npz with the field maps (field_maps: per-vertex peak, integral, arrival and exposure of ECS K+ over
    maps_threshold, in mM -- default: 0.001 mM above the initial ECS concentration, which the ECS next to the stimulated end
    passes within the first 20 steps -- and peak / trough of phi_M), or None.
    monitor: path of a .npz with the series of the membrane monitors (membrane_monitors), or None."""
    mesh_data = read_mesh(mesh_file) if mesh_file else None
    if mesh_data is None and cell_type not in (None, "triangle"):
        if kind != "2d":
            raise ValueError("--cell-type selects the cells of the generated 2-D mesh")
        from knpemi.fem import make_mesh_2D
        mesh_data = make_mesh_2D(res, cell_type=cell_type)
    s = Setup(kind, res, g_syn=g_syn, mesh_data=mesh_data)
    obs = figure_observables(s) if series else None
    ev = membrane_events(s, event_threshold) if events else None
    fl = ion_fluxes(s) if fluxes else None
    ex = membrane_exchange(s) if exchange else None
    if maps_threshold is None:
        maps_threshold = float(s.ion_list[0]["c_init"][0]) + 1e-3
    fm = field_maps(s, maps_threshold) if maps else None
    mon = membrane_monitors(s) if monitor else None
    problem_emi = create_solver_emi(s.a_emi, s.L_emi, s.phi, s.entity_maps, s.subdomain_list, None,
                                    direct=direct, p=s.p_emi, atol=1e-40, rtol=1e-5)
    problem_knp = create_solver_knp(s.a_knp, s.L_knp, s.c, s.entity_maps, s.subdomain_list, None,
                                    direct=direct, p=s.p_knp, atol=2e-40, rtol=1e-7)
    num_it_emi, num_it_knp = [], []
    t = 0.0
    for k in range(n_steps):
        print(f'Solving for t = {t:.4f} s')
        solve_odes(s, k, ode_method, ode_substeps)
        problem_emi.solve()
        if ex is not None:      # the new potential with the old concentrations: what the KNP right-hand side is formed from
            ex.record_host(t + s.dt, s.phi, s.c_prev, phi_M_prev=s.phi_M_prev, dt=s.dt,
                           splitting=s.a_emi.splitting_scheme)
        problem_knp.solve()
        num_it_emi.append(problem_emi.solver.getIterationNumber())
        num_it_knp.append(problem_knp.solver.getIterationNumber())
        update_pde_variables(s.c, s.c_prev, s.phi, s.phi_M_prev, s.physical_parameters, s.ion_list,
                             s.subdomain_list, s.mesh, s.ct)
        t += s.dt
        if obs is not None:
            obs.record_host(t, s.phi, s.c, s.phi_M_prev)
        if ev is not None:
            ev.record_host(t, s.phi_M_prev)
        if fl is not None:
            fl.record_host(t, s.phi, s.c_prev)
        if fm is not None:
            fm.record_host(t, s.phi, s.c, s.phi_M_prev)
        if mon is not None:
            mon.record_host(t, monitor_state(s))
    if mon is not None:
        mon.save(monitor)
    if fm is not None:
        fm.save(maps)
        for name in fm.watches:
            print(fm.summary(name))
    if fl is not None:
        fl.save(fluxes)
    if ex is not None:
        ex.save(exchange)
    if obs is not None:
        obs.save(series)
    if ev is not None:
        ev.save(events)
        x = ev.locations(1)
        print(ev.summary(1, origin=x[np.argmin(x[:, 0])]))      # the stimulated end: the smallest x
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        fields = {f.name: f.x._a for tag in s.subdomain_list for f in [s.phi[tag]] + s.c[tag]}
        fields.update({f.name: f.x._a for f in s.phi_M_prev.values()})
        np.savez_compressed(out, t=t, **fields)
    return s, num_it_emi, num_it_knp


def build_parser(res=1, steps=10, mesh_script="make_mesh_2D.py", cell_types=None):
    """cell_types: the choices of --cell-type (the first is the default), or None: no such option."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=res)
    if cell_types:
        ap.add_argument("--cell-type", choices=list(cell_types), default=cell_types[0],
                        help="cells of the generated mesh (a --mesh-file brings its own)")
    ap.add_argument("--steps", type=int, default=steps)
    ap.add_argument("--iterative", action="store_true")
    ap.add_argument("--mesh-file", default=None, help=f"XDMF mesh written by {mesh_script} (default: generate)")
    ap.add_argument("--series", metavar="PATH", default=None, help="time series at the figures' points (.npz)")
    ap.add_argument("--events", metavar="PATH", default=None, help="membrane events of cell 1 per dof (.npz)")
    ap.add_argument("--event-threshold", type=float, default=-20e-3, metavar="V", help="crossing level of --events (V)")
    ap.add_argument("--fluxes", metavar="PATH", default=None, help="series of the ion fluxes of every sub-domain (.npz)")
    ap.add_argument("--exchange", metavar="PATH", default=None,
                    help="series of what every ion carries across the membrane of cell 1 (.npz)")
    ap.add_argument("--maps", metavar="PATH", default=None,
                    help="per-vertex maps of ECS K+ (peak, integral, arrival, exposure) and peak / trough of phi_M (.npz)")
    ap.add_argument("--maps-threshold", type=float, default=None, metavar="MM",
                    help="level of --maps for ECS K+ in mM (default: 0.001 above the initial concentration)")
    ap.add_argument("--monitor", metavar="PATH", default=None,
                    help="series of the membrane model's monitored quantities at the membrane point and over the membrane (.npz)")
    ap.add_argument("--ode-method", choices=["lsoda", "euler", "rk4", "rush_larsen"], default="lsoda")
    ap.add_argument("--ode-substeps", type=int, default=None, help="sub-steps per time step of a fixed-step method (25)")
    return ap


CELL_TYPES_2D = ("triangle", "quadrilateral")


def recorder_arguments(a):
    """The recorder options of a parsed command line as keyword arguments of solve_system."""
    return dict(series=a.series, ode_method=a.ode_method, ode_substeps=a.ode_substeps, events=a.events,
                event_threshold=a.event_threshold, fluxes=a.fluxes, exchange=a.exchange, maps=a.maps,
                maps_threshold=a.maps_threshold, monitor=a.monitor)


if __name__ == "__main__":
    a = build_parser(cell_types=CELL_TYPES_2D).parse_args()
    s, it_emi, it_knp = solve_system("2d", a.res, a.steps, direct=not a.iterative, mesh_file=a.mesh_file,
                                     out=os.path.join(HERE, "results", f"2D_{a.res}.npz"), cell_type=a.cell_type,
                                     **recorder_arguments(a))
    v = s.phi_M_prev[1].x._a
    print(f"phi_M after {a.steps} steps: min {v.min():.6f} V, max {v.max():.6f} V")
    print(f"average number of iterations emi solver: {sum(it_emi) / len(it_emi)}")
    print(f"average number of iterations knp solver: {sum(it_knp) / len(it_knp)}")
