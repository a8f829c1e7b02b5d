"""Rest states of the membrane models the examples ship, found on the GPU without a PDE problem.

Every model is set up on the dofs of a CG-1 space of a small interval mesh, with the concentrations and constants of
the driver that uses it, and stepped with `MembraneModel.steady_state` (one launch runs many LSODA steps) until every
state changes by less than the tolerance for `--window` steps in a row.  The rest state is printed in the form the
drivers' parameter blocks take.

    python run_calibration.py                                 # every shipped model
    python run_calibration.py --model hh_mv --history hist.npz
    python run_calibration.py --model glial --sweep K_e=3:12:64 --out sweep.npz
    python run_calibration.py --model glial --currents        # Kir, pump and leak currents of the rest state

`--sweep NAME=lo:hi:n` gives parameter NAME n values from lo to hi, one per node, and writes one rest state per value.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EXAMPLES = os.path.dirname(HERE)
ROOT = os.path.dirname(EXAMPLES)
for p in (os.path.join(ROOT, "knp-emi-fenics-x_amd"), os.path.join(EXAMPLES, "idealized_geometries")):
    if p not in sys.path:
        sys.path.insert(0, p)

from knpemi.fem import GhostMode, create_interval, functionspace, meshtags  # noqa: E402
from knpemi.odeSolver import MembraneModel  # noqa: E402


def _load(rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(EXAMPLES, *rel.split("/")))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _idealized():
    import setup_problem as sp
    return dict(psi=sp.PSI, Cm=sp.C_M, z_Na=1.0, z_K=1.0, z_Cl=-1.0, K_e=sp.K_E, K_i=sp.K_I, Na_e=sp.NA_E,
                Na_i=sp.NA_I, Cl_e=sp.CL_E, Cl_i=sp.CL_I), sp.DT


def _astrocyte(cell):
    # examples/local_astrocyte_depolarization/run_stim_duration.py: INIT[ion] = (ECS, neuron, glia), mV / ms units
    psi = 96500e3 / (8.315e3 * 307e3)
    K, Na, Cl = (3.092970607490389, 124.13988964240784, 99.3100014897692), \
        (144.60625137617149, 12.850454639128186, 15.775818906083778), (133.62525154406637, 5.0, 5.203660274163705)
    return dict(psi=psi, Cm=1.0, z_Na=1.0, z_K=1.0, z_Cl=-1.0, K_e=K[0], K_i=K[cell], Na_e=Na[0], Na_i=Na[cell],
                Cl_e=Cl[0], Cl_i=Cl[cell]), 0.1


# name -> (plug-in module, conditions)
MODELS = {
    "hh_si": ("idealized_geometries/mm_hh.py", _idealized),
    "hh_mv": ("local_astrocyte_depolarization/mm_hh.py", lambda: _astrocyte(1)),
    "glial": ("local_astrocyte_depolarization/mm_glial.py", lambda: _astrocyte(2)),
    "glial_benchmark": ("benchmark/mm_glial.py", lambda: _astrocyte(2)),
}


def load_model(name):
    return _load(MODELS[name][0], f"mm_calib_{name}")


def conditions(name):
    """(parameter values, dt) of the driver that uses model `name`."""
    return MODELS[name][1]()


def make_membrane(module, n_cells, params):
    """MembraneModel over the n_cells + 1 dofs of CG-1 on an interval mesh, parameters set everywhere."""
    omega = create_interval(None, n_cells, (0.0, 1.0), ghost_mode=GhostMode.shared_facet)
    tag = 1
    n_local = omega.topology.index_map(omega.topology.dim).size_local
    ct = meshtags(omega, omega.topology.dim, np.arange(n_local, dtype=np.int32), np.full(n_local, tag, np.int32))
    membrane = MembraneModel(module, ct, tag, functionspace(omega, ("CG", 1)))
    for key, value in params.items():
        membrane.parameters[:, module.parameter_indices(key)] = value
    return membrane


def state_names(module):
    n = len(module.init_state_values())
    names = []
    for name in ("m", "h", "n", "V"):
        try:
            i = module.state_indices(name)
        except ValueError:
            continue
        names.append((i, name))
    assert len(names) == n, "a model with other state names"
    return [name for _, name in sorted(names)]


def calibrate(name, max_steps=200000, rtol=1e-10, atol=1e-12, window=20, n_cells=10, record=None, every=1,
              sweep=None, method="lsoda", substeps=None):
    """Steady state of model `name`; returns (membrane, steps_taken, history).  sweep = (param, values) sets one value
    per node (n_cells is then len(values) - 1)."""
    module = load_model(name)
    params, dt = conditions(name)
    if sweep is not None:
        n_cells = len(sweep[1]) - 1
    membrane = make_membrane(module, n_cells, params)
    if sweep is not None:
        membrane.parameters[:, module.parameter_indices(sweep[0])] = sweep[1]
    membrane.set_integrator(method, substeps)
    out = membrane.steady_state(dt, max_steps, rtol=rtol, atol=atol, window=window, record=record, every=every)
    steps, hist = out if record is not None else (out, None)
    return membrane, steps, hist


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", choices=sorted(MODELS), action="append", help="model(s) to calibrate (default: all)")
    ap.add_argument("--max-steps", type=int, default=200000)
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--atol", type=float, default=1e-12)
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--sweep", help="NAME=lo:hi:n -- one rest state per value of parameter NAME")
    ap.add_argument("--history", help="write the recorded trajectory of every state to this .npz")
    ap.add_argument("--every", type=int, default=10, help="record every n-th step (--history)")
    ap.add_argument("--out", default="calibration.npz", help="rest states of a --sweep")
    ap.add_argument("--method", choices=["lsoda", "euler", "rk4", "rush_larsen"], default="lsoda",
                    help="membrane integrator (MembraneModel.set_integrator)")
    ap.add_argument("--substeps", type=int, default=None, help="sub-steps per step of a fixed-step method (default 25)")
    ap.add_argument("--currents", action="store_true",
                    help="print the currents by mechanism, the Nernst potentials and the conductances of the rest state "
                         "(MembraneModel.monitor; shipped models)")
    a = ap.parse_args(argv)
    names = a.model or sorted(MODELS)
    sweep = None
    if a.sweep:
        key, rng = a.sweep.split("=")
        lo, hi, n = rng.split(":")
        sweep = (key, np.linspace(float(lo), float(hi), int(n)))
    for name in names:
        module = load_model(name)
        record = state_names(module) if a.history else None
        membrane, steps, hist = calibrate(name, a.max_steps, a.rtol, a.atol, a.window, record=record,
                                          every=a.every, sweep=sweep, method=a.method, substeps=a.substeps)
        if (steps < 0).any():
            print(f"{name}: {int((steps < 0).sum())} node(s) not steady after {a.max_steps} steps", file=sys.stderr)
        print(f"# {name}: steady after {int(steps.max())} steps (t = {membrane.time:g})")
        if sweep is None:
            row = membrane.states[0]
            for s in state_names(module):
                print(f"{s}_init = {float(row[module.state_indices(s)])!r}")
            if a.currents:      # what the reference's run_calibration.py:148-212 plots over the run: here at its end
                if membrane.monitor_names():
                    for q, v in membrane.monitor().items():
                        print(f"{q} = {float(v[0])!r}")
                else:
                    print(f"# {name}: the model brings no monitor", file=sys.stderr)
        else:
            fn = a.out if len(names) == 1 else f"{os.path.splitext(a.out)[0]}_{name}.npz"
            np.savez(fn, **{sweep[0]: sweep[1]}, states=membrane.states, steps_taken=steps,
                     state_names=np.array(state_names(module)))
            print(f"wrote {fn}: {len(sweep[1])} rest states over {sweep[0]} = {sweep[1][0]:g} .. {sweep[1][-1]:g}")
        if a.history:
            fn = a.history if len(names) == 1 else f"{os.path.splitext(a.history)[0]}_{name}.npz"
            np.savez(fn, every=a.every, dt=conditions(name)[1], **hist)
            print(f"wrote {fn}")


if __name__ == "__main__":
    main()
