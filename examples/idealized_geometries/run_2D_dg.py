"""The 2D idealized run (`run_2D.py:137-372` of the reference: one cell in the ECS, K / Cl / Na, Hodgkin-Huxley membrane,
synaptic stimulus on x < 20 um) with the DG(P1) + interior-penalty variant (`knpemi.dg.DGProblem`):
membrane ODEs at the facet nodes, both assemblies, both linear solves (CG / BiCGStab + auxiliary-space AMG,
`knpemi_dg_solve_emi/knp`) and the end-of-step update on the GPU; `--host-solves` solves the two systems with SciPy
from the CSR the kernels fill instead.

    python run_2D_dg.py [--resolution 1] [--steps 100] [--host-solves] [--series s.npz] [--events e.npz] [--balance b.npz]
                        [--snapshots DIR [--save-every N] [--snapshot-form vertex|broken|cell_mean]]

`--series` records on the device, at the end of every step, phi and the ions at the ECS and ICS points of run_2D.py's
`--series`, phi_M and the traces at its membrane point, the maximum and the average of K in the ECS and the jump seminorms
of phi and of K in both sub-domains (`knpemi.dg_recording.DGObservables`); `--events` the upward crossings of -20 mV per
membrane node (`DGMembraneEvents`, re-armed 20 mV below, the latest 8 times kept); `--balance` the per-cell ion balance
(`knpemi.dg_balance.DGIonBalance`): per sub-domain and ion the mass, the summed outflow, the penalty share and the largest
conservation defect, per membrane tag the ion transfer on both sides and the currents, and the cell table of the last step.
`--snapshots DIR` saves the fields every `--save-every` steps without stopping the run (`knpemi.dg_snapshots.DGSnapshots`):
phi and every ion per sub-domain and phi_M of the membrane, packed on the device in the form `--snapshot-form` -- "vertex"
(one value per mesh vertex, the layout of the reference's results_sub_<tag>.xdmf / results_mem_<tag>.xdmf), "broken" (every
dof, on the exploded mesh) or "cell_mean" -- into DIR/step_%06d.npz and, for the two nodal forms, XDMF time series.

`--cell-type quadrilateral` is parsed, as in run_2D.py, and refused with the DG module's message: the DG variant has no
quadrilateral kernels.
"""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "knp-emi-fenics-x_amd"))
sys.path.insert(0, HERE)

import mm_hh                                                       # noqa: E402
from setup_problem import (C_M, CL_E, CL_I, D_CL, D_K, D_NA, DT, FARADAY, K_E, K_I, NA_E, NA_I, PSI)  # noqa: E402
from knpemi import _lib as L                                       # noqa: E402
from knpemi.dg import DGProblem                                    # noqa: E402
from knpemi.dg_balance import DGIonBalance                         # noqa: E402
from knpemi.dg_recording import DGMembraneEvents, DGObservables    # noqa: E402
from knpemi.dg_snapshots import DGSnapshots, DGXdmfSink, NpzSink   # noqa: E402
from knpemi.fem.idealized import make_mesh_2D                      # noqa: E402


def solve_singular(A, b):
    """Pure Neumann potential system: bordered solve orthogonal to the constants (pdeSolver.py:74-78)."""
    n = A.shape[0]
    e = np.full((n, 1), 1.0 / np.sqrt(n))
    K = sp.bmat([[A, sp.csr_matrix(e)], [sp.csr_matrix(e.T), None]], format="csc")
    return spla.splu(K).solve(np.concatenate([b, [0.0]]))[:n]


FIGURE_POINTS = dict(ECS=(25e-6, 3.5e-6), ICS=(25e-6, 2e-6), mem=(25e-6, 3e-6))      # run_2D.py: FIGURE_POINTS[2], in m
EVENT_THRESHOLD = -20e-3                                           # run_2D.py: --event-threshold


class DGRun:
    def __init__(self, resolution=1, g_syn=10.0, dt=DT, device_solves=True, rtol=(1e-5, 1e-7), cell_type="triangle",
                 series=None, events=None, balance=None, snapshots=None, save_every=1, snapshot_form="vertex", sinks=None):
        """series / events / balance: paths of the .npz files `save` writes (None: not recorded).  snapshots: the directory
        of the field files (None: no fields saved), one frame every `save_every` steps in the form `snapshot_form`; sinks:
        the sinks to use instead of the files (a list; `snapshots` may then be any true value)."""
        self.device_solves, self.rtol, self.iterations = device_solves, rtol, []
        self.series, self.events, self.obs, self.ev = series, events, None, None
        self.balance, self.bal = balance, None
        self.snap = None
        mesh, ct, ft = make_mesh_2D(resolution, cell_type=cell_type)      # quadrilaterals: DGProblem refuses them
        self.dp = dp = DGProblem(mesh, ct, ft, [0, 1], [1])
        self.ions = [dict(name="K", z=1.0, D=[D_K] * 2), dict(name="Cl", z=-1.0, D=[D_CL] * 2), dict(name="Na", z=1.0, D=[D_NA] * 2)]
        dp.set_params(dict(dt=dt, F=FARADAY, psi=PSI, C_M=C_M), self.ions)
        ins = (dp.cell_sub > 0)[:, None] * np.ones((1, dp.nv), bool)
        for k, (e, i) in enumerate(((K_E, K_I), (CL_E, CL_I), (NA_E, NA_I))):
            dp.set_concentration(k, np.where(ins, i, e))
        nq = dp.nmf * dp.nf
        ode = mm_hh
        states = np.tile(np.asarray(ode.init_state_values(), float), (nq, 1))
        params = np.tile(np.asarray(ode.init_parameter_values(), float), (nq, 1))
        pi = ode.parameter_indices
        params[:, pi("Cm")] = C_M
        params[:, pi("psi")] = PSI
        for n, z in (("Na", 1.0), ("K", 1.0), ("Cl", -1.0)):
            params[:, pi("z_" + n)] = z
        self.stimulated = dp.XM.reshape(nq, 2)[:, 0] < 20e-6       # stimulus_locator of run_2D.py:268-270
        params[self.stimulated, pi("stim_amplitude")] = g_syn
        ion_param = sum(([pi(f"{i['name']}_e"), pi(f"{i['name']}_i"), pi(f"I_ch_{i['name']}")] for i in self.ions), [])
        self.v_index = ode.state_indices("V")
        dp.ode_bind(L.MODEL_HH_SI, states, params, ion_param, self.v_index)
        if device_solves:
            dp.set_extrapolation(True)
        self.dt, self.time, self.k = dt, 0.0, 0
        if series:
            self.obs = obs = DGObservables(mesh, ct, ft, [0, 1], [1], [i["name"] for i in self.ions])
            obs.point("ECS", FIGURE_POINTS["ECS"], tag=0)
            obs.point("ICS", FIGURE_POINTS["ICS"], tag=1)
            obs.membrane_point("mem", FIGURE_POINTS["mem"], 1)
            obs.reduce("K_ecs_max", "c", 0, "max", ion="K")
            obs.reduce("K_ecs_avg", "c", 0, "average", ion="K")
            for tag, side in ((0, "ecs"), (1, "ics")):
                obs.jump(f"J_phi_{side}", "phi", tag)
                obs.jump(f"J_K_{side}", "c", tag, ion="K")
            dp.observe(obs)
        if events:
            self.ev = ev = DGMembraneEvents(mesh, ft, [1])
            ev.watch(EVENT_THRESHOLD, reset=EVENT_THRESHOLD - 20e-3, keep=8)
            dp.detect(ev)
        if balance:
            self.bal = DGIonBalance(mesh, ct, ft, [0, 1], [1], [i["name"] for i in self.ions])
            dp.balance(self.bal)
        if snapshots:
            self.snap = snap = DGSnapshots(mesh, ct, ft, [0, 1], [1], [i["name"] for i in self.ions])
            snap.watch_results(form=snapshot_form)
            if sinks is None:
                sinks = [NpzSink(snapshots)] + ([] if snapshot_form == "cell_mean" else [DGXdmfSink(snap, snapshots)])
            for s in sinks:
                snap.add_sink(s)
            dp.snapshot(snap, every=save_every)           # behind the other recorders: attached last

    def step(self):
        dp = self.dp
        dp.ode_step(self.time, self.dt, set_v=self.k > 0)           # traces -> LSODA -> phi_M, I_ch
        dp.assemble_emi()
        if self.device_solves:                                       # pdeSolver.py:24-35,99-110 (rtol 1e-5 / 1e-7)
            it_emi = dp.solve_emi(rtol=self.rtol[0])[0]
            dp.assemble_knp()
            dp.record_membrane()                                     # the ion balance's first launch, when one is due
            it_knp = dp.solve_knp(rtol=self.rtol[1], update=True)[0]
            self.iterations.append((it_emi, it_knp))
        else:
            phi = solve_singular(dp.matrix(0), dp.rhs(0))
            dp.set_potential(phi)
            dp.assemble_knp()
            dp.record_membrane()
            c_new = np.stack([spla.splu(dp.matrix(1 + k).tocsc()).solve(dp.rhs(1 + k)) for k in range(2)])
            dp.update(c_new)
        n_rhs, n_steps, n_failed = dp.ode_stats()
        assert n_failed == 0                                         # odeSolver.py:121
        self.time += self.dt
        self.k += 1
        dp.record(self.time)

    def save(self):
        if self.obs is not None:
            self.obs.save(self.series)
        if self.ev is not None:
            self.ev.save(self.events)
        if self.bal is not None:
            self.bal.save(self.balance)
        if self.snap is not None:
            self.snap.close()


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--host-solves", action="store_true")
    ap.add_argument("--cell-type", choices=["triangle", "quadrilateral"], default="triangle")
    ap.add_argument("--series", metavar="PATH", default=None, help="time series of the observables and jump seminorms (.npz)")
    ap.add_argument("--events", metavar="PATH", default=None, help="membrane events per membrane node (.npz)")
    ap.add_argument("--balance", metavar="PATH", default=None, help="per-cell ion balance: series and last cell table (.npz)")
    ap.add_argument("--snapshots", metavar="DIR", default=None, help="field files: step_%%06d.npz and XDMF time series")
    ap.add_argument("--save-every", type=int, default=1, help="steps between two saved frames")
    ap.add_argument("--snapshot-form", choices=["vertex", "broken", "cell_mean"], default="vertex")
    return ap


if __name__ == "__main__":
    a = build_parser().parse_args()
    run = DGRun(a.resolution, device_solves=not a.host_solves, cell_type=a.cell_type, series=a.series, events=a.events,
                balance=a.balance, snapshots=a.snapshots, save_every=a.save_every, snapshot_form=a.snapshot_form)
    for k in range(a.steps):
        run.step()
        if (k + 1) % 10 == 0:
            v = run.dp.get_membrane_potential()
            its = f"   iterations {run.iterations[-1]}" if run.iterations else ""
            print(f"t = {run.time * 1e3:5.1f} ms   phi_M: mean {v.mean() * 1e3:8.3f} mV, max {v.max() * 1e3:8.3f} mV{its}")
    run.save()
