"""Device-resident time stepping of the hot path.

The reference API keeps every field in host numpy arrays (`Function.x.array`), so its drop-in
(`pdeSolver.LinearProblem.solve`, `MembraneModel.step_lsoda`) mirrors data across PCIe at every
call.  `DeviceStepper` runs the same sequence of one time step of `run_3D.py:345-368`

    solve_odes  ->  assemble EMI (A, P, b)  ->  [solve]  ->  assemble KNP (A, b)  ->  [solve]
                ->  update_pde_variables

with all fields, tables and operators resident in HBM, calling the C ABI directly.  The linear
solves are not part of the hot path; a caller plugs them in through
`solve_emi` / `solve_knp` callbacks that receive the device problem (device CSR pointers are
available from `knpemi_device_csr`).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .recording import Tap


class DeviceStepper:
    def __init__(self, forms_emi, forms_knp, c, c_prev, phi, phi_M_prev, solve_emi=None, solve_knp=None,
                 assemble_knp_twice=False, overlap=True, device_solves=None, extrapolate_guess=True,
                 fuse_update=None, fuse_membrane=False, early_membrane=False, knp_method="gmres",
                 ode_method="lsoda", ode_substeps=None):
        a = forms_emi[0]
        self.dp = a.dp
        self.a = a
        self.lib = self.dp.lib
        self.c, self.c_prev, self.phi, self.phi_M_prev = c, c_prev, phi, phi_M_prev
        if device_solves is not None:
            # (rtol_emi, rtol_knp): Krylov solves on the device between the assemblies (knpemi_solve_emi/knp)
            # extrapolate_guess: start each solve from 2 x_n - x_(n-1) instead of x_n (knpemi_extrapolate_guess)
            rtol_emi, rtol_knp = device_solves
            self.iterations = []
            # the concentration solve: "gmres" = the reference's options as PETSc runs them (pdeSolver.py:99-110),
            # "bicgstab" = the faster device path (knpemi.pdeSolver.set_knp_solver_options)
            from .pdeSolver import set_emi_solver_options, set_knp_solver_options
            set_knp_solver_options(a.dp, knp_method)
            set_emi_solver_options(a.dp, "preconditioned" if knp_method == "gmres" else "true")

            def _solve(dp, which, name, rtol, atol):
                if extrapolate_guess:
                    L.check(dp.lib.knpemi_extrapolate_guess(dp.h, which))
                self.iterations.append((name,) + dp.solve(which, rtol, atol))
            solve_emi = lambda dp: _solve(dp, L.B_EMI, "emi", rtol_emi, 1e-40)
            solve_knp = lambda dp: _solve(dp, L.B_KNP, "knp", rtol_knp, 2e-40)
        self.solve_emi, self.solve_knp = solve_emi, solve_knp
        # fuse_update: the write-back kernel of the device KNP solve (or of a device-side set_solution) also performs
        # update_pde_variables, which follows the solve directly in the reference's loop (run_3D.py:356,362): one
        # launch fewer per step.  Default: on with the device solves, off with caller-supplied callbacks.
        self.fuse_update = bool(device_solves is not None) if fuse_update is None else bool(fuse_update)
        self.assemble_knp_twice = assemble_knp_twice
        self.overlap = overlap
        # Which of the two overlapped kernels runs on the auxiliary stream: the one that finishes first, so that the
        # kernels after the join follow the longer one on the same stream without a cross-stream signal (~15 us).
        # Decided from their measured durations at the first step (None = not yet known).
        self.ode_on_aux = None
        import os
        self.overlap_threshold_ms = float(os.environ.get("KNPEMI_OVERLAP_THRESHOLD_MS", "0.025"))     # (0: always side by side)
        # With one membrane model the overlapped step first asks the library for ONE launch that holds the sweep and
        # the matrix (knpemi_ode_step_emi; eligibility is the library's, KNPEMI_FUSED_SWEEP=0 disables it).  fused_sweep:
        # None = not asked yet, False = the library declined (the streams above take over); last_fused: what the
        # latest step's call reported (None: the step made no such call).
        self.fused_sweep = None
        self.last_fused = None
        self.k = 0
        self.models = []   # MembraneModel objects, in registration order
        self._model_setup = []   # (MembraneModel, stimulus, locator, initial time) for reset()
        # integrator of every membrane model (MembraneModel.set_integrator): "lsoda", or "euler" / "rk4" / "rush_larsen"
        # with ode_substeps sub-steps per time step (None: 25, the reference drivers' n_steps_ODE)
        if ode_method not in L.ODE_METHODS:
            raise ValueError(f"unknown ode_method {ode_method!r}: one of {sorted(L.ODE_METHODS)}")
        self.ode_method, self.ode_substeps = ode_method, ode_substeps
        dp = self.dp
        dp.set_params(a.physical_params, a.ion_list, a.dt)
        L.check(self.lib.knpemi_set_option(dp.h, L.OPT_FUSE_UPDATE, 1 if self.fuse_update else 0))
        # membrane-facet integrals of b_knp inside the KNP row kernel (default) or as a launch of their own
        self.fuse_membrane = bool(fuse_membrane)
        # membrane-facet integrals of b_knp prepared beside the EMI solve (knpemi_assemble_knp_membrane_early): takes the
        # facet kernel off the chain between the two solves but lengthens the membrane rows of the KNP row kernel by
        # more than it saves (config 2: 0.187 -> 0.193 ms per step), hence off by default
        self.early_membrane = bool(early_membrane) and not self.fuse_membrane
        L.check(self.lib.knpemi_set_option(dp.h, L.OPT_FUSE_MEMBRANE, 1 if self.fuse_membrane else 0))
        self.dt = float(a.dt)
        self.flags_emi = L.WANT_P | (0 if a.splitting_scheme else L.NO_SPLITTING)
        self.flags_knp = 0 if a.splitting_scheme else L.NO_SPLITTING
        # the attached recorders (knpemi.recording.Tap) by the method that attached them: "exchange" records behind the
        # last KNP assembly of a step, "observe", "detect", "fluxes", "track", "monitor" and "snapshot", in this order,
        # behind the end-of-step update
        self.taps = {}
        self.upload()

    # -- host <-> device ------------------------------------------------------------------
    def upload(self):
        """Push every Function and ODE table to the device (start of a run)."""
        dp, a = self.dp, self.a
        n_solved = len(a.ion_list) - 1
        for tag, sd in a.subdomain_list.items():
            s = dp.sub_index[tag]
            dp.push(L.F_PHI, s, 0, self.phi[tag])
            for k in range(n_solved):
                dp.push(L.F_C_PREV, s, k, self.c_prev[tag][k])
                dp.push(L.F_C, s, k, self.c[tag][k])
            dp.push(L.F_C_ELIM, s, 0, a.ion_list[-1][f'c_{tag}'])
            if tag > 0:
                dp.push(L.F_PHI_M, s, 0, self.phi_M_prev[tag])
                for j, mm in enumerate(sd.get('mem_models', [])):
                    for k, ion in enumerate(a.ion_list):
                        dp.push(L.F_I_CH, s, j * L.MAX_IONS + k, mm['I_ch_k'][ion['name']])

    def set_source(self, ion_index, values):
        """Nodal ECS source term of solved ion `ion_index` (`ion['f_source']`, knpWeakForm.py:164-166)."""
        self.dp.push_array(L.F_SOURCE, 0, int(ion_index), np.ascontiguousarray(values, np.float64))

    def add_membrane_model(self, ode_model, stimulus=None, stimulus_locator=None):
        """Register a bound MembraneModel: uploads its tables and stimulus once."""
        dp = self.dp
        ode_model.set_integrator(self.ode_method, self.ode_substeps)
        stimulus = stimulus or {}
        if stimulus_locator is None:
            mask = np.ones(ode_model.nodes, np.uint8)
        else:
            mask = np.fromiter(map(stimulus_locator, ode_model.dof_locations), dtype=bool).astype(np.uint8)
        sidx = np.array([ode_model.ode.parameter_indices(k) for k in stimulus], np.int32)
        sval = np.array([float(v) for v in stimulus.values()], np.float64)
        L.check(self.lib.knpemi_ode_set_stimulus(
            dp.h, ode_model._sub, ode_model._model, mask.ctypes.data_as(L.c_u8_p), len(sidx),
            L.iptr(sidx) if len(sidx) else None, L.dptr(sval) if len(sval) else None))
        st = np.ascontiguousarray(ode_model.states)
        pa = np.ascontiguousarray(ode_model.parameters)
        L.check(self.lib.knpemi_ode_set_tables(dp.h, ode_model._sub, ode_model._model, L.dptr(st), L.dptr(pa)))
        if ode_model not in self.models:
            self.models.append(ode_model)
            self.fused_sweep = None        # another set of models: the library decides again
            self._model_setup.append((ode_model, dict(stimulus), stimulus_locator, float(ode_model.time)))

    def reset(self):
        """Back to the state of the host objects (fields, ODE tables, times): a second run from the same start."""
        self.dp._uploaded.clear()      # the device copies have moved on although the host versions have not
        self.upload()
        for m, stim, loc, t0 in self._model_setup:
            m.time = t0
            self.add_membrane_model(m, stim, loc)
        self.k = 0
        self.ode_failures()            # clears the counters of the previous run
        for tap in self.taps.values():      # new series, new maps
            tap.reset()

    # -- observables -------------------------------------------------------------------------------
    def observe(self, obs, every=1, capacity=1024, t0=0.0, halo=None):
        """Record the observables `obs` (knpemi.observables.Observables) on the device after every `every`-th step,
        at time t0 + k dt for step k.  Rows collect in a device buffer of `capacity` rows; the host keeps the times of
        the rows it has enqueued and drains the buffer into `obs` (one synchronisation) whenever it holds `capacity`
        of them, and when `obs.series()` is called.

        halo: this rank's attached halo on a cell-partitioned problem (collective: every rank calls observe with the
        same definitions, every and capacity).  Every rank then records the global row -- partial rows summed over the
        ranks on the device at each record (Observables.partition) -- and `step(halo)` records with the same halo.
        Draining stays rank-local."""
        lib, dp = self.lib, self.dp
        read = self._reader(lib.knpemi_observe_read)
        self._attach("observe", obs, "observables", every, capacity, t0, halo=halo, read=read,
                     attached="these observables are attached to a stepper already",
                     set_up=lambda: (obs.upload(dp, capacity) if halo is None
                                     else obs.upload_partitioned(dp, capacity, halo, every)),
                     record=lambda t, f: lib.knpemi_observe_record(dp.h), rewind=lambda: read(0, None),
                     partition_refusal="observables attached without a halo are not recorded on partitioned steps: "
                                       "pass halo= to DeviceStepper.observe")

    def _attach(self, name, rec, label, every, capacity, t0, *, set_up, record, rewind, busy=None, attached=None,
                read=None, fields=False, offset=0, halo=None, partition_refusal=None):
        """The attach path of every recorder: the checks (capacity None: a recorder without a row buffer; busy / attached:
        the messages of a second recorder of this kind on the stepper / of a recorder that drains into a stepper
        already), set_up() -> what the handle then refers to, and the tap `self.taps[name]`.  record(t, fields) returns
        the status of knpemi_*_record."""
        if capacity is None and every < 1:
            raise ValueError("every must be positive")
        if capacity is not None and (every < 1 or capacity < 1):
            raise ValueError("every and capacity must be positive")
        if busy is not None and name in self.taps:
            raise RuntimeError(busy)
        if attached is not None and rec._drain is not None:
            raise RuntimeError(attached)
        if halo is not None and halo.dp is not self.dp:
            raise ValueError(f"{name}(halo=...): attach the halo to this stepper's problem first (halo.attach)")
        keep = set_up()

        def enqueue(t, f):
            rc = record(t, f)
            err = getattr(halo, "_hook_error", None)
            if rc != L.OK and err is not None:      # the all-reduce of a partitioned record failed in Python
                raise err
            L.check(rc)
        self.taps[name] = Tap(rec, label, every, enqueue, t0, offset, capacity if read is not None else None, read,
                              rec.n_cols if read is not None else 0, rewind, fields, halo=halo,
                              partition_refusal=partition_refusal, keep=keep)

    def _reader(self, fn):
        """read(n, buf) -> (rows, dropped) of a tap, from the recorder's knpemi_*_read with reset."""
        def read(n, buf):
            rows, over = C.c_int64(), C.c_int64()
            L.check(fn(self.dp.h, n, None if buf is None else L.dptr(buf), C.byref(rows), C.byref(over), 1))
            return rows.value, over.value
        return read

    # -- membrane events ---------------------------------------------------------------------------
    def detect(self, ev, every=1, t0=0.0):
        """Record the membrane events `ev` (knpemi.events.MembraneEvents) on the device after every `every`-th step,
        at time t0 + k dt for step k: one launch over the membrane dofs of every watched cell, nothing synchronised;
        `ev.maps(tag)` reads the maps back.  Works unchanged on a cell-partitioned problem (`step(halo)`): the kernel
        needs no halo, every rank holds the events of its local dofs, and `ev.maps(tag, halo=halo)` selects the owned
        ones."""
        lib, dp = self.lib, self.dp

        def set_up():
            ev._attach(lib, dp.h, dp.sub_index)
            ev.reset_host()

        def rewind():
            L.check(lib.knpemi_events_reset(dp.h))
            ev.reset_host()
        self._attach("detect", ev, "membrane events", every, None, t0, set_up=set_up, rewind=rewind,
                     busy="this stepper records membrane events already",
                     record=lambda t, f: lib.knpemi_events_record(dp.h, t))

    # -- ion fluxes ---------------------------------------------------------------------------------
    def fluxes(self, fl, every=1, capacity=1024, t0=0.0, fields=False, halo=None):
        """Record the ion fluxes `fl` (knpemi.fluxes.IonFluxes) on the device after every `every`-th step, at time
        t0 + k dt for step k: one launch over the cells of every watched sub-domain on the main stream, behind the
        end-of-step update, where observables and events record.  Rows collect in a device buffer of `capacity` rows;
        the host keeps the times of the rows it has enqueued and drains the buffer into `fl` (one synchronisation)
        whenever it holds `capacity` of them, and when `fl.series()` is called.  fields: every record also writes the
        per-cell vectors (`fl.fields(tag)` reads those of the latest record).

        halo: this rank's attached halo on a cell-partitioned problem (collective: every rank calls fluxes with the same
        watches, every and capacity).  Every rank then records the global row -- every cell counted by one rank, the
        partial rows summed over the ranks on the device at each record (WatchedIons.partition) -- and `step(halo)`
        records with the same halo; `fl.fields(tag, halo=halo)` reads the local cells.  Draining stays rank-local.
        Without it, partitioned steps (`step(halo)`) are refused: a rank's sums would include its ghost cells."""
        self._attach_watched("fluxes", "flux", fl, "ion fluxes", every, capacity, t0, fields, halo,
                             busy="this stepper records ion fluxes already",
                             attached="these fluxes are attached to a stepper already",
                             partition_refusal="ion fluxes attached without a halo are not recorded on partitioned steps "
                                               "(a rank's sums would include its ghost cells): pass halo= to "
                                               "DeviceStepper.fluxes")

    def _attach_watched(self, name, kind, rec, label, every, capacity, t0, fields, halo, offset=0, **messages):
        """`_attach` for the watches of `rec` (IonFluxes, MembraneExchange: knpemi_<kind>_*), with a halo their
        partitioned table."""
        lib, h = self.lib, self.dp.h
        record, reset = getattr(lib, f"knpemi_{kind}_record"), getattr(lib, f"knpemi_{kind}_reset")
        self._attach(name, rec, label, every, capacity, t0, fields=fields, offset=offset, halo=halo,
                     set_up=lambda: rec._attach(self.dp, capacity, halo, every), record=lambda t, f: record(h, f),
                     read=self._reader(getattr(lib, f"knpemi_{kind}_read")), rewind=lambda: L.check(reset(h)), **messages)

    # -- membrane ion exchange --------------------------------------------------------------------------
    def exchange(self, ex, every=1, capacity=1024, t0=0.0, fields=False, halo=None):
        """Record the membrane exchange `ex` (knpemi.exchange.MembraneExchange) on the device in every `every`-th
        step: one launch over the membrane facets of the watched cells on the main stream, directly behind the last
        KNP assembly of the step and before the KNP solve -- the only moment the device holds the new potential, the old
        c_prev, the post-ODE phi_M_prev and the new I_ch together (the fused KNP write-back and the end-of-step update
        overwrite three of them).  The row of step k (counted from 0) carries the time t0 + (k + 1) dt, the end of the
        step whose mean rate it is.  Rows collect in a device buffer of `capacity` rows; the host keeps the times of the
        rows it has enqueued and drains the buffer into `ex` (one synchronisation) whenever it holds `capacity` of them,
        and when `ex.series()` is called.  fields: every record also writes the per-facet means (`ex.fields(tag)`
        reads those of the latest record).

        halo: this rank's attached halo on a cell-partitioned problem (collective, as `fluxes`): every membrane facet is
        counted by one rank, every rank records the global row, `step(halo)` records with the same halo and
        `ex.fields(tag, halo=halo)` reads the local facets.  `ex.budget` then pairs the series with that of
        `observe(obs, halo=halo)`.
        Without it, partitioned steps (`step(halo)`) are refused: a rank's sums would include its ghost facets."""
        # offset 1: the record sits inside step k, counted from 0, and carries the time of the step's end
        self._attach_watched("exchange", "exchange", ex, "membrane exchange", every, capacity, t0, fields, halo, offset=1,
                             busy="this stepper records a membrane exchange already",
                             attached="this exchange is attached to a stepper already",
                             partition_refusal="a membrane exchange attached without a halo is not recorded on "
                                               "partitioned steps (a rank's sums would include its ghost facets): pass "
                                               "halo= to DeviceStepper.exchange")
        ex._dt, ex._every = self.dt, int(every)

    # -- field maps -----------------------------------------------------------------------------------
    def track(self, fm, every=1, capacity=1024, t0=0.0, halo=None):
        """Record the field maps `fm` (knpemi.maps.FieldMaps) on the device after every `every`-th step, at time
        t0 + k dt for step k: one launch over the items of every watched space on the main stream, behind the end-of-step
        update and the other recorders, nothing synchronised; `fm.maps(name)` reads the maps back.  With a series watch
        the launch also appends a row to a device buffer of `capacity` rows, drained into `fm` as the other series are
        (whenever it holds `capacity` rows, and when `fm.series()` is called); without one there is no buffer.
        Works unchanged on a cell-partitioned problem (`step(halo)`) without a series watch: the kernel needs no halo,
        every rank holds the maps of its local items, and `fm.maps(name, halo=halo)` selects the owned ones.

        halo: this rank's attached halo on a cell-partitioned problem, for maps with a series watch (collective: every rank
        calls track with the same watches, every and capacity).  Every rank then records the global series row -- the
        measure from the cells (facets) one rank records, n from the items one rank owns, the partial rows summed over the
        ranks on the device at each record (FieldMaps.partition) -- and `step(halo)` records with the same halo.
        Without it, partitioned steps are refused with a series watch: a rank's sums would include its ghost items."""
        lib, dp = self.lib, self.dp
        series = fm.has_series
        if halo is not None and not series:
            raise ValueError("track(halo=...): no watch has a series; maps without one need no halo")

        def set_up():
            keep = fm._attach(dp, capacity, halo, every)
            fm.reset_host()
            return keep

        def rewind():
            L.check(lib.knpemi_maps_reset(dp.h))
            fm.reset_host()
        self._attach("track", fm, "field maps", every, capacity, t0, set_up=set_up, rewind=rewind, halo=halo,
                     busy="this stepper records field maps already",
                     attached="these maps are attached to a stepper already",
                     record=lambda t, f: lib.knpemi_maps_record(dp.h, t),
                     read=self._reader(lib.knpemi_maps_series_read) if series else None,
                     partition_refusal="field maps with a series watch are not recorded on partitioned steps (a rank's "
                                       "sums would include its ghost items): track maps without series=True"
                                       if series else None)

    # -- membrane monitors ------------------------------------------------------------------------------
    def monitor(self, mon, every=1, capacity=1024, t0=0.0, fields=False, halo=None):
        """Record the membrane monitors `mon` (knpemi.monitor.MembraneMonitor) on the device after every `every`-th
        step, at time t0 + k dt for step k: one launch over the membrane dofs of the watched model slots on the main
        stream, behind the end-of-step update and the other recorders.  It sees the state the next sweep would start
        from and writes nothing but its own buffers.  Rows collect in a device buffer of `capacity` rows, drained into
        `mon` as the other series are (whenever it holds `capacity` rows, and when `mon.series()` is called).  fields:
        every record also writes the per-dof arrays (`mon.values(tag)` reads those of the latest record).

        halo: this rank's attached halo on a cell-partitioned problem (collective: every rank calls monitor with the same
        watches, points, reductions, every and capacity; `mon` is built with partitioned=True).  Every rank then records
        the global row -- every membrane facet counted by one rank, the partial rows exchanged and folded on the device at
        each record (MembraneMonitor.partition) -- and `step(halo)` records with the same halo; `mon.values(tag, halo=halo)`
        reads the owned dofs.  Draining stays rank-local.
        Without it, partitioned steps (`step(halo)`) are refused: a rank's reductions would include its ghost dofs."""
        lib, dp = self.lib, self.dp
        self._attach("monitor", mon, "membrane monitors", every, capacity, t0, fields=fields, halo=halo,
                     busy="this stepper records membrane monitors already",
                     attached="this monitor is attached to a stepper already",
                     set_up=lambda: mon._attach(dp, capacity, halo, every), read=self._reader(lib.knpemi_monitor_read),
                     record=lambda t, f: lib.knpemi_monitor_record(dp.h, float(t), f),
                     rewind=lambda: L.check(lib.knpemi_monitor_reset(dp.h)),
                     partition_refusal="membrane monitors are not recorded on partitioned steps (a rank's reductions "
                                       "would include its ghost dofs): run DeviceStepper.monitor on one rank")

    # -- field snapshots --------------------------------------------------------------------------------
    def snapshot(self, snap, every=1, depth=4, t0=0.0):
        """Snapshot the watched fields of `snap` (knpemi.snapshots.Snapshots) after every `every`-th step, at time
        t0 + k dt for step k: one pack launch on the main stream, behind the end-of-step update and every other recorder,
        then the copy of the frame to pinned host memory on a stream of its own; nothing waits for the host.  The ring
        holds `depth` frames; a tick first hands the frames whose copy is done to the writer, and only a full ring makes
        it wait, for the oldest frame alone (`snap.stalls`).  `snap.flush()` brings every recorded frame to the sinks.
        Works unchanged on a cell-partitioned problem (`step(halo)`): the kernel needs no halo and every rank snapshots
        its local items; `snap.select_owned(halo)` stores the owned ones only."""
        lib, dp = self.lib, self.dp
        if depth < 1:
            raise ValueError("depth must be positive")

        def rewind():
            snap._rewind()
        self._attach("snapshot", snap, "field snapshots", every, None, t0, rewind=rewind,
                     busy="this stepper takes field snapshots already",
                     attached="these snapshots are attached to a stepper already",
                     set_up=lambda: snap._attach(dp, int(depth)), record=lambda t, f: snap._tick(t, self.k))

    def check_ode_failures(self):
        """`assert success` of odeSolver.py:121 for the device-resident loop: raises KnpemiError(EODE) when LSODA
        failed on any membrane dof since the last check (the counters live on the device; this synchronises)."""
        n = self.ode_failures()
        if n:
            if self.ode_method != "lsoda":
                raise L.KnpemiError(L.EODE, f"{self.ode_method} left a non-finite state on {n} membrane dof(s)")
            raise L.KnpemiError(L.EODE, f"LSODA failed on {n} membrane dof(s) (odeSolver.py:121 `assert success`)")

    def download(self):
        """Pull fields and ODE tables back into the host objects (end of a run / output).  A dof on which LSODA
        failed keeps a wrong V / I_ch that has fed the PDEs: the download refuses to hand such results out."""
        self.check_ode_failures()
        dp, a = self.dp, self.a
        n_solved = len(a.ion_list) - 1
        for tag, sd in a.subdomain_list.items():
            s = dp.sub_index[tag]
            dp.pull(L.F_PHI, s, 0, self.phi[tag])
            for k in range(n_solved):
                dp.pull(L.F_C_PREV, s, k, self.c_prev[tag][k])
                dp.pull(L.F_C, s, k, self.c[tag][k])
            dp.pull(L.F_C_ELIM, s, 0, a.ion_list[-1][f'c_{tag}'])
            if tag > 0:
                dp.pull(L.F_PHI_M, s, 0, self.phi_M_prev[tag])
                for j, mm in enumerate(sd.get('mem_models', [])):
                    for k, ion in enumerate(a.ion_list):
                        dp.pull(L.F_I_CH, s, j * L.MAX_IONS + k, mm['I_ch_k'][ion['name']])
        for m in self.models:
            st = np.ascontiguousarray(m.states)
            pa = np.ascontiguousarray(m.parameters)
            L.check(self.lib.knpemi_ode_get_tables(dp.h, m._sub, m._model, L.dptr(st), L.dptr(pa)))
            m.states[...] = st
            m.parameters[...] = pa

    # -- one time step, everything enqueued on the handle's stream ---------------------------
    def step(self, halo=None):
        dp, lib = self.dp, self.lib
        for tap in self.taps.values():
            tap.refuse_partitioned(halo)
        if halo is not None and (self.solve_emi is not None or self.solve_knp is not None) \
                and not getattr(halo, "supports_solves", False):
            raise NotImplementedError(
                "this halo does not distribute the linear solves: knpemi_solve_emi/knp on a partitioned problem "
                "need the halo'd SpMV and the all-reduced dot products (knpemi.fem.partition.DistributedSolves)")
        flags = L.ODE_SET_TRACES | (L.ODE_SET_V if self.k > 0 else 0)
        self.last_fused = None
        if self.overlap and len(self.models) == 1 and self.fused_sweep is not False:
            # the sweep and the EMI matrix (A, P, volume part of b: they do not depend on the sweep's output) in one
            # launch where the library finds the problem eligible, one after the other on the main stream where not;
            # no stream calibration in such a step: there is no emi_rows bracket to read
            m = self.models[0]
            fused = C.c_int(0)
            L.check(lib.knpemi_ode_step_emi(dp.h, m._sub, m._model, float(m.time), self.dt, m.rtol, m.atol, flags,
                                            L.iptr(m._ion_param), int(m.V_index), self.flags_emi, C.byref(fused)))
            m.time = m.time + self.dt
            self.last_fused = fused.value
            self.fused_sweep = bool(fused.value)     # declined: the next steps run the two on two streams
            L.check(lib.knpemi_assemble_emi_membrane_rhs(dp.h, self.flags_emi))
        else:
            self._sweeps_and_emi(flags)
        self._rest_of_step(halo)

    def _sweeps_and_emi(self, flags):
        """The membrane sweeps and the assembly of the potential system as launches of their own: side by side on two
        streams (overlap) or in the reference's order on one."""
        dp, lib = self.dp, self.lib
        calibrate = self.overlap and self.ode_on_aux is None and self.models
        if calibrate:
            L.check(lib.knpemi_profile(dp.h, (1 << L.KERNEL_NAMES.index("ode_step_kernel"))
                                       | (1 << L.KERNEL_NAMES.index("emi_rows_kernel"))))
        ode_aux = bool(self.overlap and self.ode_on_aux)
        if self.overlap and not ode_aux:
            # the EMI matrix (A, P, volume part of b) does not depend on the ODE output: assemble it on the
            # auxiliary stream while the ODE sweep runs on the main one
            L.check(lib.knpemi_assemble_emi(dp.h, self.flags_emi | L.SKIP_MEMBRANE_RHS | L.ON_AUX_STREAM))
        side_of_sub = {}
        for m in self.models:
            # The sweeps of different cells (sub-domains) are independent: the first cell's models share the main /
            # auxiliary stream pair with the EMI assembly, the other cells' run beside them on the second auxiliary
            # stream.  Several models of ONE cell integrate the same dofs and overwrite phi_M_prev in turn
            # (odeSolver.py:31-38, benchmark/run_stim_duration.py:163-166): they stay in order on one stream.
            if m._sub not in side_of_sub:
                side_of_sub[m._sub] = L.ODE_ON_AUX2 if side_of_sub else (L.ODE_ON_AUX if ode_aux else 0)
        # side streams first: a side launch is ordered after what the main stream holds at that moment, so it must be
        # enqueued before this step's main-stream kernels to run beside them
        for wanted in (L.ODE_ON_AUX2, L.ODE_ON_AUX, 0):
            for m in self.models:
                if side_of_sub[m._sub] != wanted:
                    continue
                L.check(lib.knpemi_ode_step(dp.h, m._sub, m._model, float(m.time), self.dt, m.rtol, m.atol,
                                            flags | wanted, L.iptr(m._ion_param), int(m.V_index)))
                m.time = m.time + self.dt
        if ode_aux:     # the assembly is the longer kernel here: it stays on the main stream
            L.check(lib.knpemi_assemble_emi(dp.h, self.flags_emi | L.SKIP_MEMBRANE_RHS))
        # Partitioned runs: the membrane dofs of the ghost cell layer are integrated redundantly on both ranks
        # (same inputs after the bulk halo, deterministic LSODA => identical bits, tools/check_partition_steps.py),
        # so phi_M / I_ch need no exchange of their own.
        if len(side_of_sub) > 1 and not self.overlap:
            L.check(lib.knpemi_join(dp.h))      # the sweeps on the second auxiliary stream
        if self.overlap:
            L.check(lib.knpemi_join(dp.h))
            L.check(lib.knpemi_assemble_emi_membrane_rhs(dp.h, self.flags_emi))
            if calibrate:
                us = {}
                for name in ("ode_step_kernel", "emi_rows_kernel"):
                    n, ms = C.c_int64(), C.c_double()
                    L.check(lib.knpemi_profile_read(dp.h, L.KERNEL_NAMES.index(name), C.byref(n), C.byref(ms)))
                    us[name] = ms.value
                L.check(lib.knpemi_profile(dp.h, 0))
                self.ode_on_aux = us["emi_rows_kernel"] > us["ode_step_kernel"]
                # Running the two side by side costs a cross-stream join and a separate launch for the membrane
                # Robin term (~25 us together on this stack): not worth it when the shorter kernel is shorter than that
                if min(us.values()) < self.overlap_threshold_ms:
                    self.overlap = False
        else:
            L.check(lib.knpemi_assemble_emi(dp.h, self.flags_emi))

    def _rest_of_step(self, halo):
        """Everything behind the potential system's assembly: the solves, the concentration system, the update, the taps."""
        dp, lib = self.dp, self.lib
        knp_flags = self.flags_knp
        if self.early_membrane:
            # everything of the membrane integrals that does not need the new potential: now, beside the EMI solve
            L.check(lib.knpemi_assemble_knp_membrane_early(dp.h, self.flags_knp | (L.ON_AUX_STREAM if self.overlap else 0)))
            knp_flags |= L.MEMBRANE_EARLY
        if self.solve_emi is not None:
            self.solve_emi(dp)
            if halo is not None:
                halo.exchange_bulk()
        L.check(lib.knpemi_assemble_knp(dp.h, knp_flags))
        if self.assemble_knp_twice:   # the reference assembles p = a a second time (knpWeakForm.py:319)
            L.check(lib.knpemi_assemble_knp(dp.h, knp_flags))
        if "exchange" in self.taps:
            # behind the assembly, before the solve: the fields the membrane part of b_knp has just been formed from
            self.taps["exchange"].tick(self.k, self.dt)
        if self.solve_knp is not None:
            self.solve_knp(dp)
        if not (self.fuse_update and self.solve_knp is not None):
            L.check(lib.knpemi_update_pde(dp.h))
        if halo is not None:
            halo.exchange_bulk()
        self.k += 1
        # On the main stream behind the end-of-step update (update_pde_kernel or the fused KNP write-back); the next
        # step's side-stream launches fork from the main stream after it (ev_fork), so none of them overtakes these: the
        # observables' launch, the events' over the membrane dofs, the fluxes' over the cells of the watched sub-domains.
        # the field maps' over the items of the watched spaces, the monitors' over the dofs of the watched model slots.
        # The snapshot's pack launch comes last: its frame holds what every other recorder of the step has seen.
        for name in ("observe", "detect", "fluxes", "track", "monitor", "snapshot"):
            if name in self.taps:
                self.taps[name].tick(self.k, self.dt)

    def ode_failures(self):
        n = 0
        for m in self.models:
            nf = C.c_int32()
            nr, ns = C.c_int64(), C.c_int64()
            self.lib.knpemi_ode_stats(self.dp.h, m._sub, m._model, C.byref(nr), C.byref(ns), C.byref(nf))
            n += nf.value
        return n
