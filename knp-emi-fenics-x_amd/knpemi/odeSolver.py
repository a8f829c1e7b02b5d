"""`MembraneModel`: the membrane ODE systems, integrated on the GPU.

Drop-in for `src/knpemi/odeSolver.py` of the reference: same constructor,
attributes (`states`, `parameters`, `dof_locations`, `indices`, `nodes`, `tag`,
`ode`, `prefix`, `time`) and methods.  `step_lsoda` replaces the reference's
serial Python loop over numbalsoda calls (`odeSolver.py:107-122`) by one launch
of the HIP kernel `ode_step_kernel` (csrc/kernels_ode.hip): one thread per
membrane dof running LSODA.

Membrane-model plug-ins keep the reference's module protocol
(`init_state_values`, `init_parameter_values`, `state_indices`,
`parameter_indices`, `__name__`).  Where the reference takes the address of a
numba `cfunc` (`rhs_numba.address`, `odeSolver.py:96`) -- a host function a GPU
cannot call -- a plug-in here either names one of the right-hand sides compiled
into the library (`MODEL_ID` = "hh_si", "hh_mv" or "glial") or brings its own
as HIP source in `RHS_HIP`: a `__device__ void rhs(double t, const double*
states, double* values, double* parameters)` with the cfunc's semantics, compiled
for gfx950 with hipRTC when the model is bound (csrc/kernels_rtc.hip) -- or has
only what the reference's modules have, a Python `rhs_numba` / `rhs` made of
assignments: `knpemi.rhs_codegen` translates its source text into that function.

A model that no PDE problem has claimed runs on a handle of its own
(`knpemi_ode_create`), as the reference's model steps over the dofs of any CG-1
space; `advance` and `steady_state` run many steps in one launch
(`ode_advance_kernel`).  Passed to `emi_system` / `knp_system` later, the model
moves to that problem with its current tables.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

_MODEL_IDS = {"hh_si": L.MODEL_HH_SI, "hh_mv": L.MODEL_HH_MV, "glial": L.MODEL_GLIAL}


class OdeProblem:
    """Membrane models without a mesh (knpemi_ode_create): model i is addressed as (sub = 1 + i, model = 0)."""

    def __init__(self, nq, device=None):
        lib = L.load()
        if lib.knpemi_device_count() < 1:
            raise RuntimeError("no HIP device visible: the knpemi hot path runs on MI355X only "
                               "(there is no CPU fallback)")
        if device is None:
            import os
            device = int(os.environ.get("LOCAL_RANK", "0")) % lib.knpemi_device_count()
        self.lib = lib
        nq = np.ascontiguousarray(nq, np.int32)
        h = C.c_void_p()
        L.check(lib.knpemi_ode_create(int(device), len(nq), L.iptr(nq), C.byref(h)))
        self.h = h

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            self.lib.knpemi_destroy(h)
            self.h = None

    def timer_start(self):
        L.check(self.lib.knpemi_timer_start(self.h))

    def timer_stop_ms(self):
        ms = C.c_double()
        L.check(self.lib.knpemi_timer_stop_ms(self.h, C.byref(ms)))
        return ms.value


class MembraneModel:
    '''ODE on membrane defined by tagged facet function'''

    def __init__(self, ode, ft, tag, Q):
        assert isinstance(tag, int)
        # All dofs of Q carry an ODE system (odeSolver.py:31-38: the restriction
        # to ft.find(tag) is commented out in the reference).
        self.dof_locations = Q.tabulate_dof_coordinates()
        self.indices = np.arange(len(self.dof_locations))
        nodes = len(self.indices)
        self.nodes = nodes
        s0 = np.asarray(ode.init_state_values(), dtype=np.float64)
        p0 = np.asarray(ode.init_parameter_values(), dtype=np.float64)
        self.states = np.tile(s0, (nodes, 1))
        self.parameters = np.tile(p0, (nodes, 1))
        self.tag = tag
        self.ode = ode
        self.prefix = ode.__name__
        self.time = 0
        self.rtol, self.atol = 1.0e-8, 1.0e-10   # odeSolver.py:120
        self.method, self.substeps = "lsoda", None   # set_integrator
        self.last_stats = None
        # device binding (set by DeviceProblem through emi_system / knp_system)
        self._dp = None
        self._sub = None
        self._model = None
        self._pending_flags = 0
        self._ion_param = None
        self._mask_cache = {}
        self._standalone = None   # OdeProblem of a model no PDE problem has claimed
        self._events = None       # MembraneEvents recorded after every step of a stand-alone model (detect)
        self._monitor_cache = None   # (names, device source of a plug-in's monitor), filled on first use
        self.monitor_refused = None  # why a plug-in's Python `monitor` could not be translated, if it could not
        print(f'\t{self.prefix} Number of ODE points on the membrane {nodes}')

    # --- device binding ------------------------------------------------------
    def _bind(self, dp, sub, model, ion_names):
        if self._dp is dp:
            return
        model_id = getattr(self.ode, "MODEL_ID", None)
        source = getattr(self.ode, "RHS_HIP", None)
        if model_id not in _MODEL_IDS and source is None:
            # a module written for the reference: its Python right-hand side (rhs_numba / rhs, odeSolver.py:96 takes the
            # cfunc's address) is plain arithmetic -- translate the source text into the device function
            from .rhs_codegen import hip_source_from_module
            source = hip_source_from_module(self.ode)
        if model_id in _MODEL_IDS:
            L.check(dp.lib.knpemi_ode_bind(dp.h, sub, model, _MODEL_IDS[model_id],
                                           self.states.shape[1], self.parameters.shape[1]))
        elif source is not None:
            # the plug-in's own right-hand side, compiled for gfx950 now (a few seconds, cached per process)
            L.check(dp.lib.knpemi_ode_bind_source(dp.h, sub, model, self.states.shape[1], self.parameters.shape[1],
                                                  source.encode()))
            # the plug-in's monitor, if it brings one (MONITOR_HIP, or a Python `monitor` translated), with its names:
            # a hipRTC program of its own
            names, mon_source = self._plug_in_monitor()
            if mon_source is not None:
                L.check(dp.lib.knpemi_monitor_bind_source(dp.h, sub, model, len(names), mon_source.encode()))
        else:
            raise NotImplementedError(
                f"membrane model module '{self.prefix}' has neither a MODEL_ID naming a shipped device RHS "
                f"(one of {sorted(_MODEL_IDS)}), nor its own RHS_HIP source, nor a Python right-hand side (rhs_numba / "
                f"rhs) whose source knpemi.rhs_codegen could translate (see examples/benchmark/mm_glial.py)")
        self._dp, self._sub, self._model = dp, sub, model
        idx = []
        for name in ion_names:
            idx += [self.ode.parameter_indices(f"{name}_e"), self.ode.parameter_indices(f"{name}_i"),
                    self.ode.parameter_indices(f"I_ch_{name}")]
        # (a handle without a mesh has no ions; the ABI still wants a pointer)
        self._ion_param = np.array(idx if idx else [0], np.int32)
        if not isinstance(dp, OdeProblem):
            self._standalone = None   # moved to a PDE problem: the host tables travel with every step
            if self._events is not None:   # ... and the events stay behind with the handle that recorded them
                self._events._detach()
                self._events = None
        self._apply_integrator()

    def _device(self):
        """The bound problem; a model no PDE problem has claimed gets a handle of its own."""
        if self._dp is None:
            self._standalone = OdeProblem([self.nodes])
            self._bind(self._standalone, 1, 0, [])
        return self._dp

    def detect(self, ev):
        """Record the membrane events `ev` (knpemi.events.MembraneEvents built from {self.tag: self.nodes}, the cell
        watched) of a model no PDE problem has claimed: every `step` / `step_lsoda` records V at the model's new time.
        `advance` and `steady_state` run many steps inside one launch without writing the samples: they record
        nothing.  A model of a PDE problem records through `DeviceStepper.detect`."""
        dp = self._device()
        if not isinstance(dp, OdeProblem):
            raise RuntimeError("this model belongs to a PDE problem: record its events with DeviceStepper.detect")
        if self._events is not None:
            raise RuntimeError("this model records membrane events already")
        if ev.n_q.get(self.tag) != self.nodes:
            raise ValueError(f"events for {{{self.tag}: {self.nodes}}} expected, got {ev.n_q}")
        ev._x.setdefault(self.tag, self.dof_locations)
        ev._attach(dp.lib, dp.h, {self.tag: self._sub})
        ev.reset_host()
        self._events = ev

    def monitor_names(self):
        """The monitored quantities of the model, from the library's catalogue; [] for a model that brings none."""
        if getattr(self.ode, "MODEL_ID", None) in _MODEL_IDS:
            if self._monitor_cache is None:
                from .monitor import catalogue
                self._monitor_cache = (catalogue(self.ode.MODEL_ID), None)
            return list(self._monitor_cache[0])
        return list(self._plug_in_monitor()[0])

    def _plug_in_monitor(self):
        """(names, device source) of the monitor a plug-in brings, ([], None) if it brings none; translated once per model.
        A Python `monitor` with a construct the translation refuses leaves the model without a monitor -- its right-hand
        side is bound all the same -- and `monitor_refused` says why."""
        if self._monitor_cache is None:
            from .rhs_codegen import hip_monitor_from_module, monitor_names_of
            try:
                source = hip_monitor_from_module(self.ode)
            except NotImplementedError as e:
                source, self.monitor_refused = None, str(e)
            self._monitor_cache = (monitor_names_of(self.ode) if source is not None else [], source)
        return self._monitor_cache

    def monitor(self, names=None, t=None):
        """{name: (nodes,)}: the named intermediates of the right-hand side (`monitor_names`; None: all) at time t
        (None: the model's time), evaluated on the device from the HOST tables as they stand: one launch of the monitor
        kernel over a scratch copy of them (knpemi_monitor_eval).  The tables of the handle are not touched."""
        all_names = self.monitor_names()
        if not all_names:
            why = f": its Python `monitor` cannot be translated ({self.monitor_refused})" if self.monitor_refused else ""
            raise ValueError(f"membrane model '{self.prefix}' brings no monitor" + why)
        names = list(all_names if names is None else names)
        unknown = [n for n in names if n not in all_names]
        if unknown:
            raise ValueError(f"unknown quantity {unknown[0]!r}: one of {all_names}")
        idx = sorted({all_names.index(n) for n in names})
        dp = self._device()
        states = np.ascontiguousarray(self.states, np.float64)
        params = np.ascontiguousarray(self.parameters, np.float64)
        out = np.empty((len(idx), self.nodes), np.float64)
        L.check(dp.lib.knpemi_monitor_eval(dp.h, self._sub, self._model, float(self.time if t is None else t),
                                           sum(1 << i for i in idx), L.dptr(states), L.dptr(params), None,
                                           int(self.V_index), L.dptr(out), out.size))
        by_index = {i: out[j] for j, i in enumerate(idx)}
        return {n: by_index[all_names.index(n)] for n in names}

    def _set_stimulus(self, stimulus, stimulus_locator):
        dp, lib = self._dp, self._dp.lib
        # keyed on the locator object itself (the cache holds a reference, so a fresh lambda can never reuse the id
        # of a dead one and pick up its mask)
        key = stimulus_locator
        if key not in self._mask_cache:
            if stimulus_locator is None:
                mask = np.ones(self.nodes, np.uint8)
            else:
                mask = np.fromiter(map(stimulus_locator, self.dof_locations), dtype=bool).astype(np.uint8)
            self._mask_cache = {key: np.ascontiguousarray(mask)}
        mask = self._mask_cache[key]
        sidx = np.array([self.ode.parameter_indices(k) for k in stimulus], np.int32)
        sval = np.array([float(v) for v in stimulus.values()], np.float64)
        L.check(lib.knpemi_ode_set_stimulus(dp.h, self._sub, self._model, mask.ctypes.data_as(L.c_u8_p),
                                            len(sidx), L.iptr(sidx) if len(sidx) else None,
                                            L.dptr(sval) if len(sval) else None))

    def _read_stats(self, ms):
        lib = self._dp.lib
        nrhs, nst, nfail = C.c_int64(), C.c_int64(), C.c_int32()
        rc = lib.knpemi_ode_stats(self._dp.h, self._sub, self._model, C.byref(nrhs), C.byref(nst), C.byref(nfail))
        self.last_stats = dict(n_rhs=nrhs.value, n_steps=nst.value, n_failed=nfail.value, ms=ms)
        return rc

    # --- PDE <-> ODE column copies (odeSolver.py:52-85, 130-188) -------------------
    def _table(self, what):
        if what == 'state':
            return self.states, self.ode.state_indices
        return self.parameters, self.ode.parameter_indices

    def _rows(self, locator):
        if locator is None:
            return slice(None)
        return np.flatnonzero(np.fromiter(map(locator, self.dof_locations), dtype=bool))

    def _from_function(self, what, which, u, locator):
        table, col_of = self._table(what)
        rows = self._rows(locator)
        table[rows, col_of(which)] = u.x.array[self.indices[rows]]
        return self.states

    def _to_function(self, what, which, u, locator):
        table, col_of = self._table(what)
        rows = self._rows(locator)
        u.x.array[self.indices[rows]] = table[rows, col_of(which)]
        return u

    def _from_callables(self, what, value_dict, locator):
        table, col_of = self._table(what)
        rows = np.arange(self.nodes)[self._rows(locator)]
        print(f'\t{self.prefix} Set {what} for {len(rows)} ODES')
        for name, fn in value_dict.items():
            if len(rows):
                table[rows, col_of(name)] = [fn(x) for x in self.dof_locations[rows]]
        return table

    def set_state(self, which, u, locator=None):
        return self._from_function('state', which, u, locator)

    def set_parameter(self, which, u, locator=None):
        return self._from_function('parameter', which, u, locator)

    def get_state(self, which, u, locator=None):
        return self._to_function('state', which, u, locator)

    def get_parameter(self, which, u, locator=None):
        return self._to_function('parameter', which, u, locator)

    def set_state_values(self, value_dict, locator=None):
        return self._from_callables('state', value_dict, locator)

    def set_parameter_values(self, value_dict, locator=None):
        return self._from_callables('parameter', value_dict, locator)

    def set_membrane_potential(self, u, locator=None):
        return self.set_state('V', u, locator=locator)

    def get_membrane_potential(self, u, locator=None):
        return self.get_state('V', u, locator=locator)

    @property
    def V_index(self):
        return self.ode.state_indices('V')

    # ---- ODE integration ------
    def set_integrator(self, method="lsoda", substeps=None):
        '''The integrator `step`, `advance` and `steady_state` use: "lsoda" (default, rtol / atol of the model), or a
        fixed-step scheme with `substeps` equal sub-steps per step -- "euler", "rk4", "rush_larsen" (gates by their
        exponential update, the rest by Euler).  substeps=None takes 25, the reference drivers' `n_steps_ODE`.
        The currents a fixed-step method hands out are those at the end state of the step.'''
        if method not in L.ODE_METHODS:
            raise ValueError(f"unknown integrator {method!r}: one of {sorted(L.ODE_METHODS)}")
        if method == "lsoda":
            substeps = None
        else:
            substeps = L.ODE_DEFAULT_SUBSTEPS if substeps is None else int(substeps)
            if not 1 <= substeps <= 10000:
                raise ValueError("substeps must be in 1..10000")
        old = self.method, self.substeps
        self.method, self.substeps = method, substeps
        if self._dp is not None:
            try:
                self._apply_integrator()
            except L.KnpemiError:
                self.method, self.substeps = old
                raise

    def _apply_integrator(self):
        L.check(self._dp.lib.knpemi_ode_set_method(self._dp.h, self._sub, self._model, L.ODE_METHODS[self.method],
                                                   int(self.substeps or 0)))

    def step(self, dt, stimulus, stimulus_locator=None):
        '''Solve the ODEs forward by dt with the integrator of `set_integrator` (on the GPU)'''
        return self._step(dt, stimulus, stimulus_locator)

    def step_lsoda(self, dt, stimulus, stimulus_locator=None):
        '''Solve the ODEs forward by dt with optional stimulus (on the GPU)'''
        if self.method != "lsoda":
            raise RuntimeError(f"step_lsoda integrates with LSODA, but this model is configured for "
                               f"{self.method!r} (set_integrator): call step(), which uses the configured integrator")
        return self._step(dt, stimulus, stimulus_locator)

    def _step(self, dt, stimulus, stimulus_locator):
        if stimulus is None:
            stimulus = {}
        dp = self._device()
        lib = dp.lib
        self._set_stimulus(stimulus, stimulus_locator)
        print(f'\t{self.prefix} Stepping {self.nodes} ODEs')
        states = np.ascontiguousarray(self.states, np.float64)
        params = np.ascontiguousarray(self.parameters, np.float64)
        L.check(lib.knpemi_ode_set_tables(dp.h, self._sub, self._model, L.dptr(states), L.dptr(params)))
        dp.timer_start()
        L.check(lib.knpemi_ode_step(dp.h, self._sub, self._model, float(self.time), float(dt),
                                    self.rtol, self.atol, int(self._pending_flags),
                                    L.iptr(self._ion_param), int(self.V_index)))
        ms = dp.timer_stop_ms()
        if self._events is not None:
            L.check(lib.knpemi_events_record(dp.h, float(self.time + dt)))
        self._pending_flags = 0
        rc = self._read_stats(ms)
        L.check(lib.knpemi_ode_get_tables(dp.h, self._sub, self._model, L.dptr(states), L.dptr(params)))
        self.states[...] = states
        self.parameters[...] = params
        assert rc == L.OK, (
            "LSODA failed on at least one membrane dof" if self.method == "lsoda"   # odeSolver.py:121
            else f"{self.method} left a non-finite state on at least one membrane dof")
        self.time = self.time + dt
        print(f'\t{self.prefix} Stepped {self.nodes} ODES in {ms * 1e-3}s')
        return self.states

    # ---- many steps per launch (no reference counterpart: its calibration tool loops over step_lsoda) ------
    def advance(self, dt, n_steps, stimulus=None, stimulus_locator=None, record=None, every=1):
        '''n_steps successive step(dt, stimulus, stimulus_locator) calls (step_lsoda unless set_integrator chose another
        method), bit for bit, in launches of many steps.
        `record`: state names recorded after every `every`-th step; returns {name: ndarray[n_steps // every, nodes]}.'''
        _, hist = self._advance(dt, n_steps, stimulus, stimulus_locator, record, every, None)
        return hist

    def steady_state(self, dt, max_steps, rtol=1e-8, atol=1e-10, window=10, stimulus=None, stimulus_locator=None,
                     record=None, every=1):
        '''Step by dt until every node is steady: a node is still after a step when each state moved by at most
        atol + rtol |y|, and steady after `window` still steps in a row; it is frozen from then on.  At most max_steps
        steps.  Returns steps_taken[nodes] (the step count at which each node became steady, -1 if it did not), and
        with `record` also the history as `advance` returns it.  `time` advances by the steps the run needed.'''
        ss = L.OdeSS(ss_rtol=float(rtol), ss_atol=float(atol), window=int(window))
        steps, hist = self._advance(dt, max_steps, stimulus, stimulus_locator, record, every, ss)
        return steps if record is None else (steps, hist)

    def _advance(self, dt, n_steps, stimulus, stimulus_locator, record, every, ss):
        n_steps, every = int(n_steps), int(every)
        if n_steps < 0 or every < 1:
            raise ValueError("n_steps >= 0 and every >= 1")
        names = list(record or [])
        if len(names) > 8:
            raise ValueError("at most 8 recorded states")
        dp = self._device()
        lib = dp.lib
        self._set_stimulus(stimulus or {}, stimulus_locator)
        states = np.ascontiguousarray(self.states, np.float64)
        params = np.ascontiguousarray(self.parameters, np.float64)
        L.check(lib.knpemi_ode_set_tables(dp.h, self._sub, self._model, L.dptr(states), L.dptr(params)))
        rec = np.array([self.ode.state_indices(n) for n in names] or [0], np.int32)
        hist = np.zeros((n_steps // every, len(names), self.nodes)) if names else None
        steps = np.full(self.nodes, -1, np.int32)
        failed = np.full(self.nodes, -1, np.int32)
        dp.timer_start()
        rc = lib.knpemi_ode_advance(dp.h, self._sub, self._model, float(self.time), float(dt), n_steps, self.rtol,
                                    self.atol, L.iptr(rec), len(names), every,
                                    L.dptr(hist) if hist is not None else None, C.byref(ss) if ss is not None else None,
                                    L.iptr(steps), L.iptr(failed))
        ms = dp.timer_stop_ms()
        if rc not in (L.OK, L.EODE):
            L.check(rc)
        self._read_stats(ms)
        L.check(lib.knpemi_ode_get_tables(dp.h, self._sub, self._model, L.dptr(states), L.dptr(params)))
        self.states[...] = states
        self.parameters[...] = params
        # the time of the last step run: every node steady -> the step on which the last one became so
        ran = int(steps.max()) if ss is not None and self.nodes and (steps >= 0).all() else n_steps
        for _ in range(ran):
            self.time = self.time + dt   # step_lsoda's arithmetic
        out = {n: hist[:, i, :] for i, n in enumerate(names)} if names else {}
        if rc == L.EODE:   # odeSolver.py:121 `assert success`
            bad = np.flatnonzero(failed >= 0)
            what = "LSODA" if self.method == "lsoda" else f"the {self.method} integrator"
            raise RuntimeError(f"{what} failed on {len(bad)} membrane dof(s): dofs {bad[:10].tolist()} at steps "
                               f"{failed[bad[:10]].tolist()}")
        print(f'\t{self.prefix} Advanced {self.nodes} ODES by {n_steps} steps in {ms * 1e-3}s')
        return steps, out
