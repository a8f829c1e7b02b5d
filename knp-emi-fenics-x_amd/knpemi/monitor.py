"""Membrane monitors: Nernst potentials, conductances and the channel currents by mechanism, recorded on the device.

The reference's users read a membrane run through quantities its figure scripts re-derive by hand from checkpoints of
every step, restating the model's formulas and constants (`examples/local_astrocyte_depolarization/make_figures.py:169-195,
279-327`: E_K, E_Na, E_Cl, i_kir, i_pump at a glial membrane point; `examples/idealized_geometries/make_figures.py:146-149`;
`calibrate_initial_conditions/run_calibration.py:148-212`).  The membrane models' device code computes every one of them
inside its right-hand side; `MembraneMonitor` records them -- users of Gotran-generated modules know this as `monitor` /
`monitor_indices` -- in one launch per record (csrc/kernels_monitor.hip, quantities in csrc/membrane_monitors.h):

    mon = MembraneMonitor(subdomain_list, ion_list, ft=ft)
    mon.names(tag)                                 # the library's catalogue for the model of cell `tag`
    mon.watch(tag, model=0, quantities=None)       # default: all
    mon.point("glia", tag, x)                      # columns "glia/E_K", "glia/i_Kir", ...
    mon.reduce("glia_mean", tag, op="average", quantities=("E_K", "i_pump"))
    stepper.monitor(mon, every=1)                  # ... stepper.step() ...
    mon.series()                                   # {"t", "glia/E_K", ...}
    mon.values(tag)                                # {name: (n_q,)} of the latest record taken with fields=True

The state a monitor sees (include/knpemi_hip.h states the rule, `compute_host` restates it in numpy): the state the next
sweep would start from.  Per membrane dof, a private copy of the parameter row in which the `<ion>_e` / `<ion>_i` columns
hold the traces of the concentrations on the two sides, V = phi_M of the dof, the gates of the state table, every other
column -- the stimulus columns included -- as the table holds it, and t the record's time.  Nothing is written anywhere.

Plug-in models bring their own monitor (`MONITOR_HIP` or a Python `monitor(states, t, parameters, monitored)` that
`knpemi.rhs_codegen` translates, with `MONITOR_NAMES` / `monitor_names()`): `MembraneModel` compiles it with hipRTC as a
program of its own when it binds the model, and the slot is watched like a shipped one.

Columns.  A point column is sum_j w_j v(q_j) over the dofs of the membrane facet that holds the point
(`fem.probe`).  Reductions run over the dofs q of the model's membrane with weight w_q > 0, w_q the integral of the dof's
hat function over the facets that carry the model: "integral" = sum_q w_q v_q, "average" = integral / sum_q w_q, "min",
"max".  Units are the model's own.  A non-finite value is kept and makes the columns it enters non-finite.

Cell-partitioned runs (`MembraneMonitor(..., partitioned=True)`, `stepper.monitor(mon, halo=halo)`).  A rank's local mesh
holds its cells and a ghost layer, whose membrane dofs are integrated redundantly with identical bits.  `partition` gives
every membrane facet one recorder -- the lowest owner among its vertices, the rule of `Observables.partition` -- and the
weights carry it: on a rank w_q is the integral of the hat function over the facets that carry the model AND that the rank
records, so the kernel's rule "the dofs with w_q > 0" needs no ownership test, and a rank's weights may all be zero.  Every
rank sums w_q v_q and takes minimum and maximum over its dofs with w_q > 0; the partial rows are exchanged on the device and
folded in rank order (`recording.combine_partials` restates it): integrals and averages summed -- the average then divided
by the global sum of weights, the ranks' sums added in rank order -- minima and maxima folded keeping a NaN.  Every facet
that carries the model is recorded by exactly one rank, so each of its dofs has w_q > 0 on some rank, and a dof two ranks
see has the same bits on both: the fold of the extrema is the global extremum bit for bit.  A point goes to the lowest
rank whose recorded facets hold it (its column is summed: the other ranks contribute 0).  `values(tag, halo=halo)` returns
the dofs the rank owns.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L
from .fem.probe import Locator, integral_weights
from .recording import (FOLD_MAX, FOLD_MIN, FOLD_SUM, RowSeries, agree_across_ranks, gather_objects, item_owners, lib_int,
                        membrane_meshes, nodal_values as _values, rank_slots, recorded_items)

OPS = {"integral": L.MON_INTEGRAL, "average": L.MON_AVERAGE, "min": L.MON_MIN, "max": L.MON_MAX_OP}
_MODEL_IDS = {"hh_si": L.MODEL_HH_SI, "hh_mv": L.MODEL_HH_MV, "glial": L.MODEL_GLIAL}


def fold_depth():
    """Workgroup partials the record kernel's fold of a column has in flight."""
    return lib_int("kn_monitor_fold_depth")


def catalogue(model_id):
    """The names of the monitored quantities of shipped model `model_id` ("hh_si", "hh_mv", "glial" or its number), in
    the library's order; [] for anything else."""
    mid = _MODEL_IDS.get(model_id, model_id)
    if not isinstance(mid, int):
        return []
    lib = L.load()
    return [lib.knpemi_monitor_name(mid, i).decode() for i in range(lib.knpemi_monitor_count(mid))]


# -- numpy restatement of csrc/membrane_monitors.h (host drivers, and what the device tests compare with) -------------
# units of the two Hodgkin-Huxley models: scale of u, scale of the rates, stimulus period, decay time and end
_HH = {L.MODEL_HH_SI: (1.0e3, 65.0e-3, 1.0e3, 0.03, 0.002, 125e-3), L.MODEL_HH_MV: (1.0, 65.0, 1.0, 30.0, 2.0, 125.0)}


def _hh(mid, t, y, p):
    su, v0, sr, period, tau, t_end = _HH[mid]
    m, h, n, V = y[:, 0], y[:, 1], y[:, 2], y[:, 3]
    gNa, gK, glNa, glK, stim = p[:, 0], p[:, 1], p[:, 2], p[:, 3], p[:, 8]
    psi, zK = p[:, 21], p[:, 19]
    E_Na = 1.0 / psi * 1.0 / zK * np.log(p[:, 11] / p[:, 12])
    E_K = 1.0 / psi * 1.0 / zK * np.log(p[:, 9] / p[:, 10])
    a1, a2 = 1 + p[:, 4] / p[:, 9], 1 + p[:, 5] / p[:, 12]
    i_pump = p[:, 6] / ((a1 * a1) * (a2 * a2 * a2))
    g_Na = gNa * h * (m * m * m)
    g_K = gK * ((n * n) * (n * n))
    g_stim = stim * np.exp(-np.fmod(t, period) / tau) * (1.0 if t < t_end else 0.0)
    u = su * (V + v0)
    am = 0.1 * sr * (25. - u) / (np.exp((25. - u) / 10.) - 1)
    bm = 4. * sr * np.exp(-u / 18.)
    ah = 0.07 * sr * np.exp(-u / 20.)
    bh = 1. * sr / (np.exp((30. - u) / 10.) + 1)
    an = 0.01 * sr * (10. - u) / (np.exp((10. - u) / 10.) - 1.)
    bn = 0.125 * sr * np.exp(-u / 80.)
    return np.stack([
        E_Na, E_K, i_pump, g_Na, g_K, g_stim, glNa * (V - E_Na), g_Na * (V - E_Na), g_stim * (V - E_Na),
        glK * (V - E_K), g_K * (V - E_K), (glNa + g_Na + g_stim) * (V - E_Na) + 3 * i_pump,
        (glK + g_K) * (V - E_K) - 2 * i_pump, am / (am + bm), ah / (ah + bh), an / (an + bn), 1.0 / (am + bm),
        1.0 / (ah + bh), 1.0 / (an + bn)])


def _glial(t, y, p):
    V = y[:, 0]
    glCl, glNa, glK = p[:, 0], p[:, 1], p[:, 2]
    psi, zK, zCl = p[:, 22], p[:, 20], p[:, 21]
    E_Na = 1.0 / psi * 1.0 / zK * np.log(p[:, 15] / p[:, 16])
    E_K = 1.0 / psi * 1.0 / zK * np.log(p[:, 13] / p[:, 14])
    E_Cl = 1.0 / psi * 1.0 / zCl * np.log(p[:, 17] / p[:, 18])
    temperature, R, F = 307e3, 8.315e3, 96500e3
    na15, mna15 = p[:, 16] * np.sqrt(p[:, 16]), p[:, 9] * np.sqrt(p[:, 9])
    i_pump = p[:, 10] * (p[:, 13] / (p[:, 13] + p[:, 8])) * (na15 / (na15 + mna15))
    E_K_init = R * temperature / F * np.log(p[:, 11] / p[:, 12])
    A = 1 + np.exp(18.5 / 42.4)
    B = 1 + np.exp(-(118.6 + E_K_init) / 44.1)
    gfac = np.sqrt(p[:, 13] / p[:, 11]) * (A * B)
    Cc = 1 + np.exp((V - E_K + 18.5) / 42.4)
    Dd = 1 + np.exp(-(118.6 + V) / 44.1)
    g_Kir = gfac / (Cc * Dd)
    i_Kir = glK * g_Kir * (V - E_K)
    return np.stack([E_Na, E_K, E_Cl, i_pump, g_Kir, i_Kir, glNa * (V - E_Na), glCl * (V - E_Cl),
                     glNa * (V - E_Na) + 3 * i_pump, i_Kir - 2 * i_pump, glCl * (V - E_Cl)])


def evaluate_host(model_id, t, states, params):
    """(quantities, rows): the catalogue's quantities of shipped model `model_id` at time t for every row of the state
    and parameter tables, with numpy."""
    mid = _MODEL_IDS.get(model_id, model_id)
    y, p = np.atleast_2d(np.asarray(states, np.float64)), np.atleast_2d(np.asarray(params, np.float64))
    with np.errstate(all="ignore"):
        if mid in _HH:
            return _hh(mid, float(t), y, p)
        if mid == L.MODEL_GLIAL:
            return _glial(float(t), y, p)
    raise ValueError(f"no monitor for model {model_id!r}")


class MembraneMonitor(RowSeries):
    def __init__(self, subdomain_list, ion_list, ft=None, partitioned=False):
        """subdomain_list: the problem's sub-domain dictionary (the ECS, tag 0, first; every cell carries "mesh_sub",
        "mesh_mem" and its "mem_models"); ion_list: the ions in the problem's order, the eliminated one last.  ft: the
        facet tags of the parent mesh, needed where a cell has several membrane models or facets that belong to none: a
        facet goes to the first model whose `ode.tag` is its tag (as the device problem decides).  Without it every
        facet of a cell belongs to the cell's first model.  partitioned: the sub-domain list is that of one rank of a cell
        partition: a point is located by `partition` (this rank may not hold it), and a reduction may run over a model
        no local facet carries."""
        self.partitioned = bool(partitioned)
        self._point_x = []         # the coordinates of the points, as given
        self._ptab = None          # the table of `partition`
        self.tags = list(subdomain_list)
        if self.tags[0] != 0:
            raise ValueError("the first sub-domain must be the ECS with tag 0")
        self._init_series()
        self.subdomain_list, self.ion_list, self.ft = subdomain_list, ion_list, ft
        self.ion_names = [ion["name"] for ion in ion_list]
        self.cells = [t for t in self.tags[1:] if "mesh_mem" in subdomain_list[t]]
        self.watched = {}          # (tag, model) -> quantity indices, ascending
        self._points = []          # (name, (tag, model), dofs (<= 4,), weights)
        self._cols = []            # (key, kind, (tag, model), quantity index, point index)
        self._dev = None           # (lib, handle) once attached
        self._geo = {}

    # -- the models ---------------------------------------------------------------------------------------
    def _model(self, tag, model):
        if tag not in self.subdomain_list:
            raise ValueError(f"no sub-domain with tag {tag}")
        if tag not in self.cells:
            raise ValueError("the ECS (tag 0) has no membrane of its own: give the tag of a cell")
        mms = self.subdomain_list[tag].get("mem_models", [])
        if not 0 <= int(model) < len(mms):
            raise ValueError(f"cell {tag} has no membrane model {model}")
        return mms[int(model)]["ode"]

    def model_id(self, tag, model=0):
        """The shipped model ("hh_si", "hh_mv", "glial") behind slot (tag, model), None for a plug-in's own."""
        mid = getattr(self._model(tag, model).ode, "MODEL_ID", None)
        return mid if mid in _MODEL_IDS else None

    def names(self, tag, model=0):
        """The monitored quantities of the model of slot (tag, model): the library's catalogue for a shipped model, the
        plug-in's own names (`MONITOR_NAMES` / `monitor_names()`, beside its `MONITOR_HIP` or Python `monitor`) for a
        model bound from source; [] for a model that brings no monitor."""
        return self._model(tag, model).monitor_names()

    # -- definition ---------------------------------------------------------------------------------------
    def _defining(self):
        if self._dev is not None:
            raise RuntimeError("the monitor is attached to a device problem: define watches, points and reductions "
                               "before DeviceStepper.monitor()")

    def _indices(self, key, quantities, among=None):
        names = self.names(*key)
        if quantities is None:
            idx = list(range(len(names))) if among is None else list(among)
        else:
            unknown = [q for q in quantities if q not in names]
            if unknown:
                raise ValueError(f"unknown quantity {unknown[0]!r} of the model of cell {key[0]}: one of {names}")
            idx = sorted({names.index(q) for q in quantities})
        if among is not None and not set(idx) <= set(among):
            raise ValueError(f"slot {key} does not watch {[names[i] for i in idx if i not in among]}")
        return idx

    def watch(self, tag, model=0, quantities=None):
        """Watch the quantities named in `quantities` (None: all) of membrane model `model` of cell `tag`."""
        self._defining()
        key = (tag, int(model))
        self._model(*key)
        if key in self.watched:
            raise ValueError(f"model {model} of cell {tag} is watched already")
        if not self.names(*key):
            raise ValueError(f"model {model} of cell {tag} brings no monitor")
        idx = self._indices(key, quantities)
        if not idx:
            raise ValueError("nothing to watch")
        self.watched[key] = idx

    def _watched_key(self, tag, model):
        key = (tag, int(model))
        self._model(*key)
        if key not in self.watched:
            raise ValueError(f"model {model} of cell {tag} is not watched: call watch() first")
        return key

    def _name_free(self, name):
        if any(k.split("/", 1)[0] == name for k, *_ in self._cols):
            raise ValueError(f"the name {name!r} is taken")

    def point(self, name, tag, x, model=0):
        """Columns "<name>/<quantity>" for every watched quantity of slot (tag, model) at the membrane point x."""
        self._defining()
        key = self._watched_key(tag, model)
        self._name_free(name)
        if self.partitioned:       # located by `partition`
            q, w = np.zeros(0, np.int64), np.zeros(0)
        else:
            q, w = self._locate(key, x)
        self._point_x.append(np.array(x, np.float64))
        names = self.names(*key)
        self._points.append((name, key, np.asarray(q, np.int64), np.asarray(w, np.float64)))
        for i in self.watched[key]:
            self._cols.append((f"{name}/{names[i]}", L.MON_POINT, key, i, len(self._points) - 1))

    def _locate(self, key, x, recorded=None):
        """(dofs, weights) of the membrane point x in the facets that carry the model of `key` (and, recorded, that this
        rank records); ValueError when none holds it."""
        tag, model = key
        fmask = self._geometry(*key)[2]
        mem = self.subdomain_list[tag]["mesh_mem"]
        q, w = Locator(mem, f"the membrane of model {model} of cell {tag}",
                       cell_mask=fmask if recorded is None else fmask & recorded).weights(x)
        if len(q) > 4:
            raise ValueError("a membrane facet has at most 4 vertices")
        return q, w

    def reduce(self, name, tag, op="average", model=0, quantities=None):
        """Columns "<name>/<quantity>": `op` ("integral", "average", "min", "max") over the membrane of slot (tag, model)
        of the watched quantities named in `quantities` (None: all watched)."""
        self._defining()
        if op not in OPS:
            raise ValueError(f"unknown op {op!r}: one of {sorted(OPS)}")
        key = self._watched_key(tag, model)
        self._name_free(name)
        if not self.partitioned and not self.weights(*key).sum() > 0.0:      # (partitioned: `partition` checks the global sum)
            raise ValueError(f"no membrane facet carries model {model} of cell {tag}")
        names = self.names(*key)
        for i in self._indices(key, quantities, among=self.watched[key]):
            self._cols.append((f"{name}/{names[i]}", OPS[op], key, i, 0))

    def columns(self):
        """[(key, 1)] of the series row in the device's order: points and reductions in the order of their definition,
        the quantities of each in the catalogue's order."""
        return [(k, 1) for k, *_ in self._cols]

    # -- geometry -----------------------------------------------------------------------------------------
    def _geometry(self, tag, model):
        """(q2e, q2i, facet mask of the model) of the membrane of cell `tag`: the vertex matching of
        `knpemi.device.flatten_problem` and the facet-to-model rule of `DeviceProblem`."""
        key = (tag, int(model))
        if key not in self._geo:
            sd = self.subdomain_list[tag]
            mem, ecs, ics = sd["mesh_mem"], self.subdomain_list[0]["mesh_sub"], sd["mesh_sub"]
            q2e = np.searchsorted(ecs.parent_vertices, mem.parent_vertices)
            q2i = np.searchsorted(ics.parent_vertices, mem.parent_vertices)
            nf, models = np.asarray(mem.cells).shape[0], sd.get("mem_models", [])
            if self.ft is None:
                fmodel = np.full(nf, 0 if models else -1)
            else:
                ftag = self.ft.dense()[mem.parent_entities]
                fmodel = np.full(nf, -1)
                for j in reversed(range(len(models))):      # the first model with a given tag wins
                    fmodel[ftag == int(models[j]["ode"].tag)] = j
            self._geo[key] = (q2e, q2i, fmodel == int(model))
        return self._geo[key]

    def weights(self, tag, model=0, halo=None):
        """w_q: the integral of every membrane dof's hat function over the facets that carry the model; halo: over those
        of them this rank of the partition records (after `partition` with that halo)."""
        if halo is not None:
            return self._partitioned(halo, "weights")["weights"][(tag, int(model))].copy()
        return integral_weights(self.subdomain_list[tag]["mesh_mem"], cell_mask=self._geometry(tag, model)[2])

    # -- cell-partitioned runs ------------------------------------------------------------------------------
    def _definition(self):
        """What every rank of a partition must agree on."""
        return dict(watches=[(key, self.mask(*key)) for key in self.watched],
                    columns=[(ckey, kind, key, i, p) for ckey, kind, key, i, p in self._cols],
                    points=[(name, key, x.tolist()) for (name, key, _, _), x in zip(self._points, self._point_x)])

    def partition(self, halo, gather=None, every=1, capacity=1024):
        """The table of this rank of a cell-partitioned run (see the module docstring), set in `self._ptab`: {"rank",
        "world", "recorded": {tag: bool per local membrane facet}, "owner": {tag: owner rank per local membrane dof},
        "weights": {(tag, model): the rank's w_q}, "wsum": {(tag, model): the global sum of weights}, "taker": [rank per
        point]}; the points this rank takes get their dofs and weights, the others none.  halo: the rank's
        `knpemi.fem.distributed.Halo` with its plans built; gather(obj) -> [obj of every rank] (default:
        `recording.gather_objects`).  Collective: every rank calls it once with the same watches, points, reductions, every
        and capacity, or every rank raises ValueError; so does a point no rank holds and a reduction over a model no facet
        of any rank carries."""
        if not self.partitioned:
            raise ValueError("partition: construct the monitor with partitioned=True")
        if not self.watched:
            raise ValueError("nothing is watched")
        rank = int(halo.rank)
        owner = item_owners(membrane_meshes(self.subdomain_list), halo, "mem",
                            "membrane monitors: the halo does not number the membrane dofs of these cells")
        recorded = {tag: recorded_items(self.subdomain_list[tag]["mesh_mem"], owner[tag], rank) for tag in self.cells}
        weights = {}
        for key in self.watched:
            mem = self.subdomain_list[key[0]]["mesh_mem"]
            weights[key] = integral_weights(mem, cell_mask=self._geometry(*key)[2] & recorded[key[0]]) \
                if mem.num_vertices else np.zeros(0)
        found = []
        for (name, key, _, _), x in zip(self._points, self._point_x):
            try:
                found.append(self._locate(key, x, recorded[key[0]]))
            except ValueError:
                found.append(None)
        mine = dict(self._definition(), every=int(every), capacity=int(capacity), found=[f is not None for f in found],
                    share=[float(weights[key].sum()) for key in self.watched])
        allr = (gather or gather_objects)(mine)
        world = len(allr)
        agree_across_ranks(allr, ("watches", "points", "columns", "every", "capacity"), "membrane monitors",
                           "every rank must define the same watches, points and reductions in the same order and pass the "
                           "same every and capacity")
        taker = []
        for p, (name, key, _, _) in enumerate(self._points):
            ranks = [r for r in range(world) if allr[r]["found"][p]]
            if not ranks:
                raise ValueError(f"point {self._point_x[p].tolist()} is not on the membrane of model {key[1]} of cell "
                                 f"{key[0]} on any rank")
            taker.append(ranks[0])
        wsum = {}
        for j, key in enumerate(self.watched):
            tot = allr[0]["share"][j]
            for r in range(1, world):                   # rank order: the same bits on every rank
                tot += allr[r]["share"][j]
            wsum[key] = tot
        for ckey, kind, key, _, _ in self._cols:
            if kind != L.MON_POINT and not wsum[key] > 0.0:
                raise ValueError(f"no membrane facet of any rank carries model {key[1]} of cell {key[0]} ({ckey})")
        for p, (name, key, _, _) in enumerate(self._points):
            q, w = found[p] if taker[p] == rank else (np.zeros(0, np.int64), np.zeros(0))
            self._points[p] = (name, key, np.asarray(q, np.int64), np.asarray(w, np.float64))
        self._ptab = dict(rank=rank, world=world, recorded=recorded, owner=owner, weights=weights, wsum=wsum, taker=taker)
        return self._ptab

    def _partitioned(self, halo, what):
        if self._ptab is None:
            raise RuntimeError(f"{what}(halo=...): the monitor is not partitioned (attach with halo=, or call partition)")
        if int(halo.rank) != self._ptab["rank"]:
            raise ValueError(f"{what}(halo=...): not the halo of this monitor's partition")
        return self._ptab

    def column_folds(self):
        """(FOLD_* per column, divisor per column) of `recording.combine_partials`: how the device folds the ranks' slots."""
        how = [FOLD_MIN if kind == L.MON_MIN else (FOLD_MAX if kind == L.MON_MAX_OP else FOLD_SUM) for _, kind, *_ in self._cols]
        denom = [self._ptab["wsum"][key] if kind == L.MON_AVERAGE else 1.0 for _, kind, key, _, _ in self._cols]
        return np.array(how), np.array(denom, np.float64)

    def evaluate_partial_host(self, t, state=None):
        """This rank's slot row of a partitioned run (after `partition`) with numpy, as the record kernel writes it: a
        point it takes, else 0; w_q v_q summed over its dofs with w_q > 0 (the average undivided), their minimum and
        maximum, the operation's identity without such a dof.  state: as `compute_host`."""
        if self._ptab is None:
            raise RuntimeError("evaluate_partial_host: call partition first")
        values = self._values_host(t, state or {})
        row = np.empty(len(self._cols))
        for c, (ckey, kind, key, i, p) in enumerate(self._cols):
            v = values[key][self.names(*key)[i]]
            if kind == L.MON_POINT:
                row[c] = self._point_value(p, v)
                continue
            w = self._ptab["weights"][key]
            on = w > 0.0
            if kind == L.MON_MIN:
                row[c] = np.min(v[on]) if on.any() else np.inf
            elif kind == L.MON_MAX_OP:
                row[c] = np.max(v[on]) if on.any() else -np.inf
            else:
                row[c] = np.sum(w[on] * v[on]) if on.any() else 0.0
        return row

    def n_dofs(self, tag):
        return int(self.subdomain_list[tag]["mesh_mem"].x.shape[0])

    # -- host restatement -----------------------------------------------------------------------------------
    def compute_host(self, t, state=None):
        """(values, row) with numpy: values[(tag, model)] = {name: (n_q,)} for every watched quantity, row = {column
        key: float}.  state: {"c": {tag: the K nodal concentrations of the ECS (tag 0) and of every watched cell},
        "phi_M": {tag: the membrane potential}, "tables": {(tag, model): (states, parameters)}}; `Function`s or arrays;
        what is missing is taken from the host objects of the sub-domain list ("tables": the models' host tables).  The
        rule of the module docstring: traces into the <ion>_e / <ion>_i columns of a copy of the table, V = phi_M."""
        values, row = self._values_host(t, state or {}), {}
        wcache = {}
        for ckey, kind, key, i, p in self._cols:
            v = values[key][self.names(*key)[i]]
            if kind == L.MON_POINT:
                row[ckey] = self._point_value(p, v)
                continue
            if key not in wcache:
                wcache[key] = self.weights(*key)
            w = wcache[key]
            on = w > 0.0
            if kind == L.MON_MIN:
                row[ckey] = float(np.min(v[on]))
            elif kind == L.MON_MAX_OP:
                row[ckey] = float(np.max(v[on]))
            else:
                s = float(np.sum(w[on] * v[on]))
                row[ckey] = s / float(np.sum(w)) if kind == L.MON_AVERAGE else s
        return values, row

    def _values_host(self, t, state):
        """{(tag, model): {name: (n_q,)}} of every watched quantity with numpy."""
        values = {}
        for key, idx in self.watched.items():
            tag, model = key
            st, pa = self.rows_host(tag, model, state)
            v = self._evaluate_host(tag, model, t, st, pa)
            names = self.names(tag, model)
            values[key] = {names[i]: v[i] for i in idx}
        return values

    def _point_value(self, p, v):
        """sum_j w_j v(q_j) of point p in the order of the facet's dofs (0 for a point another rank takes)."""
        _, _, q, w = self._points[p]
        acc = 0.0
        for qq, ww in zip(q, w):
            acc = acc + ww * v[qq]
        return float(acc)

    def _evaluate_host(self, tag, model, t, st, pa):
        """(quantities, dofs) on the host: the numpy restatement of a shipped model, the plug-in's own Python `monitor`
        row by row."""
        mid = self.model_id(tag, model)
        if mid is not None:
            return evaluate_host(mid, t, st, pa)
        ode = self._model(tag, model).ode
        fn = getattr(ode, "monitor", None)
        if fn is None:
            raise NotImplementedError(f"model {model} of cell {tag} brings its monitor as device source only: no host "
                                      "restatement")
        out = np.zeros((len(self.names(tag, model)), st.shape[0]))
        for q in range(st.shape[0]):
            m = np.zeros(out.shape[0])
            fn(st[q], float(t), pa[q], m)
            out[:, q] = m
        return out

    def rows_host(self, tag, model=0, state=None):
        """(states, parameters) of slot (tag, model) as a monitor sees them: copies of the tables with the traces in the
        ion columns and V = phi_M (see `compute_host` for `state`)."""
        state = state or {}
        key = (tag, int(model))
        mm = self._model(tag, model)
        q2e, q2i, _ = self._geometry(tag, model)
        st, pa = state.get("tables", {}).get(key, (mm.states, mm.parameters))
        st, pa = np.array(st, np.float64), np.array(pa, np.float64)
        if "c" in state:
            ce, ci = state["c"][0], state["c"][tag]
            for k, name in enumerate(self.ion_names):
                pa[:, mm.ode.parameter_indices(f"{name}_e")] = _values(ce[k])[q2e]
                pa[:, mm.ode.parameter_indices(f"{name}_i")] = _values(ci[k])[q2i]
        if "phi_M" in state:
            st[:, mm.V_index] = _values(state["phi_M"][tag])
        return st, pa

    def record_host(self, t, state=None):
        """Append the row of `compute_host` to the series (drivers without a device loop)."""
        self._t.append(float(t))
        self._rows.append(self.row_vector(self.compute_host(t, state)[1]))

    # -- device ---------------------------------------------------------------------------------------------
    def mask(self, tag, model=0):
        return sum(1 << i for i in self.watched[(tag, int(model))])

    def _attach(self, dp, capacity, halo=None, every=1):
        """knpemi_monitor_set on the device problem dp, or with a halo `partition` and knpemi_monitor_set_partitioned
        (`rank_slots`).  Returns the objects the handle refers to (keep them alive while it records)."""
        if self._dev is not None:
            raise RuntimeError("this monitor is attached to a device problem already")
        if not self.watched:
            raise ValueError("nothing is watched")
        if halo is not None:
            if not self._cols:
                raise ValueError("a partitioned monitor records a series: define a point or a reduction")
            self.partition(halo, None, every, capacity)
        keys = list(self.watched)
        spec, ionp, wts = [], [], []
        for tag, model in keys:
            mm = self._model(tag, model)
            if not self.names(tag, model):
                raise ValueError(f"model {model} of cell {tag} brings no monitor")
            spec += [dp.sub_index[tag], model, self.mask(tag, model), int(mm.V_index)]
            for name in self.ion_names:
                ionp += [mm.ode.parameter_indices(f"{name}_e"), mm.ode.parameter_indices(f"{name}_i")]
            wts.append(self.weights(tag, model, halo))
        cols = np.array([[kind, keys.index(key), i, p] for _, kind, key, i, p in self._cols] or [[0, 0, 0, 0]], np.int32)
        n_pts = len(self._points)
        pt_watch = np.array([keys.index(key) for _, key, _, _ in self._points] or [0], np.int32)
        pt_q = np.full((max(n_pts, 1), 4), -1, np.int32)
        pt_w = np.zeros((max(n_pts, 1), 4))
        for p, (_, _, q, w) in enumerate(self._points):
            pt_q[p, :len(q)], pt_w[p, :len(q)] = q, w
        spec, ionp = np.array(spec, np.int32), np.array(ionp, np.int32)
        wts = np.ascontiguousarray(np.concatenate(wts), np.float64)
        wts = wts if wts.size else np.zeros(1)                # a rank without a dof still passes an array
        args = (dp.h, len(keys), L.iptr(spec), L.iptr(ionp), L.dptr(wts), len(self._cols), L.iptr(cols), n_pts,
                L.iptr(pt_watch), L.iptr(pt_q), L.dptr(pt_w), int(capacity))
        keep = None
        if halo is None:
            L.check(dp.lib.knpemi_monitor_set(*args))
        else:
            wsum = np.array([self._ptab["wsum"][key] for key in keys], np.float64)
            world = self._ptab["world"]
            slots, keep = rank_slots(dp, halo, world, len(self._cols))
            L.check(dp.lib.knpemi_monitor_set_partitioned(*args, L.dptr(wsum), self._ptab["rank"], world, *slots))
        self._dev = (dp.lib, dp.h)
        return keep

    def values(self, tag, model=0, halo=None):
        """{name: (n_q,)}: the watched quantities of slot (tag, model) per membrane dof, as the latest device record
        taken with fields=True wrote them (one synchronisation).  halo: on a cell-partitioned problem only the dofs this
        rank owns (`Halo.vertex_owner("mem")`), with "dofs" (their local indices) and "locations" (their coordinates);
        the union over the ranks is the single-rank array."""
        key = self._watched_key(tag, model)
        if self._dev is None:
            raise RuntimeError("values(): not attached to a device problem (DeviceStepper.monitor); compute_host "
                               "evaluates host data")
        lib, h = self._dev
        names, w = self.names(*key), list(self.watched).index(key)
        out = {}
        for i in self.watched[key]:
            buf = np.empty(self.n_dofs(tag), np.float64)
            L.check(lib.knpemi_monitor_fields(h, w, i, L.dptr(buf if buf.size else np.zeros(1)), buf.size))
            out[names[i]] = buf
        if halo is not None:
            mine = np.flatnonzero(self._partitioned(halo, "values")["owner"][tag] == int(halo.rank))
            out = {k: v[mine] for k, v in out.items()}
            out["dofs"] = mine
            out["locations"] = np.array(self.subdomain_list[tag]["mesh_mem"].x, np.float64)[mine]
        return out
