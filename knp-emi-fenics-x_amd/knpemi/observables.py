"""Observables: time series of point values and field statistics, recorded on the device during a run.

The reference's users read a run through time series that its figure scripts evaluate from a checkpoint of every
step: phi and the ion concentrations at one ECS and one ICS point, phi_M and the ECS/ICS traces at one membrane point
(`examples/idealized_geometries/make_figures.py:24-117`, `scifem.evaluate_function`), and means / maxima of fields
(`local_astrocyte_depolarization/run_stim_duration.py:239-246`).  Here each such quantity is a linear functional
(sparse or dense weights on the nodal values) or a min / max of one nodal field; `DeviceStepper.observe` evaluates
all of them in one launch at the end of a step and appends a row to a device buffer, and the host reads the buffer
only when asked.  `record_host` evaluates the same functionals with numpy from host `Function` arrays (host drivers,
and the reference of the device evaluation).

Quantities are those the reference writes at the end of a step (run_3D.py:356-368): `phi`, the new `c` of the solved
ions, the eliminated ion's `c_<tag>` and the updated `phi_M_prev`.  Membrane traces come from the bulk fields of the
two sides.

    obs = Observables(mesh, ct, ft, subdomain_list, ion_list)
    obs.point("ECS", tag=0, x=[25e-6, 3.5e-6])           # ECS/phi, ECS/K, ECS/Cl, ECS/Na
    obs.membrane_point("mem", tag=1, x=[25e-6, 3e-6])    # mem/phi_M, mem/K_e, mem/K_i, ...
    obs.reduce("K_ecs_max", "c", ion="K", tag=0, op="max")
    stepper.observe(obs)                                  # ... stepper.step() ...
    obs.series()                                          # {"t": (n,), "ECS/phi": (n,), ...}

Cell-partitioned runs (knpemi.fem.distributed / knpemi.fem.partition): every rank builds the same definitions on its
local mesh with `partitioned=True` (points in global coordinates; a point outside the local mesh is resolved at set-up)
and passes its halo to `DeviceStepper.observe(obs, halo=halo)`.  `partition` decides, without communication, what each
rank counts: a vertex (membrane dof) belongs to its owner (`Halo.vertex_owner`), a cell (membrane facet) is recorded by
the lowest owner among its vertices -- a rank that owns a vertex keeps every cell touching it, so the recorder holds the
whole cell and both sides of a membrane facet.  Points go to the lowest rank whose recorded cells contain them,
integrals sum the weights of recorded cells, nodal means / min / max run over owned vertices, and the denominators are
global.  One `all_gather_object` at set-up resolves the points, the denominators and checks that all ranks agree on the
definitions.  Each record then sums the ranks' partial rows on the device (knpemi_observe_set_partitioned); every rank
holds the global series.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .recording import RowSeries, agree_across_ranks, gather_objects, item_owners, rank_slots, recorded_items
from .fem.probe import Locator, integral_weights, membrane_weights, point_weights

OPS = ("integral", "nodal_mean", "average", "min", "max")


class _Obs:
    __slots__ = ("key", "field", "tag", "idx", "op", "ids", "w", "denom", "src")

    def __init__(self, key, field, tag, idx, op, ids, w, denom=1.0, src=None):
        self.key, self.field, self.tag, self.idx, self.op = key, field, int(tag), int(idx), op
        self.ids = np.ascontiguousarray(ids, np.int64)
        self.w = np.ascontiguousarray(w, np.float64)
        self.denom = float(denom)
        # how the entries were made, for the per-rank table of a partitioned run:
        # ("point", k, j) = entry j of point definition k, ("reduce", mode) with mode "owned" (min / max / nodal mean)
        # or "measure" (integral / average)
        self.src = src


class Observables(RowSeries):
    def __init__(self, mesh, ct, ft, subdomain_list, ion_list, partitioned=False):
        """partitioned: the mesh is one rank's local mesh -- points are located at set-up (`partition`), where a
        point found on no rank raises on every rank."""
        self.partitioned = bool(partitioned)
        self._points = []             # (membrane?, tag, x) of every point definition
        self._ptab = None             # the per-rank table of a partitioned run (partition)
        self.mesh, self.ct, self.ft = mesh, ct, ft
        self.subdomain_list = subdomain_list
        self.ion_list = ion_list
        self.tags = list(subdomain_list.keys())
        self.sub_index = {t: s for s, t in enumerate(self.tags)}
        self.ion_names = [ion["name"] for ion in ion_list]
        self.items = []
        self._init_series()
        self._integral = {}

    # -- definition ------------------------------------------------------------------------------------
    def _add(self, item):
        if self._drain is not None:
            raise RuntimeError("observables are attached to a stepper: define them all before DeviceStepper.observe")
        if any(o.key == item.key for o in self.items):
            raise ValueError(f"observable {item.key!r} defined twice")
        self.items.append(item)

    def _ion_field(self, k):
        """(field id, index) of ion k: a solved ion's new c, or the eliminated one's c_<tag>."""
        return (L.F_C, k) if k < len(self.ion_names) - 1 else (L.F_C_ELIM, 0)

    def _check_tag(self, tag, cell=False):
        if tag not in self.subdomain_list:
            raise ValueError(f"no sub-domain with tag {tag}")
        if cell and tag == 0:
            raise ValueError("the ECS (tag 0) has no membrane: give the tag of a cell")

    def point(self, name, tag, x):
        """phi and every ion (the eliminated one included) at the point x of sub-domain `tag`:
        keys "<name>/phi", "<name>/<ion>"."""
        self._check_tag(tag)
        if self.partitioned:
            ids = w = np.zeros(0)
        else:
            ids, w = point_weights(self.subdomain_list[tag]["mesh_sub"], x, tag)
        k0 = self._new_point(False, tag, x)
        self._add(_Obs(f"{name}/phi", L.F_PHI, tag, 0, L.OBS_SUM, ids, w, src=("point", k0, 0)))
        for k, ion in enumerate(self.ion_names):
            f, i = self._ion_field(k)
            self._add(_Obs(f"{name}/{ion}", f, tag, i, L.OBS_SUM, ids, w, src=("point", k0, 0)))

    def _new_point(self, membrane, tag, x):
        """Index of a new point definition (recorded for `partition`)."""
        self._points.append((membrane, tag, np.asarray(x, np.float64).ravel()))
        return len(self._points) - 1

    def membrane_point(self, name, tag, x):
        """phi_M and the ECS / ICS traces of every ion at the point x of the membrane of cell `tag`:
        keys "<name>/phi_M", "<name>/<ion>_e", "<name>/<ion>_i"."""
        self._check_tag(tag, cell=True)
        if self.partitioned:
            e = i = q = w = np.zeros(0)
        else:
            e, i, q, w = membrane_weights(self.subdomain_list, tag, x)
        k0 = self._new_point(True, tag, x)
        self._add(_Obs(f"{name}/phi_M", L.F_PHI_M, tag, 0, L.OBS_SUM, q, w, src=("point", k0, 2)))
        for k, ion in enumerate(self.ion_names):
            f, j = self._ion_field(k)
            self._add(_Obs(f"{name}/{ion}_e", f, 0, j, L.OBS_SUM, e, w, src=("point", k0, 0)))
            self._add(_Obs(f"{name}/{ion}_i", f, tag, j, L.OBS_SUM, i, w, src=("point", k0, 1)))

    def reduce(self, name, quantity, tag, op, ion=None):
        """`op` of `quantity` ("phi", "c" with `ion`, or "phi_M") over sub-domain `tag` (phi_M: over the membrane of
        cell `tag`).  op: "integral" (exact for P1 / Q1), "nodal_mean" (`.mean()` of the nodal array), "average"
        (integral / measure), "min", "max"."""
        if op not in OPS:
            raise ValueError(f"op must be one of {OPS}")
        if quantity == "phi":
            self._check_tag(tag)
            field, idx, mesh = L.F_PHI, 0, self.subdomain_list[tag]["mesh_sub"]
        elif quantity == "c":
            self._check_tag(tag)
            if ion not in self.ion_names:
                raise ValueError(f"unknown ion {ion!r} (ions: {self.ion_names})")
            field, idx = self._ion_field(self.ion_names.index(ion))
            mesh = self.subdomain_list[tag]["mesh_sub"]
        elif quantity == "phi_M":
            self._check_tag(tag, cell=True)
            field, idx, mesh = L.F_PHI_M, 0, self.subdomain_list[tag]["mesh_mem"]
        else:
            raise ValueError("quantity must be 'phi', 'c' or 'phi_M'")
        n = mesh.num_vertices
        ids = np.arange(n)
        mem = quantity == "phi_M"
        if op in ("min", "max"):
            self._add(_Obs(name, field, tag, idx, L.OBS_MIN if op == "min" else L.OBS_MAX, ids, np.ones(n),
                           src=("reduce", "owned", mem, False)))
        elif op == "nodal_mean":
            self._add(_Obs(name, field, tag, idx, L.OBS_SUM, ids, np.ones(n), n, src=("reduce", "owned", mem, True)))
        else:
            w = self.integral_weights(mem, tag)
            self._add(_Obs(name, field, tag, idx, L.OBS_SUM, ids, w, w.sum() if op == "average" else 1.0,
                           src=("reduce", "measure", mem, op == "average")))

    def integral_weights(self, membrane, tag):
        key = (bool(membrane), tag)
        if key not in self._integral:
            sd = self.subdomain_list[tag]
            self._integral[key] = integral_weights(sd["mesh_mem"] if membrane else sd["mesh_sub"])
        return self._integral[key]

    @property
    def keys(self):
        return [o.key for o in self.items]

    def columns(self):
        """[(key, 1)] of the series row: one column per observable."""
        return [(o.key, 1) for o in self.items]

    # -- the device table (knpemi_observe_set) ----------------------------------------------------------
    def table(self, sub_index=None):
        """(spec [n][4] int32, ptr [n+1] int64, idx int32, w, denom) of knpemi_observe_set."""
        si = sub_index or self.sub_index
        spec = np.array([[o.field, si[o.tag], o.idx, o.op] for o in self.items], np.int32).reshape(-1, 4)
        ptr = np.zeros(len(self.items) + 1, np.int64)
        np.cumsum([o.ids.shape[0] for o in self.items], out=ptr[1:])
        idx = np.ascontiguousarray(np.concatenate([o.ids for o in self.items]).astype(np.int32))
        w = np.ascontiguousarray(np.concatenate([o.w for o in self.items]))
        denom = np.array([o.denom for o in self.items], np.float64)
        return spec, ptr, idx, w, denom

    def upload(self, dp, capacity):
        if not self.items:
            raise ValueError("no observables defined")
        spec, ptr, idx, w, denom = self.table(dp.sub_index)
        L.check(dp.lib.knpemi_observe_set(dp.h, len(self.items), L.iptr(spec.ravel()),
                                          ptr.ctypes.data_as(C.POINTER(C.c_int64)), L.iptr(idx), L.dptr(w),
                                          L.dptr(denom), int(capacity)))

    # -- partitioned runs -----------------------------------------------------------------------------------
    def partition(self, halo, gather=None, every=1, capacity=1024):
        """The table of this rank of a cell-partitioned run (see the module docstring), set in `self._ptab`.
        halo: the rank's `knpemi.fem.distributed.Halo` with its plans built; gather(obj) -> [obj of every rank]
        (default: `recording.gather_objects`).  Collective: every rank calls it once, with the same
        definitions in the same order and the same every / capacity, or every rank raises ValueError."""
        if not self.items:
            raise ValueError("no observables defined")
        rank = int(halo.rank)
        message = "observables: the halo does not number the vertices of these sub-domains"
        subs = self.subdomain_list
        owner = {(False, tag): ow for tag, ow in
                 item_owners({tag: sd["mesh_sub"] for tag, sd in subs.items()}, halo, "bulk", message).items()}
        owner.update({(True, tag): ow for tag, ow in
                      item_owners({tag: sd["mesh_mem"] for tag, sd in subs.items() if tag > 0}, halo, "mem", message).items()})
        # the recorder of a cell (membrane facet): the lowest owner among its vertices
        rec = {key: recorded_items(subs[key[1]]["mesh_mem" if key[0] else "mesh_sub"], ow, rank) for key, ow in owner.items()}
        # points: this rank's weights in the cells it records, or None
        found = []
        for membrane, tag, x in self._points:
            try:
                if membrane:
                    mem = self.subdomain_list[tag]["mesh_mem"]
                    q, w = Locator(mem, f"the membrane of cell {tag}", rec[(True, tag)]).weights(x)
                    pv = mem.parent_vertices[q]
                    e = np.searchsorted(self.subdomain_list[0]["mesh_sub"].parent_vertices, pv)
                    i = np.searchsorted(self.subdomain_list[tag]["mesh_sub"].parent_vertices, pv)
                    found.append((e.astype(np.int64), i.astype(np.int64), q, w))
                else:
                    ids, w = Locator(self.subdomain_list[tag]["mesh_sub"], f"sub-domain {tag}",
                                     rec[(False, tag)]).weights(x)
                    found.append((ids, w))
            except ValueError:
                found.append(None)
        # reductions: entries over owned vertices / recorded cells, and this rank's share of the denominator
        entries, share = [], []
        for o in self.items:
            if o.src[0] != "reduce":
                entries.append(None)
                share.append(0.0)
                continue
            _, mode, mem, _ = o.src
            ow = owner[(mem, o.tag)]
            if mode == "owned":
                ids = np.flatnonzero(ow == rank)
                entries.append((ids, np.ones(ids.shape[0])))
                share.append(float(ids.shape[0]))
            else:
                mesh = self.subdomain_list[o.tag]["mesh_mem" if mem else "mesh_sub"]
                w = integral_weights(mesh, rec[(mem, o.tag)])
                touched = np.zeros(mesh.num_vertices, bool)
                touched[mesh.cells[rec[(mem, o.tag)]].ravel()] = True
                ids = np.flatnonzero(touched)
                entries.append((ids, w[ids]))
                share.append(float(w.sum()))
        mine = dict(keys=self.keys, every=int(every), capacity=int(capacity), found=[f is not None for f in found],
                    share=share)
        allr = (gather or gather_objects)(mine)
        world = len(allr)
        agree_across_ranks(allr, ("keys", "every", "capacity"), "observables",
                           "every rank must define the same observables in the same order and pass the same every and "
                           "capacity")
        taker = []
        for k, (membrane, tag, x) in enumerate(self._points):
            ranks = [r for r in range(world) if allr[r]["found"][k]]
            if not ranks:
                where = f"the membrane of cell {tag}" if membrane else f"sub-domain {tag}"
                raise ValueError(f"point {x.tolist()} is not in {where} on any rank")
            taker.append(ranks[0])
        tab = []
        for j, o in enumerate(self.items):
            if o.src[0] == "point":
                _, k, part = o.src
                if taker[k] == rank:
                    f = found[k]
                    ids, w = (f[part], f[3]) if self._points[k][0] else f
                else:
                    ids, w = np.zeros(0, np.int64), np.zeros(0)
                denom = 1.0
            else:
                ids, w = entries[j]
                tot = allr[0]["share"][j]
                for r in range(1, world):               # rank order: the same bits on every rank
                    tot += allr[r]["share"][j]
                denom = tot if o.src[3] else 1.0
            tab.append((np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(w, np.float64), float(denom)))
        self._ptab = dict(rank=rank, world=world, entries=tab, taker=taker, recorded=rec, owner=owner)
        return self._ptab

    def partitioned_table(self, sub_index=None):
        """(spec, ptr, idx, w, denom) of knpemi_observe_set_partitioned, from `partition`."""
        si = sub_index or self.sub_index
        tab = self._ptab["entries"]
        spec = np.array([[o.field, si[o.tag], o.idx, o.op] for o in self.items], np.int32).reshape(-1, 4)
        ptr = np.zeros(len(self.items) + 1, np.int64)
        np.cumsum([t[0].shape[0] for t in tab], out=ptr[1:])
        idx = np.ascontiguousarray(np.concatenate([t[0] for t in tab]).astype(np.int32))
        w = np.ascontiguousarray(np.concatenate([t[1] for t in tab]))
        denom = np.array([t[2] for t in tab], np.float64)
        return spec, ptr, idx, w, denom

    def upload_partitioned(self, dp, capacity, halo, every=1):
        """`partition`, then knpemi_observe_set_partitioned (`rank_slots`).  Returns the objects the handle refers to
        (keep them alive while it records)."""
        self.partition(halo, None, every, capacity)
        spec, ptr, idx, w, denom = self.partitioned_table(dp.sub_index)
        n, world = len(self.items), self._ptab["world"]
        slots, keep = rank_slots(dp, halo, world, n)
        L.check(dp.lib.knpemi_observe_set_partitioned(
            dp.h, n, L.iptr(spec.ravel()), ptr.ctypes.data_as(C.POINTER(C.c_int64)), L.iptr(idx) if idx.size else None,
            L.dptr(w) if w.size else None, L.dptr(denom), int(capacity), self._ptab["rank"], world, *slots))
        return keep

    def _fields(self, o, phi, c, phi_M_prev):
        if o.field == L.F_PHI:
            return phi[o.tag].x._a
        if o.field == L.F_C:
            return c[o.tag][o.idx].x._a
        if o.field == L.F_C_ELIM:
            return self.ion_list[-1][f"c_{o.tag}"].x._a
        return phi_M_prev[o.tag].x._a

    def evaluate_partial_host(self, phi, c, phi_M_prev):
        """This rank's slot row of a partitioned run (after `partition`) from its host `Function`s: per observable
        the fold of its entries without the denominator, the op's identity without entries."""
        row = np.empty(len(self.items))
        for j, (o, (ids, w, _)) in enumerate(zip(self.items, self._ptab["entries"])):
            v = self._fields(o, phi, c, phi_M_prev)[ids]
            if o.op == L.OBS_MIN:
                row[j] = v.min() if v.size else np.inf
            elif o.op == L.OBS_MAX:
                row[j] = v.max() if v.size else -np.inf
            else:
                row[j] = np.dot(w, v) if v.size else 0.0
        return row

    # -- host evaluation ---------------------------------------------------------------------------------
    def evaluate_host(self, phi, c, phi_M_prev):
        """One row from host `Function`s: phi[tag], c[tag][k] (solved ions), phi_M_prev[tag]; the eliminated ion
        is read from ion_list[-1]["c_<tag>"]."""
        row = np.empty(len(self.items))
        for j, o in enumerate(self.items):
            u = self._fields(o, phi, c, phi_M_prev)
            v = u[o.ids]
            if o.op == L.OBS_MIN:
                row[j] = v.min()
            elif o.op == L.OBS_MAX:
                row[j] = v.max()
            else:
                row[j] = np.dot(o.w, v) / o.denom
        return row

    def record_host(self, t, phi, c, phi_M_prev):
        """Append the row of time t evaluated from host arrays (the host drivers' path)."""
        self._t.append(float(t))
        self._rows.append(self.evaluate_host(phi, c, phi_M_prev))


def combine_partials(obs, rows_by_rank):
    """The row of a partitioned run from the ranks' slot rows (`Observables.evaluate_partial_host`, one per rank in
    rank order), folded as record_combine_kernel does: in rank order with each observable's op, sums divided by the
    global denominator."""
    rows = np.asarray(rows_by_rank, np.float64)
    out = np.empty(rows.shape[1])
    for j, (o, (_, _, denom)) in enumerate(zip(obs.items, obs._ptab["entries"])):
        if o.op == L.OBS_MIN:
            v = np.inf
            for r in range(rows.shape[0]):
                v = min(v, rows[r, j])
        elif o.op == L.OBS_MAX:
            v = -np.inf
            for r in range(rows.shape[0]):
                v = max(v, rows[r, j])
        else:
            v = 0.0
            for r in range(rows.shape[0]):
                v += rows[r, j]
            v /= denom
        out[j] = v
    return out
