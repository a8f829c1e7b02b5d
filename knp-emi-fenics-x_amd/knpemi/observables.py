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
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .fem.probe import integral_weights, membrane_weights, point_weights

OPS = ("integral", "nodal_mean", "average", "min", "max")


class _Obs:
    __slots__ = ("key", "field", "tag", "idx", "op", "ids", "w", "denom")

    def __init__(self, key, field, tag, idx, op, ids, w, denom=1.0):
        self.key, self.field, self.tag, self.idx, self.op = key, field, int(tag), int(idx), op
        self.ids = np.ascontiguousarray(ids, np.int64)
        self.w = np.ascontiguousarray(w, np.float64)
        self.denom = float(denom)


class Observables:
    def __init__(self, mesh, ct, ft, subdomain_list, ion_list):
        self.mesh, self.ct, self.ft = mesh, ct, ft
        self.subdomain_list = subdomain_list
        self.ion_list = ion_list
        self.tags = list(subdomain_list.keys())
        self.sub_index = {t: s for s, t in enumerate(self.tags)}
        self.ion_names = [ion["name"] for ion in ion_list]
        self.items = []
        self._t = []
        self._rows = []
        self._drain = None            # set by DeviceStepper.observe: moves device rows into _t / _rows
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
        ids, w = point_weights(self.subdomain_list[tag]["mesh_sub"], x, tag)
        self._add(_Obs(f"{name}/phi", L.F_PHI, tag, 0, L.OBS_SUM, ids, w))
        for k, ion in enumerate(self.ion_names):
            f, i = self._ion_field(k)
            self._add(_Obs(f"{name}/{ion}", f, tag, i, L.OBS_SUM, ids, w))

    def membrane_point(self, name, tag, x):
        """phi_M and the ECS / ICS traces of every ion at the point x of the membrane of cell `tag`:
        keys "<name>/phi_M", "<name>/<ion>_e", "<name>/<ion>_i"."""
        self._check_tag(tag, cell=True)
        e, i, q, w = membrane_weights(self.subdomain_list, tag, x)
        self._add(_Obs(f"{name}/phi_M", L.F_PHI_M, tag, 0, L.OBS_SUM, q, w))
        for k, ion in enumerate(self.ion_names):
            f, j = self._ion_field(k)
            self._add(_Obs(f"{name}/{ion}_e", f, 0, j, L.OBS_SUM, e, w))
            self._add(_Obs(f"{name}/{ion}_i", f, tag, j, L.OBS_SUM, i, w))

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
        if op in ("min", "max"):
            self._add(_Obs(name, field, tag, idx, L.OBS_MIN if op == "min" else L.OBS_MAX, ids, np.ones(n)))
        elif op == "nodal_mean":
            self._add(_Obs(name, field, tag, idx, L.OBS_SUM, ids, np.ones(n), n))
        else:
            w = self.integral_weights(quantity == "phi_M", tag)
            self._add(_Obs(name, field, tag, idx, L.OBS_SUM, ids, w, w.sum() if op == "average" else 1.0))

    def integral_weights(self, membrane, tag):
        key = (bool(membrane), tag)
        if key not in self._integral:
            sd = self.subdomain_list[tag]
            self._integral[key] = integral_weights(sd["mesh_mem"] if membrane else sd["mesh_sub"])
        return self._integral[key]

    @property
    def keys(self):
        return [o.key for o in self.items]

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

    # -- host evaluation ---------------------------------------------------------------------------------
    def evaluate_host(self, phi, c, phi_M_prev):
        """One row from host `Function`s: phi[tag], c[tag][k] (solved ions), phi_M_prev[tag]; the eliminated ion
        is read from ion_list[-1]["c_<tag>"]."""
        row = np.empty(len(self.items))
        for j, o in enumerate(self.items):
            if o.field == L.F_PHI:
                u = phi[o.tag].x._a
            elif o.field == L.F_C:
                u = c[o.tag][o.idx].x._a
            elif o.field == L.F_C_ELIM:
                u = self.ion_list[-1][f"c_{o.tag}"].x._a
            else:
                u = phi_M_prev[o.tag].x._a
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

    # -- output ------------------------------------------------------------------------------------------
    def _append_rows(self, times, rows):
        self._t.extend(float(t) for t in times)
        self._rows.extend(np.asarray(rows, np.float64).reshape(len(times), len(self.items)))

    def clear(self):
        self._t, self._rows = [], []

    def series(self):
        """{"t": (n,), key: (n,) for every observable}; reads the device buffer of an attached stepper first."""
        if self._drain is not None:
            self._drain()
        rows = np.array(self._rows, np.float64).reshape(len(self._rows), len(self.items))
        out = {"t": np.array(self._t, np.float64)}
        for j, key in enumerate(self.keys):
            out[key] = rows[:, j].copy()
        return out

    def save(self, path):
        np.savez(path, **self.series())
