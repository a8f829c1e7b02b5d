"""Ion fluxes and current density per cell: which way the ions move, and how much of it is diffusion and how much drift.

The reference writes these quantities in its manufactured-solution scripts only (`tests/run_mms.py:270-301`:
`J_k = -D_k grad c_k - z_k D_k psi c_k grad phi`, total flux `F sum_k z_k J_k`).  `Observables` records linear
functionals of the nodal fields and `MembraneEvents` the firing of the membranes; a flux is a product of fields
(`c grad phi`) and needs a gradient, so neither can express it, and without this module a user downloads every field at
every step and differentiates on the host.  Here one launch behind the end-of-step update (csrc/kernels_flux.hip,
`DeviceStepper.fluxes`) evaluates the per-cell vectors from the vertex records the device already holds and appends their
integrals and maxima to a time series; the host reads either only when asked.

    fl = IonFluxes(subdomain_list, ion_list, physical_parameters)
    fl.watch(tag=0)                                   # every ion and the current in the ECS
    fl.watch(tag=1, ions=["K"], current=False)
    stepper.fluxes(fl, every=1, fields=True)          # ... stepper.step() ...
    ser = fl.series()                                 # "t", "0/K/diffusive" (n, gdim), "0/K/drift", "0/K/max", "0/current", ...
    f = fl.fields(0)                                  # "K/diffusive" (n_cell, gdim), ..., "current"

Definitions, the same for triangles, tetrahedra, hexahedra and quadrilaterals.  For a cell T of sub-domain s and every ion
k = 0 .. K-1, the eliminated one included:

  * c_k and g(u) are the value and the gradient, at the cell's centroid, of the P1 / Q1 interpolant of the nodal
    field.  Simplices: c_k is the mean of the vertex values and g the constant gradient.  Hexahedra (tensor vertex
    order, x[1 << t]): c_k is the mean of the eight values; the reference derivative along t is 1/4 sum_v +-u_v with
    the sign taken from bit t of v, mapped by the Jacobian at the centre.  Quadrilaterals (tensor vertex order
    [v00, v10, v01, v11]) are the same rule in 2-D: c_k is the mean of the four values, E_t = 1/2 sum_v +-x_v is
    column t of the Jacobian at the centre, d_t = 1/2 sum_v +-u_v, and the gradient solves E g = d.
  * J_diff = -D_k^s g(c_k),  J_drift = -z_k psi D_k^s c_k g(phi),  J = J_diff + J_drift.
  * Current density i = F sum_k z_k J_k, split the same way into i_diff and i_drift.
  * vol_T = |det| / d! on simplices and |det J(centre)| = |det E| on hexahedra and
    quadrilaterals (the midpoint rule).  The orientation of a cell
    does not matter: left-handed cells give the same answer.
  * The fields are phi, c_prev of the solved ions and the eliminated ion's c as the device holds them: at the end of a
    step that is the new state.

Series row: per watched (sub-domain, ion) the integrals sum_T vol_T J_diff and sum_T vol_T J_drift (gdim values each)
and max_T |J| (Euclidean norm); per watched sub-domain with `current=True` sum_T vol_T i and max_T |i|.  On simplices
the sums are the exact integrals of the discrete flux.

Cell-partitioned runs (`DeviceStepper.fluxes(fl, halo=halo)`, `WatchedIons.partition`): every cell of the global mesh is
recorded by one rank, the lowest owner among its vertices; a rank's ghost cells get their per-cell vectors and enter none
of its sums and maxima.  Every rank holds the global series -- maxima bit for bit those of one rank holding the whole
mesh, sums to rounding -- and `fields(tag, halo=halo)` the vectors of its local cells with the mask of the ones it
records.
"""
from __future__ import annotations

import numpy as np

from .fem.function import as_float
from .recording import (CURRENT_BIT, WatchedIons, combine_partials, item_owners, lib_int,  # noqa: F401
                        nodal_values as _values)

PARTS = ("diffusive", "drift")


def chunk():
    """Cells per workgroup of the record kernel."""
    return lib_int("kn_flux_chunk")


def fold_depth():
    """Workgroup partials the record kernel's fold of a column has in flight."""
    return lib_int("kn_flux_fold_depth")


_TENSOR_DIM = {"hexahedron": 3, "quadrilateral": 2}


def _tensor_signs(dim):
    """sign[t, v] = +1 where bit t of local vertex v is set, and the weight 2 / 2^dim of a reference derivative."""
    sign = np.array([[1.0 if (v >> t) & 1 else -1.0 for v in range(1 << dim)] for t in range(dim)])
    return sign, 2.0 / (1 << dim)


def cell_geometry(x, cells, cell_type):
    """(E, vol) of every cell: E[c, t] is edge vector t (simplices: x_(t+1) - x_0; hexahedra and quadrilaterals: column
    t of the Jacobian at the centre, 1/4 resp. 1/2 sum_v +-x_v), vol the cell's measure by the module docstring's rule."""
    xc = x[cells]
    if cell_type in _TENSOR_DIM:
        sign, w = _tensor_signs(_TENSOR_DIM[cell_type])
        E = w * np.einsum("tv,cva->cta", sign, xc)
        return E, np.abs(np.linalg.det(E))
    d = cells.shape[1] - 1
    E = xc[:, 1:] - xc[:, :1]
    return E, np.abs(np.linalg.det(E)) / (2.0 if d == 2 else 6.0)


def cell_value_and_gradient(E, cells, cell_type, u):
    """(value, gradient) at the centroids of the interpolant of the nodal field u: the gradient solves E g = d with d
    the field's differences along the edge vectors."""
    uc = u[cells]
    if cell_type in _TENSOR_DIM:
        sign, w = _tensor_signs(_TENSOR_DIM[cell_type])
        d = w * uc @ sign.T
    else:
        d = uc[:, 1:] - uc[:, :1]
    return uc.mean(axis=1), np.linalg.solve(E, d[:, :, None])[:, :, 0]


def norm(J):
    """Euclidean norm of every row, the squares added in component order."""
    n2 = J[:, 0] * J[:, 0]
    for a in range(1, J.shape[1]):
        n2 = n2 + J[:, a] * J[:, a]
    return np.sqrt(n2)


class IonFluxes(WatchedIons):
    _NAME, _WATCH, _SELF = "flux", "sub-domain", "these fluxes are"

    def __init__(self, subdomain_list, ion_list, physical_params):
        """subdomain_list: the problem's sub-domain dictionary (every entry carries its "mesh_sub"); ion_list: the ions
        in the problem's order, the eliminated one last; physical_params: "F" and "psi" are read."""
        self._init_watched(ion_list)
        self.tags = list(subdomain_list)
        self.mesh = {t: subdomain_list[t]["mesh_sub"] for t in self.tags}
        self.D = {t: [as_float(ion["D"][t]) for ion in ion_list] for t in self.tags}
        self.F, self.psi = as_float(physical_params["F"]), as_float(physical_params["psi"])
        self.gdim = int(self.mesh[self.tags[0]].x.shape[1])
        self._geo = {}

    # -- definition ------------------------------------------------------------------------------------
    def watch(self, tag, ions=None, current=True):
        """Watch sub-domain `tag`: the ions named in `ions` (names or indices; None: all, the eliminated one included)
        and, with `current`, the current density."""
        if self._dev is not None:
            raise RuntimeError("fluxes are attached to a device problem: watch every sub-domain before fluxes()")
        if tag not in self.mesh:
            raise ValueError(f"no sub-domain with tag {tag}")
        self._watch_ions(tag, ions, current)

    def columns(self):
        """[(key, width)] of the series row in the device's order: "<tag>/<ion>/diffusive" and "<tag>/<ion>/drift" (gdim
        wide), "<tag>/<ion>/max", "<tag>/current" (gdim wide) and "<tag>/current_max"."""
        out, g = [], self.gdim
        for tag, (idx, cur) in self.watched.items():
            for k in idx:
                n = self.names[k]
                out += [(f"{tag}/{n}/diffusive", g), (f"{tag}/{n}/drift", g), (f"{tag}/{n}/max", 1)]
            if cur:
                out += [(f"{tag}/current", g), (f"{tag}/current_max", 1)]
        return out

    def n_cells(self, tag):
        return int(self.mesh[tag].cells.shape[0])

    def max_columns(self):
        return np.concatenate([np.full(w, key.endswith("max")) for key, w in self.columns()])

    def _item_owners(self, halo):
        own = item_owners(self.mesh, halo, "bulk", "fluxes: the halo does not number the vertices of these sub-domains")
        return {tag: (self.mesh[tag], own[tag]) for tag in self.tags if tag in self.watched}

    # -- host restatement ----------------------------------------------------------------------------------
    def _geometry(self, tag):
        if tag not in self._geo:
            m = self.mesh[tag]
            x, cells = np.asarray(m.x, np.float64), np.asarray(m.cells)
            self._geo[tag] = (cells, m.cell_type) + cell_geometry(x, cells, m.cell_type)
        return self._geo[tag]

    def compute_host(self, phi, c, c_elim=None, recorded=None):
        """(fields, row) from host data, written from the definitions of the module docstring: the numpy restatement of
        the device kernel and the reference of the device tests.  phi[tag]: the potential of every watched sub-domain;
        c[tag]: the nodal concentrations of its ions, K of them, or the K - 1 solved ones with the eliminated ion's
        taken from c_elim[tag] (default: `ion_list[-1]["c_<tag>"]`).  `Function`s or arrays.
        fields[tag]: what `fields(tag)` returns; row: the series row as {key: (gdim,) array or float}.
        recorded: {tag: bool per cell} -- the partial row of one rank of a partition (`partition`): the sums and the
        maxima (from 0) run over the recorded cells only; the fields are those of every cell."""
        fields, row = {}, {}
        for tag, (idx, cur) in self.watched.items():
            cells, kind, E, vol = self._geometry(tag)
            rec = slice(None) if recorded is None else np.asarray(recorded[tag], bool)
            top = (lambda a: float(a.max())) if recorded is None else (lambda a: float(a.max(initial=0.0)))
            ck = list(c[tag])
            if len(ck) == self.K - 1:
                ck.append(self.ion_list[-1][f"c_{tag}"] if c_elim is None else c_elim[tag])
            if len(ck) != self.K:
                raise ValueError(f"sub-domain {tag}: {len(ck)} concentrations for {self.K} ions")
            _, gphi = cell_value_and_gradient(E, cells, kind, _values(phi[tag]))
            out = {}
            i_diff, i_drift = np.zeros_like(gphi), np.zeros_like(gphi)
            for k in (range(self.K) if cur else idx):
                cbar, gc = cell_value_and_gradient(E, cells, kind, _values(ck[k]))
                Dk, zk = self.D[tag][k], self.z[k]
                Jd = -Dk * gc
                Jr = -(zk * self.psi * Dk) * cbar[:, None] * gphi
                i_diff += self.F * zk * Jd
                i_drift += self.F * zk * Jr
                if k in idx:
                    n = self.names[k]
                    out[f"{n}/diffusive"], out[f"{n}/drift"] = Jd, Jr
                    row[f"{tag}/{n}/diffusive"] = (vol[:, None] * Jd)[rec].sum(axis=0)
                    row[f"{tag}/{n}/drift"] = (vol[:, None] * Jr)[rec].sum(axis=0)
                    row[f"{tag}/{n}/max"] = top(norm(Jd + Jr)[rec])
            if cur:
                out["current/diffusive"], out["current/drift"], out["current"] = i_diff, i_drift, i_diff + i_drift
                row[f"{tag}/current"] = (vol[:, None] * out["current"])[rec].sum(axis=0)
                row[f"{tag}/current_max"] = top(norm(out["current"])[rec])
            fields[tag] = out
        return fields, row

    def volumes(self, tag):
        """vol_T of every cell of sub-domain `tag`."""
        return self._geometry(tag)[3]

    def record_host(self, t, phi, c, c_elim=None):
        """Append the row of `compute_host` to the series (host drivers)."""
        self._t.append(float(t))
        self._rows.append(self.row_vector(self.compute_host(phi, c, c_elim)[1]))

    # -- output --------------------------------------------------------------------------------------------
    def fields(self, tag, halo=None):
        """Per-cell arrays (n_cell, gdim) of the last device record made with fields: "<ion>/diffusive" and
        "<ion>/drift" for every watched ion, "current/diffusive", "current/drift" and their sum "current" where the
        current is watched (one synchronisation).  halo: on a cell-partitioned run the arrays cover this rank's local
        cells, ghosts included, and "recorded" is the mask of the cells this rank records."""
        self._check_watched(tag)
        get = self._getter(tag, (self.gdim, self.n_cells(tag)), "DeviceStepper.fluxes")
        idx, cur = self.watched[tag]
        out = {}
        for k in idx:
            for p, name in enumerate(PARTS):
                out[f"{self.names[k]}/{name}"] = np.ascontiguousarray(get(k, p).T)
        if cur:
            for p, name in enumerate(PARTS):
                out[f"current/{name}"] = np.ascontiguousarray(get(-1, p).T)
            out["current"] = out["current/diffusive"] + out["current/drift"]
        if halo is not None:
            out["recorded"] = self._recorded_of(tag, halo, self.n_cells(tag))
        return out
