"""Recorders of a DG run (knpemi.dg.DGProblem): observables, jump seminorms and membrane events on the device.

The reference has no DG code (knpemi/dg.py says what it does have), so there is no reference interface here either; the
two classes are the DG counterparts of `knpemi.observables.Observables` and `knpemi.events.MembraneEvents` and share their
machinery: the row series and the tap of `knpemi.recording`, the event rules and helpers of `knpemi.events`, the point
location of `knpemi.fem.probe`, and on the device the observe and event kernels of the CG path.

Indices are those of the DG handle: broken dof (cell c, local vertex j) = c * nv + j, membrane node (facet f, vertex a) =
f * nf + a.  Fields are arrays (n_cells, nv) and (n_mem_facets, nf).

    obs = DGObservables(mesh, ct, ft, [0, 1], [1], ["Na", "K", "Cl"])
    obs.point("ECS", [25e-6, 3.5e-6], tag=0)               # ECS/phi, ECS/Na, ECS/K, ECS/Cl
    obs.membrane_point("mem", [25e-6, 3e-6], 1)            # mem/phi_M, mem/Na_e, mem/Na_i, ...
    obs.reduce("K_max", "c", 0, "max", ion="K")
    obs.jump("J_phi", "phi", 0)                            # the jump seminorm of phi over the ECS
    dp.observe(obs)                                        # ... dp.update(c); dp.record(t) ...
    obs.series()

The jump seminorm of a field u over sub-domain s,

    J_s(u) = sum over the interior facets F with both cells in s of  int_F (1 / h_F) [u]^2 dS,

is what the interior penalty of the DG kernels controls (1 / h_F is their penalty weight): it vanishes for a continuous
field and grows with an under-resolved front or too small a penalty parameter.  It is recorded as is, without a square
root.  Both classes are constructible without a GPU and without the library; `evaluate_host` and `record_host` are the
numpy restatements the device is tested against.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .dg import cell_subdomains, membrane_facets
from .events import MembraneEvents
from .fem.probe import _G2, Locator, _simplex_coords, _tensor_coords, _tensor_shape
from .recording import RowSeries

OPS = ("integral", "nodal_mean", "average", "min", "max")
_SIMPLEX = ("interval", "triangle", "tetrahedron")
_FACET_TYPE = {"triangle": "interval", "tetrahedron": "triangle", "hexahedron": "quadrilateral"}


class _Broken:
    """The broken counterpart of a mesh for `Locator`: every element with vertices of its own."""

    def __init__(self, X, cell_type):
        n, nv, d = X.shape
        self.x = X.reshape(n * nv, d)
        self.cells = np.arange(n * nv, dtype=np.int64).reshape(n, nv)
        self.cell_type = cell_type


def element_integral_weights(X, cell_type):
    """(n, nv) integrals of the P1 / Q1 basis functions over the elements X (n, nv, gdim): measure / nv on simplices, the
    2-point Gauss rule per direction on hexahedra and quadrilaterals."""
    n, nv, g = X.shape
    if cell_type in _SIMPLEX:
        d = nv - 1
        E = X[:, 1:, :] - X[:, :1, :]
        G = np.einsum("nig,njg->nij", E, E)
        vol = np.sqrt(np.abs(np.linalg.det(G))) / np.prod(np.arange(1, d + 1))
        return np.repeat(vol[:, None] / nv, nv, axis=1)
    d = int(np.log2(nv))
    pts = np.stack(np.meshgrid(*([_G2] * d), indexing="ij"), axis=-1).reshape(-1, d)
    N, dN = _tensor_shape(pts)
    J = np.einsum("qvu,nvg->nqgu", dN, X)
    det = np.abs(np.linalg.det(J)) if d == g else np.sqrt(np.abs(np.linalg.det(np.einsum("nqgu,nqgw->nquw", J, J))))
    return np.einsum("nq,qv->nv", det, N) * 0.5 ** d


def facet_local_vertices(cell_type):
    """(n facets per cell, nf): local vertex of local facet f at facet position m, as knpemi_dg_create numbers them --
    simplices: facet f is opposite vertex f, its vertices in increasing local order; hexahedra: facet f = 2 a + b is
    xi_a = b, position m has bit 0 along the lower and bit 1 along the higher remaining axis."""
    if cell_type == "hexahedron":
        out = []
        for a in range(3):
            a1, a2 = (1 if a == 0 else 0), (1 if a == 2 else 2)
            for b in range(2):
                out.append([(b << a) | ((m & 1) << a1) | ((m >> 1) << a2) for m in range(4)])
        return np.array(out, np.int64)
    nv = {"triangle": 3, "tetrahedron": 4}[cell_type]
    return np.array([[j for j in range(nv) if j != f] for f in range(nv)], np.int64)


class DGTopology:
    """The facets two cells share, from the cells alone: `interior` facets (both cells in one sub-domain, not a membrane)
    as arrays over the facets -- cT < cN the two cells, fT / fN their local facets, lT / lN (m, nf) the local vertices at
    T's facet positions and the matching ones of N -- and the membrane nodes' dofs `dof_e`, `dof_i` (nmf, nf)."""

    def __init__(self, cells, cell_type, cell_sub, mem_facets):
        cells = np.asarray(cells, np.int64)
        nc, nv = cells.shape
        FV = facet_local_vertices(cell_type)
        nfc, nf = FV.shape
        verts = cells[:, FV].reshape(nc * nfc, nf)
        keys = np.sort(verts, axis=1)
        order = np.lexsort(keys.T[::-1])                    # stable: equal keys keep increasing (cell, facet)
        ks = keys[order]
        same = np.flatnonzero(np.all(ks[1:] == ks[:-1], axis=1))
        a, b = order[same], order[same + 1]
        cT, fT, cN, fN = a // nfc, a % nfc, b // nfc, b % nfc
        mem = {tuple(k): i for i, k in enumerate(np.sort(np.asarray(mem_facets, np.int64).reshape(-1, nf), axis=1))}
        which = np.array([mem.get(tuple(k), -1) for k in ks[same]], np.int64)
        lT = FV[fT]                                          # (m, nf)
        vT = np.take_along_axis(cells[cT], lT, axis=1)
        lN = np.argmax(cells[cN][:, None, :] == vT[:, :, None], axis=2)
        inner = which < 0
        if np.any(cell_sub[cT[inner]] != cell_sub[cN[inner]]):
            raise ValueError("a facet between two sub-domains is not a membrane facet")
        self.cT, self.cN, self.fT, self.fN, self.lT, self.lN = (v[inner] for v in (cT, cN, fT, fN, lT, lN))
        nmf = len(mem)
        self.dof_e = np.full((nmf, nf), -1, np.int64)
        self.dof_i = np.full((nmf, nf), -1, np.int64)
        mf = np.asarray(mem_facets, np.int64).reshape(-1, nf)
        for j in np.flatnonzero(~inner):
            f = which[j]
            e, i = (cT[j], cN[j]) if cell_sub[cT[j]] == 0 else (cN[j], cT[j])
            for node, v in enumerate(mf[f]):
                self.dof_e[f, node] = e * nv + int(np.flatnonzero(cells[e] == v)[0])
                self.dof_i[f, node] = i * nv + int(np.flatnonzero(cells[i] == v)[0])
        if nmf and (self.dof_e.min() < 0 or self.dof_i.min() < 0):
            raise ValueError("a membrane facet is not shared by two cells")


def jump_weights(X, topo, cell_type):
    """(w (m, q), N (q, nf)) of the interior facets of `topo`: J_F(u) = sum_q w[F, q] (sum_a N[q, a] d_a)^2 with d the nodal
    jumps at T's facet positions.  Simplices: the closed form (1 / h_F) |F| (sum d^2 + (sum d)^2) / (nf (nf + 1)) -- the
    rows of N are the unit vectors and the row of ones, every w the common factor.  Hexahedra: the 2 x 2 Gauss rule, w the
    surface weight of the point times 1 / h_F there."""
    cT, cN, lT, lN = topo.cT, topo.cN, topo.lT, topo.lN
    m, nf = lT.shape
    P = np.take_along_axis(X[cT], lT[:, :, None], axis=1)              # (m, nf, d)
    if cell_type != "hexahedron":
        d = X.shape[2]
        oT = X[cT, topo.fT]
        oN = X[cN, topo.fN]
        if d == 2:
            e = P[:, 1] - P[:, 0]
            cr = np.stack([e[:, 1], -e[:, 0]], axis=1)
            area = np.linalg.norm(cr, axis=1)
        else:
            cr = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
            area = 0.5 * np.linalg.norm(cr, axis=1)
        n = cr / np.linalg.norm(cr, axis=1)[:, None]
        hT = np.abs(np.einsum("md,md->m", oT - P[:, 0], n))
        hN = np.abs(np.einsum("md,md->m", oN - P[:, 0], n))
        inv_h = 0.5 * (1.0 / hT + 1.0 / hN)
        N = np.concatenate([np.eye(nf), np.ones((1, nf))], axis=0)
        w = np.repeat((inv_h * area / (nf * (nf + 1)))[:, None], nf + 1, axis=1)
        return w, N
    aT, aN = topo.fT // 2, topo.fN // 2
    bT = np.take_along_axis(X[cT], (lT ^ (1 << aT)[:, None])[:, :, None], axis=1)      # the vertices behind the facet
    bN = np.take_along_axis(X[cN], (lN ^ (1 << aN)[:, None])[:, :, None], axis=1)
    st = np.array([[_G2[p & 1], _G2[p >> 1]] for p in range(4)])
    N, dN = _tensor_shape(st)                                          # (q, 4), (q, 4, 2)
    ts = np.einsum("qa,mad->mqd", dN[:, :, 0], P)
    tt = np.einsum("qa,mad->mqd", dN[:, :, 1], P)
    eT = np.einsum("qa,mad->mqd", N, bT - P)
    eN = np.einsum("qa,mad->mqd", N, bN - P)
    cr = np.cross(ts, tt)
    A = np.linalg.norm(cr, axis=2)
    cT_ = A / np.abs(np.einsum("mqd,mqd->mq", cr, eT))                 # |grad xi_normal| of T at the point
    cN_ = A / np.abs(np.einsum("mqd,mqd->mq", cr, eN))
    return 0.25 * A * 0.5 * (cT_ + cN_), N


class _Item:
    __slots__ = ("key", "field", "sub", "idx", "op", "ids", "w", "denom")

    def __init__(self, key, field, sub, idx, op, ids, w, denom=1.0):
        self.key, self.field, self.sub, self.idx, self.op = key, int(field), int(sub), int(idx), int(op)
        self.ids = np.ascontiguousarray(ids, np.int64)
        self.w = np.ascontiguousarray(w, np.float64)
        self.denom = float(denom)


class DGObservables(RowSeries):
    def __init__(self, mesh, ct, ft, subdomain_tags, membrane_tags, ion_names):
        """`mesh`, `ct`, `ft`, `subdomain_tags`, `membrane_tags`: as for `DGProblem`; `ion_names`: the K ions in the
        problem's order, the eliminated one last."""
        if mesh.cell_type not in _FACET_TYPE:
            raise ValueError("the DG variant is built for triangles, tetrahedra and hexahedra")
        self.mesh = mesh
        self.cell_type, self.facet_type = mesh.cell_type, _FACET_TYPE[mesh.cell_type]
        self.cell_sub = cell_subdomains(ct, subdomain_tags)
        self.mem_facets, self.mem_tags = membrane_facets(mesh, ft, membrane_tags)
        self.sub_index = {t: s for s, t in enumerate(subdomain_tags)}
        self.membrane_tags = list(membrane_tags)
        self.ion_names = list(ion_names)
        self.K = len(self.ion_names)
        x = np.asarray(mesh.x, np.float64)
        self.cells = np.asarray(mesh.cells, np.int64)
        self.n_cells, self.nv = self.cells.shape
        self.nmf, self.nf = self.mem_facets.shape
        self.n, self.nq = self.n_cells * self.nv, self.nmf * self.nf
        self.X = x[self.cells]                                        # (n_cells, nv, d)
        self.XM = x[self.mem_facets]                                  # (nmf, nf, d)
        self.items = []
        self._init_series()
        self._topo = self._jw = None
        self._locators, self._cell_w = {}, None

    # -- what the definitions are built from -------------------------------------------------------------------
    @property
    def topology(self):
        if self._topo is None:
            self._topo = DGTopology(self.cells, self.cell_type, self.cell_sub, self.mem_facets)
        return self._topo

    def membrane_dofs(self):
        """(dof_e, dof_i) (nmf, nf): the broken dofs of the ECS cell / of the intracellular cell at every membrane node,
        as `DGProblem.membrane_dofs` returns them."""
        return self.topology.dof_e, self.topology.dof_i

    def _sub(self, tag):
        if tag not in self.sub_index:
            raise ValueError(f"no sub-domain with tag {tag}")
        return self.sub_index[tag]

    def _ion(self, ion):
        if ion not in self.ion_names:
            raise ValueError(f"unknown ion {ion!r} (ions: {self.ion_names})")
        return self.ion_names.index(ion)

    def _membrane(self, tag):
        if tag not in self.membrane_tags or not np.any(self.mem_tags == tag):
            raise ValueError(f"no membrane facet with tag {tag}")
        return np.flatnonzero(self.mem_tags == tag)

    def _add(self, item):
        if self._drain is not None:
            raise RuntimeError("observables are attached to a problem: define them all before DGProblem.observe")
        if any(o.key == item.key for o in self.items):
            raise ValueError(f"observable {item.key!r} defined twice")
        self.items.append(item)

    # -- definition --------------------------------------------------------------------------------------------
    def point_weights(self, x, tag=None):
        """(broken dofs, shape-function weights) of the point x: through the lowest-numbered cell that contains it, of
        sub-domain `tag` when given."""
        if tag not in self._locators:
            mask = None if tag is None else self.cell_sub == self._sub(tag)
            what = "the mesh" if tag is None else f"sub-domain {tag}"
            self._locators[tag] = Locator(_Broken(self.X, self.cell_type), what, mask)
        return self._locators[tag].weights(x)

    def point(self, name, x, tag=None):
        """phi and every ion (the eliminated one included) at the point x, through the one cell that contains it (on a
        facet: the lowest-numbered containing cell, of sub-domain `tag` when given): keys "<name>/phi", "<name>/<ion>"."""
        ids, w = self.point_weights(x, tag)
        self._add(_Item(f"{name}/phi", L.DG_PHI, 0, 0, L.OBS_SUM, ids, w))
        for k, ion in enumerate(self.ion_names):
            self._add(_Item(f"{name}/{ion}", L.DG_C, 0, k, L.OBS_SUM, ids, w))

    def membrane_weights(self, x, membrane_tag):
        """(facet, weights (nf,)): the nearest membrane facet tagged `membrane_tag` (ties: the lowest) and its shape
        functions at the point of it closest to x."""
        fac = self._membrane(membrane_tag)
        p = np.asarray(x, np.float64).ravel()
        X = self.XM[fac]
        if p.shape[0] != X.shape[2]:
            raise ValueError(f"point {p.tolist()} has {p.shape[0]} coordinates, the mesh {X.shape[2]}")
        if self.facet_type == "quadrilateral":
            xi, _ = _tensor_coords(X, p)
            W, _ = _tensor_shape(np.clip(xi, 0.0, 1.0).reshape(-1, 2))
        else:
            W = _closest_on_simplices(X, p)
        dist = np.linalg.norm(np.einsum("na,nad->nd", W, X) - p[None, :], axis=1)
        j = int(np.argmin(dist))                            # the first minimum: ties go to the lowest facet
        return int(fac[j]), W[j]

    def membrane_point(self, name, x, membrane_tag):
        """phi_M at the nearest facet of the membrane tagged `membrane_tag` and the traces of every ion on its ECS and its
        intracellular side: keys "<name>/phi_M", "<name>/<ion>_e", "<name>/<ion>_i"."""
        f, w = self.membrane_weights(x, membrane_tag)
        de, di = self.membrane_dofs()
        self._add(_Item(f"{name}/phi_M", L.DG_PHI_M, 0, 0, L.OBS_SUM, f * self.nf + np.arange(self.nf), w))
        for k, ion in enumerate(self.ion_names):
            self._add(_Item(f"{name}/{ion}_e", L.DG_C, 0, k, L.OBS_SUM, de[f], w))
            self._add(_Item(f"{name}/{ion}_i", L.DG_C, 0, k, L.OBS_SUM, di[f], w))

    def integral_weights(self, quantity, tag):
        """(ids, w): sum_j w_j u[ids_j] is the exact integral of the broken field over the cells of sub-domain `tag`
        (phi_M: over the membrane facets tagged `tag`)."""
        if quantity == "phi_M":
            fac = self._membrane(tag)
            w = element_integral_weights(self.XM[fac], self.facet_type)
            return (fac[:, None] * self.nf + np.arange(self.nf)[None, :]).ravel(), w.ravel()
        if self._cell_w is None:
            self._cell_w = element_integral_weights(self.X, self.cell_type)
        c = np.flatnonzero(self.cell_sub == self._sub(tag))
        return (c[:, None] * self.nv + np.arange(self.nv)[None, :]).ravel(), self._cell_w[c].ravel()

    def reduce(self, name, quantity, tag, op, ion=None):
        """`op` of `quantity` -- "phi" or "c" (with `ion`) over the broken dofs of the cells of sub-domain `tag`, "phi_M"
        over the nodes of the membrane facets tagged `tag`.  op: "integral" (exact for broken P1 / Q1), "nodal_mean",
        "average" (integral / measure), "min", "max"."""
        if op not in OPS:
            raise ValueError(f"op must be one of {OPS}")
        if quantity == "phi":
            field, idx = L.DG_PHI, 0
        elif quantity == "c":
            field, idx = L.DG_C, self._ion(ion)
        elif quantity == "phi_M":
            field, idx = L.DG_PHI_M, 0
        else:
            raise ValueError("quantity must be 'phi', 'c' or 'phi_M'")
        ids, w = self.integral_weights(quantity, tag)
        if ids.size == 0:
            raise ValueError(f"sub-domain {tag} has no cells")
        n = ids.shape[0]
        if op in ("min", "max"):
            self._add(_Item(name, field, 0, idx, L.OBS_MIN if op == "min" else L.OBS_MAX, ids, np.ones(n)))
        elif op == "nodal_mean":
            self._add(_Item(name, field, 0, idx, L.OBS_SUM, ids, np.ones(n), n))
        else:
            self._add(_Item(name, field, 0, idx, L.OBS_SUM, ids, w, w.sum() if op == "average" else 1.0))

    def jump(self, name, quantity, tag, ion=None):
        """The jump seminorm J_tag(u) of u = "phi" or "c" (with `ion`) over the interior facets of sub-domain `tag`,
        recorded as is (no square root)."""
        if quantity == "phi":
            idx = -1
        elif quantity == "c":
            idx = self._ion(ion)
        else:
            raise ValueError("quantity must be 'phi' or 'c'")
        self._add(_Item(name, L.DG_JUMP, self._sub(tag), idx, L.OBS_SUM, [0], [1.0]))

    @property
    def keys(self):
        return [o.key for o in self.items]

    def columns(self):
        """[(key, 1)] of the series row: one column per observable."""
        return [(o.key, 1) for o in self.items]

    # -- the device table (knpemi_dg_observe_set) --------------------------------------------------------------
    def table(self):
        """(spec [n][4] int32, ptr [n+1] int64, idx int32, w, denom) of knpemi_dg_observe_set."""
        spec = np.array([[o.field, o.sub, o.idx, o.op] for o in self.items], np.int32).reshape(-1, 4)
        ptr = np.zeros(len(self.items) + 1, np.int64)
        np.cumsum([o.ids.shape[0] for o in self.items], out=ptr[1:])
        idx = np.ascontiguousarray(np.concatenate([o.ids for o in self.items]).astype(np.int32))
        w = np.ascontiguousarray(np.concatenate([o.w for o in self.items]))
        denom = np.array([o.denom for o in self.items], np.float64)
        return spec, ptr, idx, w, denom

    def upload(self, dp, capacity):
        if not self.items:
            raise ValueError("no observables defined")
        if dp.n != self.n or dp.nmf != self.nmf or dp.K != self.K:
            raise ValueError("these observables were defined on another mesh or for another number of ions")
        spec, ptr, idx, w, denom = self.table()
        L.check(dp.lib.knpemi_dg_observe_set(dp.h, len(self.items), L.iptr(spec.ravel()),
                                             ptr.ctypes.data_as(C.POINTER(C.c_int64)), L.iptr(idx), L.dptr(w),
                                             L.dptr(denom), int(capacity)))

    # -- host restatement ----------------------------------------------------------------------------------------
    def jump_host(self, u, tag, squares=False):
        """J_tag(u) of the broken field u (n_cells, nv) with numpy; squares: the same sum with [u]^2 replaced by
        u_T^2 + u_N^2, the scale the jump's rounding error is measured against."""
        s = self._sub(tag)
        topo = self.topology
        if self._jw is None:
            self._jw = jump_weights(self.X, topo, self.cell_type)
        w, N = self._jw
        u = np.asarray(u, np.float64).reshape(self.n_cells, self.nv)
        sel = np.flatnonzero(self.cell_sub[topo.cT] == s)
        uT = np.take_along_axis(u[topo.cT[sel]], topo.lT[sel], axis=1)
        uN = np.take_along_axis(u[topo.cN[sel]], topo.lN[sel], axis=1)
        if squares:
            return float(np.sum(w[sel] * ((uT @ N.T) ** 2 + (uN @ N.T) ** 2)))
        return float(np.sum(w[sel] * ((uT - uN) @ N.T) ** 2))

    def evaluate_host(self, c_all, phi, phi_M):
        """The row of the device with numpy: c_all the K concentration fields (n_cells, nv), the eliminated ion last,
        phi (n_cells, nv), phi_M (nmf, nf)."""
        c_all = [np.asarray(c, np.float64).reshape(-1) for c in c_all]
        phi = np.asarray(phi, np.float64).reshape(-1)
        phi_M = np.asarray(phi_M, np.float64).reshape(-1)
        tags = {s: t for t, s in self.sub_index.items()}
        row = np.zeros(len(self.items))
        for j, o in enumerate(self.items):
            if o.field == L.DG_JUMP:
                u = phi if o.idx < 0 else c_all[o.idx]
                row[j] = o.w[0] * self.jump_host(u, tags[o.sub]) / o.denom
                continue
            u = {L.DG_PHI: phi, L.DG_PHI_M: phi_M}.get(o.field)
            v = (c_all[o.idx] if u is None else u)[o.ids]
            row[j] = np.dot(o.w, v) / o.denom if o.op == L.OBS_SUM else v.min() if o.op == L.OBS_MIN else v.max()
        return row

    def record_host(self, t, c_all, phi, phi_M):
        """Append the row of time t from host arrays."""
        self._append_rows([t], self.evaluate_host(c_all, phi, phi_M)[None, :])


def _closest_on_simplices(X, p):
    """(n, nf) barycentric weights of the point of every segment / triangle X (n, nf, d) closest to p."""
    lam, _ = _simplex_coords(X, p)
    if X.shape[1] == 2:
        t = np.clip(lam[:, 1], 0.0, 1.0)
        return np.stack([1.0 - t, t], axis=1)
    W = lam.copy()
    out = np.flatnonzero(lam.min(axis=1) < 0.0)
    if out.size:                                            # outside the triangle: the closest point lies on an edge
        best = np.full(out.shape[0], np.inf)
        for a, b in ((0, 1), (0, 2), (1, 2)):
            A, B = X[out, a], X[out, b]
            e = B - A
            t = np.clip(np.einsum("nd,nd->n", p[None, :] - A, e) / np.einsum("nd,nd->n", e, e), 0.0, 1.0)
            dist = np.linalg.norm(A + t[:, None] * e - p[None, :], axis=1)
            take = dist < best
            cand = np.zeros((out.shape[0], 3))
            cand[:, a], cand[:, b] = 1.0 - t, t
            W[out[take]] = cand[take]
            best = np.where(take, dist, best)
    return W


class _NodeEvents(MembraneEvents):
    """`MembraneEvents` over the membrane nodes of a DG handle as one watched "cell": the rules, the host restatement and
    the maps are the base class's, the device calls are knpemi_dg_events_*."""
    TAG = "membrane"

    def _attach(self, dp):
        if self._dev is not None:
            raise RuntimeError("these events are attached to a device problem already")
        if not self.watched:
            raise ValueError("no threshold is watched: call watch() before DGProblem.detect")
        if dp.nmf * dp.nf != self.n_q[self.TAG]:
            raise ValueError("these events were defined on another mesh")
        thr, rst = self.watched[self.TAG]
        L.check(dp.lib.knpemi_dg_events_set(dp.h, thr, rst, int(self.keep)))
        self._dev = (dp.lib, dp.h, None)

    def _read_device(self, tag):
        lib, h, _ = self._dev
        n = self.n_q[tag]
        count = np.zeros(n, np.int32)
        out = [np.empty(n) for _ in range(4)]
        ring = np.empty((self.keep, n))
        L.check(lib.knpemi_dg_events_read(h, L.iptr(count), *(L.dptr(a) for a in out), L.dptr(ring)))
        return dict(count=count, t_first=out[0], t_last=out[1], v_peak=out[2], t_peak=out[3], ring=ring)


class DGMembraneEvents:
    """When every membrane node of a DG run fired: upward crossings of a threshold of phi_M, activation times and peaks per
    node (facet f, vertex a), by the rules of knpemi_events_record.  Maps have the shape (nmf, nf); "times" (nmf, nf, keep).

        ev = DGMembraneEvents(mesh, ft, [1]); ev.watch(-20e-3, keep=4); dp.detect(ev)     # ... dp.record(t) ...
        ev.maps()["t_first"]
    """

    def __init__(self, mesh, ft, membrane_tags):
        self.mem_facets, self.mem_tags = membrane_facets(mesh, ft, membrane_tags)
        self.nmf, self.nf = self.mem_facets.shape
        self.XM = np.asarray(mesh.x, np.float64)[self.mem_facets]
        self._ev = _NodeEvents({_NodeEvents.TAG: self.nmf * self.nf})
        self._ev._x[_NodeEvents.TAG] = self.XM.reshape(self.nmf * self.nf, -1)

    def watch(self, threshold, reset=None, keep=0):
        """Upward crossings of `threshold`, re-armed below `reset` (default: the threshold), the latest `keep` crossing
        times kept per node."""
        if self._ev.watched:
            raise ValueError("a threshold is watched already")
        self._ev.watch(_NodeEvents.TAG, threshold, reset, keep)

    def _attach(self, dp):
        self._ev._attach(dp)
        self._ev.reset_host()

    def reset_host(self):
        self._ev.reset_host()

    def record_host(self, t, phi_M):
        """One record at time t from the host array phi_M (nmf, nf): the numpy restatement of the device kernel."""
        self._ev.record_host(t, {_NodeEvents.TAG: np.asarray(phi_M, np.float64).reshape(-1)})

    def locations(self):
        """(nmf, nf, gdim) coordinates of the membrane nodes."""
        return self.XM.copy()

    def maps(self):
        """{"count" int32, "t_first", "t_last", "v_peak", "t_peak" (nmf, nf), "times" (nmf, nf, keep) oldest first and NaN
        padded, "locations" (nmf, nf, gdim)}: the device state of an attached problem (one synchronisation), else the
        state of `record_host`."""
        m = self._ev.maps(_NodeEvents.TAG)
        return {k: v.reshape((self.nmf, self.nf) + v.shape[1:]) for k, v in m.items()}

    def fired(self):
        return self.maps()["count"] > 0

    def firing_rate(self, t_start, t_end):
        """Crossings per unit time of every node in [t_start, t_end] (`MembraneEvents.firing_rate`)."""
        return self._ev.firing_rate(_NodeEvents.TAG, t_start, t_end).reshape(self.nmf, self.nf)

    def conduction_velocity(self, origin):
        """(speed, rms of the residual distances, nodes used): `MembraneEvents.conduction_velocity` over the nodes."""
        return self._ev.conduction_velocity(_NodeEvents.TAG, origin)

    def save(self, path):
        """.npz of `maps()`."""
        np.savez(path, **self.maps())
