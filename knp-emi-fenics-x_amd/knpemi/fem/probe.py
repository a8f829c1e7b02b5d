"""Point location and functional weights on the P1/Q1 sub-meshes (host side of `knpemi.observables`).

The reference's figure scripts evaluate fields at fixed points with `scifem.evaluate_function`
(`examples/idealized_geometries/make_figures.py:24-117`); here a point becomes a short list of
(vertex id, shape-function weight) pairs, so that the value at the point is a sparse dot product with
the nodal array.  Reductions over a sub-domain (integral, nodal mean, average) are dense weight vectors
of the same kind.

Everything is numpy and runs once at set-up.
"""
from __future__ import annotations

import numpy as np

TOL = 1e-10        # how far outside a cell (relative to its size) a point may lie and still count as inside

_G2 = np.array([0.5 - 0.5 / np.sqrt(3.0), 0.5 + 0.5 / np.sqrt(3.0)])       # 2-point Gauss on [0, 1]
_G4X, _G4W = np.polynomial.legendre.leggauss(4)
_G4X, _G4W = 0.5 * (_G4X + 1.0), 0.5 * _G4W                                 # 4-point Gauss on [0, 1]


# -- shape functions -------------------------------------------------------------------------------
def _tensor_shape(xi):
    """Q1 shape functions on [0,1]^d in lexicographic vertex order (bit t of the vertex number = axis t),
    and their derivatives: (n, 2^d), (n, 2^d, d)."""
    xi = np.atleast_2d(xi)
    n, d = xi.shape
    nv = 1 << d
    N = np.ones((n, nv))
    dN = np.ones((n, nv, d))
    for v in range(nv):
        for t in range(d):
            f = xi[:, t] if (v >> t) & 1 else 1.0 - xi[:, t]
            df = 1.0 if (v >> t) & 1 else -1.0
            N[:, v] *= f
            for u in range(d):
                dN[:, v, u] *= df if u == t else f
    return N, dN


def _simplex_coords(X, p):
    """Barycentric coordinates of p in the simplices X (n, d+1, gdim), least squares when d < gdim.
    Returns (lam (n, d+1), distance of p from the simplex's affine hull (n,))."""
    E = X[:, 1:, :] - X[:, :1, :]                      # (n, d, gdim)
    r = p[None, :] - X[:, 0, :]
    G = np.einsum("nig,njg->nij", E, E)
    rhs = np.einsum("nig,ng->ni", E, r)
    mu = np.linalg.solve(G, rhs[..., None])[..., 0]
    lam = np.concatenate([1.0 - mu.sum(axis=1, keepdims=True), mu], axis=1)
    off = r - np.einsum("ni,nig->ng", mu, E)
    return lam, np.linalg.norm(off, axis=1)


def _tensor_coords(X, p, iters=30):
    """Reference coordinates of p in the Q1 cells X (n, 2^d, gdim) by Newton (Gauss-Newton when d < gdim).
    Returns (xi (n, d), distance of p from the mapped cell surface/volume at xi (n,))."""
    n, nv, g = X.shape
    d = int(np.log2(nv))
    xi = np.full((n, d), 0.5)
    for _ in range(iters):
        N, dN = _tensor_shape(xi)
        r = p[None, :] - np.einsum("nv,nvg->ng", N, X)
        J = np.einsum("nvu,nvg->ngu", dN, X)           # (n, gdim, d)
        JtJ = np.einsum("ngu,ngw->nuw", J, J)
        step = np.linalg.solve(JtJ, np.einsum("ngu,ng->nu", J, r)[..., None])[..., 0]
        xi = np.clip(xi + step, -1.0, 2.0)             # keep far-away candidates from running off
        if np.abs(step).max() < 1e-15:
            break
    N, _ = _tensor_shape(xi)
    off = p[None, :] - np.einsum("nv,nvg->ng", N, X)
    return xi, np.linalg.norm(off, axis=1)


def _weights_in(X, p, simplex):
    """(inside slack (n,), shape-function weights (n, nv)): slack >= -TOL means p lies in the element."""
    h = np.ptp(X, axis=1).max(axis=1)                  # size of every element
    if simplex:
        lam, dist = _simplex_coords(X, p)
        slack = np.minimum(lam.min(axis=1), -dist / h)
        return slack, lam
    xi, dist = _tensor_coords(X, p)
    slack = np.minimum(np.minimum(xi, 1.0 - xi).min(axis=1), -dist / h)
    N, _ = _tensor_shape(xi)
    return slack, N


class BucketGrid:
    """Uniform grid of buckets over the bounding boxes of a set of elements (cells or facets): a point's
    candidates are the elements whose padded box overlaps its bucket."""

    def __init__(self, x, cells):
        self.x = np.asarray(x, np.float64)
        self.cells = np.asarray(cells, np.int64)
        X = self.x[self.cells]
        h = np.ptp(X, axis=1).max(axis=1)
        pad = (4 * TOL * np.maximum(h, 1e-300))[:, None]
        lo, hi = X.min(axis=1) - pad, X.max(axis=1) + pad
        self.lo0 = lo.min(axis=0)
        ext = np.maximum(hi.max(axis=0) - self.lo0, 1e-300)
        g = ext.shape[0]
        n = max(1, self.cells.shape[0])
        # buckets about as wide as a typical element along every axis, at most ~4^g buckets per element
        # (membrane facets are flat boxes: their median width along some axis is the padding alone)
        w = np.maximum(np.median(hi - lo, axis=0), ext / (4.0 * n ** (1.0 / g)))
        self.nb = np.maximum(1, np.ceil(ext / w)).astype(np.int64)
        self.w = ext / self.nb
        a = self._idx(lo)
        b = self._idx(hi)
        # every element into each bucket its box overlaps (boxes span few buckets on these meshes)
        span = b - a + 1
        cnt = np.prod(span, axis=1)
        el = np.repeat(np.arange(self.cells.shape[0]), cnt)
        loc = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        keys = np.zeros(el.shape[0], np.int64)
        for t in range(g):
            s = span[el, t]
            keys = keys * self.nb[t] + a[el, t] + loc % s
            loc //= s
        order = np.lexsort((el, keys))
        self.keys, self.el = keys[order], el[order]

    def _idx(self, p):
        return np.clip(np.floor((p - self.lo0) / self.w).astype(np.int64), 0, self.nb - 1)

    def candidates(self, p):
        i = self._idx(np.asarray(p, np.float64))
        key = 0
        for t in range(i.shape[0]):
            key = key * self.nb[t] + i[t]
        a, b = np.searchsorted(self.keys, key), np.searchsorted(self.keys, key, side="right")
        return self.el[a:b]                 # ascending element numbers


def _locate(grid, simplex, p, what, mask=None):
    p = np.asarray(p, np.float64).ravel()
    if p.shape[0] != grid.x.shape[1]:
        raise ValueError(f"point {p.tolist()} has {p.shape[0]} coordinates, the mesh {grid.x.shape[1]}")
    cand = grid.candidates(p)
    if mask is not None:
        cand = cand[mask[cand]]
    if cand.size:
        slack, W = _weights_in(grid.x[grid.cells[cand]], p, simplex)
        ok = np.flatnonzero(slack >= -TOL)
        if ok.size:
            j = ok[0]                        # lowest-index containing element
            return int(cand[j]), W[j]
    raise ValueError(f"point {p.tolist()} is not in {what}")


class Locator:
    """Point location in one (sub-)mesh: `weights(p)` -> (vertex ids, shape-function weights)."""

    def __init__(self, mesh, what="the mesh", cell_mask=None):
        self.mesh = mesh
        self.simplex = mesh.cell_type in ("triangle", "tetrahedron", "interval")
        self.grid = BucketGrid(mesh.x, mesh.cells)
        self.what = what
        self.mask = None if cell_mask is None else np.asarray(cell_mask, bool)    # only these cells may take a point

    def cell(self, p):
        return _locate(self.grid, self.simplex, p, self.what, self.mask)

    def weights(self, p):
        c, w = self.cell(p)
        return self.mesh.cells[c].astype(np.int64), np.asarray(w, np.float64)


def point_weights(sub_mesh, p, tag=None):
    """(sub-mesh vertex ids, weights) of the point p in a sub-domain's sub-mesh; ValueError if p is outside."""
    return Locator(sub_mesh, f"sub-domain {tag}" if tag is not None else "the mesh").weights(p)


def membrane_weights(subdomain_list, tag, p):
    """A point on the membrane of cell `tag`: weights over the vertices of the containing membrane facet,
    as three index sets (ECS sub-mesh ids, the cell's sub-mesh ids, membrane-space Q ids) sharing one weight
    vector -- the vertex matching of `knpemi.device.flatten_problem` (facet_e / facet_i / facet_q)."""
    mem = subdomain_list[tag]["mesh_mem"]
    q, w = Locator(mem, f"the membrane of cell {tag}").weights(p)
    ecs = subdomain_list[0]["mesh_sub"]
    ics = subdomain_list[tag]["mesh_sub"]
    pv = mem.parent_vertices[q]
    e = np.searchsorted(ecs.parent_vertices, pv)
    i = np.searchsorted(ics.parent_vertices, pv)
    return e.astype(np.int64), i.astype(np.int64), q, w


# -- reduction weights -------------------------------------------------------------------------------
def integral_weights(mesh, cell_mask=None):
    """w_j = integral of the j-th P1/Q1 basis function over the mesh (cells, or facets of a membrane
    sub-mesh): sum_j w_j u_j is the exact integral of u.  Simplices: |K| / (d + 1) per vertex; Q1: 2-point
    Gauss per direction on cells (exact: the integrand is of degree <= 3 per variable), 4-point on
    quadrilateral facets (exact on planar ones).  cell_mask: integrate over these cells only (the cells one rank
    of a partitioned run records)."""
    x = np.asarray(mesh.x, np.float64)
    cells = np.asarray(mesh.cells, np.int64)
    if cell_mask is not None:
        cells = cells[np.asarray(cell_mask, bool)]
    X = x[cells]
    nc, nv, g = X.shape
    w = np.zeros(x.shape[0])
    if mesh.cell_type in ("interval", "triangle", "tetrahedron"):
        d = nv - 1
        E = X[:, 1:, :] - X[:, :1, :]
        G = np.einsum("nig,njg->nij", E, E)
        vol = np.sqrt(np.abs(np.linalg.det(G))) / np.prod(np.arange(1, d + 1))
        np.add.at(w, cells.ravel(), np.repeat(vol / nv, nv))
        return w
    d = int(np.log2(nv))
    gx, gw = (_G2, np.array([0.5, 0.5])) if d == g else (_G4X, _G4W)
    pts = np.stack(np.meshgrid(*([gx] * d), indexing="ij"), axis=-1).reshape(-1, d)
    wts = np.prod(np.stack(np.meshgrid(*([gw] * d), indexing="ij"), axis=-1).reshape(-1, d), axis=1)
    N, dN = _tensor_shape(pts)                          # (nq, nv), (nq, nv, d)
    J = np.einsum("qvu,nvg->nqgu", dN, X)               # (nc, nq, g, d)
    if d == g:
        det = np.abs(np.linalg.det(J))
    else:
        det = np.sqrt(np.abs(np.linalg.det(np.einsum("nqgu,nqgw->nquw", J, J))))
    contrib = np.einsum("nq,q,qv->nv", det, wts, N)
    np.add.at(w, cells.ravel(), contrib.ravel())
    return w
