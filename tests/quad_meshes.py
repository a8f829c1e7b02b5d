"""Quadrilateral meshes for the Q1 kernels in 2-D, in the style of tests/hex_meshes.py: the 62 x 4 um rectangle of
make_mesh_2D on squares -- plain, sheared (parallelograms with a full metric), jittered (general bilinear cells), stretched
(4 : 1 cells) -- the star meshes with one vertex shared by n quadrilaterals (a structured mesh has 4), and `reorient`: every
cell in its own one of the 8 tensor orders of the square (half of them left-handed), vertex numbers and cell order shuffled.
Every function returns (mesh, ct, ft) as the idealized mesh functions do: cell tag 0 = ECS, 1 = ICS, facet tag
1 = membrane, 5 = exterior.  Plain numpy, seeded."""
import functools
import itertools

import numpy as np

from hex_meshes import L_BOX, tag_cells
from knpemi.fem import Mesh, MeshTags, make_mesh_2D, match_facets

SHEAR = 0.4          # x += SHEAR * y
JITTER = 0.15        # of the grid spacing h = 1 um / 2^r
STRETCH = 0.25       # y scaled by this: cells 4 : 1


def _symmetries():
    """(pi, s, g) for the 8 tensor-order symmetries of the square: axis permutation pi, flips s in {0,1}^2; new local
    vertex j takes old local vertex g[j], where bit pi[a] of g[j] is (bit a of j) XOR s[a]."""
    out = []
    for pi in itertools.permutations(range(2)):
        for s in itertools.product((0, 1), repeat=2):
            g = [sum((((j >> a) & 1) ^ s[a]) << pi[a] for a in range(2)) for j in range(4)]
            out.append((pi, s, np.array(g, np.int64)))
    return out


SYMMETRIES = _symmetries()
IDENTITY = next(k for k, (pi, s, g) in enumerate(SYMMETRIES) if pi == (0, 1) and s == (0, 0))
MIRROR = next(k for k, (pi, s, g) in enumerate(SYMMETRIES) if pi == (0, 1) and s == (1, 0))


def symmetry_is_left_handed(k):
    pi, s, _ = SYMMETRIES[k]
    return bool((int(pi[0] > pi[1]) + sum(s)) & 1)


def corner_determinants(x, cells):
    """(n_cells, 4): the Jacobian determinant of the bilinear map at each corner (edge vectors along the two local axes,
    oriented towards increasing reference coordinate).  One sign on all four corners: a valid tensor-order quadrilateral
    (negative: left-handed); mixed signs: folded (a cell in counter-clockwise order) or not convex."""
    det = np.empty((cells.shape[0], 4))
    for j in range(4):
        e = np.stack([(1.0 - 2.0 * ((j >> a) & 1)) * (x[cells[:, j ^ (1 << a)]] - x[cells[:, j]]) for a in range(2)], axis=1)
        det[:, j] = np.linalg.det(e)
    return det


def left_handed_fraction(mesh):
    return float((corner_determinants(mesh.x, mesh.cells)[:, 0] < 0).mean())


def reorient(mesh_data, seed, per_cell=True, shuffle=True, symmetry=None):
    """The same quadrilateral mesh in another description.  per_cell: one symmetry drawn per cell; symmetry=k: SYMMETRIES[k]
    on every cell.  shuffle: vertex numbers and cell order permuted.  Facet tags are carried over with match_facets, cell
    tags through the cell permutation.  Returns ((mesh, ct, ft), (vperm, cperm, G)): vperm[v] is the new number of old
    vertex v, new cell i is old cell cperm[i], and its local vertex j is old local vertex G[i, j] of that cell."""
    m0, ct0, ft0 = mesh_data
    rng = np.random.default_rng(seed)
    nc, nvert = m0.num_cells, m0.num_vertices
    if symmetry is not None:
        which = np.full(nc, symmetry)
    elif per_cell:
        which = rng.integers(0, len(SYMMETRIES), nc)
    else:
        which = np.full(nc, IDENTITY)
    vperm = rng.permutation(nvert) if shuffle else np.arange(nvert)
    cperm = rng.permutation(nc) if shuffle else np.arange(nc)
    G = np.stack([SYMMETRIES[k][2] for k in which])
    x = np.empty_like(m0.x)
    x[vperm] = m0.x
    cells = vperm[np.take_along_axis(m0.cells[cperm].astype(np.int64), G, axis=1)].astype(np.int32)
    mesh = Mesh(x, cells, m0.cell_type)
    ct = MeshTags(mesh, mesh.tdim, np.arange(nc, dtype=np.int32), ct0.dense()[cperm])

    class _V:                                  # sub_to_parent of the identity "sub-mesh" mesh -> m0 vertex ids
        sub_to_parent = np.argsort(vperm)
    pf = match_facets(m0, mesh, _V)
    assert (pf >= 0).all()
    ft = MeshTags(mesh, mesh.tdim - 1, np.arange(mesh.num_facets, dtype=np.int32), ft0.dense(fill=0)[pf])
    return (mesh, ct, ft), (vperm, cperm, G)


@functools.lru_cache(maxsize=None)
def rect(r):
    return make_mesh_2D(r, cell_type="quadrilateral")


def _moved(r, f):
    """rect(r) with the coordinates replaced by f(x): the same topology and tags on a fresh mesh."""
    m0, ct0, ft0 = rect(r)
    mesh = Mesh(f(m0.x.copy()), m0.cells.copy(), m0.cell_type)
    ct = MeshTags(mesh, mesh.tdim, ct0.indices.copy(), ct0.values.copy())
    ft = MeshTags(mesh, mesh.tdim - 1, ft0.indices.copy(), ft0.values.copy())
    return mesh, ct, ft


@functools.lru_cache(maxsize=None)
def sheared(r):
    def f(x):
        x[:, 0] += SHEAR * x[:, 1]
        return x
    return _moved(r, f)


@functools.lru_cache(maxsize=None)
def jittered(r, seed=3):
    h = 1e-6 / 2 ** r
    rng = np.random.default_rng(seed)
    return _moved(r, lambda x: x + JITTER * h * (2.0 * rng.random(x.shape) - 1.0))


@functools.lru_cache(maxsize=None)
def stretched(r):
    return _moved(r, lambda x: x * np.array([1.0, STRETCH]))


@functools.lru_cache(maxsize=None)
def star_quad(n, k):
    """The 2-D base of hex_meshes.star_hex_base without the extrusion: a regular n-gon cut into n quadrilateral sectors
    (sector i: centre, midpoint of edge i-1, midpoint of edge i, corner i), each split k x k by its bilinear map,
    duplicate points merged; circumradius L_BOX / 2.  The centre is shared by n cells.  ICS: sectors 0 and 1, so the
    irregular vertex lies on the membrane.  Cells in tensor order, right-handed, numbered sector by sector."""
    ang = 2.0 * np.pi * np.arange(n) / n
    corner = np.c_[np.cos(ang), np.sin(ang)]
    mid = 0.5 * (corner + np.roll(corner, -1, axis=0))
    pts, index, quads, sector = [], {}, [], []

    def point(p):
        key = (int(round(p[0] * 1e9)), int(round(p[1] * 1e9)))
        if key not in index:
            index[key] = len(pts)
            pts.append(p)
        return index[key]
    for i in range(n):
        p00, p10, p01, p11 = np.zeros(2), mid[i - 1], mid[i], corner[i]
        ids = np.empty((k + 1, k + 1), np.int64)
        for b in range(k + 1):
            for a in range(k + 1):
                u, v = a / k, b / k
                ids[b, a] = point((1 - u) * (1 - v) * p00 + u * (1 - v) * p10 + (1 - u) * v * p01 + u * v * p11)
        for b in range(k):
            for a in range(k):
                quads.append([ids[b, a], ids[b, a + 1], ids[b + 1, a], ids[b + 1, a + 1]])
                sector.append(i)
    mesh = Mesh(np.array(pts) * 0.5 * L_BOX, np.array(quads, np.int32), "quadrilateral")
    return (mesh,) + tag_cells(mesh, np.array(sector) <= 1)


# ---- moving fields between the two descriptions (continuous spaces): hex_meshes.cg_dof_maps / transfer_cg_fields work on
# any cell kind; re-exported here so that a test of the quadrilaterals imports one module
from hex_meshes import cg_dof_maps, transfer_cg_fields  # noqa: E402,F401
