"""Membrane topologies of dense tissue on the smallest grids that hold them, for every cell kind: cells that meet at a corner
or along an edge, one sub-domain made of two bodies pinched together, cells that share facets, a cell cut by the bounding
box, the smallest cell, several membrane tags on one cell, a cellular sub-domain without cells -- and the two contacts whose
shared facets carry a membrane tag, which no ECS cell touches and which the set-up must refuse.

`build(kind, case, jittered)` returns (mesh, ct, ft) as the idealized mesh functions do: cell tag 0 = ECS, facet tag of a
membrane = the cell tag on its inner side (knpemi.fem.idealized._tag), 5 = exterior, 0 = every other facet.  Grids have 1 um
spacing; 2-D grids use the first two entries of every triple below.  Plain numpy, seeded."""
import functools

import numpy as np

from knpemi.fem import Mesh, MeshTags, create_box, create_rectangle, match_facets
from knpemi.fem.idealized import _tag
from knpemi.fem.mesh import find_interface

H = 1e-6
JITTER = 0.1          # of the grid spacing
SEED = 23
KINDS = ("triangle", "quadrilateral", "tetrahedron", "hexahedron")
# case -> (n, [((lo, hi), cell tag)]) in grid units
_E1, _E2 = ((1, 1, 1), (2, 2, 2)), ((2, 2, 1), (3, 3, 2))
_F1, _F2 = ((1, 1, 1), (3, 3, 2)), ((3, 1, 1), (5, 3, 2))
_B1 = ((0, 1, 1), (3, 3, 2))
CASES = {"edge_touch": ((5, 5, 3), [(_E1, 1), (_E2, 2)]),
         "pinch": ((5, 5, 3), [(_E1, 1), (_E2, 1)]),
         "face_contact": ((6, 4, 3), [(_F1, 1), (_F2, 2)]),
         "to_boundary": ((5, 4, 3), [(_B1, 1)]),
         "one_cell": ((3, 3, 3), [(((1, 1, 1), (2, 2, 2)), 1)]),
         "tags": ((5, 4, 3), [(_B1, 1)]),
         "empty": ((3, 3, 3), [])}
# case -> {cell tag: [(facet tag, membrane model or None)]}: what tests/topology_cases.problem binds
SPECS = {"edge_touch": {1: [(1, "hh_si")], 2: [(2, "glial")]},
         "pinch": {1: [(1, "hh_si")]},
         "face_contact": {1: [(1, "hh_si")], 2: [(2, "glial")]},
         "to_boundary": {1: [(1, "hh_si")]},
         "one_cell": {1: [(1, "hh_si")]},
         "tags": {1: [(1, "hh_si"), (6, "hh_si"), (7, None)]},
         "empty": {1: [(1, "hh_si")]}}
# the probe of the acceptance bug: both on the n = (6, 4, 3) grid, cells tagged 1 and 2, contact facets tagged 1
CONTACTS = {"single": [(((1, 1, 1), (2, 2, 2)), 1), (((2, 1, 1), (3, 2, 2)), 2)],
            "wide": [(((1, 1, 1), (3, 3, 2)), 1), (((3, 1, 1), (5, 3, 2)), 2)]}
CONTACT_N = (6, 4, 3)
CONTACT_SPEC = {1: [(1, "hh_si")], 2: [(2, "glial")]}


def _grid(kind, n):
    dim = 2 if kind in ("triangle", "quadrilateral") else 3
    n = tuple(n[:dim])
    lo, hi = np.zeros(dim), H * np.array(n, float)
    mesh = create_rectangle(None, [lo, hi], n, kind) if dim == 2 else create_box(None, [lo, hi], n, kind)
    return mesh, dim


def _tagged(kind, n, boxes):
    mesh, dim = _grid(kind, n)
    ct, ft = _tag(mesh, [(H * np.array(lo[:dim], float), H * np.array(hi[:dim], float)) for (lo, hi), _ in boxes],
                  [t for _, t in boxes])
    return mesh, ct, ft


def _retag_thirds(mesh, ft):
    """Membrane facets (tag 1) re-tagged 1, 6, 7 by the x coordinate of their midpoint, in thirds of their extent."""
    vals = ft.values.copy()
    mem = np.flatnonzero(vals == 1)
    xm = mesh.x[mesh.facets[ft.indices[mem]]].mean(axis=1)[:, 0]
    a, b = xm.min(), xm.max()
    vals[mem[xm > a + (b - a) / 3.0]] = 6
    vals[mem[xm > a + 2.0 * (b - a) / 3.0]] = 7
    return MeshTags(mesh, mesh.tdim - 1, ft.indices.copy(), vals)


def jitter(mesh_data, seed=SEED):
    """The same topology and tags with every vertex off the exterior boundary moved by at most JITTER of the spacing.
    `uniform_cell` stays attached as the generators attach it: the coordinates no longer bear it out."""
    mesh, ct, ft = mesh_data
    lo, hi = mesh.x.min(axis=0), mesh.x.max(axis=0)
    inner = np.all((mesh.x > lo + 0.5 * H) & (mesh.x < hi - 0.5 * H), axis=1)
    rng = np.random.default_rng(seed)
    x = mesh.x.copy()
    x[inner] += JITTER * H * (2.0 * rng.random((int(inner.sum()), mesh.gdim)) - 1.0)
    m2 = Mesh(x, mesh.cells.copy(), mesh.cell_type)
    if getattr(mesh, "uniform_cell", None) is not None:
        m2.uniform_cell = mesh.uniform_cell
    assert np.array_equal(m2.facets, mesh.facets)             # the facet numbering depends on the cells alone
    return (m2, MeshTags(m2, m2.tdim, ct.indices.copy(), ct.values.copy()),
            MeshTags(m2, m2.tdim - 1, ft.indices.copy(), ft.values.copy()))


@functools.lru_cache(maxsize=None)
def build(kind, case, jittered=False):
    n, boxes = CASES[case]
    data = _tagged(kind, n, boxes)
    if case == "tags":
        data = (data[0], data[1], _retag_thirds(data[0], data[2]))
    return jitter(data) if jittered else data


@functools.lru_cache(maxsize=None)
def contact(kind, which, tagged=True, jittered=False):
    """Two cells sharing facets.  tagged: the shared facets carry membrane tag 1 (no ECS cell touches them)."""
    mesh, ct, ft = _tagged(kind, CONTACT_N, CONTACTS[which])
    if tagged:
        vals = ft.dense(fill=0)
        shared = find_interface(ct, 1, 2)
        assert len(shared) > 0
        vals[shared] = 1
        ft = MeshTags(mesh, mesh.tdim - 1, np.arange(mesh.num_facets, dtype=np.int32), vals)
    return jitter((mesh, ct, ft)) if jittered else (mesh, ct, ft)


def contact_facets(mesh_data):
    """Parent facets between a cell tagged 1 and a cell tagged 2."""
    return find_interface(mesh_data[1], 1, 2)


# new local vertex j of a cell takes old local vertex _TURN[kind][j]: simplices rotate their vertex list by one (as
# unstructured_meshes.rotated does); a rolled list is no tensor order, so quadrilaterals make a quarter turn and hexahedra
# permute their axes cyclically -- the symmetries of order 4 and 3 that play the same part
_TURN = {"triangle": [2, 0, 1], "tetrahedron": [3, 0, 1, 2], "quadrilateral": [1, 3, 0, 2],
         "hexahedron": [((j & 1) << 1) | ((j & 2) << 1) | ((j & 4) >> 2) for j in range(8)]}


def rotated(mesh_data):
    """The same mesh with every cell described from its next vertex on: the same operator, summed in another order."""
    mesh, ct, ft = mesh_data
    m2 = Mesh(mesh.x.copy(), mesh.cells[:, _TURN[mesh.cell_type]], mesh.cell_type)

    class _V:
        sub_to_parent = np.arange(mesh.num_vertices)
    pf = match_facets(mesh, m2, _V)
    assert (pf >= 0).all()
    return (m2, MeshTags(m2, m2.tdim, ct.indices.copy(), ct.values.copy()),
            MeshTags(m2, m2.tdim - 1, np.arange(m2.num_facets, dtype=np.int32), ft.dense(fill=0)[pf]))
