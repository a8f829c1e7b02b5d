"""Simplex meshes that are NOT Kuhn-split boxes: Delaunay triangulations with high-valence "fan" vertices and shuffled
numbering (committed as tests/golden/unstructured_{2d,3d}.npz, written by tests/golden/make_unstructured.py), the
tetrahedral box with jittered vertices and shuffled numbering, and a two-cell sliver.  Every function returns
(mesh, ct, ft) as the idealized mesh functions do: cell tag 0 = ECS, 1 = ICS, facet tag 1 = membrane, 5 = exterior."""
import os

import numpy as np

from knpemi.fem import Mesh, MeshTags, make_mesh_3D, match_facets, meshtags
from knpemi.fem.mesh import exterior_facet_indices, find_interface

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
L_BOX = 60e-6     # edge of the fan meshes' box
SEED = 11
# interior boxes of sub-domain 1, in units of the box edge (cells are tagged by centroid).  2D: the square of the recipe
# has 19 membrane vertices; the two strips lengthen the interface (figures: tests/test_unstructured_host.py).
ICS_BOXES = {3: [([0.25, 0.25, 0.25], [0.75, 0.75, 0.75])],
             2: [([0.25, 0.25], [0.75, 0.75]), ([0.8125, 0.0625], [0.9375, 0.9375]), ([0.25, 0.8125], [0.75, 0.9375])]}
# fan centres (grid points, in units of the box edge) and the number of points around each
FANS = {3: [((0.5, 0.5, 0.5), 40), ((0.25, 0.5, 0.5), 36), ((0.5, 0.5, 0.25), 36)],
        2: [((0.5, 0.5), 36), ((0.25, 0.5), 34), ((0.125, 0.5), 34)]}


def shuffle_numbering(x, cells, rng):
    """Permute the vertex numbers, the cell order and the vertex order inside every cell (about half the cells become
    left-handed).  Returns (x, cells, vperm, cperm): vperm[v] is the new number of old vertex v, new cell i is old cell
    cperm[i]."""
    vperm = rng.permutation(x.shape[0])
    cperm = rng.permutation(cells.shape[0])
    xs = np.empty_like(x)
    xs[vperm] = x
    cs = vperm[cells][cperm]
    order = rng.permuted(np.tile(np.arange(cells.shape[1]), (cells.shape[0], 1)), axis=1)
    return xs, np.take_along_axis(cs, order, axis=1).astype(np.int32), vperm, cperm


def build_fan_points_and_cells(dim, seed=SEED):
    """The recipe of the committed files (needs scipy.spatial.Delaunay, i.e. qhull: run by make_unstructured.py only).
    Grid points of an M-per-edge unit box (M = 8 in 2D, 4 in 3D), every one moved by up to +-20 % of the spacing; fan
    points on a circle / Fibonacci sphere of radius 0.3 spacings around three of the moved grid points; Delaunay; the
    three shuffles; scaled by L_BOX."""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    M = 8 if dim == 2 else 4
    h = 1.0 / M
    axes = [np.arange(M + 1) * h] * dim
    grid = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, dim)
    pts = grid + 0.2 * h * (2.0 * rng.random(grid.shape) - 1.0)
    extra = []
    for centre, n in FANS[dim]:
        c = pts[np.argmin(np.abs(grid - np.array(centre)).sum(axis=1))]
        if dim == 2:
            ang = 2.0 * np.pi * (np.arange(n) + 0.5) / n
            dirs = np.c_[np.cos(ang), np.sin(ang)]
        else:
            k = np.arange(n) + 0.5
            z = 1.0 - 2.0 * k / n
            ang = np.pi * (1.0 + 5.0 ** 0.5) * k
            dirs = np.c_[np.sqrt(1.0 - z * z) * np.cos(ang), np.sqrt(1.0 - z * z) * np.sin(ang), z]
        extra.append(c + 0.3 * h * dirs)
    pts = np.vstack([pts] + extra)
    cells = Delaunay(pts).simplices
    x, cells, _, _ = shuffle_numbering(pts, cells, rng)
    return x * L_BOX, cells


def tag_by_centroid(mesh, boxes):
    """Cell tag 1 where the centroid lies in one of `boxes`, facet tags as knpemi.fem.idealized._tag sets them."""
    cent = mesh.x[mesh.cells].mean(axis=1)
    marker = np.zeros(mesh.num_cells, np.int32)
    for lo, hi in boxes:
        marker[np.all((cent >= np.asarray(lo)) & (cent <= np.asarray(hi)), axis=1)] = 1
    ct = meshtags(mesh, mesh.tdim, np.arange(mesh.num_cells, dtype=np.int32), marker)
    fmark = np.zeros(mesh.num_facets, np.int32)
    fmark[find_interface(ct, 1, 0)] = 1
    fmark[exterior_facet_indices(mesh)] = 5
    ft = meshtags(mesh, mesh.tdim - 1, np.arange(mesh.num_facets, dtype=np.int32), fmark)
    return ct, ft


def fan_mesh_from_arrays(x, cells):
    dim = x.shape[1]
    mesh = Mesh(x, cells, "triangle" if dim == 2 else "tetrahedron")
    boxes = [(np.array(lo) * L_BOX, np.array(hi) * L_BOX) for lo, hi in ICS_BOXES[dim]]
    return (mesh,) + tag_by_centroid(mesh, boxes)


def fan_mesh(dim):
    """The committed fan mesh (x, cells from tests/golden/unstructured_{2d,3d}.npz) with its tags."""
    g = np.load(os.path.join(GOLDEN, f"unstructured_{dim}d.npz"))
    return fan_mesh_from_arrays(g["x"].copy(), g["cells"].copy())


def jittered_tet_box(seed=5, r=0, l=2, jitter=0.2):
    """make_mesh_3D(r, "tetrahedron", l) with every vertex moved by up to `jitter` of the smallest spacing and the three
    shuffles applied; tags carried over by matching cells and facets.  `uniform_cell` stays attached on purpose: the
    coordinates no longer bear it out and knpemi_create must notice."""
    m0, ct0, ft0 = make_mesh_3D(r, "tetrahedron", l=l)
    rng = np.random.default_rng(seed)
    hmin = np.abs(np.diag(m0.uniform_cell)).min()
    x0 = m0.x + jitter * hmin * (2.0 * rng.random(m0.x.shape) - 1.0)
    x, cells, vperm, cperm = shuffle_numbering(x0, m0.cells, rng)
    mesh = Mesh(x, cells, m0.cell_type)
    mesh.uniform_cell = m0.uniform_cell
    ct = MeshTags(mesh, mesh.tdim, np.arange(mesh.num_cells, dtype=np.int32), ct0.dense()[cperm])

    class _V:                                  # sub_to_parent of the identity "sub-mesh" mesh -> m0 vertex ids
        sub_to_parent = np.argsort(vperm)
    pf = match_facets(m0, mesh, _V)
    assert (pf >= 0).all()
    ft = MeshTags(mesh, mesh.tdim - 1, np.arange(mesh.num_facets, dtype=np.int32), ft0.dense(fill=0)[pf])
    return mesh, ct, ft


def sliver_mesh(height):
    """Two tetrahedra on one triangle of edge ~1 um: the ECS cell above, the intracellular cell below, apexes at
    +-height um (height = 1: well shaped, 1e-3: aspect 1 : 1000).  Vertex order chosen so that one cell is left-handed."""
    x = 1e-6 * np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.0], [0.37, 0.31, height], [0.43, 0.29, -height]])
    cells = np.array([[0, 1, 2, 3], [2, 4, 0, 1]], np.int32)
    mesh = Mesh(x, cells, "tetrahedron")
    ct = meshtags(mesh, 3, np.arange(2, dtype=np.int32), np.array([0, 1], np.int32))
    fmark = np.zeros(mesh.num_facets, np.int32)
    fmark[find_interface(ct, 1, 0)] = 1
    fmark[exterior_facet_indices(mesh)] = 5
    ft = meshtags(mesh, 2, np.arange(mesh.num_facets, dtype=np.int32), fmark)
    return mesh, ct, ft


def rotated(mesh_data):
    """The same mesh with every cell's vertex list rotated by one: the same operator, summed in another order."""
    mesh, ct, ft = mesh_data
    m2 = Mesh(mesh.x.copy(), np.roll(mesh.cells, 1, axis=1), mesh.cell_type)
    ct2 = meshtags(m2, m2.tdim, ct.indices, ct.values)

    class _V:
        sub_to_parent = np.arange(mesh.num_vertices)
    pf = match_facets(mesh, m2, _V)
    assert (pf >= 0).all()
    ft2 = MeshTags(m2, m2.tdim - 1, np.arange(m2.num_facets, dtype=np.int32), ft.dense(fill=0)[pf])
    return m2, ct2, ft2


def left_handed_fraction(mesh):
    e = mesh.x[mesh.cells[:, 1:]] - mesh.x[mesh.cells[:, :1]]
    return float((np.linalg.det(e) < 0).mean())


def mesh_statistics(mesh_data):
    """Figures of the layout knpemi_create builds from a two-sub-domain mesh, computed on the host: row lengths of the
    EMI pattern (sub-mesh Laplacian pattern plus, on membrane rows, the vertices of the other side's membrane facets),
    cells per sub-mesh vertex, membrane facets per membrane vertex."""
    mesh, ct, ft = mesh_data
    dense = ct.dense()
    mem = mesh.facets[ft.indices[ft.values == 1]]
    mem_v = np.unique(mem)
    out = dict(vertices=mesh.num_vertices, cells=mesh.num_cells, membrane_facets=len(mem), membrane_vertices=len(mem_v),
               left_handed=left_handed_fraction(mesh))
    facets_at = np.bincount(mem.ravel(), minlength=mesh.num_vertices)
    out["membrane_vertices_with_5_facets"] = int((facets_at >= 5).sum())
    rows, valence = {}, 0
    for t in (0, 1):
        cells = mesh.cells[dense == t]
        nb = [set() for _ in range(mesh.num_vertices)]
        for c in cells:
            for v in c:
                nb[v].update(int(w) for w in c)
        valence = max(valence, int(np.bincount(cells.ravel(), minlength=mesh.num_vertices).max()))
        rows[t] = nb
    for f in mem:                       # membrane coupling: a facet's rows on one side see its vertices on the other
        for v in f:
            for t in (0, 1):
                rows[t][v].update(-1 - int(w) for w in f)
    length = {t: np.array([len(s) for s in rows[t]]) for t in (0, 1)}
    on_mem = np.zeros(mesh.num_vertices, bool)
    on_mem[mem_v] = True
    out["longest_row"] = int(max(length[0].max(), length[1].max()))
    out["longest_ecs_row"] = int(length[0][~on_mem].max())
    out["longest_ics_row"] = int(length[1][~on_mem].max()) if (length[1][~on_mem] > 0).any() else 0
    out["longest_membrane_row"] = int(max(length[0][on_mem].max(), length[1][on_mem].max()))
    out["rows_over_31"] = int((length[0] > 31).sum() + (length[1] > 31).sum())
    out["most_cells_at_a_submesh_vertex"] = valence
    e = mesh.x[mesh.cells[:, 1:]] - mesh.x[mesh.cells[:, :1]]
    vol = np.abs(np.linalg.det(e))
    i, j = np.triu_indices(mesh.cells.shape[1], 1)
    edge = np.linalg.norm(mesh.x[mesh.cells[:, i]] - mesh.x[mesh.cells[:, j]], axis=2).max(axis=1)
    q = vol / edge ** mesh.tdim
    out["quality_ratio"] = float(q.min() / q.max())
    return out


NAMES = ("A_emi", "P_emi", "b_emi", "A_knp", "b_knp")


def oracle_objects(mesh_data, splitting=True):
    """The five assembled objects of the oracle on `mesh_data` with the seeded fields of Setup.perturb()."""
    import contextlib
    import io
    import knpemi_oracle as o
    from helpers import Setup
    with contextlib.redirect_stdout(io.StringIO()):
        s = Setup("tet", 0, mesh_data=mesh_data, build_forms=False)
    s.perturb()
    _, P, params, ions = s.oracle()
    c_all, phi, phiM, mm = s.oracle_fields()
    A, Pm, b = o.assemble_emi(P, params, ions, c_all, phiM, mm, splitting_scheme=splitting)
    Ak, bk = o.assemble_knp(P, params, ions, c_all, phi, phiM, mm, s.dt, splitting_scheme=splitting)
    return s, dict(zip(NAMES, (A, Pm, b, Ak, bk)))


def rounding_sensitivity(mesh_data):
    """Largest relative difference, over the five objects, between the oracle on the mesh and on the same mesh with every
    cell's vertex list rotated by one: the same operator with its sums taken in another order."""
    from helpers import csr_rel_err, rel_err
    _, a = oracle_objects(mesh_data)
    _, b = oracle_objects(rotated(mesh_data))
    return {k: (rel_err(a[k], b[k]) if isinstance(a[k], np.ndarray) else csr_rel_err(a[k].tocsr(), b[k].tocsr()))
            for k in NAMES}
