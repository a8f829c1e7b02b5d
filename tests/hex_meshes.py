"""Hexahedral meshes that are NOT what create_box numbers: the r = 0 box of make_mesh_3D with every cell's local vertex
order replaced by one of the 48 tensor-order symmetries of the cube (half of them left-handed), vertex numbers and cell
order shuffled -- plain, jittered, sheared, and under ONE global symmetry -- and `star_hex`, an extruded n-gon cut into
n sectors whose axis is an edge shared by n hexahedra (n = 3: valence 3, n = 7: valence 7; a structured mesh has 4).
Every function returns (mesh, ct, ft) as the idealized mesh functions do: cell tag 0 = ECS, 1 = ICS, facet tag
1 = membrane, 5 = exterior.  Plain numpy, seeded."""
import functools
import itertools

import numpy as np

from knpemi.fem import Mesh, MeshTags, make_mesh_3D, match_facets, meshtags
from knpemi.fem.mesh import exterior_facet_indices, find_interface

L_BOX = 60e-6        # extent of the star meshes (the edge of the fan meshes' box, tests/unstructured_meshes.py)
SHEAR = np.array([[1.0, 0.8, -0.5], [0.02, 1.0, 0.3], [-0.01, 0.25, 1.0]])   # test_assembly_matches_oracle_on_sheared_hexahedra
JITTER = 0.15        # of the smallest grid spacing of the r = 0 box (0.1 um)


def _symmetries():
    """(pi, s, g) for the 48 tensor-order symmetries: axis permutation pi, flips s in {0,1}^3; new local vertex j takes
    old local vertex g[j], where bit pi[a] of g[j] is (bit a of j) XOR s[a]."""
    out = []
    for pi in itertools.permutations(range(3)):
        for s in itertools.product((0, 1), repeat=3):
            g = [sum((((j >> a) & 1) ^ s[a]) << pi[a] for a in range(3)) for j in range(8)]
            out.append((pi, s, np.array(g, np.int64)))
    return out


SYMMETRIES = _symmetries()
IDENTITY = next(k for k, (pi, s, g) in enumerate(SYMMETRIES) if pi == (0, 1, 2) and s == (0, 0, 0))
MIRROR = next(k for k, (pi, s, g) in enumerate(SYMMETRIES) if pi == (0, 1, 2) and s == (1, 0, 0))
CYCLIC = next(k for k, (pi, s, g) in enumerate(SYMMETRIES) if pi == (1, 2, 0) and s == (0, 0, 0))


def symmetry_is_left_handed(k):
    pi, s, _ = SYMMETRIES[k]
    inversions = sum(pi[a] > pi[b] for a in range(3) for b in range(a + 1, 3))
    return bool((inversions + sum(s)) & 1)


def corner_determinants(x, cells):
    """(n_cells, 8): the Jacobian determinant of the trilinear map at each corner (edge vectors along the three local
    axes, oriented towards increasing reference coordinate).  One sign on all eight corners: a valid tensor-order
    hexahedron (negative: left-handed); mixed signs: folded, e.g. a cell given in counter-clockwise (VTK) order."""
    det = np.empty((cells.shape[0], 8))
    for j in range(8):
        e = np.stack([(1.0 - 2.0 * ((j >> a) & 1)) * (x[cells[:, j ^ (1 << a)]] - x[cells[:, j]]) for a in range(3)], axis=1)
        det[:, j] = np.linalg.det(e)
    return det


def left_handed_fraction(mesh):
    return float((corner_determinants(mesh.x, mesh.cells)[:, 0] < 0).mean())


def reorient(mesh_data, seed, per_cell=True, shuffle=True, symmetry=None):
    """The same hexahedral mesh in another description.  per_cell: one symmetry drawn per cell; symmetry=k: SYMMETRIES[k]
    on every cell.  shuffle: vertex numbers and cell order permuted.  Facet tags are carried over with match_facets, cell
    tags through the cell permutation (as unstructured_meshes.jittered_tet_box does); a `uniform_cell` attribute stays
    attached on purpose.  Returns ((mesh, ct, ft), (vperm, cperm, G)): vperm[v] is the new number of old vertex v, new
    cell i is old cell cperm[i], and its local vertex j is old local vertex G[i, j] of that cell."""
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
    if getattr(m0, "uniform_cell", None) is not None:
        mesh.uniform_cell = m0.uniform_cell
    ct = MeshTags(mesh, mesh.tdim, np.arange(nc, dtype=np.int32), ct0.dense()[cperm])

    class _V:                                  # sub_to_parent of the identity "sub-mesh" mesh -> m0 vertex ids
        sub_to_parent = np.argsort(vperm)
    pf = match_facets(m0, mesh, _V)
    assert (pf >= 0).all()
    ft = MeshTags(mesh, mesh.tdim - 1, np.arange(mesh.num_facets, dtype=np.int32), ft0.dense(fill=0)[pf])
    return (mesh, ct, ft), (vperm, cperm, G)


def tag_cells(mesh, marker):
    """Cell tags from `marker`, facet tags as knpemi.fem.idealized._tag sets them."""
    ct = meshtags(mesh, mesh.tdim, np.arange(mesh.num_cells, dtype=np.int32), marker.astype(np.int32))
    fmark = np.zeros(mesh.num_facets, np.int32)
    fmark[find_interface(ct, 1, 0)] = 1
    fmark[exterior_facet_indices(mesh)] = 5
    ft = meshtags(mesh, mesh.tdim - 1, np.arange(mesh.num_facets, dtype=np.int32), fmark)
    return ct, ft


def star_hex_base(n, k, nz):
    """A regular n-gon cut into n quadrilateral sectors (sector i: centre, midpoint of edge i-1, midpoint of edge i,
    corner i), each split k x k by its bilinear map, duplicate points merged, extruded into nz layers; circumradius
    L_BOX / 2, height L_BOX.  The axis is an edge shared by n hexahedra.  ICS: sectors 0 and 1 in layers 1 .. nz-2, so
    the irregular edge lies on the membrane.  Cells in tensor order, right-handed, numbered sector by sector."""
    ang = 2.0 * np.pi * np.arange(n) / n
    corner = np.c_[np.cos(ang), np.sin(ang)]
    mid = 0.5 * (corner + np.roll(corner, -1, axis=0))          # mid[i]: midpoint of edge i = (corner i, corner i+1)
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
    pts, quads, sector = np.array(pts), np.array(quads), np.array(sector)
    n2 = len(pts)
    x = np.concatenate([np.c_[pts * 0.5 * L_BOX, np.full(n2, L_BOX * z / nz)] for z in range(nz + 1)])
    cells = np.concatenate([np.c_[quads + z * n2, quads + (z + 1) * n2] for z in range(nz)]).astype(np.int32)
    layer = np.repeat(np.arange(nz), len(quads))
    mesh = Mesh(x, cells, "hexahedron")
    ics = (np.tile(sector, nz) <= 1) & (layer >= 1) & (layer <= nz - 2)
    return (mesh,) + tag_cells(mesh, ics)


def star_hex(n, k, nz, seed=23):
    """star_hex_base re-oriented per cell and shuffled.  Returns what `reorient` returns."""
    return reorient(star_hex_base(n, k, nz), seed)


def _box(kind):
    mesh, ct, ft = make_mesh_3D(0, "hexahedron")
    if kind == "jittered":
        rng = np.random.default_rng(3)
        hmin = np.abs(np.diag(mesh.uniform_cell)).min()
        mesh.x[:] = mesh.x + JITTER * hmin * (2.0 * rng.random(mesh.x.shape) - 1.0)
    elif kind == "sheared":
        mesh.x[:] = mesh.x @ SHEAR.T
    return mesh, ct, ft


_VARIANTS = {
    "reoriented_box": lambda: (_box("box"), dict(seed=31)),
    "reoriented_jittered": lambda: (_box("jittered"), dict(seed=32)),
    "reoriented_sheared": lambda: (_box("sheared"), dict(seed=33)),
    "global_mirror": lambda: (_box("box"), dict(seed=34, symmetry=MIRROR)),
    "global_permuted": lambda: (_box("box"), dict(seed=35, symmetry=CYCLIC)),
    "star3": lambda: (star_hex_base(3, 2, 3), dict(seed=36)),
    "star7": lambda: (star_hex_base(7, 3, 4), dict(seed=37)),
}
NAMES = tuple(_VARIANTS)
PER_CELL = ("reoriented_box", "reoriented_jittered", "reoriented_sheared", "star3", "star7")


@functools.lru_cache(maxsize=None)
def variant(name):
    """(base, data, maps): the un-reoriented mesh, the re-oriented one, and (vperm, cperm, G) between them."""
    base, kw = _VARIANTS[name]()
    data, maps = reorient(base, **kw)
    return base, data, maps


# local vertex of local facet f = 2 a + b (xi_a = b) at facet position m: bit 0 of m runs along the lower, bit 1 along the
# higher remaining axis (the convention of knpemi_dg_create)
def facet_vertex(f, m):
    a, b = f >> 1, f & 1
    a1, a2 = (1 if a == 0 else 0), (1 if a == 2 else 2)
    return (b << a) | ((m & 1) << a1) | ((m >> 1) << a2)


def facet_pairings(mesh):
    """One (my facet, neighbour's facet, neighbour's local vertex at each of my four facet positions) per side of every
    interior facet."""
    cells = mesh.cells
    fv = np.array([[facet_vertex(f, m) for m in range(4)] for f in range(6)])
    seen, out = {}, []
    for c in range(cells.shape[0]):
        for f in range(6):
            key = tuple(sorted(cells[c, fv[f]]))
            if key in seen:
                c1, f1 = seen.pop(key)
                for (ca, fa), (cb, fb) in (((c, f), (c1, f1)), ((c1, f1), (c, f))):
                    other = {int(v): j for j, v in enumerate(cells[cb])}
                    out.append((fa, fb, tuple(other[int(cells[ca, fv[fa, m]])] for m in range(4))))
            else:
                seen[key] = (c, f)
    return out


def hex_statistics(mesh_data):
    """Figures of what the kernels meet on a two-sub-domain hexahedral mesh, computed on the host: left-handed fraction,
    most cells at a sub-mesh vertex, longest row of the EMI pattern (sub-mesh Laplacian pattern plus, on membrane rows,
    the vertices of the other side's membrane facets), and the facet pairings that occur."""
    mesh, ct, ft = mesh_data
    dense = ct.dense()
    mem = mesh.facets[ft.indices[ft.values == 1]]
    out = dict(vertices=mesh.num_vertices, cells=mesh.num_cells, membrane_facets=len(mem),
               left_handed=left_handed_fraction(mesh))
    rows, valence = {}, 0
    for t in (0, 1):
        cells = mesh.cells[dense == t]
        nb = [set() for _ in range(mesh.num_vertices)]
        for c in cells:
            for v in c:
                nb[v].update(int(w) for w in c)
        valence = max(valence, int(np.bincount(cells.ravel(), minlength=mesh.num_vertices).max()))
        rows[t] = nb
    for f in mem:
        for v in f:
            for t in (0, 1):
                rows[t][v].update(-1 - int(w) for w in f)
    out["longest_row"] = int(max(max(len(s) for s in rows[t]) for t in (0, 1)))
    out["most_cells_at_a_submesh_vertex"] = valence
    out["most_cells_at_a_vertex"] = int(np.bincount(mesh.cells.ravel()).max())
    pairs = facet_pairings(mesh)
    out["pairings"] = len(set(pairs))
    out["position_maps"] = len({p[2] for p in pairs})
    out["neighbour_facets_per_axis"] = [len({p[1] for p in pairs if p[0] >> 1 == a}) for a in range(3)]
    return out


# ---- moving fields and dofs between the two descriptions ------------------------------------------------------------------
def cg_dof_maps(s_old, s_new, vperm):
    """For the continuous spaces of two Setups (helpers.Setup) on a mesh and its re-oriented twin: {tag: p} with new
    sub-mesh vertex i of sub-domain `tag` = old sub-mesh vertex p[i], and the same for the membrane mesh under "mem"."""
    inv = np.argsort(vperm)
    out = {}
    for tag in s_old.subdomain_list:
        old, new = (s.subdomain_list[tag]["mesh_sub"].parent_vertices for s in (s_old, s_new))
        out[tag] = np.searchsorted(old, inv[new])
        assert np.array_equal(old[out[tag]], inv[new])
    old, new = (s.subdomain_list[1]["mesh_mem"].parent_vertices for s in (s_old, s_new))
    out["mem"] = np.searchsorted(old, inv[new])
    assert np.array_equal(old[out["mem"]], inv[new])
    return out


def transfer_cg_fields(s_old, s_new, vperm):
    """Copy every field perturb() sets from `s_old` to the same vertices of `s_new`.  Returns cg_dof_maps."""
    p = cg_dof_maps(s_old, s_new, vperm)
    for tag in s_old.subdomain_list:
        pairs = list(zip(s_old.c_prev[tag], s_new.c_prev[tag])) + list(zip(s_old.c[tag], s_new.c[tag]))
        pairs += [(s_old.ion_list[-1][f'c_{tag}'], s_new.ion_list[-1][f'c_{tag}']), (s_old.phi[tag], s_new.phi[tag])]
        for a, b in pairs:
            b.x.array[:] = a.x._a[p[tag]]
    s_new.phi_M_prev[1].x.array[:] = s_old.phi_M_prev[1].x._a[p["mem"]]
    for ma, mb in zip(s_old.mem_models, s_new.mem_models):
        for name, f in ma['I_ch_k'].items():
            mb['I_ch_k'][name].x.array[:] = f.x._a[p["mem"]]
    return p


def dg_dof_map(cperm, G):
    """p with new broken dof i * 8 + j = old broken dof p[i * 8 + j] = cperm[i] * 8 + G[i, j]."""
    return (cperm[:, None] * 8 + G).ravel()


def dg_membrane_map(mem_old, mem_new, vperm):
    """(f, t): new membrane node (m, a) is old membrane node (f[m], t[m, a]); mem_*: (nmf, 4) membrane facet vertices."""
    inv = np.argsort(vperm)
    as_old = inv[mem_new]
    where = {tuple(sorted(row)): i for i, row in enumerate(mem_old)}
    f = np.array([where[tuple(sorted(row))] for row in as_old])
    t = np.array([[int(np.flatnonzero(mem_old[f[m]] == v)[0]) for v in as_old[m]] for m in range(len(f))])
    return f, t
