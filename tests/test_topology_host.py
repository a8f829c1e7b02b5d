"""Host tests of the membrane-topology meshes (tests/topology_meshes.py): each mesh provably contains what it is there for
(counts from the host tables that knpemi_create receives), the oracle's invariants and its own rounding on every
kind x case x form, and the refusal of a tagged facet between two cells at the two host sites (flatten_problem,
OracleProblem).

Oracle rounding sensitivity (every cell described from its next vertex on), largest over the five objects and the seven
cases, plain / jittered:
    triangle 5.5e-14 / 1.6e-13   quadrilateral 2.2e-13 / 1.4e-13   tetrahedron 2.9e-14 / 3.0e-14
    hexahedron 6.0e-14 / 7.2e-14
always on b_emi (whose volume part is a sum of cancelling terms); the other four objects stay below 2.6e-15.  The bound is
1e-12, that of tests/test_unstructured_host.py; no mesh exceeds it, so the device tolerance stays 1e-10."""
import functools

import numpy as np
import pytest

import topology_cases as tc
import topology_meshes as tm
from helpers import csr_rel_err, rel_err

NAMES = ("A_emi", "P_emi", "b_emi", "A_knp", "b_knp")
FORMS = (False, True)
# membrane vertices per cell, per case: 2-D / 3-D
N_Q = {"edge_touch": ([4, 4], [8, 8]), "pinch": ([7], [14]), "face_contact": ([7, 7], [18, 18]),
       "to_boundary": ([9], [24]), "one_cell": ([4], [8]), "tags": ([9], [24]), "empty": ([0], [0])}
SHARED_ECS = {"edge_touch": (1, 2), "face_contact": (2, 6)}
MOST_FACETS_AT_Q = {"triangle": 4, "quadrilateral": 4, "tetrahedron": 10, "hexahedron": 6}       # pinch
SMALLEST_CELL = {"triangle": 2, "quadrilateral": 1, "tetrahedron": 6, "hexahedron": 1}            # one_cell


def _dim(kind):
    return 0 if kind in ("triangle", "quadrilateral") else 1


@functools.lru_cache(maxsize=None)
def _problem(kind, case, jittered):
    return tc.build(kind, case, jittered, forms=False)


@functools.lru_cache(maxsize=None)
def _flat(kind, case, jittered=False):
    from knpemi.device import flatten_problem
    s = _problem(kind, case, jittered)
    return s, flatten_problem(s.mesh, s.ft, s.subdomain_list)


def shared_ecs_vertices(flat):
    """ECS vertices that are membrane vertices of both cells (two-cell cases)."""
    return np.intersect1d(flat["q_to_e"][1], flat["q_to_e"][2])


# ---- 1: the meshes contain what they are there for ---------------------------------------------------------------------------
@pytest.mark.parametrize("jittered", FORMS)
@pytest.mark.parametrize("case", list(tm.CASES))
@pytest.mark.parametrize("kind", tm.KINDS)
def test_counts_of_the_host_tables(kind, case, jittered):
    s, flat = _flat(kind, case, jittered)
    d = _dim(kind)
    assert s.mesh.cell_type == kind and s.mesh.num_cells <= 450
    assert list(flat["n_q"][1:]) == N_Q[case][d]
    n_vert = [a.shape[0] for a in flat["x"]]
    n_cell = [a.shape[0] for a in flat["cells"]]
    for i in range(1, len(n_vert)):                              # every facet couples an ECS vertex to its twin
        assert np.array_equal(flat["x"][0][flat["facet_e"][i]], flat["x"][i][flat["facet_i"][i]])
    if case in SHARED_ECS:
        assert len(shared_ecs_vertices(flat)) == SHARED_ECS[case][d]
        assert s.subdomain_list[1]["membrane_tags"] == [1] and s.subdomain_list[2]["membrane_tags"] == [2]
    if case == "face_contact":                                   # cells sharing untagged facets: open membranes
        shared = tm.contact_facets((s.mesh, s.ct, s.ft))
        assert len(shared) > 0 and (s.ft.dense(fill=0)[shared] == 0).all()
        rim = np.intersect1d(s.subdomain_list[1]["mesh_sub"].parent_vertices, s.subdomain_list[2]["mesh_sub"].parent_vertices)
        in_ecs = np.isin(rim, s.subdomain_list[0]["mesh_sub"].parent_vertices)
        assert in_ecs.sum() == SHARED_ECS[case][d]              # rim vertices: in the ECS and in both cells
    if case == "pinch":                                          # one sub-domain, two bodies: non-manifold membrane
        assert n_vert[1] == N_Q[case][d][0]
        assert np.bincount(flat["facet_q"][1].ravel()).max() == MOST_FACETS_AT_Q[kind]
        manifold = {"triangle": 2, "quadrilateral": 2, "tetrahedron": 6, "hexahedron": 3}[kind]
        assert MOST_FACETS_AT_Q[kind] > manifold
    if case in ("to_boundary", "tags"):                          # membranes end on the exterior boundary
        exterior = np.unique(s.mesh.facets[s.ft.indices[s.ft.values == 5]])
        assert np.isin(s.subdomain_list[1]["mesh_mem"].parent_vertices, exterior).sum() == (2, 6)[d]
        ptr, f2c, _ = s.mesh.facet_cells()
        ext_cells = f2c[ptr[s.ft.indices[s.ft.values == 5]]]
        assert (s.ct.dense()[ext_cells] == 1).any()              # cells of the cell with exterior facets
    if case == "one_cell":                                       # every intracellular vertex is a membrane vertex
        assert n_cell[1] == SMALLEST_CELL[kind] and n_vert[1] == flat["n_q"][1]
    if case == "tags":
        assert s.subdomain_list[1]["membrane_tags"] == [1, 6, 7] and len(s.subdomain_list[1]["mem_models"]) == 2
        assert all((flat["facet_tag"][1] == t).sum() >= 1 for t in (1, 6, 7))
    if case == "empty":
        assert n_cell[1] == 0 and flat["n_q"][1] == 0 and n_vert[1] == 0
    if jittered:
        plain = tm.build(kind, case)[0]
        moved = np.abs(s.mesh.x - plain.x)
        assert moved.max() <= tm.JITTER * tm.H
        on_box = np.any((plain.x == plain.x.min(axis=0)) | (plain.x == plain.x.max(axis=0)), axis=1)
        assert (moved[on_box] == 0).all() and (moved[~on_box].max(axis=1) > 0).all()


# ---- 2: the oracle on every mesh ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_objects(kind, case, jittered):
    return tc.oracle_objects(_problem(kind, case, jittered))


@pytest.mark.parametrize("jittered", FORMS)
@pytest.mark.parametrize("case", list(tm.CASES))
@pytest.mark.parametrize("kind", tm.KINDS)
def test_oracle_invariants(kind, case, jittered):
    """A_emi symmetric with the constants in its null space; the membrane part of b_emi (b_emi minus b_emi without
    membrane models) sums to zero: what leaves one side enters the other; P = A on ECS rows (the preconditioner adds a
    mass term on the cells only)."""
    import adapters
    s = _problem(kind, case, jittered)
    A, Pm, b = _oracle_objects(kind, case, jittered)[:3]
    scale = np.abs(A.data).max()
    assert np.abs(A @ np.ones(A.shape[0])).max() < 1e-13 * scale
    assert csr_rel_err(A, A.T.tocsr()) < 1e-13
    o, P, params, ions = adapters.oracle_problem(s)
    c_all, phi, phiM, mm = adapters.oracle_fields(s)
    _, _, b_vol = o.assemble_emi(P, params, ions, c_all, phiM, {t: [] for t in mm})
    b_mem = b - b_vol
    n0 = P.N[0]
    if case == "empty":
        assert not b_mem.any()
    else:
        assert np.abs(b_mem).max() > 0 and abs(b_mem.sum()) < 1e-13 * np.abs(b_mem).sum()
    D = (Pm - A).tocsr()[:n0]
    assert D.nnz == 0 or np.abs(D.data).max() == 0.0
    if case != "empty":
        assert np.abs((Pm - A).tocsr()[n0:].data).max() > 0


@functools.lru_cache(maxsize=None)
def rounding_sensitivity(kind, case, jittered):
    """Largest relative change of the five oracle objects when every cell is described from its next vertex on."""
    a = _oracle_objects(kind, case, jittered)
    b = tc.oracle_objects(tc.problem(tm.rotated(tm.build(kind, case, jittered)), tm.SPECS[case], forms=False))
    return {k: (rel_err(x, y) if isinstance(x, np.ndarray) else csr_rel_err(x.tocsr(), y.tocsr()))
            for k, x, y in zip(NAMES, a, b)}


@pytest.mark.parametrize("jittered", FORMS)
@pytest.mark.parametrize("kind", tm.KINDS)
def test_oracle_rounding_sensitivity(kind, jittered):
    """The figure the 1e-10 device tolerance stands on: 1e-12, the bound of tests/test_unstructured_host.py, on all
    seven cases.  Measured: the module docstring."""
    worst = {}
    for case in tm.CASES:
        sens = rounding_sensitivity(kind, case, jittered)
        print(kind, case, "jittered" if jittered else "plain", sens)
        worst[case] = max(sens.values())
    print(kind, "jittered" if jittered else "plain", "largest", max(worst.values()))
    assert max(worst.values()) <= 1e-12, worst


# ---- 3: a tagged facet between two cells is no membrane facet ----------------------------------------------------------------
@pytest.mark.parametrize("which", list(tm.CONTACTS))
@pytest.mark.parametrize("kind", tm.KINDS)
def test_tagged_contact_facets_are_refused_on_the_host(kind, which):
    """Cells 1 and 2 share facets that carry membrane tag 1: no ECS cell touches them, although on the single-facet
    contact (and on the wide one in 3-D) all their vertices lie on the rim, where the ECS has them too.  flatten_problem
    names the parent facet and the two cell tags it found, OracleProblem refuses by its own count."""
    import adapters
    from knpemi.device import flatten_problem
    from knpemi.fem import extract_submesh
    data = tm.contact(kind, which)
    shared = tm.contact_facets(data)
    s = tc.problem(data, tm.CONTACT_SPEC, forms=False)
    with pytest.raises(RuntimeError, match=r"membrane facet (\d+) of sub-domain 1 .* tags \[1, 2\]") as e:
        flatten_problem(s.mesh, s.ft, s.subdomain_list)
    assert int(e.value.args[0].split()[2]) in shared
    with pytest.raises(ValueError, match="membrane facet .* of sub-domain 1 .* is a facet of 0 cells tagged 0"):
        adapters.oracle_problem(s)
    # what the vertex look-up alone says: it refuses only where a contact vertex lies inside the contact
    ecs = extract_submesh(s.mesh, s.ct, 0)[0].parent_vertices
    rim_only = np.isin(np.unique(s.mesh.facets[shared]), ecs).all()
    assert rim_only == (which == "single" or kind in ("tetrahedron", "hexahedron"))
    assert len(shared) == {"single": dict(triangle=1, quadrilateral=1, tetrahedron=2, hexahedron=1),
                           "wide": dict(triangle=2, quadrilateral=2, tetrahedron=4, hexahedron=2)}[which][kind]


@pytest.mark.parametrize("which", list(tm.CONTACTS))
@pytest.mark.parametrize("kind", tm.KINDS)
def test_untagged_contact_facets_are_accepted_on_the_host(kind, which):
    import adapters
    from knpemi.device import flatten_problem
    s = tc.problem(tm.contact(kind, which, tagged=False), tm.CONTACT_SPEC, forms=False)
    flat = flatten_problem(s.mesh, s.ft, s.subdomain_list)
    _, P, _, _ = adapters.oracle_problem(s)
    for i, t in ((1, 1), (2, 2)):
        assert flat["n_q"][i] == P.NQ[t] > 0
        assert np.array_equal(flat["facet_e"][i], P.mem[t]["e"]) and np.array_equal(flat["facet_i"][i], P.mem[t]["i"])


def test_membrane_facet_on_the_exterior_boundary_is_refused_on_the_host():
    """A facet of one cell only (exterior) tagged as membrane: not shared by two cells."""
    from knpemi.device import flatten_problem
    from knpemi.fem import MeshTags
    mesh, ct, ft = tm.build("quadrilateral", "to_boundary")
    ptr, f2c, _ = mesh.facet_cells()
    ext = [f for f in ft.indices[ft.values == 5] if ct.dense()[f2c[ptr[f]]] == 1]
    vals = ft.dense(fill=0)
    vals[ext[0]] = 1
    ft2 = MeshTags(mesh, 1, np.arange(mesh.num_facets, dtype=np.int32), vals)
    s = tc.problem((mesh, ct, ft2), tm.SPECS["to_boundary"], forms=False)
    with pytest.raises(RuntimeError, match=rf"membrane facet {ext[0]} of sub-domain 1 .* tags \[1\]"):
        flatten_problem(s.mesh, s.ft, s.subdomain_list)
