"""Host tests of the committed unstructured meshes (tests/golden/unstructured_{2d,3d}.npz): the properties the GPU tests of
tests/test_unstructured_gpu.py rely on, and the numpy oracle's own rounding on them.

Figures of the committed files (tests/golden/make_unstructured.py):

                                         3D        2D
    vertices                             237       185
    cells                                1 308     355
    membrane facets                      118       56
    membrane vertices                    61        43
    longest matrix row                   47        37
    rows longer than 31 entries          6         3
    most cells at one sub-mesh vertex    76        36
    left-handed cells                    46 %      49 %
    min / max cell quality ratio         1.3e-4    5.9e-3
    oracle rounding sensitivity          1.2e-13   4.9e-14
"""
import numpy as np
import pytest

import unstructured_meshes as um
from helpers import csr_rel_err


@pytest.fixture(scope="module", params=[2, 3])
def fan(request):
    data = um.fan_mesh(request.param)
    s, objs = um.oracle_objects(data)
    return request.param, data, s, objs


def test_committed_files_hold_two_arrays_only():
    for dim in (2, 3):
        g = np.load(f"{um.GOLDEN}/unstructured_{dim}d.npz")
        assert sorted(g.files) == ["cells", "x"]
        assert g["x"].dtype == np.float64 and g["cells"].dtype == np.int32
        assert g["x"].shape[1] == dim and g["cells"].shape[1] == dim + 1
        assert g["cells"].min() == 0 and g["cells"].max() == g["x"].shape[0] - 1


def test_fan_meshes_reach_the_long_row_layout(fan):
    dim, (mesh, ct, ft), s, objs = fan
    st = um.mesh_statistics((mesh, ct, ft))
    print(dim, st)
    A = objs["A_emi"].tocsr()
    length = np.diff(A.indptr)
    n0 = s.subdomain_list[0]["mesh_sub"].num_vertices
    mem_parent = np.unique(mesh.facets[ft.indices[ft.values == 1]])
    on_mem = np.concatenate([np.isin(s.subdomain_list[t]["mesh_sub"].parent_vertices, mem_parent) for t in (0, 1)])
    # rows longer than the 31 entries the lattice layout can address: in the ECS block, in the intracellular block, on
    # the membrane
    assert length[:n0].max() > 31 and length[n0:].max() > 31 and length[on_mem].max() > 31
    assert length.max() == st["longest_row"]                  # the host model of the pattern is the oracle's pattern
    assert length.max() <= 255 and st["most_cells_at_a_submesh_vertex"] <= 255      # knpemi_create refuses more
    assert st["most_cells_at_a_submesh_vertex"] > 8 * 4       # KN_PREFETCH pairs on each of 4 lanes: the tail loop runs
    assert 0.30 <= st["left_handed"] <= 0.70
    assert st["membrane_vertices"] >= 40
    if dim == 3:
        assert st["membrane_vertices_with_5_facets"] >= 6


def test_oracle_invariants_on_the_fan_meshes(fan):
    dim, _, _, objs = fan
    A = objs["A_emi"].tocsr()
    scale = np.abs(A.data).max()
    assert np.abs(A @ np.ones(A.shape[0])).max() < 1e-13 * scale
    assert csr_rel_err(A, A.T.tocsr()) < 1e-13


def test_oracle_rounding_sensitivity(fan):
    """The reference's own rounding on these meshes stays far inside the project's 1e-10: measured 3D 1.2e-13 (b_emi),
    2D 4.9e-14 (b_emi); the bound is 1e-12."""
    dim, data, _, _ = fan
    sens = um.rounding_sensitivity(data)
    print(dim, sens)
    assert max(sens.values()) <= 1e-12, sens
