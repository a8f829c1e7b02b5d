"""What the host and the GPU tests of the per-cell ion balance share (tests/test_dg_balance_host.py,
tests/test_dg_balance_gpu.py): the smallest meshes of tests/test_dg_gpu.py with a dense facet marker, its parameters and
random states, and the cell-block sums the identities are stated in."""
import numpy as np

import dg_record_cases as R

TOL = 1e-10                      # the project's DG parity bound (tests/test_dg_gpu.py), of the largest magnitude compared
GAMMA = 7.5
ZS = [1.0, -1.0, 2.0, -1.0]
PARAMS = dict(dt=0.05, F=1.3, psi=0.8, C_M=0.7)
# (kind, M): triangles M = 8, tetrahedra M = 4, hexahedra M = 4 as boxes, sheared and with interior vertices moved
MESHES = [("tri", 8), ("tet", 4), ("hex", 4), ("hex_shear", 4), ("hex_random", 4)]


def ions(K):
    return [dict(name=f"i{k}", z=ZS[k], D=[1.0 + 0.3 * k, 0.6 + 0.2 * k]) for k in range(K)]


def mesh(kind, M):
    """(mesh, dense cell marker, dense facet marker); the distortions are those of test_dg_gpu._hex_problem."""
    m, ct, ft = R.mesh({"tri": "2d", "tet": "tet"}.get(kind, "hex"), M)
    x = m.x
    if kind == "hex_shear":
        S = np.array([[1.0, 0.25, -0.15], [0.1, 0.9, 0.2], [-0.2, 0.05, 1.1]])
        x[:] = x @ S.T
    elif kind == "hex_random":
        rng = np.random.default_rng(5)
        inner = np.all((x > 1e-9) & (x < 1 - 1e-9), axis=1)
        x[inner] += (0.18 / M) * (rng.random((inner.sum(), 3)) - 0.5)
    return m, ct, ft


def balance(kind, M, K):
    from knpemi.dg_balance import DGIonBalance
    m, ct, ft = mesh(kind, M)
    return DGIonBalance(m, ct, ft, [0, 1], [1], [f"i{k}" for k in range(K)]), (m, ct, ft)


def oracle(bal):
    import knpemi_dg_oracle as dgo
    return dgo.make_dg_oracle(bal.mesh.x, bal.mesh.cells, bal.mesh.cell_type, bal.cell_sub, bal.mem_facets, bal.mem_tags)


def random_state(shapes, K, seed):
    """test_dg_gpu._random_state on anything with n_cells, nv, nmf, nf and X."""
    from test_dg_gpu import _random_state
    return _random_state(shapes, K, seed)


def block_sums(v, nv):
    """Sum over the dofs of every cell of a dof vector (..., n_cells * nv) -> (..., n_cells)."""
    v = np.asarray(v)
    return v.reshape(v.shape[:-1] + (-1, nv)).sum(axis=-1)


def close(got, want, scale=None, what=""):
    """|got - want| <= TOL * scale, scale the largest magnitude of `want` unless given; prints the figure first."""
    scale = float(np.abs(want).max()) if scale is None else float(scale)
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    print(f"{what}: max |difference| {err:.3e}, bound {TOL * scale:.3e} (scale {scale:.3e})")
    return err <= TOL * scale
