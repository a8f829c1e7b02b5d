"""What the host and the GPU tests of the DG recorders share (tests/test_dg_record_host.py, tests/test_dg_record_gpu.py):
the meshes of dg_cases.make_mesh with a dense facet marker, one set of definitions with every kind of observable, and the
jump seminorm restated from the oracle's own facet tables."""
import numpy as np

import dg_cases as C

KINDS = ("2d", "tet", "hex", "hex_jittered")


def mesh(kind, M):
    """(mesh, dense cell marker, dense facet marker): unit square / cube of M cells per edge, the middle half the
    intracellular sub-domain 1, its boundary the membrane tagged 1.  "hex_jittered": interior vertices moved by up to 20 %
    of the spacing along every axis (general trilinear cells, curved membrane facets)."""
    dim = 2 if kind == "2d" else 3
    m, ct, mfac, mtag = C.make_mesh(dim, M, True, "hexahedron" if kind.startswith("hex") else "simplex")
    if kind == "hex_jittered":
        rng = np.random.default_rng(5)
        x = m.x
        inner = np.all((x > 1e-9) & (x < 1 - 1e-9), axis=1)
        x[inner] += (0.2 / M) * (2.0 * rng.random((int(inner.sum()), 3)) - 1.0)
    key = {tuple(sorted(f)): i for i, f in enumerate(np.asarray(m.facets).tolist())}
    ft = np.zeros(len(m.facets), np.int32)
    for f, t in zip(np.asarray(mfac).tolist(), mtag):
        ft[key[tuple(sorted(f))]] = t
    return m, np.asarray(ct, np.int32), ft


def facet_marker(obs):
    """The dense facet marker the observables `obs` were built from."""
    key = {tuple(sorted(f)): i for i, f in enumerate(np.asarray(obs.mesh.facets).tolist())}
    ft = np.zeros(len(obs.mesh.facets), np.int32)
    for f, t in zip(obs.mem_facets.tolist(), obs.mem_tags):
        ft[key[tuple(sorted(f))]] = t
    return ft


def observables(kind, M, K=3):
    from knpemi.dg_recording import DGObservables
    m, ct, ft = mesh(kind, M)
    return DGObservables(m, ct, ft, [0, 1], [1], [f"i{k}" for k in range(K)]), (m, ct, ft)


def define_all(obs):
    """Every kind of observable: points in both sub-domains and on a vertex many cells share, a membrane point, every
    reduction of phi, of the eliminated ion and of phi_M, the jump seminorms of phi and of the eliminated ion in both
    sub-domains and of a solved ion in one."""
    d = obs.X.shape[2]
    last = obs.ion_names[-1]
    obs.point("ecs", [0.1, 0.15, 0.12][:d], tag=0)
    obs.point("ics", [0.45, 0.55, 0.4][:d], tag=1)
    obs.point("shared", [0.5] * d)
    obs.membrane_point("mem", [0.25, 0.4, 0.6][:d], 1)
    for op in ("integral", "nodal_mean", "average", "min", "max"):
        obs.reduce(f"phi_ecs_{op}", "phi", 0, op)
        obs.reduce(f"c_ics_{op}", "c", 1, op, ion=last)
        obs.reduce(f"phi_M_{op}", "phi_M", 1, op)
    for tag in (0, 1):
        obs.jump(f"J_phi_{tag}", "phi", tag)
        obs.jump(f"J_c_{tag}", "c", tag, ion=last)
    obs.jump("J_c0_0", "c", 0, ion=obs.ion_names[0])
    return obs


def jump_keys(obs):
    """{key: (field of evaluate_host's arguments: "phi" or ion index, tag)} of the jump observables of define_all."""
    K = obs.K
    out = {"J_c0_0": (0, 0)}
    for tag in (0, 1):
        out[f"J_phi_{tag}"] = ("phi", tag)
        out[f"J_c_{tag}"] = (K - 1, tag)
    return out


def row_tolerances(obs, rows, fields):
    """Per column of `rows` (n, n_obs): 1e-13 of the column's largest magnitude for linear functionals and extrema,
    1e-10 S for a jump, S the largest over the records of the same sum with [u]^2 replaced by u_T^2 + u_N^2.
    fields: per record (c_all, phi, phi_M)."""
    tol = 1e-13 * np.abs(rows).max(axis=0)
    jk = jump_keys(obs)
    for j, key in enumerate(obs.keys):
        if key in jk:
            f, tag = jk[key]
            tol[j] = 1e-10 * max(obs.jump_host(phi if f == "phi" else c_all[f], tag, squares=True) for c_all, phi, _ in fields)
    return tol


def oracle_jump(obs, u, tag):
    """J_tag(u) from the oracle's own facet tables: DGOracle._interior_arrays + _facet_frame(verts, 2) on simplices,
    DGOracleQ1._interior_q1() on hexahedra."""
    import knpemi_dg_oracle as dgo
    o = dgo.make_dg_oracle(obs.mesh.x, obs.mesh.cells, obs.mesh.cell_type, obs.cell_sub, obs.mem_facets, obs.mem_tags)
    u = np.asarray(u, float).reshape(obs.n_cells, obs.nv)
    if obs.cell_type == "hexahedron":
        cT, cN, wA, _, inv_h, (lamT, lamN), _ = o._interior_q1()
        jq = np.einsum("mqj,mj->mq", lamT, u[cT]) - np.einsum("mqj,mj->mq", lamN, u[cN])
        per = np.einsum("mq,mq->m", inv_h * wA, jq ** 2)
    else:
        cT, cN, verts, _, inv_h = o._interior_arrays()
        Xq, w, _ = o._facet_frame(verts, 2)
        jq = np.einsum("mqj,mj->mq", o.basis_at(cT, Xq), u[cT]) - np.einsum("mqj,mj->mq", o.basis_at(cN, Xq), u[cN])
        per = inv_h * np.einsum("mq,mq->m", w, jq ** 2)
    return float(per[obs.cell_sub[cT] == obs.sub_index[tag]].sum())
