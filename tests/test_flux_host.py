"""CPU tests of the ion fluxes' numpy restatement (knpemi.fluxes.IonFluxes.compute_host), the reference of the device
tests: exact on affine fields, covariant under rotations, consistent with the oracle's assembled operators, and its row
equal to plain sums of its fields.  TOL is relative to the largest magnitude of the compared component over the
sub-domain."""
import functools
import math
import os
import re

import numpy as np
import pytest

import unstructured_meshes as um
from helpers import TOL
from knpemi.fem import Mesh, extract_submesh, make_mesh_2D, make_mesh_3D, meshtags
from knpemi.fluxes import IonFluxes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, PSI = 96485.0, 96485.0 / (8.314 * 300.0)
Z = [1.0, -1.0, 2.0, -1.0]
NAMES = ["K", "Cl", "Ca", "X"]


def _ions(K):
    return [dict(name=NAMES[k], z=Z[k], D={0: (1.3 + 0.4 * k) * 1e-9, 1: (0.7 + 0.3 * k) * 1e-9}) for k in range(K)]


def _jittered_hex():
    """The hexahedral r = 0 box with every interior vertex moved by up to 10 % of the grid spacing: the cells are no
    longer parallelepipeds."""
    mesh, ct, ft = make_mesh_3D(0, "hexahedron")
    h = np.abs(np.diag(np.asarray(mesh.uniform_cell).reshape(3, 3)))
    lo, hi = mesh.x.min(axis=0), mesh.x.max(axis=0)
    inner = np.all((mesh.x > lo + 0.5 * h) & (mesh.x < hi - 0.5 * h), axis=1)
    rng = np.random.default_rng(3)
    x = mesh.x.copy()
    x[inner] += 0.1 * h * (2.0 * rng.random((int(inner.sum()), 3)) - 1.0)
    m2 = Mesh(x, mesh.cells.copy(), mesh.cell_type)
    return m2, meshtags(m2, m2.tdim, ct.indices, ct.values), None


def _left_handed():
    """The tetrahedral r = 0 box with the first two vertices of every second cell swapped."""
    mesh, ct, ft = make_mesh_3D(0, "tetrahedron")
    cells = mesh.cells.copy()
    cells[::2, [0, 1]] = cells[::2, [1, 0]]
    m2 = Mesh(mesh.x.copy(), cells, mesh.cell_type)
    return m2, meshtags(m2, m2.tdim, ct.indices, ct.values), None


MESHES = {
    "tri_r1": lambda: make_mesh_2D(1),
    "tet_r0": lambda: make_mesh_3D(0, "tetrahedron"),
    "hex_r0": lambda: make_mesh_3D(0, "hexahedron"),
    "jittered_tet": um.jittered_tet_box,
    "fan2d": lambda: um.fan_mesh(2),
    "fan3d": lambda: um.fan_mesh(3),
    "jittered_hex": _jittered_hex,
    "left_handed": _left_handed,
}


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return MESHES[name]()


def _subdomains(mesh, ct):
    out = {}
    for tag in (0, 1):
        sm, e, v, _, _ = extract_submesh(mesh, ct, tag)
        out[tag] = dict(mesh_sub=sm, sub_to_parent=e, sub_vertex_to_parent=v)
    return out


def _fluxes(mesh, ct, K=3):
    subs = _subdomains(mesh, ct)
    fl = IonFluxes(subs, _ions(K), dict(F=F, psi=PSI))
    for tag in subs:
        fl.watch(tag)
    return fl, subs


def _affine(mesh, K):
    """phi = a.x + a0 and c_k = b_k.x + b0_k > 0 with coefficients scaled by the mesh's extent: each axis carries a
    fixed fraction of the value across the box, so a cell carries that fraction divided by the cells along the axis."""
    g = mesh.x.shape[1]
    lo, ext = mesh.x.min(axis=0), np.ptp(mesh.x, axis=0)
    frac = np.array([0.9, -0.7, 0.8])[:g]
    a0, a = -0.02, -0.02 * frac / ext
    b0 = [100.0 + 40.0 * k for k in range(K)]
    b = [b0[k] * np.roll(frac, k) * (1.0 - 0.1 * k) / ext for k in range(K)]
    return lo, a0, a, b0, b


def _rel(got, want):
    """Largest error of every component, relative to the component's largest magnitude over the sub-domain."""
    scale = np.abs(want).max(axis=0)
    return float((np.abs(got - want).max(axis=0) / np.where(scale > 0, scale, 1.0)).max())


@pytest.mark.parametrize("name", list(MESHES))
def test_affine_fields_are_exact(name):
    mesh, ct, _ = _mesh(name)
    K = 3
    fl, subs = _fluxes(mesh, ct, K)
    lo, a0, a, b0, b = _affine(mesh, K)
    phi, c = {}, {}
    for tag, sd in subs.items():
        x = sd["mesh_sub"].x - lo
        phi[tag] = a0 + x @ a
        c[tag] = [b0[k] + x @ b[k] for k in range(K)]
        assert min(ck.min() for ck in c[tag]) > 0
        # the variation across one cell is at least 1e-3 of the value: the code, not cancellation, sets the error
        for u in [phi[tag]] + c[tag]:
            uc = u[sd["mesh_sub"].cells]
            assert (np.ptp(uc, axis=1) / np.abs(uc).mean(axis=1)).min() >= 1e-3
    fields, _ = fl.compute_host(phi, c)
    worst = 0.0
    for tag, sd in subs.items():
        m = sd["mesh_sub"]
        cent = m.x[m.cells].mean(axis=1) - lo
        i_want = np.zeros((m.cells.shape[0], mesh.x.shape[1]))
        for k, ion in enumerate(fl.ion_list):
            D, z = ion["D"][tag], ion["z"]
            Jd = np.tile(-D * b[k], (m.cells.shape[0], 1))
            Jr = -z * PSI * D * (b0[k] + cent @ b[k])[:, None] * a[None, :]
            i_want += F * z * (Jd + Jr)
            worst = max(worst, _rel(fields[tag][f"{ion['name']}/diffusive"], Jd),
                        _rel(fields[tag][f"{ion['name']}/drift"], Jr))
        worst = max(worst, _rel(fields[tag]["current"], i_want))
    print(name, "largest relative error", worst)
    assert worst < TOL
    if name in ("left_handed", "fan3d", "jittered_tet"):
        assert 0.2 < um.left_handed_fraction(mesh) < 0.8


def _random_fields(subs, K, seed=7):
    rng = np.random.default_rng(seed)
    phi, c = {}, {}
    for tag, sd in subs.items():
        n = sd["mesh_sub"].x.shape[0]
        phi[tag] = 1e-2 * rng.uniform(-1, 1, n)
        c[tag] = [rng.uniform(50.0, 150.0, n) for _ in range(K)]
    return phi, c


@pytest.mark.parametrize("name", ["tri_r1", "fan2d", "fan3d", "jittered_tet"])
def test_vertex_order_of_a_cell_does_not_matter(name):
    """The `rotated` mesh (every cell's vertex list rotated by one) with the same nodal values: the same fluxes."""
    data = _mesh(name)
    fl, subs = _fluxes(data[0], data[1])
    m2, ct2, _ = um.rotated(data)
    fl2, subs2 = _fluxes(m2, ct2)
    phi, c = _random_fields(subs, 3)
    fa, ra = fl.compute_host(phi, c)
    fb, rb = fl2.compute_host(phi, c)
    for tag in subs:
        assert np.array_equal(subs[tag]["mesh_sub"].x, subs2[tag]["mesh_sub"].x)
        for key in fa[tag]:
            assert _rel(fb[tag][key], fa[tag][key]) < TOL, (tag, key)
    for key in ra:
        assert np.abs(rb[key] - ra[key]).max() <= TOL * np.abs(ra[key]).max(), key


def _rotation(g):
    if g == 2:
        t = 0.7
        return np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]])
    q, _ = np.linalg.qr(np.array([[1.0, 2.0, -1.0], [0.5, -1.0, 3.0], [2.0, 0.3, 1.0]]))
    return q * np.sign(np.linalg.det(q))


@pytest.mark.parametrize("name", ["tri_r1", "tet_r0", "hex_r0", "jittered_hex", "fan3d"])
def test_rotation_covariance(name):
    """The mesh rotated in space with the same nodal values: every flux vector rotates with it (a swapped pair of
    components in the layout would not), the integrals with them, the maxima stay."""
    mesh, ct, _ = _mesh(name)
    R = _rotation(mesh.x.shape[1])
    assert abs(np.linalg.det(R) - 1.0) < 1e-14 and np.abs(R - np.eye(len(R))).max() > 0.1
    m2 = Mesh(mesh.x @ R.T, mesh.cells.copy(), mesh.cell_type)
    ct2 = meshtags(m2, m2.tdim, ct.indices, ct.values)
    fl, subs = _fluxes(mesh, ct)
    fl2, subs2 = _fluxes(m2, ct2)
    phi, c = _random_fields(subs, 3)
    fa, ra = fl.compute_host(phi, c)
    fb, rb = fl2.compute_host(phi, c)
    for tag in subs:
        for key in fa[tag]:
            want = fa[tag][key] @ R.T
            assert np.abs(fb[tag][key] - want).max() <= TOL * np.abs(want).max(), (tag, key)
    for key in ra:
        want = ra[key] @ R.T if np.ndim(ra[key]) else ra[key]
        assert np.abs(rb[key] - want).max() <= TOL * np.abs(ra[key]).max(), key


@pytest.mark.parametrize("name", ["tri_r1", "tet_r0", "fan2d", "fan3d", "jittered_tet"])
def test_agreement_with_the_assembled_operators(name):
    """On simplices, for every vertex v that carries no membrane entry:
        sum_{T containing v} vol_T i_drift,T . grad N_v = -(A_emi phi)_v,
        sum_{T containing v} vol_T i_diff,T  . grad N_v =  (b_emi)_v
    with A_emi, b_emi from the oracle for the same c (kappa is the P1 function F psi sum z^2 D c, so its integral over
    T is vol_T times its mean).  TOL against max |A phi|, respectively max |b|, over those vertices."""
    import knpemi_oracle as o
    mesh, ct, ft = _mesh(name)
    K = 3
    fl, subs = _fluxes(mesh, ct, K)
    phi, c = _random_fields(subs, K)
    P = o.OracleProblem(mesh.x, mesh.cells, mesh.cell_type, ct.dense(), mesh.facets[ft.indices], ft.values,
                        {0: [], 1: [1]})
    params = dict(dt=1e-4, F=F, psi=PSI, C_M=0.02, C_phi=200.0)
    ions = [dict(name=i["name"], z=i["z"], D=i["D"]) for i in fl.ion_list]
    nq = P.NQ[1]
    mm = {1: [dict(tag=1, I_ch_k={i["name"]: np.zeros(nq) for i in ions})]}
    A, _, b = o.assemble_emi(P, params, ions, c, {1: np.full(nq, -0.07)}, mm)
    fields, _ = fl.compute_host(phi, c)
    lhs_drift, lhs_diff = np.zeros(P.Ntot), np.zeros(P.Ntot)
    for tag, sd in subs.items():
        m = sd["mesh_sub"]
        assert np.array_equal(m.parent_vertices, P.sub[tag]["pv"])
        xc = m.x[m.cells]
        E = xc[:, 1:] - xc[:, :1]
        G = np.linalg.inv(E)                               # G[c, :, t] = grad N_(t+1)
        gradN = np.concatenate([-G.sum(axis=2)[:, None, :], np.swapaxes(G, 1, 2)], axis=1)      # (cell, vertex, gdim)
        vol = fl.volumes(tag)
        for lhs, key in ((lhs_drift, "current/drift"), (lhs_diff, "current/diffusive")):
            np.add.at(lhs, m.cells + P.off[tag], vol[:, None] * np.einsum("ca,cva->cv", fields[tag][key], gradN))
    on_mem = np.zeros(P.Ntot, bool)
    on_mem[P.mem[1]["e"].ravel() + P.off[0]] = True
    on_mem[P.mem[1]["i"].ravel() + P.off[1]] = True
    free = ~on_mem
    assert free.sum() > 10 and on_mem.sum() > 0
    Aphi = A @ np.concatenate([phi[t] for t in P.tags])
    e_drift = np.abs(lhs_drift + Aphi)[free].max() / np.abs(Aphi[free]).max()
    e_diff = np.abs(lhs_diff - b)[free].max() / np.abs(b[free]).max()
    print(name, "drift", e_drift, "diffusive", e_diff)
    assert e_drift < TOL and e_diff < TOL


@pytest.mark.parametrize("name", ["tri_r1", "hex_r0", "fan3d"])
def test_row_equals_plain_sums_of_the_fields(name):
    mesh, ct, _ = _mesh(name)
    fl, subs = _fluxes(mesh, ct)
    phi, c = _random_fields(subs, 3)
    fields, row = fl.compute_host(phi, c)
    g = mesh.x.shape[1]
    for tag in subs:
        vol = fl.volumes(tag)
        for n in [i["name"] for i in fl.ion_list] + ["current"]:
            parts = [fields[tag]["current"]] if n == "current" else [fields[tag][f"{n}/diffusive"], fields[tag][f"{n}/drift"]]
            keys = [f"{tag}/current"] if n == "current" else [f"{tag}/{n}/diffusive", f"{tag}/{n}/drift"]
            for J, key in zip(parts, keys):
                for a in range(g):
                    exact = math.fsum(float(v) * float(j) for v, j in zip(vol, J[:, a]))
                    scale = math.fsum(float(v) * abs(float(j)) for v, j in zip(vol, J[:, a]))
                    assert abs(row[key][a] - exact) <= 1e-12 * scale, key
            J = parts[0] if n == "current" else parts[0] + parts[1]
            mx = max(math.sqrt(sum(float(J[i, a]) * float(J[i, a]) for a in range(g))) for i in range(J.shape[0]))
            assert row[f"{tag}/current_max" if n == "current" else f"{tag}/{n}/max"] == mx
    # the flat row has the columns in the documented order
    flat = fl.row_vector(row)
    assert flat.shape == (fl.n_cols,) and fl.n_cols == 2 * (3 * (2 * g + 1) + g + 1)
    assert np.array_equal(flat[:g], row["0/K/diffusive"]) and flat[-1] == row["1/current_max"]


def test_watch_arguments_and_series_keys():
    mesh, ct, _ = _mesh("tri_r1")
    subs = _subdomains(mesh, ct)
    fl = IonFluxes(subs, _ions(3), dict(F=F, psi=PSI))
    fl.watch(1, ions=["Cl"], current=False)
    assert fl.mask(1) == 0b010 and [k for k, _ in fl.columns()] == ["1/Cl/diffusive", "1/Cl/drift", "1/Cl/max"]
    fl.watch(0, ions=[2, "K"])
    assert fl.mask(0) == 0x100 | 0b101
    with pytest.raises(ValueError):
        fl.watch(0)
    with pytest.raises(ValueError):
        fl.watch(7)
    fl2 = IonFluxes(subs, _ions(3), dict(F=F, psi=PSI))
    with pytest.raises(ValueError):
        fl2.watch(0, ions=[], current=False)
    with pytest.raises(ValueError):
        fl2.watch(0, ions=[3])
    phi, c = _random_fields(subs, 3)
    fl.record_host(0.5, phi, c)
    fl.record_host(1.0, phi, c)
    ser = fl.series()
    assert ser["t"].tolist() == [0.5, 1.0] and ser["1/Cl/drift"].shape == (2, 2) and ser["0/current_max"].shape == (2,)
    assert np.array_equal(ser["0/Ca/diffusive"][0], fl.compute_host(phi, c)[1]["0/Ca/diffusive"])
    # K - 1 concentrations: the eliminated ion's come from c_elim
    fields, _ = fl.compute_host(phi, {t: c[t][:2] for t in c}, c_elim={t: c[t][2] for t in c})
    assert np.array_equal(fields[0]["Ca/drift"], fl.compute_host(phi, c)[0][0]["Ca/drift"])


def test_abi_declares_and_exports_the_flux_entries(hip_lib):
    header = open(os.path.join(ROOT, "include", "knpemi_hip.h")).read()
    declared = set(re.findall(r"\bint (knpemi_flux_[a-z_]+)\s*\(", header))
    assert declared == {"knpemi_flux_set", "knpemi_flux_record", "knpemi_flux_read", "knpemi_flux_fields",
                        "knpemi_flux_reset", "knpemi_flux_clear"}
    for name in declared:
        assert hasattr(hip_lib, name), name
        assert "run_mms.py:270-301" in header[header.rfind("/*", 0, header.index("int " + name + "(")):header.index("int " + name + "(")]
    from knpemi import fluxes
    assert fluxes.chunk() == 256
