"""CPU tests of the observables' host side: point location (knpemi.fem.probe), functional weights and record_host."""
import contextlib
import io

import numpy as np
import pytest

from knpemi.fem import extract_submesh, make_mesh_2D, make_mesh_3D
from knpemi.fem.mesh import Mesh
from knpemi.fem.probe import Locator, _weights_in, integral_weights, membrane_weights, point_weights


def _jittered_hex(seed=3):
    """make_mesh_3D(0) hexahedra with every interior vertex moved by up to 20 % of the cell size: non-affine Q1 cells."""
    mesh, ct, ft = make_mesh_3D(0, "hexahedron")
    x = mesh.x.copy()
    lo, hi = x.min(axis=0), x.max(axis=0)
    h = np.array([2e-6 / 2, 0.9e-6 / 9, 0.9e-6 / 9])
    inner = np.all((x > lo + 1e-12) & (x < hi - 1e-12), axis=1)
    rng = np.random.default_rng(seed)
    x[inner] += 0.2 * h * rng.uniform(-1, 1, (inner.sum(), 3))
    m2 = Mesh(x, mesh.cells, "hexahedron")
    from knpemi.fem.idealized import _tag
    from knpemi.fem.idealized import axon_boxes
    ct2, ft2 = _tag(m2, axon_boxes(2), [1, 1, 1, 1])
    return m2, ct2, ft2


MESHES = {
    "2d": lambda: make_mesh_2D(1),
    "tet": lambda: make_mesh_3D(0, "tetrahedron"),
    "hex": lambda: make_mesh_3D(0, "hexahedron"),
    "hex_jittered": _jittered_hex,
}


def _subdomains(mesh, ct, ft, cells=(1,)):
    subs = {}
    for t in (0,) + tuple(cells):
        sm, _, _, _, _ = extract_submesh(mesh, ct, t)
        subs[t] = dict(tag=t, mesh_sub=sm)
        if t > 0:
            g, _, _, _, _ = extract_submesh(mesh, ft, [t])
            subs[t]["mesh_mem"] = g
    return subs


def _sample_points(m, rng, n=200):
    """Random points inside random cells, vertices and facet midpoints of the (sub-)mesh m."""
    X = m.x[m.cells]
    nv = X.shape[1]
    pts = []
    for _ in range(n - 40):
        c = rng.integers(m.num_cells)
        if m.cell_type in ("triangle", "tetrahedron"):
            lam = rng.dirichlet(np.ones(nv))
            pts.append(lam @ X[c])
        else:
            xi = rng.uniform(0, 1, 3)
            from knpemi.fem.probe import _tensor_shape
            pts.append(_tensor_shape(xi[None])[0][0] @ X[c])
    pts += list(m.x[rng.integers(m.num_vertices, size=20)])
    f = m.facets[rng.integers(m.num_facets, size=20)]
    pts += list(m.x[f].mean(axis=1))
    return np.array(pts)


def _field(m, rng):
    """A linear field (simplices) or a trilinear one in x (Q1: reproduced exactly by the trilinear interpolant only on
    affine cells, so on hexahedra the test field is the Q1 interpolant of a trilinear field, evaluated through the
    reference coordinates)."""
    a = rng.standard_normal(m.gdim + 1)
    return lambda x: a[0] + (x - m.x.min(axis=0)) / np.ptp(m.x, axis=0) @ a[1:]


@pytest.mark.parametrize("kind", list(MESHES))
def test_point_location_reproduces_linear_fields(kind):
    mesh, ct, ft = MESHES[kind]()
    rng = np.random.default_rng(7)
    for tag in (0, 1):
        m = extract_submesh(mesh, ct, tag)[0]
        loc = Locator(m, f"sub-domain {tag}")
        f = _field(m, rng)
        u = f(m.x)
        for p in _sample_points(m, rng):
            ids, w = loc.weights(p)
            assert ids.shape[0] <= 8 and abs(w.sum() - 1.0) < 1e-12
            if m.cell_type != "hexahedron" or kind == "hex":
                # P1, or Q1 on affine cells: a linear field is reproduced exactly
                assert abs(w @ u[ids] - f(p)) <= 1e-12 * max(1.0, np.abs(u).max())
            # the interpolant reproduces the point itself (x is a Q1 / P1 field)
            assert np.abs(w @ m.x[ids] - p).max() <= 1e-12 * np.ptp(m.x, axis=0).max()


def _trilinear_check(kind):
    """Q1 on the jittered mesh: a trilinear field of the reference coordinates of each cell is reproduced."""
    mesh, ct, ft = MESHES[kind]()
    m = extract_submesh(mesh, ct, 0)[0]
    rng = np.random.default_rng(11)
    u = rng.standard_normal(m.num_vertices)
    loc = Locator(m)
    from knpemi.fem.probe import _tensor_shape
    for _ in range(200):
        c = rng.integers(m.num_cells)
        xi = rng.uniform(0, 1, 3)
        N = _tensor_shape(xi[None])[0][0]
        p = N @ m.x[m.cells[c]]
        ids, w = loc.weights(p)
        assert abs(w @ u[ids] - N @ u[m.cells[c]]) <= 1e-12 * np.abs(u).max()


def test_point_location_jittered_hex_reproduces_trilinear_fields():
    _trilinear_check("hex_jittered")


@pytest.mark.parametrize("kind", list(MESHES))
def test_point_location_matches_brute_force(kind):
    mesh, ct, ft = MESHES[kind]()
    m = extract_submesh(mesh, ct, 0)[0]
    rng = np.random.default_rng(5)
    loc = Locator(m)
    simplex = m.cell_type != "hexahedron"
    for p in _sample_points(m, rng, 60):
        slack, _ = _weights_in(m.x[m.cells], p, simplex)
        brute = int(np.flatnonzero(slack >= -1e-10)[0])          # every cell, lowest index first
        assert loc.cell(p)[0] == brute


@pytest.mark.parametrize("kind", list(MESHES))
def test_point_outside_raises(kind):
    mesh, ct, ft = MESHES[kind]()
    ics = extract_submesh(mesh, ct, 1)[0]
    p = mesh.x.min(axis=0) + 1e-9            # a corner of the box: ECS, never the cell
    with pytest.raises(ValueError, match="not in sub-domain 1"):
        point_weights(ics, p, tag=1)
    with pytest.raises(ValueError, match="is not in"):
        point_weights(ics, mesh.x.max(axis=0) * 2.0, tag=1)


def test_location_is_fast_at_config_scale():
    import time
    mesh, ct, ft = make_mesh_3D(1, "tetrahedron")
    m = extract_submesh(mesh, ct, 0)[0]
    t0 = time.perf_counter()
    loc = Locator(m)
    for p in _sample_points(m, np.random.default_rng(0), 50):
        loc.weights(p)
    assert time.perf_counter() - t0 < 5.0


@pytest.mark.parametrize("kind", list(MESHES))
def test_membrane_point_weights(kind):
    mesh, ct, ft = MESHES[kind]()
    subs = _subdomains(mesh, ct, ft)
    mem = subs[1]["mesh_mem"]
    ecs, ics = subs[0]["mesh_sub"], subs[1]["mesh_sub"]
    rng = np.random.default_rng(2)
    a = rng.standard_normal(mesh.gdim + 1)
    f = lambda x: a[0] + (x / np.ptp(mesh.x, axis=0)) @ a[1:]      # noqa: E731
    for _ in range(50):
        c = rng.integers(mem.num_cells)
        X = mem.x[mem.cells[c]]
        if X.shape[0] == 4:       # quadrilateral facet
            s, t = rng.uniform(0, 1, 2)
            p = (1 - s) * (1 - t) * X[0] + s * (1 - t) * X[1] + (1 - s) * t * X[2] + s * t * X[3]
        else:
            p = rng.dirichlet(np.ones(X.shape[0])) @ X
        e, i, q, w = membrane_weights(subs, 1, p)
        assert np.array_equal(ecs.x[e], mem.x[q]) and np.array_equal(ics.x[i], mem.x[q])
        for xs, ids in ((mem.x, q), (ecs.x, e), (ics.x, i)):
            assert abs(w @ f(xs[ids]) - f(p)) < 1e-12
    with pytest.raises(ValueError, match="membrane of cell 1"):
        membrane_weights(subs, 1, mesh.x.min(axis=0))


@pytest.mark.parametrize("kind", ["2d", "tet", "hex"])
def test_integral_weights(kind):
    mesh, ct, ft = MESHES[kind]()
    subs = _subdomains(mesh, ct, ft)
    ecs, ics, mem = subs[0]["mesh_sub"], subs[1]["mesh_sub"], subs[1]["mesh_mem"]
    if kind == "2d":
        vol_ics, area = 60e-6 * 2e-6, 2 * (60e-6 + 2e-6)
        vol_box = 62e-6 * 4e-6
    else:
        # four axons of 22 x 0.2 x 0.2 um (make_mesh_3D.py:12-24) in a 32 x 0.9 x 0.9 um box
        vol_ics, area = 4 * 22e-6 * 0.2e-6 * 0.2e-6, 4 * (4 * 22e-6 * 0.2e-6 + 2 * 0.2e-6 * 0.2e-6)
        vol_box = 32e-6 * 0.9e-6 * 0.9e-6
    w_i, w_e, w_m = integral_weights(ics), integral_weights(ecs), integral_weights(mem)
    assert abs(w_i.sum() - vol_ics) < 1e-12 * vol_ics
    assert abs(w_e.sum() - (vol_box - vol_ics)) < 1e-12 * vol_box
    assert abs(w_m.sum() - area) < 1e-12 * area
    # exact for a linear field: the integral of x_0 over the ICS = volume * centroid
    cx = ics.x[:, 0].min() + 0.5 * np.ptp(ics.x[:, 0])
    assert abs(w_i @ ics.x[:, 0] - vol_ics * cx) < 1e-12 * vol_ics * cx


def test_integral_weights_jittered_hex():
    mesh, ct, ft = _jittered_hex()
    w = integral_weights(mesh)
    assert abs(w.sum() - 32e-6 * 0.9e-6 * 0.9e-6) < 1e-12 * 32e-6 * 0.9e-6 * 0.9e-6
    # a linear field in x: the integral over the box, exact also for the non-affine cells
    assert abs(w @ mesh.x[:, 0] - 32e-6 * 0.9e-6 * 0.9e-6 * 16e-6) < 1e-12 * 32e-6 * 0.9e-6 * 0.9e-6 * 16e-6


def _setup(kind="2d", r=1):
    from setup_problem import Setup
    with contextlib.redirect_stdout(io.StringIO()):
        return Setup(kind, r, build_forms=False)


def _observables(s):
    from knpemi import Observables
    obs = Observables(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list)
    obs.point("ECS", tag=0, x=[25e-6, 3.5e-6])
    obs.point("ICS", tag=1, x=[25e-6, 2e-6])
    obs.membrane_point("mem", tag=1, x=[25e-6, 3e-6])
    obs.reduce("phi_M_neuron", "phi_M", tag=1, op="nodal_mean")
    obs.reduce("K_ecs_max", "c", ion="K", tag=0, op="max")
    obs.reduce("Na_ecs_min", "c", ion="Na", tag=0, op="min")
    obs.reduce("phi_ics_int", "phi", tag=1, op="integral")
    obs.reduce("phi_M_avg", "phi_M", tag=1, op="average")
    return obs


def test_record_host_keys_and_values():
    s = _setup()
    rng = np.random.default_rng(0)
    for t in s.subdomain_list:
        s.phi[t].x.array[:] = rng.standard_normal(s.phi[t].x.array.shape[0])
        for k in range(2):
            s.c[t][k].x.array[:] = s.c_prev[t][k].x._a * (1 + 0.01 * rng.standard_normal(s.c[t][k].x._a.shape[0]))
        s.ion_list[-1][f"c_{t}"].x.array[:] *= 1.0 + 0.01 * rng.standard_normal(s.phi[t].x._a.shape[0])
    s.phi_M_prev[1].x.array[:] = rng.standard_normal(s.phi_M_prev[1].x._a.shape[0])
    obs = _observables(s)
    for k in range(3):
        obs.record_host(k * s.dt, s.phi, s.c, s.phi_M_prev)
    ser = obs.series()
    want = {"t", "ECS/phi", "ECS/K", "ECS/Cl", "ECS/Na", "ICS/phi", "ICS/K", "ICS/Cl", "ICS/Na", "mem/phi_M",
            "mem/K_e", "mem/K_i", "mem/Cl_e", "mem/Cl_i", "mem/Na_e", "mem/Na_i", "phi_M_neuron", "K_ecs_max",
            "Na_ecs_min", "phi_ics_int", "phi_M_avg"}
    assert set(ser) == want
    assert all(v.shape == (3,) for v in ser.values())
    phiM = s.phi_M_prev[1].x._a
    assert ser["phi_M_neuron"][0] == phiM.mean() or abs(ser["phi_M_neuron"][0] - phiM.mean()) < 1e-15 * np.abs(phiM).max()
    assert ser["K_ecs_max"][0] == s.c[0][0].x._a.max()
    assert ser["Na_ecs_min"][0] == s.ion_list[-1]["c_0"].x._a.min()
    # the membrane point lies on the upper membrane y = 3 um: its traces are the sub-mesh values there
    ecs = s.subdomain_list[0]["mesh_sub"]
    near = np.flatnonzero(np.abs(ecs.x[:, 1] - 3e-6) < 1e-12)
    assert near.size
    # interpolation at a vertex of the 2D r=1 mesh (cell size 1 um) returns the nodal value
    v = np.flatnonzero((np.abs(ecs.x[:, 0] - 25e-6) < 1e-12) & (np.abs(ecs.x[:, 1] - 3e-6) < 1e-12))[0]
    assert abs(ser["mem/K_e"][0] - s.c[0][0].x._a[v]) < 1e-14 * s.c[0][0].x._a[v]
    with pytest.raises(ValueError, match="not in sub-domain 1"):
        obs.point("bad", tag=1, x=[0.5e-6, 0.5e-6])


def test_save_writes_npz(tmp_path):
    s = _setup()
    obs = _observables(s)
    obs.record_host(0.0, s.phi, s.c, s.phi_M_prev)
    obs.save(tmp_path / "s.npz")
    d = np.load(tmp_path / "s.npz")
    assert set(d.files) == set(obs.series()) and d["t"].shape == (1,)


@pytest.mark.parametrize("kind,r", [("2d", 1), ("hex", 0), ("tet", 0)])
def test_figure_points_fall_where_the_reference_means(kind, r):
    """run_2D / run_3D --series: the ECS and ICS points of make_figures.py lie in those sub-domains, the membrane point
    on the membrane of cell 1 (2D: y = 3 um, the upper side of [1,61] x [1,3] um; 3D: the face z = 0.4 um of axon 1)."""
    from run_2D import FIGURE_POINTS, figure_observables
    s = _setup(kind, r)
    obs = figure_observables(s)
    assert {"ECS/phi", "ICS/K", "mem/phi_M", "mem/Na_i"} <= set(obs.keys)
    P = {k: np.array(v) * 1e-6 for k, v in FIGURE_POINTS[s.mesh.gdim].items()}
    with pytest.raises(ValueError):
        point_weights(s.subdomain_list[1]["mesh_sub"], P["ECS"], 1)
    with pytest.raises(ValueError):
        point_weights(s.subdomain_list[0]["mesh_sub"], P["ICS"], 0)
    mem = s.subdomain_list[1]["mesh_mem"]
    e, i, q, w = membrane_weights(s.subdomain_list, 1, P["mem"])
    axis = 1 if kind == "2d" else 2
    assert np.allclose(mem.x[q, axis], 3e-6 if kind == "2d" else 0.4e-6, rtol=0, atol=1e-15)
