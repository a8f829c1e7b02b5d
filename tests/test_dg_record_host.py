"""CPU tests of the host side of the DG recorders (knpemi.dg_recording): the weights of points, integrals and reductions,
the jump seminorm of `evaluate_host` against closed forms and against the oracle's own facet tables, the event rules on
node arrays, and the refusals.  Meshes: dg_cases.make_mesh with M = 4 in 2-D, on tetrahedra and on hexahedra, and the
hexahedra with interior vertices moved by up to 20 % of the spacing."""
import numpy as np
import pytest

import dg_record_cases as R

CASES = [(k, 4) for k in R.KINDS]


@pytest.fixture(scope="module", params=CASES, ids=[k for k, _ in CASES])
def obs(request):
    o = R.observables(*request.param)[0]
    o.kind = request.param[0]
    return o


def _affine(X):
    d = X.shape[-1]
    return 0.7 + X @ np.array([1.3, -0.4, 2.1][:d])


def _gauss3_cell_integrals(obs, f):
    """Integral of f over every cell with a rule of its own: 3 x 3 x 3 Gauss through the trilinear map on hexahedra, the
    exact mean-of-vertices rule for an affine f on simplices."""
    X = obs.X
    if obs.nv != 8:
        d = obs.nv - 1
        E = X[:, 1:] - X[:, :1]
        vol = np.abs(np.linalg.det(E)) / {2: 2.0, 3: 6.0}[d]
        return vol * f(X).mean(axis=1)
    g, w = np.polynomial.legendre.leggauss(3)
    g, w = 0.5 * (g + 1.0), 0.5 * w
    tot = np.zeros(X.shape[0])
    for a, wa in zip(g, w):
        for b, wb in zip(g, w):
            for c, wc in zip(g, w):
                xi = (a, b, c)
                N = np.array([np.prod([xi[t] if (j >> t) & 1 else 1 - xi[t] for t in range(3)]) for j in range(8)])
                dN = np.array([[(1.0 if (j >> t) & 1 else -1.0) * np.prod([xi[u] if (j >> u) & 1 else 1 - xi[u]
                                                                            for u in range(3) if u != t]) for t in range(3)]
                               for j in range(8)])
                J = np.einsum("jt,cjd->cdt", dN, X)
                tot += wa * wb * wc * np.abs(np.linalg.det(J)) * f(np.einsum("j,cjd->cd", N, X))
    return tot


def test_point_weights(obs):
    d = obs.X.shape[2]
    u = _affine(obs.X)
    for p, tag in (([0.1, 0.15, 0.12], 0), ([0.45, 0.55, 0.4], 1), ([0.31, 0.62, 0.5], None)):
        p = np.array(p[:d])
        ids, w = obs.point_weights(p, tag)
        assert abs(w.sum() - 1.0) < 1e-13 and (w > -1e-9).all()
        c = ids[0] // obs.nv
        assert np.array_equal(ids, c * obs.nv + np.arange(obs.nv))
        assert tag is None or obs.cell_sub[c] == tag
        # (Q1 reproduces an affine field on a general cell too: the weights are the shape functions at the point's own xi)
        assert abs(np.dot(w, u.ravel()[ids]) - _affine(p)) < 1e-13


def test_point_on_a_shared_facet_takes_the_documented_cell(obs):
    """A vertex of the membrane lies in cells of both sub-domains: with a tag the lowest-numbered containing cell of that
    sub-domain, without one the lowest-numbered containing cell."""
    p = obs.XM[0, 0]
    has = np.flatnonzero((obs.X == p).all(axis=2).any(axis=1))      # the cells with p as a vertex
    assert {0, 1} <= set(obs.cell_sub[has].tolist())
    for tag in (0, 1, None):
        ids, w = obs.point_weights(p, tag)
        want = has[obs.cell_sub[has] == tag].min() if tag is not None else has.min()
        assert ids[0] // obs.nv == want, tag
        assert abs(w.max() - 1.0) < 1e-9


def test_integral_weights(obs):
    u = _affine(obs.X)
    per_cell = _gauss3_cell_integrals(obs, _affine)
    vol = _gauss3_cell_integrals(obs, lambda X: np.ones(X.shape[:-1]))
    total = 0.0
    for tag in (0, 1):
        ids, w = obs.integral_weights("phi", tag)
        sel = obs.cell_sub == tag
        assert abs(w.sum() - vol[sel].sum()) < 1e-13
        assert abs(np.dot(w, u.ravel()[ids]) - per_cell[sel].sum()) < 1e-13
        total += np.dot(w, u.ravel()[ids])
        if obs.kind != "hex_jittered" and tag == 1:      # the middle half: measure 2^-d, centroid the domain's
            assert abs(w.sum() - 0.5 ** obs.X.shape[2]) < 1e-13
            assert abs(np.dot(w, u.ravel()[ids]) - 0.5 ** obs.X.shape[2] * _affine(np.full(obs.X.shape[2], 0.5))) < 1e-13
    assert abs(total - _affine(np.full(obs.X.shape[2], 0.5))) < 1e-13       # the unit square / cube, whatever moved inside
    # the membrane: the boundary of the middle half on the uniform meshes
    ids, w = obs.integral_weights("phi_M", 1)
    assert ids.shape == (obs.nq,) and (w > 0).all()
    d = obs.X.shape[2]
    if obs.kind != "hex_jittered":
        assert abs(w.sum() - 2 * d * 0.5 ** (d - 1)) < 1e-13
        assert abs(np.dot(w, _affine(obs.XM).ravel()[ids]) - 2 * d * 0.5 ** (d - 1) * _affine(np.full(d, 0.5))) < 1e-13


def test_reductions_through_evaluate_host_are_numpys_own():
    obs = R.define_all(R.observables("tet", 4)[0])
    rng = np.random.default_rng(0)
    c_all = [rng.random((obs.n_cells, obs.nv)) for _ in range(3)]
    phi, phi_M = rng.random((obs.n_cells, obs.nv)), rng.random((obs.nmf, obs.nf))
    row = dict(zip(obs.keys, obs.evaluate_host(c_all, phi, phi_M)))
    ecs, ics = obs.cell_sub == 0, obs.cell_sub == 1
    assert row["phi_ecs_min"] == phi[ecs].min() and row["phi_ecs_max"] == phi[ecs].max()
    assert abs(row["phi_ecs_nodal_mean"] - phi[ecs].mean()) < 1e-15
    assert row["c_ics_min"] == c_all[2][ics].min() and row["c_ics_max"] == c_all[2][ics].max()
    assert abs(row["c_ics_nodal_mean"] - c_all[2][ics].mean()) < 1e-15
    assert row["phi_M_min"] == phi_M.min() and row["phi_M_max"] == phi_M.max() and abs(row["phi_M_nodal_mean"] - phi_M.mean()) < 1e-15
    assert abs(row["phi_ecs_average"] - row["phi_ecs_integral"] / (1 - 0.125)) < 1e-14
    # the membrane point: phi_M at the facet's own nodes, the traces through membrane_dofs()
    f, w = obs.membrane_weights([0.25, 0.4, 0.6], 1)
    de, di = obs.membrane_dofs()
    assert abs(row["mem/phi_M"] - np.dot(w, phi_M[f])) < 1e-15
    assert abs(row["mem/i0_e"] - np.dot(w, c_all[0].ravel()[de[f]])) < 1e-15
    assert abs(row["mem/i0_i"] - np.dot(w, c_all[0].ravel()[di[f]])) < 1e-15
    assert (obs.cell_sub[de // obs.nv] == 0).all() and (obs.cell_sub[di // obs.nv] == 1).all()
    assert np.array_equal(obs.X.reshape(-1, 3)[de], obs.XM) and np.array_equal(obs.X.reshape(-1, 3)[di], obs.XM)
    assert abs(w.sum() - 1.0) < 1e-14 and np.allclose(w @ obs.XM[f], [0.25, 0.4, 0.6])
    # the series of record_host
    obs.record_host(0.5, c_all, phi, phi_M)
    assert obs.series()["t"].tolist() == [0.5] and obs.series()["phi_ecs_max"][0] == phi[ecs].max()


def test_jump_of_a_continuous_field_vanishes(obs):
    """A field interpolated from a smooth function has equal values at shared vertices: J <= 1e-13 S."""
    X = obs.X
    u = np.cos(3.0 * X[..., 0] + 1.0) * np.sin(2.0 * X[..., 1] + 0.5) + X[..., -1] ** 2
    for tag in (0, 1):
        J, S = obs.jump_host(u, tag), obs.jump_host(u, tag, squares=True)
        assert S > 0 and 0.0 <= J <= 1e-13 * S, (tag, J, S)


def test_jump_of_an_offset_on_one_cell_by_hand():
    """Uniform 2-D mesh of right triangles with legs h: across a leg |F| = h and both opposite vertices are h away, so
    |F| / h_F = 1; across the hypotenuse |F| = sqrt(2) h and both heights are h / sqrt(2), so |F| / h_F = 2.  An offset
    delta on one cell whose three facets are interior gives J = delta^2 (1 + 1 + 2)."""
    obs = R.observables("2d", 4)[0]
    topo = obs.topology
    n_int = np.bincount(np.concatenate([topo.cT, topo.cN]), minlength=obs.n_cells)
    c = int(np.flatnonzero((n_int == 3) & (obs.cell_sub == 0))[0])
    delta = 0.37
    u = np.full((obs.n_cells, 3), 1.25)
    u[c] += delta
    assert abs(obs.jump_host(u, 0) - delta ** 2 * (1.0 + 1.0 + 2.0)) < 1e-14
    assert obs.jump_host(u, 1) == 0.0
    obs.jump("J", "phi", 0)
    row = obs.evaluate_host([u * 0] * 3, u, np.zeros((obs.nmf, obs.nf)))
    assert abs(row[0] - 4.0 * delta ** 2) < 1e-14


def test_jump_matches_the_oracles_facet_tables(obs):
    """J from knpemi.dg_recording against the restatement from DGOracle._interior_arrays + _facet_frame(verts, 2) /
    DGOracleQ1._interior_q1(): 1e-12 S for a random broken field, through evaluate_host."""
    rng = np.random.default_rng(4)
    fields = [rng.random((obs.n_cells, obs.nv)) for _ in range(4)]
    o2 = R.observables(obs.kind, 4)[0]                   # (the fixture's object is shared: define on one of its own)
    for tag in (0, 1):
        o2.jump(f"phi{tag}", "phi", tag)
        o2.jump(f"c{tag}", "c", tag, ion=obs.ion_names[-1])
    row = dict(zip(o2.keys, o2.evaluate_host(fields[:3], fields[3], np.zeros((obs.nmf, obs.nf)))))
    for tag in (0, 1):
        for key, u in ((f"phi{tag}", fields[3]), (f"c{tag}", fields[2])):
            S = obs.jump_host(u, tag, squares=True)
            assert abs(row[key] - R.oracle_jump(obs, u, tag)) <= 1e-12 * S, key
            assert row[key] > 1e-3 * S


def _events(keep=2):
    from knpemi.dg_recording import DGMembraneEvents
    m, ct, ft = R.mesh("2d", 4)
    ev = DGMembraneEvents(m, ft, [1])
    ev.watch(1.0, reset=0.5, keep=keep)
    return ev


def test_events_follow_the_rules_on_a_hand_made_sequence():
    """Node (0, 0): below, cross, stay above, fall below reset, cross again, one NaN sample, a finite one.  Node (0, 1):
    starts above the threshold (not armed), re-arms, crosses once.  Every other node stays at 0."""
    ev = _events()
    shape = (ev.nmf, ev.nf)
    seq0 = [0.0, 2.0, 3.0, 0.2, 1.2, np.nan, 0.9]
    seq1 = [2.0, 2.5, 0.4, 0.6, 0.8, 4.0, np.nan]
    for k, (a, b) in enumerate(zip(seq0, seq1)):
        v = np.zeros(shape)
        v[0, 0], v[0, 1] = a, b
        ev.record_host(float(k + 1), v)
    m = ev.maps()
    assert m["count"].shape == shape and m["count"][0, 0] == 2 and m["count"][0, 1] == 1 and m["count"].sum() == 3
    assert abs(m["t_first"][0, 0] - 1.5) < 1e-15 and abs(m["t_last"][0, 0] - 4.8) < 1e-14
    assert np.allclose(m["times"][0, 0], [1.5, 4.8], atol=1e-14)
    assert m["v_peak"][0, 0] == 3.0 and m["t_peak"][0, 0] == 3.0
    # node (0, 1): 0.8 at t = 5 -> 4.0 at t = 6 crosses 1.0 at 5 + 0.2 / 3.2
    assert abs(m["t_first"][0, 1] - (5.0 + 0.2 / 3.2)) < 1e-14 and m["t_last"][0, 1] == m["t_first"][0, 1]
    assert m["v_peak"][0, 1] == 4.0 and m["t_peak"][0, 1] == 6.0 and np.isnan(m["times"][0, 1, 1])
    assert np.isnan(m["t_first"][1:]).all() and (m["v_peak"][1:] == 0.0).all() and (m["t_peak"][1:] == 1.0).all()
    assert np.array_equal(ev.fired(), m["count"] > 0) and m["locations"].shape == shape + (2,)
    assert ev.firing_rate(0.0, 10.0)[0, 0] == 0.2
    with pytest.raises(ValueError, match="greater than the previous"):
        ev.record_host(7.0, np.zeros(shape))
    with pytest.raises(ValueError, match="phi_M"):
        ev.record_host(8.0, np.zeros(3))
    ev.reset_host()
    assert (ev.maps()["count"] == 0).all()
    ev.record_host(0.5, np.zeros(shape))                 # an earlier time after the reset


def test_events_velocity_and_save(tmp_path):
    ev = _events(keep=1)
    shape = (ev.nmf, ev.nf)
    x = ev.locations()[..., 0]
    ev.record_host(0.0, np.zeros(shape))
    for k in range(1, 12):                                # a front moving along x with speed 0.1 per unit time
        ev.record_host(float(k), np.where(x <= 0.2 + 0.1 * k, 2.0, 0.0))
    speed, rms, n = ev.conduction_velocity([0.25, 0.5])
    assert n >= 3 and np.isfinite(speed)
    ev.save(tmp_path / "e.npz")
    z = np.load(tmp_path / "e.npz")
    assert z["count"].shape == shape and z["times"].shape == shape + (1,) and z["locations"].shape == shape + (2,)


def test_refusals_by_name():
    from knpemi.dg import DGSlab
    from knpemi.dg_recording import DGMembraneEvents, DGObservables
    obs, (m, ct, ft) = R.observables("2d", 4)
    with pytest.raises(ValueError, match="unknown ion 'Ca'"):
        obs.reduce("x", "c", 0, "max", ion="Ca")
    with pytest.raises(ValueError, match="unknown ion"):
        obs.jump("x", "c", 0, ion=None)
    with pytest.raises(ValueError, match="no sub-domain with tag 5"):
        obs.reduce("x", "phi", 5, "max")
    with pytest.raises(ValueError, match="no sub-domain with tag 2"):
        obs.jump("x", "phi", 2)
    with pytest.raises(ValueError, match="no membrane facet with tag 3"):
        obs.membrane_point("x", [0.25, 0.4], 3)
    with pytest.raises(ValueError, match="is not in the mesh"):
        obs.point("x", [1.5, 0.5])
    with pytest.raises(ValueError, match="is not in sub-domain 1"):
        obs.point("x", [0.1, 0.1], tag=1)
    with pytest.raises(ValueError, match="op must be one of"):
        obs.reduce("x", "phi", 0, "median")
    with pytest.raises(ValueError, match="quantity must be"):
        obs.jump("x", "phi_M", 1)
    assert obs.keys == []                                # a refused definition leaves nothing behind
    obs.reduce("m", "phi", 0, "max")
    with pytest.raises(ValueError, match="'m' defined twice"):
        obs.jump("m", "phi", 0)
    obs.point("p", [0.1, 0.1])
    with pytest.raises(ValueError, match="'p/phi' defined twice"):
        obs.point("p", [0.2, 0.1])
    obs._drain = lambda: None                            # what a tap sets at attachment
    with pytest.raises(RuntimeError, match="define them all before DGProblem.observe"):
        obs.reduce("late", "phi", 0, "min")
    with pytest.raises(ValueError, match="cell tag"):
        DGObservables(m, ct, ft, [0], [1], ["a", "b"])
    ev = DGMembraneEvents(m, ft, [1])
    with pytest.raises(ValueError, match="reset must not exceed"):
        ev.watch(0.0, reset=1.0)
    ev.watch(0.0)
    with pytest.raises(ValueError, match="watched already"):
        ev.watch(1.0)
    for method in ("observe", "detect"):
        with pytest.raises(NotImplementedError, match="ghost cells"):
            getattr(DGSlab, method)(object.__new__(DGSlab), obs)


def test_driver_parser_accepts_series_and_events():
    import run_2D_dg as D
    a = D.build_parser().parse_args(["--series", "s.npz", "--events", "e.npz"])
    assert (a.series, a.events, a.resolution, a.steps, a.host_solves, a.cell_type) == ("s.npz", "e.npz", 1, 100, False, "triangle")
    b = D.build_parser().parse_args([])
    assert b.series is None and b.events is None
