"""Host tests of the per-cell ion balance (knpemi.dg_balance.DGIonBalance.evaluate_host) against the DG restatement
(oracle/knpemi_dg_oracle.py) tested with the indicator of every cell: the cell-block sums of the assembled operators and
right-hand sides.  Nothing is added to the oracle.  Every identity is exact in exact arithmetic; the bound is the
project's DG parity bound, 1e-10 of the largest magnitude in the compared array."""
import numpy as np
import pytest

import dg_balance_cases as B

CASES = [(kind, M, K) for kind, M in B.MESHES for K in (2, 3, 4)]


def _state(bal, K, seed=1):
    c_all, phi, phi_M, I_ch, src = B.random_state(bal, K, seed)
    rng = np.random.default_rng(100 + seed)
    c_new = [c + 0.1 * rng.standard_normal(c.shape) for c in c_all]
    return c_all, c_new, phi, phi_M, I_ch, src


def _operator(o, params, ions, c_all, phi, phi_M, I_ch, gamma):
    """S = 2 A(2 dt) - A(dt): the operators of the solved ions without their mass terms."""
    A1, _ = o.assemble_knp(params, ions, c_all, phi, phi_M, I_ch, gamma=gamma)
    A2, _ = o.assemble_knp(dict(params, dt=2.0 * params["dt"]), ions, c_all, phi, phi_M, I_ch, gamma=gamma)
    return [2.0 * a2 - a1 for a1, a2 in zip(A1, A2)]


def _rotated(xs):
    """The eliminated ion first: it is among the solved ones."""
    return list(xs[-1:]) + list(xs[:-1])


@pytest.mark.parametrize("kind,M,K", CASES)
def test_outflow_is_the_cell_block_sum_of_the_operator(kind, M, K):
    """S u summed over the dofs of every cell = cons + pen + drift of evaluate_host, for random u and phi; then the parts
    one by one -- the oracle at gamma = 0 has no penalty, with psi = 0 no drift, and both enter linearly; then the
    eliminated ion through the rotated ion list."""
    bal, _ = B.balance(kind, M, K)
    o = B.oracle(bal)
    ions, nv = B.ions(K), bal.nv
    c_old, c_new, phi, phi_M, I_ch, src = _state(bal, K)
    cells, _ = bal.evaluate_host(B.PARAMS, ions, c_old, c_new, phi, phi_M, I_ch, gamma=B.GAMMA)
    out = cells["cons"] + cells["pen"] + cells["drift"]
    assert np.abs(cells["pen"]).max() > 0 and np.abs(cells["drift"]).max() > 0 and np.abs(cells["cons"]).max() > 0
    no_drift = dict(B.PARAMS, psi=0.0)
    S = _operator(o, B.PARAMS, ions, c_old, phi, phi_M, I_ch, B.GAMMA)
    S0 = _operator(o, B.PARAMS, ions, c_old, phi, phi_M, I_ch, 0.0)
    S00 = _operator(o, no_drift, ions, c_old, phi, phi_M, I_ch, 0.0)
    for k in range(K - 1):
        u = c_new[k].ravel()
        full, nopen, cons = (B.block_sums(s[k] @ u, nv) for s in (S, S0, S00))
        assert B.close(out[:, k], full, what=f"{kind} K={K} ion {k} outflow")
        assert B.close(cells["cons"][:, k], cons, what=f"{kind} K={K} ion {k} consistency")
        assert B.close(cells["pen"][:, k], full - nopen, np.abs(full).max(), what=f"{kind} K={K} ion {k} penalty")
        assert B.close(cells["drift"][:, k], nopen - cons, np.abs(full).max(), what=f"{kind} K={K} ion {k} drift")
    # the eliminated ion: rotated, it is solved ion 0
    Sr = _operator(o, B.PARAMS, _rotated(ions), _rotated(c_old), phi, phi_M, _rotated(I_ch), B.GAMMA)
    full = B.block_sums(Sr[0] @ c_new[K - 1].ravel(), nv)
    assert B.close(out[:, K - 1], full, what=f"{kind} K={K} eliminated ion outflow")


@pytest.mark.parametrize("splitting", [True, False])
@pytest.mark.parametrize("kind,M,K", CASES)
def test_membrane_source_and_old_mass_are_the_cell_block_sums_of_b(kind, M, K, splitting):
    """mem + src + m_old / dt = the oracle's b tested with the indicator of every cell, with the source and both splitting
    values; the eliminated ion (no source) through the rotated ion list."""
    bal, _ = B.balance(kind, M, K)
    o = B.oracle(bal)
    ions, nv, dt = B.ions(K), bal.nv, B.PARAMS["dt"]
    c_old, c_new, phi, phi_M, I_ch, src = _state(bal, K, 2)
    cells, row = bal.evaluate_host(B.PARAMS, ions, c_old, c_new, phi, phi_M, I_ch, gamma=B.GAMMA, splitting_scheme=splitting,
                                   f_source=src)
    _, b = o.assemble_knp(B.PARAMS, ions, c_old, phi, phi_M, I_ch, splitting_scheme=splitting, gamma=B.GAMMA, f_source=src)
    got = cells["mem"] + cells["src"] + cells["m_old"] / dt
    assert np.abs(cells["mem"]).max() > 0 and np.abs(cells["src"][:, :K - 1]).max() > 0
    assert (cells["src"][bal.cell_sub > 0] == 0).all() and (cells["src"][:, K - 1] == 0).all()
    for k in range(K - 1):
        assert B.close(got[:, k], B.block_sums(b[k], nv), what=f"{kind} K={K} ion {k} right-hand side")
    _, br = o.assemble_knp(B.PARAMS, _rotated(ions), _rotated(c_old), phi, phi_M, _rotated(I_ch), splitting_scheme=splitting,
                           gamma=B.GAMMA)
    assert B.close(got[:, K - 1], B.block_sums(br[0], nv), what=f"{kind} K={K} eliminated ion right-hand side")
    # the membrane tags' columns: sum_F int j^e is what enters the ECS, sum_F int j^i what leaves the cell, and
    # F sum_k z_k int j_k = int I_cap + (1 - S) int I_ch,tot on both sides
    ser = dict(zip([c for c, _ in bal.columns()], row))
    S = 1.0 if splitting else 0.0
    want = ser["1/capacitive"] + (1.0 - S) * ser["1/channel"]
    for side, sel in (("ecs", bal.cell_sub == 0), ("ics", bal.cell_sub > 0)):
        per_ion = np.array([ser[f"1/i{k}/{side}"] for k in range(K)])
        sign = 1.0 if side == "ecs" else -1.0
        assert B.close(sign * cells["mem"][sel].sum(axis=0), per_ion, what=f"{kind} K={K} {side} transfer")
        charge = B.PARAMS["F"] * float(np.dot(B.ZS[:K], per_ion))
        scale = B.PARAMS["F"] * float(np.dot(np.abs(B.ZS[:K]), np.abs(per_ion)))
        assert B.close(charge, want, scale, what=f"{kind} K={K} {side} charge")
    assert ser["1/area"] > 0


@pytest.mark.parametrize("kind,M,K", [(kind, M, 3) for kind, M in B.MESHES])
def test_subdomain_outflow_sums_to_zero_and_defect_closes(kind, M, K):
    """The numerical outflow is antisymmetric between the two cells of a facet: per sub-domain and ion the outflows sum
    to zero within TOL * sum |out|.  The defect of a field that solves the oracle's systems is the cell-block sum of
    A c - b: rounding."""
    import scipy.sparse.linalg as spla
    bal, _ = B.balance(kind, M, K)
    o = B.oracle(bal)
    ions, nv = B.ions(K), bal.nv
    c_old, c_new, phi, phi_M, I_ch, src = _state(bal, K, 3)
    As, b = o.assemble_knp(B.PARAMS, ions, c_old, phi, phi_M, I_ch, gamma=B.GAMMA, f_source=src)
    for k in range(K - 1):
        c_new[k] = spla.spsolve(As[k].tocsc(), b[k]).reshape(bal.n_cells, nv)
    cells, row = bal.evaluate_host(B.PARAMS, ions, c_old, c_new, phi, phi_M, I_ch, gamma=B.GAMMA, f_source=src)
    ser = dict(zip([c for c, _ in bal.columns()], row))
    out = cells["cons"] + cells["pen"] + cells["drift"]
    for s in (0, 1):
        sel = bal.cell_sub == s
        for k in range(K):
            assert B.close(out[sel, k].sum(), 0.0, np.abs(out[sel, k]).sum(), what=f"{kind} sub-domain {s} ion {k} outflow sum")
            assert ser[f"{s}/i{k}/outflow"] == out[sel, k].sum() and ser[f"{s}/i{k}/mass"] == cells["m_new"][sel, k].sum()
            assert ser[f"{s}/i{k}/penalty"] == np.abs(cells["pen"][sel, k]).sum()
    for k in range(K - 1):
        scale = B.block_sums(abs(As[k]) @ np.abs(c_new[k].ravel()) + np.abs(b[k]), nv).max()
        resid = B.block_sums(As[k] @ c_new[k].ravel() - b[k], nv)
        assert B.close(cells["defect"][:, k], resid, scale, what=f"{kind} ion {k} defect")
        assert ser[f"0/i{k}/defect_max"] <= B.TOL * scale
    assert (cells["defect"][:, K - 1] == 0).all()


def test_columns_current_and_refusals_by_name(hip_lib, tmp_path):
    """The named columns, the current, the argument refusals that need no device, and the new entry points in the built
    library."""
    from knpemi import _lib as L
    from knpemi.dg import DGSlab
    from knpemi.dg_balance import CELL_COLUMNS, DGIonBalance
    bal, (m, ct, ft) = B.balance("tri", 4, 3)
    keys = [c for c, _ in bal.columns()]
    assert keys[:4] == ["0/i0/mass", "0/i0/outflow", "0/i0/penalty", "0/i0/defect_max"]
    assert keys[-9:] == ["1/i0/ecs", "1/i1/ecs", "1/i2/ecs", "1/i0/ics", "1/i1/ics", "1/i2/ics", "1/capacitive", "1/channel", "1/area"]
    assert bal.n_cols == 2 * 3 * 4 + 9 and len(CELL_COLUMNS) == 8
    c_old, c_new, phi, phi_M, I_ch, src = _state(bal, 3)
    cells, row = bal.evaluate_host(B.PARAMS, B.ions(3), c_old, c_new, phi, phi_M, I_ch, gamma=B.GAMMA)
    assert row.shape == (bal.n_cols,) and set(cells) == set(CELL_COLUMNS)
    cur = bal.current(cells, F=B.PARAMS["F"], z=B.ZS[:3])
    out = cells["cons"] + cells["pen"] + cells["drift"]
    z = np.array(B.ZS[:3])                               # a three-term sum: a few ulp of the sum of the magnitudes
    assert cur.shape == (bal.n_cells,)
    assert (np.abs(cur - B.PARAMS["F"] * (out @ z)) <= 1e-14 * B.PARAMS["F"] * (np.abs(out) @ np.abs(z))).all()
    bal._append_rows([0.5], row[None, :])
    ser = bal.series()
    assert ser["t"].tolist() == [0.5] and ser["1/area"][0] == row[-1] and set(ser) == {"t"} | set(keys)
    bal.save(tmp_path / "b.npz")
    assert set(np.load(tmp_path / "b.npz").files) == set(ser)
    with pytest.raises(RuntimeError, match="not attached"):
        bal.cells()
    with pytest.raises(RuntimeError, match="F and z are needed"):
        bal.current(cells)
    with pytest.raises(ValueError, match="cell tag"):
        DGIonBalance(m, ct, ft, [0], [1], ["a", "b"])
    with pytest.raises(ValueError, match="2 to 4 ionic species"):
        DGIonBalance(m, ct, ft, [0, 1], [1], ["a"])
    with pytest.raises(NotImplementedError, match="ghost cells"):
        DGSlab.balance(object.__new__(DGSlab), bal)
    names = ["set", "record_membrane", "record", "read", "cells", "reset", "clear"]
    for name in names:
        assert hasattr(hip_lib, f"knpemi_dg_balance_{name}") and f"knpemi_dg_balance_{name}" in L.SIGNATURES
    buf = np.zeros(8)
    for rc in (hip_lib.knpemi_dg_balance_set(None, 4, 1, 0, None), hip_lib.knpemi_dg_balance_record_membrane(None),
               hip_lib.knpemi_dg_balance_record(None, 0.0), hip_lib.knpemi_dg_balance_read(None, 0, None, None, None, 0),
               hip_lib.knpemi_dg_balance_cells(None, L.dptr(buf)), hip_lib.knpemi_dg_balance_reset(None),
               hip_lib.knpemi_dg_balance_clear(None)):
        assert rc == L.EINVAL and b"null" in hip_lib.knpemi_last_error()


def test_driver_parser_accepts_balance():
    import run_2D_dg as D
    a = D.build_parser().parse_args(["--balance", "b.npz"])
    assert a.balance == "b.npz" and D.build_parser().parse_args([]).balance is None
