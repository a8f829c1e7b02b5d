"""GPU tests of the per-cell ion balance (knpemi_dg_balance_*, csrc/kernels_dg_balance.hip; DGProblem.balance /
record_membrane / record) against the numpy restatement DGIonBalance.evaluate_host and against the assembled systems
themselves.  The bound is the project's DG parity bound: 1e-10 of the largest magnitude in the compared array
(tests/test_dg_gpu.py); the identities are exact in exact arithmetic."""
import ctypes as C

import numpy as np
import pytest

import dg_balance_cases as B

pytestmark = pytest.mark.gpu

# (kind, M, general hexahedral kernels on a box mesh)
DEVICE_MESHES = [(kind, M, False) for kind, M in B.MESHES] + [("hex", 4, True)]


def _hex_env(monkeypatch, general):
    if general:
        monkeypatch.setenv("KNPEMI_DG_HEX_GENERAL", "1")
    else:
        monkeypatch.delenv("KNPEMI_DG_HEX_GENERAL", raising=False)


def _problem(kind, M, K):
    from knpemi.dg import DGProblem
    bal, (m, ct, ft) = B.balance(kind, M, K)
    dp = DGProblem(m, ct, ft, [0, 1], [1], n_ions=K)
    dp.set_params(B.PARAMS, B.ions(K), gamma=B.GAMMA)
    return dp, bal


def _push(dp, K, seed):
    """A random state on the device: concentrations, potential, phi_M, I_ch, sources.  Returns it."""
    c_all, phi, phi_M, I_ch, src = B.random_state(dp, K, seed)
    for k, c in enumerate(c_all):
        dp.set_concentration(k, c)
    dp.set_potential(phi)
    dp.set_membrane_potential(phi_M)
    for k, I in enumerate(I_ch):
        dp.set_channel_current(k, I)
    for k, f in src.items():
        dp.set_source(k, f)
    return c_all, phi, phi_M, I_ch, src


def _recorded_step(dp, bal, K, seed, splitting, t):
    """assemble_knp, record_membrane, an update with new random concentrations, record.  Returns the host's (cells, row)."""
    c_old, phi, phi_M, I_ch, src = _push(dp, K, seed)
    dp.assemble_knp(splitting)
    dp.record_membrane()
    rng = np.random.default_rng(50 + seed)
    dp.update(np.stack([(c + 0.1 * rng.standard_normal(c.shape)).ravel() for c in c_old[:K - 1]]))
    dp.record(t)
    c_new = [dp.get_concentration(k) for k in range(K)]
    return bal.evaluate_host(B.PARAMS, B.ions(K), c_old, c_new, phi, phi_M, I_ch, gamma=B.GAMMA, splitting_scheme=splitting,
                             f_source=src)


def _row_scales(bal, cells, tags_row):
    """Per column of the row the magnitude its error is measured against.  A sum: the sum of the magnitudes of what is
    summed (for the masses and the penalty shares that is the value itself; a sub-domain's outflows cancel to rounding
    noise, which is compared against sum |out| as on the host).  defect_max: the value.  The membrane tags' block: its
    largest magnitude."""
    K = bal.K
    out = np.abs(cells["cons"] + cells["pen"] + cells["drift"])
    sc = []
    for s in range(2):
        sel = bal.cell_sub == s
        for k in range(K):
            sc += [np.abs(cells["m_new"][sel, k]).sum(), out[sel, k].sum(), np.abs(cells["pen"][sel, k]).sum(),
                   np.abs(cells["defect"][sel, k]).max()]
    return np.concatenate([np.array(sc), np.full(tags_row.shape, np.abs(tags_row).max())])


@pytest.mark.parametrize("splitting", [True, False])
@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("kind,M,general", DEVICE_MESHES)
def test_table_and_row_match_evaluate_host(hip_lib, kind, M, general, K, splitting, monkeypatch):
    """One record_membrane + record: every column of the cell table and the series row against the numpy restatement on
    the same fields."""
    _hex_env(monkeypatch, general)
    dp, bal = _problem(kind, M, K)
    dp.balance(bal)
    cells, row = _recorded_step(dp, bal, K, 1, splitting, 0.05)
    got = bal.cells()
    for c in cells:
        assert B.close(got[c], cells[c], what=f"{kind} K={K} cells/{c}"), c
    ser = bal.series()
    assert ser["t"].tolist() == [0.05]
    dev = np.array([ser[c][0] for c, _ in bal.columns()])
    sc = _row_scales(bal, cells, row[2 * K * 4:])
    err = np.abs(dev - row)
    for j, (c, _) in enumerate(bal.columns()):
        print(f"{c:18s} |dev - host| {err[j]:.3e}  bound {B.TOL * sc[j]:.3e}")
    assert (err <= B.TOL * sc).all(), [(c, err[j], B.TOL * sc[j]) for j, (c, _) in enumerate(bal.columns()) if err[j] > B.TOL * sc[j]]
    cur = bal.current()
    want = bal.current(cells, F=B.PARAMS["F"], z=B.ZS[:K])
    assert B.close(cur, want, what="current")


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("kind,M,general", DEVICE_MESHES)
def test_defect_is_the_residual_of_the_assembled_system(hip_lib, kind, M, general, K, monkeypatch):
    """assemble_knp, record_membrane, solve_knp(rtol=1e-12, update=True), record: the device's defect of every cell and
    solved ion is the cell-block sum of A c - b, computed on the host from the device's matrices, right-hand sides and
    solution.  Scale: the largest cell-block sum of |A| |c| + |b|."""
    _hex_env(monkeypatch, general)
    dp, bal = _problem(kind, M, K)
    dp.balance(bal)
    _push(dp, K, 2)
    dp.assemble_emi()
    dp.assemble_knp()
    dp.record_membrane()
    As = [dp.matrix(1 + k) for k in range(K - 1)]
    bs = [dp.rhs(1 + k) for k in range(K - 1)]
    dp.solve_knp(rtol=1e-12, update=True)                 # (the update reads the solution, it does not change it)
    c = dp.solution()
    dp.record(0.05)
    got = bal.cells()["defect"]
    for k in range(K - 1):
        resid = B.block_sums(As[k] @ c[k] - bs[k], dp.nv)
        scale = B.block_sums(abs(As[k]) @ np.abs(c[k]) + np.abs(bs[k]), dp.nv).max()
        assert B.close(got[:, k], resid, scale, what=f"{kind} K={K} ion {k} defect against A c - b")
        assert bal.series()[f"0/i{k}/defect_max"][0] == np.abs(got[bal.cell_sub == 0, k]).max()
    assert (got[:, K - 1] == 0).all()


def test_multi_workgroup_rows_are_reproducible_and_sum_the_table(hip_lib):
    """Tetrahedra M = 8 (3072 cells, 48 workgroups of 64 cells): two identical runs give identical bits, and the series
    row equals the sums (maxima) over the cell table."""
    K = 3
    outs = []
    for rep in range(2):
        dp, bal = _problem("tet", 8, K)
        dp.balance(bal)
        for j, seed in enumerate((1, 2)):
            _recorded_step(dp, bal, K, seed, True, 0.05 * (j + 1))
        ser = bal.series()
        outs.append((np.stack([ser[c] for c, _ in bal.columns()], axis=1), bal.cells()))
    assert bal.n_cells == 3072
    assert np.array_equal(outs[0][0], outs[1][0])
    for c in outs[0][1]:
        assert np.array_equal(outs[0][1][c], outs[1][1][c]), c
    rows, cells = outs[0]
    want = bal.row_of(cells, rows[-1][2 * K * 4:].reshape(1, -1))
    sc = _row_scales(bal, cells, rows[-1][2 * K * 4:])
    assert (np.abs(rows[-1] - want) <= B.TOL * sc).all()
    assert rows[-1][-1] > 0 and not np.array_equal(rows[0], rows[1])


def test_driver_balance(hip_lib, tmp_path, resolution=1):
    """DGRun with --balance, ten steps: the named columns; every defect_max within the largest cell-block sum of the
    solve's residual plus TOL times the scale; the membrane columns carry F sum_k z_k int j_k = int I_cap + (1 - S) int
    I_ch,tot on both sides (S = 1: the driver runs the splitting scheme)."""
    import run_2D_dg as D
    path = str(tmp_path / "b.npz")
    run = D.DGRun(resolution, balance=path)
    dp = run.dp
    bound = []
    for _ in range(10):
        run.step()
        # the systems of this step are still on the device, and so is the solution the update consumed
        c = dp.solution()
        resid, scale = 0.0, 0.0
        for k in range(2):
            A, b = dp.matrix(1 + k), dp.rhs(1 + k)
            resid = max(resid, np.abs(B.block_sums(A @ c[k] - b, dp.nv)).max())
            scale = max(scale, B.block_sums(abs(A) @ np.abs(c[k]) + np.abs(b), dp.nv).max())
        bound.append(resid + B.TOL * scale)
    run.save()
    s = np.load(path)
    names = [i["name"] for i in run.ions]
    for sub in (0, 1):
        for ion in names:
            for col in ("mass", "outflow", "penalty", "defect_max"):
                assert s[f"{sub}/{ion}/{col}"].shape == (10,) and np.isfinite(s[f"{sub}/{ion}/{col}"]).all()
    for col in ("capacitive", "channel", "area"):
        assert s[f"1/{col}"].shape == (10,)
    assert s["t"].shape == (10,) and s["cells/defect"].shape == (dp.n_cells, 3)
    for ion in names[:2]:
        for sub in (0, 1):
            d = s[f"{sub}/{ion}/defect_max"]
            print(f"{sub}/{ion}/defect_max", d, "bound", np.array(bound))
            assert (d <= np.array(bound)).all()
    F = run.dp.ion_params[0]
    z = np.array([i["z"] for i in run.ions])
    for side in ("ecs", "ics"):
        j = np.stack([s[f"1/{ion}/{side}"] for ion in names], axis=1)
        charge, scale = F * (j @ z), F * (np.abs(j) @ np.abs(z))
        assert (np.abs(charge - s["1/capacitive"]) <= B.TOL * np.maximum(scale, np.abs(s["1/capacitive"]))).all()


def test_mechanics_and_refusals(hip_lib):
    """every, capacity and overflow draining, reset_recorders, a second attachment, record without record_membrane, a
    refused set that keeps the old recorder recording, want_cells = 0, DGSlab.balance."""
    from knpemi import _lib as L
    from knpemi.dg import DGProblem, DGSlab
    K = 3
    dp, bal = _problem("tri", 8, K)
    lib, h = dp.lib, dp.h
    assert lib.knpemi_dg_balance_record(h, 0.0) == L.EINVAL and b"no balance set" in lib.knpemi_last_error()
    assert lib.knpemi_dg_balance_record_membrane(h) == L.EINVAL and b"no balance set" in lib.knpemi_last_error()
    dp.balance(bal, every=2, capacity=2)
    with pytest.raises(RuntimeError, match="already"):
        dp.balance(B.balance("tri", 8, K)[0])
    # every = 2: records 2, 4, 6, 8, 10; capacity 2: the tap drains a full buffer, nothing is dropped
    for j in range(10):
        _push(dp, K, 1 + j % 2)
        dp.assemble_knp()
        dp.record_membrane()
        dp.record(0.1 * (j + 1))
    ser = bal.series()
    assert np.array_equal(ser["t"], [0.1 * (j + 1) for j in (1, 3, 5, 7, 9)]) and ser["0/i0/mass"].shape == (5,)
    assert np.array_equal(ser["0/i0/mass"], np.full(5, ser["0/i0/mass"][0]))      # the even records see the same state
    # record without record_membrane: refused by name, the handle stays usable
    assert lib.knpemi_dg_balance_record(h, 2.0) == L.EINVAL
    assert b"knpemi_dg_balance_record" in lib.knpemi_last_error() and b"record_membrane" in lib.knpemi_last_error()
    assert lib.knpemi_dg_balance_record(h, float("nan")) == L.EINVAL
    # overflow through the ABI: capacity 2, three records
    dp.reset_recorders()
    for j in range(3):
        L.check(lib.knpemi_dg_balance_record_membrane(h))
        L.check(lib.knpemi_dg_balance_record(h, float(j)))
    buf, rows, over = np.zeros((3, bal.n_cols)), C.c_int64(), C.c_int64()
    L.check(lib.knpemi_dg_balance_read(h, 3, L.dptr(buf), C.byref(rows), C.byref(over), 1))
    assert (rows.value, over.value) == (2, 1) and np.array_equal(buf[0], buf[1]) and (buf[2] == 0).all()
    first = buf[0].copy()
    # a refused set: the name in the message, the previous recorder records the next row
    bad = bal.facet_tag.copy()
    bad[0] = 5
    assert lib.knpemi_dg_balance_set(h, 4, 1, 1, L.iptr(bad)) == L.EINVAL
    assert b"knpemi_dg_balance_set" in lib.knpemi_last_error() and b"out of range" in lib.knpemi_last_error()
    assert lib.knpemi_dg_balance_set(h, 0, 1, 1, L.iptr(bal.facet_tag)) == L.EINVAL and b"capacity" in lib.knpemi_last_error()
    L.check(lib.knpemi_dg_balance_record_membrane(h))
    L.check(lib.knpemi_dg_balance_record(h, 9.0))
    L.check(lib.knpemi_dg_balance_read(h, 1, L.dptr(buf), C.byref(rows), C.byref(over), 1))
    assert (rows.value, over.value) == (1, 0) and np.array_equal(buf[0], first)
    # reset_recorders rewinds the series and the record count
    dp.reset_recorders()
    assert dp.n_records == 0 and bal.series()["t"].shape == (0,)
    # without the cell table
    L.check(lib.knpemi_dg_balance_set(h, 4, 0, 1, L.iptr(bal.facet_tag)))
    L.check(lib.knpemi_dg_balance_record_membrane(h))
    L.check(lib.knpemi_dg_balance_record(h, 1.0))
    table = np.zeros((dp.n_cells, K, 8))
    assert lib.knpemi_dg_balance_cells(h, L.dptr(table)) == L.EINVAL and b"want_cells" in lib.knpemi_last_error()
    L.check(lib.knpemi_dg_balance_read(h, 1, L.dptr(buf), C.byref(rows), C.byref(over), 1))
    assert rows.value == 1 and np.array_equal(buf[0], first)
    L.check(lib.knpemi_dg_balance_clear(h))
    assert lib.knpemi_dg_balance_record_membrane(h) == L.EINVAL and b"no balance set" in lib.knpemi_last_error()
    # before knpemi_dg_set_params
    m, ct, ft = B.mesh("tri", 4)
    raw = DGProblem(m, ct, ft, [0, 1], [1])
    b2 = B.balance("tri", 4, 3)[0]
    raw.balance(b2)
    assert lib.knpemi_dg_balance_record_membrane(raw.h) == L.EINVAL and b"knpemi_dg_set_params" in lib.knpemi_last_error()
    with pytest.raises(NotImplementedError, match="ghost cells"):
        DGSlab.balance(object.__new__(DGSlab), bal)
    del raw, dp
