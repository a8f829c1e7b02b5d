"""CPU tests of tests/linalg_cases.py: the exact arithmetic behind the references, the premise of the integer-valued
cases (no partial sum near 2^53), that the generated cases contain the edges they exist for, an independent float64
recomputation of the integer references, and the refusals of knpemi_debug_linalg (no device needed)."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import linalg_cases as lc


def cases_of(op, kind=None):
    return [c for c in lc.all_cases() if c.op == op and (kind is None or c.kind == kind)]


def test_exact_sums_against_fractions():
    rng = np.random.default_rng(1)
    for kind in lc.KINDS:
        a, b, c = (lc.data(kind, rng, 200) for _ in range(3))
        index = rng.integers(0, 7, size=200)
        S, T, count = lc.exact_sums(8, index, a, b, c)
        for i in range(8):
            terms = [Fraction(a[t]) * Fraction(b[t]) * Fraction(c[t]) for t in range(200) if index[t] == i]
            assert S[i] == float(sum(terms, Fraction(0))) and T[i] == float(sum((abs(t) for t in terms), Fraction(0)))
            assert count[i] == len(terms)
    assert count[7] == 0 and S[7] == 0.0
    # both paths agree where both apply: integers pushed through the general one
    a, b = lc.data("int", rng, 50), lc.data("int", rng, 50)
    S1, T1, _ = lc.exact_sums(3, index[:50] % 3, a, b)
    S2, T2, _ = lc.exact_sums(3, index[:50] % 3, a * 0.5, b * 2.0 ** 30)
    assert np.array_equal(S1 * 2.0 ** 29, S2) and np.array_equal(T1 * 2.0 ** 29, T2)


def test_integer_cases_stay_far_below_2_53():
    """the premise of the equality tests: with |entries| <= 8 no summation order can leave the integers doubles hold"""
    seen = 0
    for case in lc.all_cases():
        if case.kind != "int" or case.op == lc.KNP_ORDER:
            continue
        for a, out in case.bufs:
            if a is not None and a.dtype == np.float64 and not out:
                a = a[~np.isnan(a)]      # (the poison the prolongation must not read)
                assert np.all(a == np.rint(a)) and np.abs(a).max(initial=0.0) <= 8, case.name
        assert all(float(v).is_integer() for v in case.dp if case.op != lc.DOTS), case.name
        for ex in case.expect.values():
            assert ex.bound is None, case.name
            if ex.T is not None:
                assert int(np.max(ex.T, initial=0.0)) < 2 ** 53 // 2 ** 20, case.name
                seen += 1
    assert seen > 400
    bounded = sum(1 for case in lc.all_cases() if case.kind == "real" and any(ex.bound is not None for ex in case.expect.values()))
    assert bounded > 300    # (copies, masks and fills are compared for equality in both kinds)


def test_real_data_spreads_over_six_decades():
    a = lc.data("real", np.random.default_rng(0), 4000)
    assert (a > 0).any() and (a < 0).any() and np.abs(a).max() / np.abs(a).min() > 1e5 and np.abs(a).min() > 0


def test_spmv_cases_contain_their_edges():
    for lpr in (4, 16):
        for kind in lc.KINDS:
            cs = lc.spmv_cases(lpr, kind)
            big = [c for c in cs if c.n == 333]
            assert big and any(c.n == 1 for c in cs)
            for c in big:
                assert c.meta["lengths"] == sorted(lc.edge_lengths(lpr))
                assert set(c.meta["slots"]) == {"0", "1", "2", "3", "tail"}, c.meta["slots"]
                assert set(c.meta["where"]) == {"at", "none", "zero"}
            assert any(c.meta["ghosts"] for c in big) and any(not c.meta["ghosts"] for c in big)
            forms = {(c.bufs[4][0] is not None, c.bufs[5][0] is not None, c.bufs[8][0] is not None) for c in big}
            assert forms == {(False, False, False), (False, True, False), (True, False, False), (False, True, True),
                             (False, False, True)}
            one = [c for c in cs if c.n == 1][0]
            assert one.bufs[1][0].tolist() == [0]
    assert lc.diag_slot(16, 3, 4) == 0 and lc.diag_slot(16, 7, 4) == 1 and lc.diag_slot(16, 15, 4) == 3
    assert lc.diag_slot(17, 16, 4) == "tail" and lc.diag_slot(15, 3, 4) == "tail" and lc.diag_slot(15, 2, 4) == 0


def test_amg_spmv_cases_contain_their_edges():
    assert lc.AMG_AVG_ROWS == {24: 4, 25: 16, 128: 16, 129: 64}
    for avg, lpr in lc.AMG_AVG_ROWS.items():
        cs = lc.amg_spmv_cases(avg, "int")
        assert [c.meta["mode"] for c in cs] == [lc.M_AX, lc.M_PRE, lc.M_ADD, lc.M_JAC, lc.M_RES]
        for c in cs:
            assert c.meta["lengths"] == sorted(lc.edge_lengths(lpr)), c.name
            nr, ncol = c.meta["shape"]
            assert (nr < ncol) if c.meta["mode"] == lc.M_AX else (nr > ncol) if c.meta["mode"] == lc.M_ADD else nr == ncol
            assert nr % (256 // lpr) != 0
        add = cs[2]
        assert np.all(add.bufs[6][0] != 99.0) and np.any(add.bufs[6][0] != 0.0)      # accumulates into a non-zero y
        jac = cs[3]
        assert jac.bufs[3][0] is not jac.bufs[6][0]


def test_block_spmv_cases_contain_their_edges():
    assert {(a, b) for a, b, _, _ in lc.BLOCK_SPMV_CONFIGS} == {(8, 7), (8, 9), (4, 5), (4, 6), (3, 4)}
    for nv, nbmax, kernel, runs in lc.BLOCK_SPMV_CONFIGS:
        # launch_block_spmv's rule, restated: the cell-wise kernel for (8, <= 7) and (4, <= 5) unless the row kernel is asked for
        assert runs == ("cell" if kernel != 0 and ((nv == 8 and nbmax <= 7) or (nv == 4 and nbmax <= 5)) else "row")
        cs = [c for c in lc.block_spmv_cases(nv, nbmax, "int") if c.ip[3] == kernel]
        assert {(c.meta["systems"], c.bufs[4][0] is not None, c.bufs[5][0] is not None) for c in cs} == \
            {(s, b, o) for s in (1, 3) for b in (False, True) for o in (False, True)}
        for c in cs:
            assert c.meta["cells"] == 37 and c.meta["counts"] == list(range(1, nbmax + 1)) and c.meta["padded"]
            assert c.n == c.meta["systems"] * 37 * nv


def test_dots_cases_contain_their_edges():
    cs = lc.dots_cases("int")
    assert {c.meta["n"] for c in cs if c.meta["op"] == lc.OP_STORE3} == set(lc.DOT_SIZES)
    assert max(lc.DOT_SIZES) > 512 * 4096
    assert {(c.meta["n"], c.meta["nd"]) for c in cs if c.meta["op"] == lc.OP_STORE3} == {(n, nd) for n in lc.DOT_SIZES for nd in (1, 2, 3)}
    assert {c.meta["op"] for c in cs} == set(range(9))
    for red in (False, True):
        assert {c.meta["op"] for c in cs if c.meta["red"] == red and c.meta["n"] == 4097} == set(range(9))
        tags = {c.meta["tag"].strip() for c in cs if c.meta["red"] == red and c.meta["tag"]}
        assert tags == {t[0] for t in lc.BREAKDOWNS}
    # the breakdown cases do what they are named after: quotient 0, the bit on top of the bits already there
    for tag, op, nd, preset, zero, bit in lc.BREAKDOWNS:
        c = [c for c in cs if c.meta["tag"].strip() == tag and not c.meta["red"]][0]
        before, after = c.bufs[6][0], c.expect[6].ref
        assert int(after[lc.S_FLAG]) == int(before[lc.S_FLAG]) | bit and int(before[lc.S_FLAG]) & bit == 0 and before[lc.S_FLAG] != 0
        quotient = {lc.OP_CG_PAP: lc.S_ALPHA, lc.OP_BI_RHO: lc.S_BETA, lc.OP_BI_ALPHA: lc.S_ALPHA, lc.OP_BI_OMEGA: lc.S_OMEGA,
                    lc.OP_CG_RHO: lc.S_BETA}[op]
        assert before[quotient] != 0.0 and after[quotient] == 0.0
    start = [c for c in cs if c.meta["op"] == lc.OP_START][0]
    assert start.bufs[6][0][lc.S_FLAG] != 0.0 and start.expect[6].ref[lc.S_FLAG] == 0.0
    real = lc.dots_cases("real")
    assert {c.meta["n"] for c in real} == set(lc.DOT_SIZES) - {2200000}


def test_small_kernel_cases_contain_their_edges():
    for kind in lc.KINDS:
        cs = lc.vec_cases(kind)
        assert {(c.meta["op"], c.meta["n"]) for c in cs if c.op == lc.VEC} == {(op, n) for op in range(9) for n in lc.VEC_SIZES}
        for op in (lc.BICG_UPDATE, lc.BICG_INIT, lc.MASK, lc.GHOST_IDENTITY, lc.DIAG_INV):
            assert {c.meta["n"] for c in cs if c.op == op} == set(lc.VEC_SIZES)
        assert {c.bufs[7][0] is not None for c in cs if c.op == lc.BICG_UPDATE} == {False, True}
        assert {c.ip[0] for c in cs if c.op == lc.MASK} == {0, 1}
        assert any(set(c.meta["where"]) == {"at", "none", "zero"} for c in cs if c.op == lc.DIAG_INV)
        se = lc.shift_extrapolate_cases(kind)
        assert {c.meta["stride"] for c in se if c.op == lc.SCATTER_SHIFT} == {1, 5}
        assert {(c.meta["stride"], c.meta["have"], c.meta["old2"]) for c in se if c.op == lc.EXTRAPOLATE} == \
            {(s, h, o) for s in (1, 5) for h in (0, 1, 2, 3) for o in (0, 1)}
    kn = lc.knp_order_cases()
    assert {(c.meta["ks"], tuple(c.meta["sizes"]), c.ip[2]) for c in kn} == \
        {(ks, tuple(s), t) for ks in (2, 3, 4) for s in lc.KNP_SUBDOMAINS for t in (0, 1)}
    assert any(0 in c.meta["sizes"][1:-1] for c in kn) and len({len(c.meta["sizes"]) for c in kn}) == 3
    # the index formula in the kernel's comment, on the smallest instance by hand: two ions, sub-domains of 2 and 1 vertices
    assert [lc.knp_block_index(2, [0, 2, 3], k, g) for k in range(2) for g in range(3)] == [0, 1, 4, 2, 3, 5]


def test_coarse_cases_contain_their_edges():
    for kind in lc.KINDS:
        cs = lc.coarse_cases(kind)
        res = [c for c in cs if c.op == lc.COARSE_RESTRICT]
        assert {(c.meta["nl"], c.meta["world"], c.meta["rank"]) for c in res} == {(nl, w, r) for nl in (1, 3) for w, r in ((1, 0), (3, 0), (3, 2))}
        assert {s for c in res for s in c.meta["sizes"]} == {0, 1, 255, 256, 257, 700}
        for c in res:      # the other ranks' entries hold garbage before and 0 after
            red, ref = c.bufs[4][0], c.expect[4].ref
            assert np.isnan(red[lc.KN_COARSE_OFF:]).all() and np.isfinite(ref).all()
            mine = slice(lc.KN_COARSE_OFF + c.meta["rank"] * c.meta["nl"], lc.KN_COARSE_OFF + (c.meta["rank"] + 1) * c.meta["nl"])
            others = np.ones(len(ref), bool)
            others[:lc.KN_COARSE_OFF] = False
            others[mine] = False
            assert np.all(ref[others] == 0.0) and np.array_equal(ref[:lc.KN_COARSE_OFF], red[:lc.KN_COARSE_OFF])
        assert {(c.meta["nl"], c.meta["world"], c.meta["rank"]) for c in cs if c.op == lc.COARSE_SOLVE} == \
            {(nl, w, r) for nl in (1, 3) for w, r in ((1, 0), (3, 0), (3, 2))}
        pro = [c for c in cs if c.op == lc.COARSE_PROLONG]
        assert {c.ip[0] for c in pro} == {0, 1}
        for c in pro:
            if c.ip[0] == 0:
                assert c.meta["ghosts"] > 0 and c.meta["zero_w_under_nan"] > 0 and np.isnan(c.bufs[2][0][-1])
                assert np.isfinite(c.expect[3].ref).all()


def test_block_inverse_cases_contain_their_edges_and_invert():
    """the measured error of the float64 restatement of the kernel's elimination on the real-valued (SPD, condition number
    <= 100) blocks, relative to the largest entry of the exact inverse: 2.04e-15 (blocks of 3), 2.24e-15 (4), 2.51e-15 (8);
    the device is allowed BLOCK_INV_MARGIN = 4 times that"""
    for bs in (3, 4, 8):
        for kind in lc.KINDS:
            cs, measured = lc.block_inv_cases(bs, kind)
            assert {(c.meta["nb"], c.meta["systems"]) for c in cs} == {(1, 1), (63, 1), (64, 1), (65, 1), (66, 2)}
            assert {c.meta["path"] for c in cs} == {"bcol", "scan"}
            for c in cs:
                if c.meta["nb"] >= 63:
                    assert set(map(tuple, c.meta["positions"])) >= {(k, p) for k in range(1, 6) for p in range(k)}
                inv = c.expect[4].ref.reshape(-1, bs, bs)
                if c.meta["path"] == "bcol":
                    rowptr, vals, bcol = c.bufs[0][0], c.bufs[2][0], c.bufs[3][0].reshape(-1, c.ip[1])
                    for cell in (0, c.meta["nb"] - 1):
                        cl = cell % c.ip[2]
                        pos = int(np.flatnonzero(bcol[cl] == cl)[0])
                        B = np.array([vals[rowptr[cell * bs + a] + pos * bs:][:bs] for a in range(bs)])
                        if kind == "int":
                            assert np.array_equal(B @ inv[cell], np.eye(bs)) and np.abs(B).max() <= 8
                        else:
                            assert np.linalg.cond(B) <= 100.0 * (1 + 1e-9)
                            assert np.abs(B @ inv[cell] - np.eye(bs)).max() < 1e-12
            if kind == "real":
                print(f"block inverse, BS = {bs}: restatement against the exact inverse {measured:.3e}")
                assert 0.0 < measured < 1e-13
            else:
                assert measured == 0.0
    for kind in lc.KINDS:
        assert {tuple(c.meta["sizes"]) for c in lc.dense_cases(kind) if len(c.meta["sizes"]) == 1} == {(s,) for s in lc.DENSE_SIZES}
        assert {len(c.meta["sizes"]) for c in lc.dense_cases(kind)} == set(range(1, 9))
        assert {c.bufs[2][0] is not None for bs in (3, 4, 8) for c in lc.block_apply_cases(bs, kind)} == {False, True}


def dense_of(rowptr, colind, vals, ncol):
    A = np.zeros((len(rowptr) - 1, ncol))
    A[lc.rows_of(rowptr), colind] = vals
    return A


def test_integer_references_against_dense_float64():
    """the references are built from one exact routine; on integer data plain float64 linear algebra is exact too and
    must say the same"""
    for lpr in (4, 16):
        for c in lc.spmv_cases(lpr, "int"):
            rowptr, colind, vals, x, dinv, b, owned = (t[0] for t in c.bufs[:7])
            A = dense_of(rowptr, colind, vals, c.n)
            y = A @ (x * dinv if dinv is not None else x)
            y = b - y if (b is not None and dinv is None) else y
            if owned is not None:
                y = np.where(owned == 1, y, 0.0)
            assert np.array_equal(y, c.expect[7].ref), c.name
    for avg in lc.AMG_AVG_ROWS:
        for c in lc.amg_spmv_cases(avg, "int"):
            rowptr, colind, vals, x, r, dinv, y0 = (t[0] for t in c.bufs[:7])
            A = dense_of(rowptr, colind, vals, c.ip[2])
            w, mode = c.dp[0], c.ip[0]
            ref = {lc.M_AX: lambda: A @ x, lc.M_PRE: lambda: r - w * (A @ (dinv * r)), lc.M_ADD: lambda: y0 + A @ x,
                   lc.M_JAC: lambda: x + w * dinv * (r - A @ x), lc.M_RES: lambda: r - A @ x}[mode]()
            assert np.array_equal(ref, c.expect[6].ref), c.name
            if mode == lc.M_PRE:
                assert np.array_equal(w * dinv * r, c.expect[7].ref)
    for nv, nbmax in sorted({(a, b) for a, b, _, _ in lc.BLOCK_SPMV_CONFIGS}):
        for c in lc.block_spmv_cases(nv, nbmax, "int"):
            rowptr, bcol, vals, x, b, owned = (t[0] for t in c.bufs[:6])
            nsys, cells = c.ip[2], c.ip[2] // nv
            bcol = bcol.reshape(cells, nbmax)
            y = np.zeros(c.n)
            for row in range(c.n):
                off, cl = (row // nsys) * nsys, (row % nsys) // nv
                v = vals[rowptr[row]:rowptr[row + 1]].reshape(-1, nv)
                for k in range(len(v)):
                    y[row] += v[k] @ x[off + bcol[cl, k] * nv:][:nv]
            y = b - y if b is not None else y
            if owned is not None:
                y = np.where(owned == 1, y, 0.0)
            assert np.array_equal(y, c.expect[6].ref), c.name
    for c in lc.dense_cases("int"):
        Minv, r = c.bufs[0][0], c.bufs[1][0]
        x, at, off = [], 0, 0
        for s in c.meta["sizes"]:
            x.append(Minv[off:off + s * s].reshape(s, s) @ r[at:at + s])
            at, off = at + s, off + s * s
        assert np.array_equal(np.concatenate(x), c.expect[2].ref), c.name
    for bs in (3, 4, 8):
        for c in lc.block_apply_cases(bs, "int"):
            binv, v, x = (t[0] for t in c.bufs[:3])
            y = c.dp[0] * np.einsum("cab,cb->ca", binv.reshape(-1, bs, bs), v.reshape(-1, bs)).ravel()
            assert np.array_equal(y + (x if x is not None else 0.0), c.expect[3].ref), c.name
    for c in lc.dots_cases("int"):
        if c.meta["op"] == lc.OP_STORE3 and not c.meta["red"]:
            for k in range(c.meta["nd"]):
                assert float(c.bufs[2 * k][0] @ c.bufs[2 * k + 1][0]) == c.expect[6].ref[c.ip[2 + k]], c.name


def test_refusals_need_no_device(hip_lib):
    from knpemi import _lib as L
    assert hip_lib.knpemi_debug_linalg(lc.SPMV, None) == L.EINVAL
    good = lc.spmv_cases(4, "int")[0]

    def refused(case, text):
        rc, _ = lc.call(hip_lib, case)
        assert rc == L.EINVAL and text.encode() in hip_lib.knpemi_last_error(), (rc, hip_lib.knpemi_last_error())
    def variant(case, **kw):
        c = lc.Case(case.name, case.op, case.n, case.kind, case.ip, case.dp, case.bufs, case.expect, case.meta)
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    refused(variant(good, op=99), "unknown op")
    refused(variant(good, n=0), "n must be positive")
    refused(variant(good, ip=[8, good.n]), "lanes per row")
    refused(variant(good, bufs=good.bufs[:3] + [(None, 0)] + good.bufs[4:]), "x (buf[3]) is null")
    refused(variant(good, bufs=good.bufs[:7] + [(np.zeros(3), 1)] + good.bufs[8:]), "y (buf[7]) holds 24 bytes")
    bad_col = good.bufs[1][0].copy()
    bad_col[5] = good.n
    refused(variant(good, bufs=[good.bufs[0], (bad_col, 0)] + good.bufs[2:]), "colind[5]")
    blk = lc.block_spmv_cases(8, 7, "int")[0]
    refused(variant(blk, ip=[5] + blk.ip[1:]), "NV (ip[0])")
    refused(variant(lc.block_inv_cases(4, "int")[0][0], ip=[5, 5, 1]), "block size (ip[0])")
    refused(variant(lc.block_apply_cases(4, "int")[0], ip=[16]), "block size (ip[0])")
    d = lc.dots_cases("int")[0]
    refused(variant(d, ip=[4] + d.ip[1:]), "nd (ip[0])")
    refused(variant(d, bufs=d.bufs[:6] + [(None, 0)] + d.bufs[7:]), "sc (buf[6]) is null")
    a = lc.amg_spmv_cases(24, "int")[0]
    refused(variant(a, ip=[7] + a.ip[1:]), "mode (ip[0])")
    if not os.path.exists("/dev/kfd"):      # a well-formed call without a device computes nothing anywhere
        rc, outs = lc.call(hip_lib, good)
        assert rc == L.EHIP and b"no HIP device" in hip_lib.knpemi_last_error()
        assert np.all(outs[7] == 99.0)
        rc, _ = lc.call(hip_lib, a)
        assert rc == L.EHIP
