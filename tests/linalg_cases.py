"""Inputs and plain references for the kernels of the device solves, one kernel at a time (knpemi_debug_linalg).

Every kernel gets two kinds of input:

* kind "int": matrix entries, vectors and scalars are small integers stored as doubles (|.| <= 8).  Every partial sum stays
  far below 2^53, so the result does not depend on the summation order and the device must reproduce the reference
  exactly.  The largest magnitude any partial sum could reach (the sum of the absolute values of the terms) is kept with
  every expectation as `T`; tests/test_linalg_host.py asserts it is below 2^53.
* kind "real": mixed sign, magnitudes spread over six decades.  The reference is the exact value (the doubles as
  integers times a power of two, summed as Python integers) rounded once; the bound is the a priori one,
  |got - ref| <= (m + 4) 2^-53 T for a sum of m terms with T = sum of the absolute values of the terms.  Any summation
  order sends a term through at most m - 1 additions and, with the roundings of its own factors, the few roundings the
  kernels add around the sum (a scaling, b - ., x + .) stay inside the + 4; a fused multiply-add only removes roundings.

Every output of every kernel is written as a polynomial in the inputs (`exact_sums`), so one exact routine serves all
of them; what is not arithmetic (copies, masks, permutations, untouched entries) is compared for equality in both kinds.
"""
import ctypes as C
import functools
import itertools
from fractions import Fraction

import numpy as np

U = 2.0 ** -53

# restated from csrc/kernels_krylov.hip and csrc/kernels_amg.hip
(S_RHO, S_RHO_OLD, S_PAP, S_ALPHA, S_BETA, S_OMEGA, S_RR, S_BB, S_TS, S_TT, S_MEAN, S_FLAG, S_RV, S_N) = range(14)
F_RHO_ZERO, F_RV_ZERO, F_OMEGA_ZERO, F_PAP_ZERO = 1, 2, 4, 8
OP_STORE3, OP_CG_INIT, OP_CG_PAP, OP_CG_RHO, OP_BI_RHO, OP_BI_ALPHA, OP_BI_OMEGA, OP_MEAN, OP_START = range(9)
V_RESID, V_SHIFT, V_CG_XR, V_CG_P, V_JACOBI, V_BI_P, V_BI_S, V_COPY, V_COPY_SHIFT = range(9)
M_AX, M_PRE, M_ADD, M_JAC, M_RES = range(5)
KN_COARSE_OFF = 8
SC_LEN = 16

(SPMV, BLOCK_SPMV, DOTS, VEC, BICG_UPDATE, BICG_INIT, MASK, GHOST_IDENTITY, DIAG_INV, SCATTER_SHIFT, EXTRAPOLATE, KNP_ORDER,
 COARSE_RESTRICT, COARSE_SOLVE, COARSE_PROLONG) = range(15)
AMG_SPMV, AMG_BLOCK_INV, AMG_BLOCK_APPLY, AMG_DENSE = range(20, 24)

KINDS = ("int", "real")
DOT_SIZES = (1, 255, 256, 257, 4095, 4096, 4097, 12293, 2200000)
VEC_SIZES = (1, 256, 257, 1000)


# ---- data -------------------------------------------------------------------------------------------------------------

def data(kind, rng, n, nonzero=False):
    if kind == "int":
        a = rng.integers(-8, 9, size=n).astype(np.float64)
        if nonzero:
            a[a == 0] = 3.0
        return a
    return rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-3.0, 3.0, size=n)


def scalars(kind, rng):
    """the device scalars sc[] with every slot set to something recognisable and non-zero; S_FLAG holds a bit set"""
    sc = data(kind, rng, SC_LEN, nonzero=True)
    sc[S_FLAG] = 0.0
    return sc


def mask_of(rng, n):
    owned = (rng.random(n) < 0.7).astype(np.uint8)
    if n >= 2:
        owned[0], owned[n - 1] = 1, 0
    return owned


# ---- exact arithmetic -------------------------------------------------------------------------------------------------

def _small_int(f):
    return bool(np.all(np.isfinite(f)) and np.all(f == np.rint(f)) and np.all(np.abs(f) <= 2 ** 24))


def exact_sums(n_out, index, *factors):
    """out[i] = sum over the terms t with index[t] == i of the product of factors[.][t], exactly.
    Returns (the sums rounded once to double, the sums of the absolute values rounded once, terms per output)."""
    index = np.asarray(index, np.int64)
    order = np.argsort(index, kind="stable")
    idx = index[order]
    fs = [np.asarray(f, np.float64)[order] for f in factors]
    rp = np.searchsorted(idx, np.arange(n_out + 1))
    count = np.diff(rp)
    if all(_small_int(f) for f in fs):          # integers: int64 is exact here (asserted)
        prod = np.ones(len(idx), np.int64)
        bound = 1.0
        for f in fs:
            prod *= f.astype(np.int64)
            bound *= max(1.0, float(np.abs(f).max())) if len(f) else 1.0
        assert bound * max(1, len(idx)) < 2.0 ** 62
        cs = np.concatenate([[0], np.cumsum(prod)])
        ca = np.concatenate([[0], np.cumsum(np.abs(prod))])
        S, T = cs[rp[1:]] - cs[rp[:-1]], ca[rp[1:]] - ca[rp[:-1]]
        assert T.max(initial=0) < 2 ** 53
        return S.astype(np.float64), T.astype(np.float64), count
    M = np.ones(len(idx), object)
    E = np.zeros(len(idx), np.int64)
    for f in fs:                                  # f = m 2^e with m an integer of at most 53 bits
        m, e = np.frexp(f)
        M = M * (m * 2.0 ** 53).astype(np.int64).astype(object)
        E += e.astype(np.int64) - 53
    emin = int(E.min()) if len(E) else 0
    vals = [int(m) << int(e - emin) for m, e in zip(M, E)]
    cs = [0] + list(itertools.accumulate(vals))
    ca = [0] + list(itertools.accumulate(abs(v) for v in vals))
    scale = Fraction(2) ** emin
    S = np.array([float((cs[rp[i + 1]] - cs[rp[i]]) * scale) for i in range(n_out)])
    T = np.array([float((ca[rp[i + 1]] - ca[rp[i]]) * scale) for i in range(n_out)])
    return S, T, count


class Expect:
    """what slot `slot` holds after the call: ref; bound None: equal, else |got - ref| <= bound; T: largest partial sum"""
    def __init__(self, ref, bound=None, T=None):
        self.ref, self.bound, self.T = np.asarray(ref), bound, T


def summed(kind, n_out, index, *factors, m=None, scale=1.0):
    """Expect of exact_sums; m: number of terms of the a priori bound (default: the terms of each output)"""
    S, T, count = exact_sums(n_out, index, *factors)
    if kind == "int":
        return Expect(S, None, T)
    mm = count if m is None else m
    return Expect(S, (mm + 4) * U * T * scale, T)


def poly(kind, n, terms):
    """out[i] = sum of the terms, a term being a tuple of factors (arrays of n entries or scalars)"""
    arity = max(len(t) for t in terms)
    idx = np.tile(np.arange(n), len(terms))
    facs = [np.concatenate([np.broadcast_to(np.asarray(t[k] if k < len(t) else 1.0, np.float64), (n,)) for t in terms])
            for k in range(arity)]
    return summed(kind, n, idx, *facs, m=len(terms))


def same(a):
    return Expect(np.array(a, copy=True))


class Case:
    def __init__(self, name, op, n, kind, ip=(), dp=(), bufs=(), expect=None, meta=None):
        self.name, self.op, self.n, self.kind = name, op, int(n), kind
        self.ip, self.dp, self.bufs = [int(v) for v in ip], [float(v) for v in dp], list(bufs)
        self.expect = expect or {}
        self.meta = meta or {}

    def __repr__(self):
        return self.name


def call(lib, case):
    """runs the case; returns (return code, the arrays after the call, slot by slot)"""
    from knpemi import _lib as L
    A = L.DebugLinalgArgs()
    A.n = case.n
    for k, v in enumerate(case.ip):
        A.ip[k] = v
    for k, v in enumerate(case.dp):
        A.dp[k] = v
    arrs = []
    for s, (a, out) in enumerate(case.bufs):
        if a is None:
            arrs.append(None)
            continue
        a = np.array(a, copy=True, order="C")
        hold = a if a.size else np.zeros(1, a.dtype)        # an empty array is still a pointer
        arrs.append((a, hold))
        A.buf[s] = hold.ctypes.data
        A.bytes[s] = a.nbytes
        A.out[s] = 1 if out else 0
    rc = lib.knpemi_debug_linalg(case.op, C.byref(A))
    return rc, [None if p is None else p[0] for p in arrs]


def check(case, outs):
    """asserts every expectation of the case; returns the largest error / bound ratio of the bounded ones"""
    worst = 0.0
    for slot, ex in case.expect.items():
        got = outs[slot]
        assert got.shape == ex.ref.shape, (case.name, slot)
        if ex.bound is None:
            bad = np.flatnonzero(~((got == ex.ref) | (np.isnan(got) & np.isnan(ex.ref))))
            assert bad.size == 0, f"{case.name}: slot {slot} differs at {bad[:8]}: got {got[bad[:8]]}, expected {ex.ref[bad[:8]]}"
        else:
            err = np.abs(got - ex.ref)
            bad = np.flatnonzero(~(err <= ex.bound))
            assert bad.size == 0, (f"{case.name}: slot {slot} out of bound at {bad[:8]}: got {got[bad[:8]]}, expected "
                                   f"{ex.ref[bad[:8]]}, error {err[bad[:8]]}, bound {ex.bound[bad[:8]]}")
            nz = ex.bound > 0
            if nz.any():
                worst = max(worst, float((err[nz] / ex.bound[nz]).max()))
    return worst


# ---- CSR operators ----------------------------------------------------------------------------------------------------

def edge_lengths(lpr):
    """boundaries of `j + 3 LPR < e` and of the tail loop"""
    return [0, 1, lpr - 1, lpr, lpr + 1, 4 * lpr - 1, 4 * lpr, 4 * lpr + 1, 8 * lpr, 8 * lpr + 3]


def diag_slot(length, pos, lpr):
    """which of the four unrolled loads (0 .. 3) or the tail loop ("tail") reads entry `pos` of a row of `length`"""
    lane, trip = pos % lpr, pos // lpr
    j, groups = lane, 0
    while j + 3 * lpr < length:
        groups, j = groups + 1, j + 4 * lpr
    return trip % 4 if trip < 4 * groups else "tail"


def make_csr(kind, rng, n, ncols, lengths, diagonal=True):
    """CSR with row i of length lengths[i % len]; the diagonal entry (rows < ncols) sits at a position that walks through
    the row, is absent ("none") or is a stored zero ("zero"), in turn.  Returns rowptr, colind, vals, where[i]."""
    rowptr, colind, where = [0], [], []
    for i in range(n):
        L = min(lengths[i % len(lengths)], ncols)
        variant = (i // len(lengths) + 2) % 7
        if not diagonal or L == 0 or i >= ncols or variant == 0:
            cols = rng.choice(np.setdiff1d(np.arange(ncols), [i]), size=min(L, ncols - 1), replace=False) if ncols > 1 else \
                np.zeros(0, np.int64)
            where.append(("none", None))
        else:
            others = rng.choice(np.setdiff1d(np.arange(ncols), [i]), size=L - 1, replace=False)
            pos = (i * 7 + variant * 13) % L if variant > 1 else int(rng.integers(0, L))
            cols = np.insert(others, pos, i)
            where.append(("zero" if variant == 1 else "at", pos))
        colind.extend(int(c) for c in cols)
        rowptr.append(len(colind))
    rowptr, colind = np.array(rowptr, np.int32), np.array(colind, np.int32)
    vals = data(kind, rng, len(colind), nonzero=True)
    for i, (w, pos) in enumerate(where):
        if w == "zero":
            vals[rowptr[i] + pos] = 0.0
    return rowptr, colind, vals, where


def rows_of(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def diag_inverse(rowptr, colind, vals):
    """diag_inv_kernel's rule: 1 / a_ii, 1 where the diagonal entry is absent or zero"""
    n = len(rowptr) - 1
    d = np.zeros(n)
    r = rows_of(rowptr)
    hit = colind == r
    d[r[hit]] = vals[hit]
    return np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 1.0)


def inverse_expect(kind, ref):
    """a correctly rounded quotient against the reference rounded once: equal; (0 + 4) 2^-53 |ref| is the a priori bound"""
    return Expect(ref, None if kind == "int" else 4 * U * np.abs(ref), np.abs(ref))


@functools.lru_cache(maxsize=None)
def spmv_cases(lpr, kind):
    rng = np.random.default_rng(100 + lpr + (kind == "real"))
    out = []
    for n, lengths in ((333, edge_lengths(lpr)), (1, [1])):
        rowptr, colind, vals, where = make_csr(kind, rng, n, n, lengths)
        x, b, dinv = data(kind, rng, n), data(kind, rng, n), data(kind, rng, n, nonzero=True)
        r = rows_of(rowptr)
        ax = summed(kind, n, r, vals, x[colind])
        scaled = summed(kind, n, r, vals, x[colind], dinv[colind])
        resid = summed(kind, n, np.concatenate([r, np.arange(n)]), np.concatenate([-vals, b]),
                       np.concatenate([x[colind], np.ones(n)]), m=np.diff(rowptr))
        dref = diag_inverse(rowptr, colind, vals)
        meta = dict(lpr=lpr, n=n, lengths=sorted(set(np.diff(rowptr).tolist())),
                    slots=sorted({str(diag_slot(int(rowptr[i + 1] - rowptr[i]), p, lpr)) for i, (w, p) in enumerate(where) if w == "at"}),
                    where=sorted({w for w, _ in where}))
        for owned in (None, mask_of(rng, n)):
            def masked(ex, fill):
                if owned is None:
                    return ex
                g = owned == 0
                return Expect(np.where(g, fill, ex.ref), None if ex.bound is None else np.where(g, 0.0, ex.bound), ex.T)
            for form, ex, use_b, use_dinv, use_dout in (("ax", ax, 0, 0, 0), ("resid", resid, 1, 0, 0), ("scaled", scaled, 0, 1, 0),
                                                        ("resid_dinv_out", resid, 1, 0, 1), ("ax_dinv_out", ax, 0, 0, 1)):
                expect = {7: masked(ex, 0.0)}
                if use_dout:
                    expect[8] = masked(inverse_expect(kind, dref), 1.0)
                out.append(Case(f"spmv lpr={lpr} n={n} {form} {'owned' if owned is not None else 'all'} {kind}", SPMV, n, kind,
                                ip=[lpr, n],
                                bufs=[(rowptr, 0), (colind, 0), (vals, 0), (x, 0), (dinv if use_dinv else None, 0),
                                      (b if use_b else None, 0), (owned, 0), (np.full(n, 99.0), 1),
                                      (np.full(n, 99.0) if use_dout else None, 1)],
                                expect=expect, meta=dict(meta, ghosts=owned is not None and bool((owned == 0).any()))))
    return out


AMG_AVG_ROWS = {24: 4, 25: 16, 128: 16, 129: 64}      # avg_row -> lanes per row launch_spmv picks


@functools.lru_cache(maxsize=None)
def amg_spmv_cases(avg_row, kind):
    lpr = AMG_AVG_ROWS[avg_row]
    rng = np.random.default_rng(200 + lpr + (kind == "real"))      # (avg_row 25 and 128: the same operators, on purpose)
    base = 333 if lpr < 64 else 523
    w = 3.0 if kind == "int" else 0.7371
    out = []
    for mode, (nr, ncol) in ((M_AX, (base, base + 150)), (M_PRE, (base, base)), (M_ADD, (base + 150, base)), (M_JAC, (base, base)),
                             (M_RES, (base, base))):
        rowptr, colind, vals, _ = make_csr(kind, rng, nr, ncol, edge_lengths(lpr))
        r_ = rows_of(rowptr)
        m = np.diff(rowptr)
        x, r, dinv, y0 = data(kind, rng, ncol), data(kind, rng, nr), data(kind, rng, nr, nonzero=True), data(kind, rng, nr)
        ar = np.arange(nr)
        cat = np.concatenate
        expect, bufs = {}, None
        sent = np.full(nr, 99.0)
        if mode == M_AX:
            expect[6] = summed(kind, nr, r_, vals, x[colind])
            bufs = [(x, 0), (None, 0), (None, 0), (sent, 1), (None, 0)]
        elif mode == M_ADD:
            expect[6] = summed(kind, nr, cat([r_, ar]), cat([vals, y0]), cat([x[colind], np.ones(nr)]), m=m)
            bufs = [(x, 0), (None, 0), (None, 0), (y0, 1), (None, 0)]
        elif mode == M_RES:
            expect[6] = summed(kind, nr, cat([r_, ar]), cat([-vals, r]), cat([x[colind], np.ones(nr)]), m=m)
            bufs = [(x, 0), (r, 0), (None, 0), (sent, 1), (None, 0)]
        elif mode == M_PRE:      # y = r - w A (dinv r), xout = w dinv r
            expect[6] = summed(kind, nr, cat([r_, ar]), cat([-w * np.ones(len(vals)), r]), cat([vals, np.ones(nr)]),
                               cat([dinv[colind], np.ones(nr)]), cat([r[colind], np.ones(nr)]), m=m)
            expect[7] = poly(kind, nr, [(w, dinv, r)])
            bufs = [(None, 0), (r, 0), (dinv, 0), (sent, 1), (sent, 1)]
        else:                    # y = x + w dinv (r - A x)
            wd = dinv[r_]
            expect[6] = summed(kind, nr, cat([r_, ar, ar]), cat([-w * np.ones(len(vals)), w * np.ones(nr), x]),
                               cat([wd, dinv, np.ones(nr)]), cat([vals, r, np.ones(nr)]), cat([x[colind], np.ones(nr), np.ones(nr)]),
                               m=m)
            bufs = [(x, 0), (r, 0), (dinv, 0), (sent, 1), (None, 0)]
        out.append(Case(f"amg_spmv mode={mode} avg_row={avg_row} {nr}x{ncol} {kind}", AMG_SPMV, nr, kind, ip=[mode, avg_row, ncol],
                        dp=[w], bufs=[(rowptr, 0), (colind, 0), (vals, 0)] + bufs, expect=expect,
                        meta=dict(lpr=lpr, mode=mode, shape=(nr, ncol), lengths=sorted(set(m.tolist())))))
    return out


# ---- block operators of the DG systems --------------------------------------------------------------------------------

BLOCK_SPMV_CONFIGS = ((8, 7, -1, "cell"), (8, 9, -1, "row"), (4, 5, -1, "cell"), (4, 6, -1, "row"), (3, 4, -1, "row"),
                      (8, 7, 0, "row"), (4, 5, 0, "row"))      # NV, nbmax, kernel asked for, kernel expected to run
BLOCK_CELLS = 37


def block_pattern(rng, cells, nbmax, counts):
    """bcol[cells][nbmax]: the cell itself and counts[c] - 1 others, increasing, -1 behind"""
    bcol = np.full((cells, nbmax), -1, np.int32)
    for c in range(cells):
        k = min(counts[c], cells)
        others = rng.choice(np.setdiff1d(np.arange(cells), [c]), size=k - 1, replace=False)
        bcol[c, :k] = np.sort(np.append(others, c))
    return bcol


@functools.lru_cache(maxsize=None)
def block_spmv_cases(nv, nbmax, kind):
    rng = np.random.default_rng(300 + 16 * nv + nbmax + (kind == "real"))
    cells = BLOCK_CELLS
    counts = [1 + c % nbmax for c in range(cells)]
    bcol = block_pattern(rng, cells, nbmax, counts)
    nsys = cells * nv
    out = []
    for systems in (1, 3):
        rows = systems * nsys
        lens = np.array([counts[(row % nsys) // nv] * nv for row in range(rows)])
        rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        vals = data(kind, rng, int(rowptr[-1]), nonzero=True)       # [row][block][NV]
        x, b = data(kind, rng, rows), data(kind, rng, rows)
        r_ = rows_of(rowptr)
        within = np.arange(len(vals)) - rowptr[r_]
        cl = (r_ % nsys) // nv
        col = (r_ // nsys) * nsys + bcol[cl, within // nv] * nv + within % nv
        ax = summed(kind, rows, r_, vals, x[col])
        resid = summed(kind, rows, np.concatenate([r_, np.arange(rows)]), np.concatenate([-vals, b]),
                       np.concatenate([x[col], np.ones(rows)]), m=lens)
        for kernel in sorted({k for (a, bm, k, _) in BLOCK_SPMV_CONFIGS if (a, bm) == (nv, nbmax)}):
            for use_b in (0, 1):
                for owned in (None, mask_of(rng, rows)):
                    ex = resid if use_b else ax
                    if owned is not None:
                        g = owned == 0
                        ex = Expect(np.where(g, 0.0, ex.ref), None if ex.bound is None else np.where(g, 0.0, ex.bound), ex.T)
                    out.append(Case(f"block_spmv nv={nv} nbmax={nbmax} kernel={kernel} systems={systems} b={use_b} "
                                    f"{'owned' if owned is not None else 'all'} {kind}", BLOCK_SPMV, rows, kind,
                                    ip=[nv, nbmax, nsys, kernel],
                                    bufs=[(rowptr, 0), (bcol.ravel(), 0), (vals, 0), (x, 0), (b if use_b else None, 0), (owned, 0),
                                          (np.full(rows, 99.0), 1)],
                                    expect={6: ex}, meta=dict(counts=sorted(set(counts)), padded=bool((bcol == -1).any()),
                                                              systems=systems, cells=cells)))
    return out


def unit_triangular_block(rng, bs):
    """B = L U with unit-diagonal triangular integer factors: elimination without pivoting meets only pivots of 1"""
    Lo = np.tril(rng.integers(-1, 2, size=(bs, bs)), -1) + np.eye(bs, dtype=np.int64)
    Up = np.triu(rng.integers(-1, 2, size=(bs, bs)), 1) + np.eye(bs, dtype=np.int64)
    return (Lo @ Up).astype(np.float64)


def spd_block(rng, bs):
    """symmetric positive definite, condition number <= 100, overall size anywhere in six decades"""
    Q, _ = np.linalg.qr(rng.standard_normal((bs, bs)))
    lam = 10.0 ** rng.uniform(0.0, 2.0, size=bs)
    return (Q * lam) @ Q.T * 10.0 ** rng.uniform(-3.0, 3.0)


def gauss_jordan(B, one, zero):
    """the kernel's elimination (amg_block_inv_kernel: no pivoting, row k scaled by 1 / pivot, then eliminated from every
    other row) on a list-of-lists copy of B in the arithmetic of `one`; returns (inverse, largest magnitude met)"""
    bs = len(B)
    m = [[B[i][j] for j in range(bs)] for i in range(bs)]
    inv = [[one if i == j else zero for j in range(bs)] for i in range(bs)]
    big = zero
    for k in range(bs):
        d = one / m[k][k]
        for j in range(bs):
            m[k][j] *= d
            inv[k][j] *= d
        for i in range(bs):
            if i == k:
                continue
            f = m[i][k]
            for j in range(bs):
                m[i][j] -= f * m[k][j]
                inv[i][j] -= f * inv[k][j]
                big = max(big, abs(m[i][j]), abs(inv[i][j]))
    return inv, big


def block_inverse_reference(kind, B):
    """-> (exact inverse rounded once, largest intermediate magnitude (int kind), error of the float64 restatement of the
    kernel's elimination relative to the largest entry of the exact inverse (real kind))"""
    bs = B.shape[0]
    exact, big = gauss_jordan([[Fraction(float(v)) for v in row] for row in B], Fraction(1), Fraction(0))
    ref = np.array([[float(v) for v in row] for row in exact])
    if kind == "int":
        assert all(v.denominator == 1 for row in exact for v in row)
        return ref, int(big), 0.0
    f64, _ = gauss_jordan([[np.float64(v) for v in row] for row in B], np.float64(1.0), np.float64(0.0))
    err = max(abs(Fraction(float(f64[i][j])) - exact[i][j]) for i in range(bs) for j in range(bs))
    return ref, None, float(err / max(abs(v) for row in exact for v in row))


BLOCK_INV_CELLS = (1, 63, 64, 65)
BLOCK_INV_MARGIN = 4.0      # device bound = margin x the measured error of the float64 restatement


@functools.lru_cache(maxsize=None)
def block_inv_cases(bs, kind):
    """-> (cases, measured relative error of the restatement over all real-valued blocks of this size)"""
    rng = np.random.default_rng(400 + bs + (kind == "real"))
    nbmax = 5
    layouts = [(nb, 1, nb) for nb in BLOCK_INV_CELLS] + [(66, 2, 33)]      # cells, systems, cells per system
    built = []
    measured = 0.0
    for nb, systems, cps in layouts:
        blocks = [unit_triangular_block(rng, bs) if kind == "int" else spd_block(rng, bs) for _ in range(nb)]
        refs = [block_inverse_reference(kind, B) for B in blocks]
        measured = max(measured, max(r[2] for r in refs))
        built.append((nb, systems, cps, blocks, refs))
    out = []
    for nb, systems, cps, blocks, refs in built:
        ref = np.array([r[0] for r in refs]).ravel()
        big = max((r[1] or 0) for r in refs)
        if kind == "int":
            ex = Expect(ref, None, np.array([float(big)]))
        else:
            per_block = np.array([BLOCK_INV_MARGIN * measured * np.abs(r[0]).max() for r in refs])
            ex = Expect(ref, np.repeat(per_block, bs * bs), None)
        # block structure known: rows [row][block][BS], the diagonal block at every position of the list in turn
        counts = [1 + (c % nbmax) for c in range(cps)]
        bcol = np.full((cps, nbmax), -1, np.int32)
        positions = set()
        for c in range(cps):
            k = min(counts[c], cps)
            pos = (c // nbmax) % k
            others = list(rng.choice(np.setdiff1d(np.arange(cps), [c]), size=k - 1, replace=False))
            bcol[c, :k] = others[:pos] + [c] + others[pos:]
            positions.add((k, pos))
        vals, rowptr = [], [0]
        for c in range(nb):
            cl = c % cps
            k = int((bcol[cl] >= 0).sum())
            pos = int(np.flatnonzero(bcol[cl] == cl)[0])
            for a in range(bs):
                row = data(kind, rng, k * bs, nonzero=True)
                row[pos * bs:(pos + 1) * bs] = blocks[c][a]
                vals.extend(row)
                rowptr.append(len(vals))
        meta = dict(bs=bs, nb=nb, systems=systems, positions=sorted(positions), measured=measured)
        out.append(Case(f"block_inv bs={bs} bcol nb={nb} systems={systems} {kind}", AMG_BLOCK_INV, nb, kind, ip=[bs, nbmax, cps],
                        bufs=[(np.array(rowptr, np.int32), 0), (None, 0), (np.array(vals), 0), (bcol.ravel(), 0),
                              (np.full(nb * bs * bs, 99.0), 1)], expect={4: ex}, meta=dict(meta, path="bcol")))
        # no block structure: the block's entries are found by their columns, anywhere in the row
        vals, colind, rowptr = [], [], [0]
        ncols = nb * bs + 40
        for c in range(nb):
            for a in range(bs):
                extra = int(rng.integers(0, 7))
                outside = rng.choice(np.setdiff1d(np.arange(ncols), np.arange(c * bs, c * bs + bs)), size=extra, replace=False)
                cols = np.concatenate([np.arange(c * bs, c * bs + bs), outside])
                v = np.concatenate([blocks[c][a], data(kind, rng, extra, nonzero=True)])
                p = rng.permutation(len(cols))
                colind.extend(int(q) for q in cols[p])
                vals.extend(v[p])
                rowptr.append(len(vals))
        out.append(Case(f"block_inv bs={bs} scan nb={nb} systems={systems} {kind}", AMG_BLOCK_INV, nb, kind, ip=[bs, 0, 1],
                        bufs=[(np.array(rowptr, np.int32), 0), (np.array(colind, np.int32), 0), (np.array(vals), 0), (None, 0),
                              (np.full(nb * bs * bs, 99.0), 1)], expect={4: ex}, meta=dict(meta, path="scan")))
    return out, measured


@functools.lru_cache(maxsize=None)
def block_apply_cases(bs, kind):
    rng = np.random.default_rng(500 + bs + (kind == "real"))
    cells = 65
    n = cells * bs
    w = 2.0 if kind == "int" else 0.6127
    binv, v, x = data(kind, rng, n * bs), data(kind, rng, n), data(kind, rng, n)
    i = np.repeat(np.arange(n), bs)
    vv = v[(i // bs) * bs + np.tile(np.arange(bs), n)]
    out = []
    for use_x in (0, 1):
        if use_x:
            ex = summed(kind, n, np.concatenate([i, np.arange(n)]), np.concatenate([w * np.ones(n * bs), x]),
                        np.concatenate([binv, np.ones(n)]), np.concatenate([vv, np.ones(n)]), m=bs)
        else:
            ex = summed(kind, n, i, w * np.ones(n * bs), binv, vv, m=bs)
        out.append(Case(f"block_apply bs={bs} x={use_x} {kind}", AMG_BLOCK_APPLY, n, kind, ip=[bs], dp=[w],
                        bufs=[(binv, 0), (v, 0), (x if use_x else None, 0), (np.full(n, 99.0), 1)], expect={3: ex}))
    return out


DENSE_SIZES = (1, 63, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def dense_cases(kind):
    rng = np.random.default_rng(600 + (kind == "real"))
    out = []
    layouts = [[s] for s in DENSE_SIZES] + [[DENSE_SIZES[(nb + k) % 5] for k in range(nb)] for nb in range(2, 9)]
    for sizes in layouts:
        nb, n = len(sizes), sum(sizes)
        start = np.concatenate([[0], np.cumsum(sizes)])[:-1]
        off = np.concatenate([[0], np.cumsum(np.square(sizes))])
        Minv, r = data(kind, rng, int(off[-1])), data(kind, rng, n)
        idx, rr = [], []
        for b, s in enumerate(sizes):
            idx.append(np.repeat(start[b] + np.arange(s), s))
            rr.append(np.tile(r[start[b]:start[b] + s], s))
        ex = summed(kind, n, np.concatenate(idx), Minv, np.concatenate(rr))
        pad = lambda a: list(a) + [0] * (8 - len(a))
        out.append(Case(f"dense sizes={sizes} {kind}", AMG_DENSE, n, kind, ip=[nb] + pad(start) + pad(sizes) + pad(off[:-1]),
                        bufs=[(Minv, 0), (r, 0), (np.full(n, 99.0), 1)], expect={2: ex}, meta=dict(sizes=sizes)))
    return out


# ---- reductions -------------------------------------------------------------------------------------------------------

def apply_dot_op_ref(sc, op, nd, v, d, scale):
    """apply_dot_op of kernels_krylov.hip on a copy of sc (float64 throughout)"""
    sc = np.array(sc, np.float64, copy=True)
    v0, v1, v2 = (np.float64(t) for t in v)

    def flag(bit):
        sc[S_FLAG] = float(int(sc[S_FLAG]) | bit)
    if op == OP_STORE3:
        sc[d[0]] = v0
        if nd > 1:
            sc[d[1]] = v1
        if nd > 2:
            sc[d[2]] = v2
    elif op == OP_MEAN:
        sc[S_MEAN] = v0 * np.float64(scale)
    elif op == OP_START:
        sc[S_RR], sc[S_BB], sc[S_FLAG] = v0, v1, 0.0
    elif op == OP_CG_INIT:
        sc[S_RHO], sc[S_RR] = v0, v1
        if nd > 2:
            sc[S_BB] = v2
    elif op == OP_CG_PAP:
        sc[S_PAP] = v0
        if v0 != 0.0:
            sc[S_ALPHA] = sc[S_RHO] / v0
        else:
            sc[S_ALPHA] = 0.0
            flag(F_PAP_ZERO)
    elif op == OP_CG_RHO:
        sc[S_BETA] = v0 / sc[S_RHO] if sc[S_RHO] != 0.0 else 0.0
        sc[S_RHO], sc[S_RR] = v0, v1
    elif op == OP_BI_RHO:
        if sc[S_RHO] != 0.0 and sc[S_OMEGA] != 0.0:
            sc[S_BETA] = (v0 / sc[S_RHO]) * (sc[S_ALPHA] / sc[S_OMEGA])
        else:
            sc[S_BETA] = 0.0
            flag(F_OMEGA_ZERO if sc[S_RHO] != 0.0 else F_RHO_ZERO)
        sc[S_RHO] = v0
    elif op == OP_BI_ALPHA:
        sc[S_RV] = v0
        if v0 != 0.0:
            sc[S_ALPHA] = sc[S_RHO] / v0
        else:
            sc[S_ALPHA] = 0.0
            flag(F_RV_ZERO)
    elif op == OP_BI_OMEGA:
        sc[S_TS], sc[S_TT] = v0, v1
        sc[S_OMEGA] = v0 / v1 if v1 != 0.0 else 0.0
    return sc


def dots_case(kind, rng, n, nd, op, d=(S_TS, S_PAP, S_RV), scale=1.0, preset=None, zero=(), red=False, tag="", vectors=None):
    """one launch of dots_kernel; preset: {slot: value} on top of the recognisable scalars; zero: the dot products made 0 (the
    first factor is the zero vector)"""
    if vectors is None:
        vectors = [data(kind, rng, n) for _ in range(2 * nd)]
    vectors = [np.zeros(n) if (k % 2 == 0 and k // 2 in zero) else a for k, a in enumerate(vectors)]
    sc = scalars(kind, rng)
    for k, val in (preset or {}).items():
        sc[k] = val
    exs = [summed(kind, 1, np.zeros(n, np.int64), vectors[2 * k], vectors[2 * k + 1], m=n) for k in range(nd)]
    v = [float(exs[k].ref[0]) if k < nd else 0.0 for k in range(3)]
    ref = apply_dot_op_ref(sc, op, nd, v, d, scale)
    T = np.array([max(float(e.T[0]) for e in exs)])
    expect = {}
    if kind == "int":
        expect[6] = Expect(ref, None, T)
    else:      # only the ops whose scalars ARE the dot products (times scale) are run on real-valued data
        assert op in (OP_STORE3, OP_MEAN, OP_START, OP_CG_INIT)
        bound = np.zeros(SC_LEN)
        slots = {OP_STORE3: list(d)[:nd], OP_MEAN: [S_MEAN], OP_START: [S_RR, S_BB], OP_CG_INIT: [S_RHO, S_RR, S_BB]}[op]
        for k, s in enumerate(slots[:nd]):
            bound[s] = float(exs[k].bound[0]) * (abs(scale) if op == OP_MEAN else 1.0)
        expect[6] = Expect(ref, bound, T)
    bufs = [(vectors[k] if k < 2 * nd else None, 0) for k in range(6)] + [(sc, 1)]
    if red:      # the rank's sums go to red[0..2]; the scalar algebra follows from there
        rref = np.array(v)
        expect[7] = Expect(rref, None if kind == "int" else np.array([float(exs[k].bound[0]) if k < nd else 0.0 for k in range(3)]), T)
        bufs.append((np.full(3, 77.0), 1))
    else:
        bufs.append((None, 0))
    return Case(f"dots n={n} nd={nd} op={op} {'red ' if red else ''}{tag}{kind}", DOTS, n, kind,
                ip=[nd, op, d[0], d[1], d[2], 1 if red else 0], dp=[scale], bufs=bufs, expect=expect,
                meta=dict(n=n, nd=nd, op=op, red=red, tag=tag))


@functools.lru_cache(maxsize=None)
def dots_cases(kind):
    rng = np.random.default_rng(700 + (kind == "real"))
    out = []
    for n in DOT_SIZES:
        if kind == "real" and n > 12293:
            continue      # (integer data at the size where the block cap binds)
        vectors = [data(kind, rng, n) for _ in range(6)]
        for nd in (1, 2, 3):
            out.append(dots_case(kind, rng, n, nd, OP_STORE3, vectors=vectors[:2 * nd]))
    ops = [(OP_STORE3, 3), (OP_MEAN, 1), (OP_START, 2), (OP_CG_INIT, 2), (OP_CG_INIT, 3)]
    if kind == "int":
        ops += [(OP_CG_PAP, 1), (OP_CG_RHO, 2), (OP_BI_RHO, 1), (OP_BI_ALPHA, 1), (OP_BI_OMEGA, 2)]
    for n in (257, 4097):
        for op, nd in ops:
            out.append(dots_case(kind, rng, n, nd, op, scale=0.25 if op == OP_MEAN else 1.0, preset={S_FLAG: float(F_RV_ZERO)}))
            out.append(dots_case(kind, rng, n, nd, op, scale=0.25 if op == OP_MEAN else 1.0, preset={S_FLAG: float(F_RV_ZERO)},
                                 red=True))
    if kind == "int":      # every breakdown branch, on top of bits already set; without and through red
        for red in (False, True):
            for tag, op, nd, preset, zero, _bit in BREAKDOWNS:
                out.append(dots_case(kind, rng, 257, nd, op, preset=preset, zero=zero, red=red, tag=tag + " "))
    return out


BREAKDOWNS = (
    ("pap_zero", OP_CG_PAP, 1, {S_FLAG: float(F_RV_ZERO)}, (0,), F_PAP_ZERO),
    ("rho_zero", OP_BI_RHO, 1, {S_FLAG: float(F_PAP_ZERO), S_RHO: 0.0}, (), F_RHO_ZERO),
    ("omega_zero", OP_BI_RHO, 1, {S_FLAG: float(F_RHO_ZERO), S_OMEGA: 0.0}, (), F_OMEGA_ZERO),
    ("rv_zero", OP_BI_ALPHA, 1, {S_FLAG: float(F_OMEGA_ZERO)}, (0,), F_RV_ZERO),
    ("tt_zero", OP_BI_OMEGA, 2, {S_FLAG: float(F_PAP_ZERO)}, (1,), 0),
    ("cg_rho_zero", OP_CG_RHO, 2, {S_FLAG: float(F_PAP_ZERO), S_RHO: 0.0}, (), 0),
)


# ---- vector updates ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def vec_cases(kind):
    rng = np.random.default_rng(800 + (kind == "real"))
    out = []
    for n in VEC_SIZES:
        for op in range(9):
            sc = scalars(kind, rng)
            a, b, c, d = (data(kind, rng, n) for _ in range(4))
            al, be, om, mean = sc[S_ALPHA], sc[S_BETA], sc[S_OMEGA], sc[S_MEAN]
            eb = same(b)
            if op == V_RESID: ea = poly(kind, n, [(c,), (-d,)])
            elif op == V_SHIFT: ea = poly(kind, n, [(a,), (-mean,)])
            elif op == V_CG_XR: ea, eb = poly(kind, n, [(a,), (al, c)]), poly(kind, n, [(b,), (-al, d)])
            elif op == V_CG_P: ea = poly(kind, n, [(c,), (be, a)])
            elif op == V_JACOBI: ea = poly(kind, n, [(c, d)])
            elif op == V_BI_P: ea = poly(kind, n, [(c,), (be, a), (-be, om, d)])
            elif op == V_BI_S: ea = poly(kind, n, [(c,), (-al, d)])
            elif op == V_COPY: ea = same(c)
            else: ea = poly(kind, n, [(c,), (-mean,)])
            out.append(Case(f"vec op={op} n={n} {kind}", VEC, n, kind, ip=[op],
                            bufs=[(sc, 1), (a, 1), (b, 1), (c, 1), (d, 1)],
                            expect={0: same(sc), 1: ea, 2: eb, 3: same(c), 4: same(d)}, meta=dict(op=op, n=n)))
        for use_dinv in (0, 1):
            sc = scalars(kind, rng)
            x, r, p, s, sres, t, dinv = (data(kind, rng, n) for _ in range(7))
            al, om = sc[S_ALPHA], sc[S_OMEGA]
            ex = poly(kind, n, [(x,), (al, p, dinv), (om, s, dinv)] if use_dinv else [(x,), (al, p), (om, s)])
            out.append(Case(f"bicg_update dinv={use_dinv} n={n} {kind}", BICG_UPDATE, n, kind,
                            bufs=[(sc, 1), (x, 1), (r, 1), (p, 1), (s, 1), (sres, 1), (t, 1), (dinv if use_dinv else None, 0)],
                            expect={0: same(sc), 1: ex, 2: poly(kind, n, [(sres,), (-om, t)]), 3: same(p), 4: same(s), 5: same(sres),
                                    6: same(t)}, meta=dict(n=n)))
        sc = scalars(kind, rng)
        ref = sc.copy()
        ref[:S_N] = 0.0
        ref[[S_RHO, S_ALPHA, S_OMEGA]] = 1.0
        out.append(Case(f"bicg_init n={n} {kind}", BICG_INIT, n, kind, bufs=[(data(kind, rng, n), 1), (data(kind, rng, n), 1), (sc, 1)],
                        expect={0: same(np.zeros(n)), 1: same(np.zeros(n)), 2: same(ref)}, meta=dict(n=n)))
        owned = mask_of(rng, n)
        for as_ones in (0, 1):
            a = data(kind, rng, n, nonzero=True)
            ref = owned.astype(np.float64) if as_ones else np.where(owned == 1, a, 0.0)
            out.append(Case(f"mask as_ones={as_ones} n={n} {kind}", MASK, n, kind, ip=[as_ones], bufs=[(owned, 0), (a, 1)],
                            expect={1: same(ref)}, meta=dict(n=n)))
        rowptr, colind, vals, where = make_csr(kind, rng, n, n, [0, 1, 2, 3, 5, 9])
        r_ = rows_of(rowptr)
        ghost = (owned == 0)[r_]
        out.append(Case(f"ghost_identity n={n} {kind}", GHOST_IDENTITY, n, kind, bufs=[(rowptr, 0), (colind, 0), (owned, 0), (vals, 1)],
                        expect={3: same(np.where(ghost, (colind == r_).astype(np.float64), vals))}, meta=dict(n=n)))
        out.append(Case(f"diag_inv n={n} {kind}", DIAG_INV, n, kind, bufs=[(rowptr, 0), (colind, 0), (vals, 0), (np.full(n, 99.0), 1)],
                        expect={3: inverse_expect(kind, diag_inverse(rowptr, colind, vals))},
                        meta=dict(n=n, where=sorted({w for w, _ in where}))))
    return out


@functools.lru_cache(maxsize=None)
def shift_extrapolate_cases(kind):
    rng = np.random.default_rng(900 + (kind == "real"))
    out = []
    for n in (1, 257):
        for stride in (1, 5):
            sc = scalars(kind, rng)
            src, dst = data(kind, rng, n), data(kind, rng, n * stride)
            ref, bound = dst.copy(), np.zeros(n * stride)
            ex = poly(kind, n, [(src,), (-sc[S_MEAN],)])
            ref[::stride] = ex.ref
            if ex.bound is not None:
                bound[::stride] = ex.bound
            out.append(Case(f"scatter_shift n={n} stride={stride} {kind}", SCATTER_SHIFT, n, kind, ip=[stride],
                            bufs=[(src, 0), (dst, 1), (sc, 1)],
                            expect={1: Expect(ref, None if kind == "int" else bound, ex.T), 2: same(sc)}, meta=dict(stride=stride)))
            for have in (0, 1, 2, 3):
                for use_old2 in (0, 1):
                    cur, old, old2 = data(kind, rng, n * stride), data(kind, rng, n), data(kind, rng, n)
                    c = cur[::stride].copy()
                    if have >= 2 and use_old2: ex = poly(kind, n, [(3.0, c), (-3.0, old), (old2,)])
                    elif have >= 1: ex = poly(kind, n, [(2.0, c), (-old,)])
                    else: ex = Expect(c, None if kind == "int" else np.zeros(n), np.abs(c))
                    ref, bound = cur.copy(), np.zeros(n * stride)
                    ref[::stride] = ex.ref
                    if ex.bound is not None:
                        bound[::stride] = ex.bound
                    expect = {0: Expect(ref, None if kind == "int" else bound, ex.T), 1: same(c)}
                    if use_old2:
                        expect[2] = same(old)
                    out.append(Case(f"extrapolate n={n} stride={stride} have={have} old2={use_old2} {kind}", EXTRAPOLATE, n, kind,
                                    ip=[stride, have], bufs=[(cur, 1), (old, 1), (old2 if use_old2 else None, 1)], expect=expect,
                                    meta=dict(stride=stride, have=have, old2=use_old2)))
    return out


KNP_SUBDOMAINS = ([7], [300, 41], [130, 0, 211])


def knp_block_index(ks, voff, k, g):
    """kernels_krylov.hip: x[ks v0 + k nv + (g - v0)] <-> csol[k ntot + g], (v0, nv) the sub-domain of vertex g"""
    sd = max(s for s in range(len(voff) - 1) if voff[s] <= g < voff[s + 1])
    v0, nv = voff[sd], voff[sd + 1] - voff[sd]
    return ks * v0 + k * nv + (g - v0)


@functools.lru_cache(maxsize=None)
def knp_order_cases():
    out = []
    for ks in (2, 3, 4):
        for sizes in KNP_SUBDOMAINS:
            voff = [0] + list(np.cumsum(sizes))
            ntot = voff[-1]
            perm = np.array([knp_block_index(ks, voff, k, g) for k in range(ks) for g in range(ntot)])
            assert sorted(perm.tolist()) == list(range(ks * ntot))
            csol = np.arange(ks * ntot, dtype=np.float64) + 1000.0
            x = -(np.arange(ks * ntot, dtype=np.float64) + 1.0)
            xb = x.copy()
            xb[perm] = csol
            for to_blocks, ex in ((1, {0: same(xb), 1: same(csol)}), (0, {0: same(x), 1: same(x[perm])})):
                out.append(Case(f"knp_order ks={ks} sizes={sizes} to_blocks={to_blocks}", KNP_ORDER, ntot, "int",
                                ip=[ks, len(sizes), to_blocks] + voff, bufs=[(x, 1), (csol, 1)], expect=ex,
                                meta=dict(ks=ks, sizes=list(sizes), perm=perm)))
    return out


# ---- coarse space of the distributed preconditioner -------------------------------------------------------------------

COARSE_LISTS = {1: ([0], [1], [255], [256], [257], [700]), 3: ([0, 255, 700], [257, 1, 256])}


@functools.lru_cache(maxsize=None)
def coarse_cases(kind):
    rng = np.random.default_rng(1000 + (kind == "real"))
    out = []
    n = 1500
    for nl in (1, 3):
        for world, rank in ((1, 0), (3, 0), (3, 2)):
            nc = world * nl
            for sizes in COARSE_LISTS[nl]:
                ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
                idx = rng.integers(0, n, size=int(ptr[-1])).astype(np.int32)
                wt, r = data(kind, rng, int(ptr[-1])), data(kind, rng, n)
                red = np.full(KN_COARSE_OFF + nc, np.nan)
                red[:KN_COARSE_OFF] = data(kind, rng, KN_COARSE_OFF, nonzero=True)
                ex = summed(kind, nl, rows_of(ptr), wt, r[idx])
                ref, bound = np.zeros(KN_COARSE_OFF + nc), np.zeros(KN_COARSE_OFF + nc)
                ref[:KN_COARSE_OFF] = red[:KN_COARSE_OFF]
                at = KN_COARSE_OFF + rank * nl
                ref[at:at + nl] = ex.ref
                if ex.bound is not None:
                    bound[at:at + nl] = ex.bound
                out.append(Case(f"coarse_restrict nl={nl} world={world} rank={rank} lists={sizes} {kind}", COARSE_RESTRICT, n, kind,
                                ip=[nl, rank, world], bufs=[(r, 0), (ptr, 0), (idx, 0), (wt, 0), (red, 1)],
                                expect={4: Expect(ref, None if kind == "int" else bound, ex.T)},
                                meta=dict(nl=nl, world=world, rank=rank, sizes=list(sizes))))
            inv, red = data(kind, rng, nc * nc), data(kind, rng, KN_COARSE_OFF + nc)
            rows = (rank * nl + np.repeat(np.arange(nl), nc)) * nc + np.tile(np.arange(nc), nl)
            ex = summed(kind, nl, np.repeat(np.arange(nl), nc), inv[rows], np.tile(red[KN_COARSE_OFF:], nl))
            zc = np.full(nl + 1, 55.0)
            out.append(Case(f"coarse_solve nl={nl} world={world} rank={rank} {kind}", COARSE_SOLVE, nl, kind, ip=[rank, nc],
                            bufs=[(inv, 0), (red, 0), (zc, 1)],
                            expect={2: Expect(np.append(ex.ref, 55.0), None if ex.bound is None else np.append(ex.bound, 0.0), ex.T)},
                            meta=dict(nl=nl, world=world, rank=rank)))
        # prolongation: ghosts (-1), weights that are exactly 0 under a NaN in the upper node's entry
        for m in (257, 1000):
            nz = nl + 1
            zc = np.append(data(kind, rng, nl), np.nan)      # what coarse_solve_kernel never writes
            agg_of = rng.integers(-1, nl, size=m).astype(np.int32)
            w = rng.integers(0, 4, size=m).astype(np.float64) if kind == "int" else np.where(rng.random(m) < 0.3, 0.0, rng.random(m))
            w[agg_of == nl - 1] = 0.0
            z = data(kind, rng, m)
            live = agg_of >= 0
            a = np.where(live, agg_of, 0)
            zlo, zhi = zc[a], np.where(w > 0.0, np.nan_to_num(zc[np.minimum(a + 1, nl)]), 0.0)
            lv = live.astype(np.float64)
            ex = poly(kind, m, [(z,), (lv, zlo), (-lv, w, zlo), (lv, w, zhi)])
            out.append(Case(f"coarse_prolong mode=0 nl={nl} n={m} {kind}", COARSE_PROLONG, m, kind, ip=[0, 0, nz],
                            bufs=[(agg_of, 0), (w, 0), (zc, 0), (z, 1)], expect={3: ex},
                            meta=dict(nl=nl, ghosts=int((~live).sum()), zero_w_under_nan=int(((agg_of == nl - 1)).sum()))))
            for pick in (0, nl, -2):
                one_minus = poly(kind, m, [(1.0,), (-w,)])
                ref = np.where(~live, 0.0, np.where(agg_of == pick, one_minus.ref, np.where(agg_of + 1 == pick, w, 0.0)))
                bound = None if kind == "int" else np.where(live & (agg_of == pick), one_minus.bound, 0.0)
                out.append(Case(f"coarse_prolong mode=1 pick={pick} nl={nl} n={m} {kind}", COARSE_PROLONG, m, kind, ip=[1, pick, 0],
                                bufs=[(agg_of, 0), (w, 0), (None, 0), (z, 1)], expect={3: Expect(ref, bound, one_minus.T)},
                                meta=dict(nl=nl)))
    return out


def all_cases():
    """every case of every kernel, both kinds (built once per process)"""
    out = []
    for kind in KINDS:
        for lpr in (4, 16):
            out += spmv_cases(lpr, kind)
        for avg in AMG_AVG_ROWS:
            out += amg_spmv_cases(avg, kind)
        for nv, nbmax in sorted({(a, b) for a, b, _, _ in BLOCK_SPMV_CONFIGS}):
            out += block_spmv_cases(nv, nbmax, kind)
        for bs in (3, 4, 8):
            out += block_inv_cases(bs, kind)[0]
            out += block_apply_cases(bs, kind)
        out += dense_cases(kind) + dots_cases(kind) + vec_cases(kind) + shift_extrapolate_cases(kind) + coarse_cases(kind)
    return out + knp_order_cases()
