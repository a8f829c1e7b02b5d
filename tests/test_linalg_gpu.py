"""The kernels of the device solves one by one (csrc/kernels_krylov.hip, csrc/block_spmv.h, the device half of
csrc/kernels_amg.hip), each run alone through knpemi_debug_linalg -- with the launch helper the solves call, so grid, lanes
per row and kernel choice are the solver's -- and held to a plain reference of the same operation (tests/linalg_cases.py):
exact equality on integer-valued data, the a priori bound (m + 4) 2^-53 sum |a_j| |x_j| on real-valued data.  A whole
solve is a poor detector for these kernels: Krylov iterations correct themselves, and the bit-for-bit tests compare the
code with itself.

The real-valued block inverse has no a priori bound without the condition number; its bound is measured on the CPU
(tests/test_linalg_host.py): the float64 restatement of the kernel's elimination against the exact inverse of SPD blocks of
condition number <= 100 gives 2.04e-15 (blocks of 3), 2.24e-15 (4), 2.51e-15 (8) of the inverse's largest entry, and the device
gets 4 times that (contraction, 1 / d multiplied instead of divided by).

The fused kernels of kernels_fused.hip are not covered here."""
import numpy as np
import pytest

import linalg_cases as lc

pytestmark = pytest.mark.gpu


def run(hip_lib, cases):
    from knpemi import _lib as L
    assert cases
    worst = 0.0
    for case in cases:
        rc, outs = lc.call(hip_lib, case)
        L.check(rc)
        worst = max(worst, lc.check(case, outs))
    print(f"{len(cases)} cases, largest error / bound = {worst:.3f}")


@pytest.mark.parametrize("kind", lc.KINDS)
@pytest.mark.parametrize("lpr", (4, 16))
def test_spmv_kernel(hip_lib, lpr, kind):
    """spmv_kernel<SCALED, LPR>: y = A x, b - A x, A (x .* dinv), the inverse diagonal as a by-product, ghost rows"""
    run(hip_lib, lc.spmv_cases(lpr, kind))


@pytest.mark.parametrize("kind", lc.KINDS)
@pytest.mark.parametrize("avg_row", sorted(lc.AMG_AVG_ROWS))
def test_amg_spmv_kernel(hip_lib, avg_row, kind):
    """amg_spmv_kernel<MODE, LPR>, all five modes through launch_spmv<MODE> at the avg_row thresholds of 4 / 16 / 64 lanes"""
    run(hip_lib, lc.amg_spmv_cases(avg_row, kind))


@pytest.mark.parametrize("kind", lc.KINDS)
@pytest.mark.parametrize("nv,nbmax", sorted({(a, b) for a, b, _, _ in lc.BLOCK_SPMV_CONFIGS}))
def test_block_spmv_kernels(hip_lib, nv, nbmax, kind):
    """block_spmv_cell_kernel<8,7>, <4,5> and block_spmv_kernel<8,16>, <4,4>, <3,4>, each selected by launch_block_spmv
    itself, and the row kernel forced where the cell kernel is the default"""
    run(hip_lib, lc.block_spmv_cases(nv, nbmax, kind))


@pytest.mark.parametrize("kind", lc.KINDS)
def test_dots_kernel_and_scalar_steps(hip_lib, kind):
    """dots_kernel + apply_dot_op at every size class of the grid, every op with the scalars preset, every breakdown
    branch, and the same through red[] and dots_apply_kernel; the whole sc[] is compared"""
    run(hip_lib, lc.dots_cases(kind))


def test_dots_back_to_back_on_one_scratch(hip_lib):
    """every size back to back on the one scratch buffer, five times over: the ticket is reset, partial sums left by a
    larger grid are not read by a smaller one, and the bits are the same every time"""
    from knpemi import _lib as L
    cases = [[c for c in lc.dots_cases("real" if n <= 12293 else "int") if c.meta["n"] == n and c.meta["nd"] == 3][0]
             for n in lc.DOT_SIZES]
    first = None
    for _ in range(5):
        bits = []
        for case in cases:
            rc, outs = lc.call(hip_lib, case)
            L.check(rc)
            lc.check(case, outs)
            bits.append(outs[6].view(np.int64).copy())
        if first is None:
            first = bits
        for a, b in zip(first, bits):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("kind", lc.KINDS)
def test_vector_kernels(hip_lib, kind):
    """vec_kernel (nine ops), bicg_update_kernel, bicg_init_kernel, mask_kernel, ghost_identity_kernel, diag_inv_kernel;
    what a kernel must leave alone is compared too"""
    run(hip_lib, lc.vec_cases(kind))


@pytest.mark.parametrize("kind", lc.KINDS)
def test_scatter_shift_and_extrapolate_kernels(hip_lib, kind):
    """strides 1 and 5, have 0 .. 3, old2 null and given; cur, old and old2 after the call"""
    run(hip_lib, lc.shift_extrapolate_cases(kind))


def test_knp_order_kernel(hip_lib):
    """both directions against the index formula in the kernel's comment, and the round trip"""
    from knpemi import _lib as L
    cases = lc.knp_order_cases()
    run(hip_lib, cases)
    for case in cases:
        if case.ip[2] != 1:
            continue
        rc, outs = lc.call(hip_lib, case)
        L.check(rc)
        back = lc.Case(case.name + " and back", lc.KNP_ORDER, case.n, "int", ip=[case.ip[0], case.ip[1], 0] + case.ip[3:],
                       bufs=[(outs[0], 1), (np.full(len(outs[1]), -7.0), 1)], expect={1: lc.same(case.bufs[1][0])})
        rc, outs2 = lc.call(hip_lib, back)
        L.check(rc)
        lc.check(back, outs2)


@pytest.mark.parametrize("kind", lc.KINDS)
def test_coarse_space_kernels(hip_lib, kind):
    """coarse_restrict_kernel (other ranks' entries zeroed over garbage), coarse_solve_kernel, coarse_prolong_kernel (both
    modes, ghosts, a NaN behind every weight that is exactly 0)"""
    run(hip_lib, lc.coarse_cases(kind))


@pytest.mark.parametrize("kind", lc.KINDS)
@pytest.mark.parametrize("bs", (3, 4, 8))
def test_amg_block_inv_kernel(hip_lib, bs, kind):
    """amg_block_inv_kernel<BS>: the diagonal block from the block list (every position) and from the columns; partial lane
    groups; two stacked systems.  Integer blocks L U exactly; SPD blocks within 4 x the measured error of the float64
    restatement of the elimination (see the module's docstring)"""
    run(hip_lib, lc.block_inv_cases(bs, kind)[0])


@pytest.mark.parametrize("kind", lc.KINDS)
def test_amg_block_apply_and_dense_kernels(hip_lib, kind):
    """amg_block_apply_kernel<3, 4, 8> with and without x; amg_dense_kernel on one to eight blocks of 1 .. 130 unknowns"""
    run(hip_lib, [c for bs in (3, 4, 8) for c in lc.block_apply_cases(bs, kind)] + lc.dense_cases(kind))
