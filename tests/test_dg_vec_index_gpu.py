"""knpemi_dg_vec_gather / knpemi_dg_vec_scatter -- the ghost refresh of a solver vector inside the halo hook of a cell
partition (knpemi.dg.DGSlab.enable_solves) -- and the lifetime of the solver state a DG handle owns.

Meshes: dg_cases.make_mesh(2, M, membrane=True) with M = 2, the smallest it builds (8 triangles, 24 dofs; the tagged box
[0.25, 0.75]^2 holds no cell centre there, so that problem has no membrane facet), and M = 4, the smallest that does have
membrane facets (32 triangles, 8 of them inside, 8 facets)."""
import ctypes as C

import numpy as np
import pytest

import dg_cases
from knpemi import _lib as L

pytestmark = pytest.mark.gpu

SIZES = [2, 4]


class Dev:
    """Device copies of host arrays through the HIP runtime (blocking copies: done when they return)."""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.held = []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
        assert self.hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
        self.held.append(p)
        return p

    def get(self, p, like):
        out = np.empty_like(like)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), p, C.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self):
        assert self.hip.hipDeviceSynchronize() == 0                 # fails if anything left a device error behind
        for p in self.held:
            assert self.hip.hipFree(p) == 0
        self.held = []


def _problem(M):
    from knpemi.dg import DGProblem
    mesh, ct, mem_facets, mem_tags = dg_cases.make_mesh(2, M, True)
    ft = np.zeros(len(mesh.facets), np.int32)                       # dense facet tags from the membrane's facet list
    key = {tuple(sorted(f)): i for i, f in enumerate(mesh.facets.tolist())}
    for f, t in zip(mem_facets.tolist(), mem_tags):
        ft[key[tuple(sorted(f))]] = t
    dp = DGProblem(mesh, ct, ft, [0, 1], [1])
    assert dp.nmf == len(mem_facets) == (0 if M == 2 else 8)
    return dp


def _assembled(M):
    """A problem with parameters, smooth fields and the potential system assembled."""
    dp = _problem(M)
    rng = np.random.default_rng(3)
    shape, mshape = (dp.n_cells, dp.nv), (dp.nmf, dp.nf)
    smooth = lambda a, b: a + b * np.cos(3.0 * dp.X[:, :, 0] + 1.0) * np.sin(2.0 * dp.X[:, :, 1] + 0.5)
    dp.set_params(dict(dt=0.05, F=1.0, psi=1.0, C_M=1.0), [dict(z=z, D=[1.0, 0.7]) for z in (1.0, -1.0, 1.0)])
    for k in range(3):
        dp.set_concentration(k, smooth(2.0 + k, 0.4))
        dp.set_channel_current(k, 0.3 * rng.standard_normal(mshape))
    dp.set_potential(smooth(0.1, 0.3))
    dp.set_membrane_potential(0.2 + 0.1 * rng.random(mshape))
    dp.assemble_emi()
    return dp


@pytest.mark.parametrize("M", SIZES)
def test_dg_vec_gather_scatter_round_trip(hip_lib, M):
    """Gather then scatter into a zeroed vector reproduces exactly the listed entries (some listed twice, in no order)
    and leaves every other entry zero."""
    dp, dev = _problem(M), Dev()
    n = dp.n
    vec = np.random.default_rng(M).standard_normal(n)
    idx = np.array([n - 1, 3, 0, 7, 3, n // 2, n - 1, 11], np.int32)
    assert idx.min() >= 0 and idx.max() < n
    d_vec, d_idx = dev.put(vec), dev.put(idx)
    d_buf, d_out = dev.put(np.full(len(idx), np.nan)), dev.put(np.zeros(n))
    L.check(hip_lib.knpemi_dg_vec_gather(dp.h, d_vec, d_idx, len(idx), d_buf))
    L.check(hip_lib.knpemi_dg_vec_scatter(dp.h, d_out, d_idx, len(idx), d_buf))
    L.check(hip_lib.knpemi_dg_sync(dp.h))
    assert np.array_equal(dev.get(d_buf, vec[idx]), vec[idx])
    want = np.zeros(n)
    want[idx] = vec[idx]
    assert np.array_equal(dev.get(d_out, want), want)
    assert np.array_equal(dev.get(d_vec, vec), vec)                 # the gather's source is untouched
    dev.free()


def test_dg_vec_index_argument_checks(hip_lib):
    dp, dev = _problem(2), Dev()
    vec, buf = np.arange(dp.n, dtype=np.float64), np.full(4, -1.0)
    v, i, b = dev.put(vec), dev.put(np.zeros(4, np.int32)), dev.put(buf)
    for name in ("knpemi_dg_vec_gather", "knpemi_dg_vec_scatter"):
        fn = getattr(hip_lib, name)
        # n == 0: nothing to do, whatever the pointers are
        assert fn(dp.h, v, i, 0, b) == L.OK and fn(dp.h, None, None, 0, None) == L.OK
        for args in ((None, v, i, 4, b), (dp.h, v, i, -1, b), (dp.h, None, i, 4, b), (dp.h, v, None, 4, b), (dp.h, v, i, 4, None)):
            assert fn(*args) == L.EINVAL, (name, args)
            assert name.encode() + b":" in hip_lib.knpemi_last_error(), (name, args)
    L.check(hip_lib.knpemi_dg_sync(dp.h))
    assert np.array_equal(dev.get(b, buf), buf) and np.array_equal(dev.get(v, vec), vec)   # none of these launched anything
    dev.free()


def _mark(hip_lib):
    """A failure of our own as the last error: whatever fails afterwards replaces it."""
    assert hip_lib.knpemi_dg_vec_gather(None, None, None, 0, None) == L.EINVAL
    mark = hip_lib.knpemi_last_error()
    assert mark.startswith(b"knpemi_dg_vec_gather:")
    return mark


def _destroy(hip_lib, dp):
    h, dp.h = dp.h, None
    hip_lib.knpemi_dg_destroy(h)


@pytest.mark.parametrize("M", SIZES)
def test_dg_handle_lifetimes_leave_no_error(hip_lib, M):
    """Create and destroy without a solve, with a solve of the potential system, and with the single-rank form of
    knpemi_dg_set_distributed: no call fails, nothing is left in knpemi_last_error, the device is healthy afterwards."""
    mark = _mark(hip_lib)
    _destroy(hip_lib, _problem(M))                                  # the solver was never set up
    assert hip_lib.knpemi_last_error() == mark
    dp = _assembled(M)
    its, rr = dp.solve_emi(rtol=1e-9)
    assert 0 < its < 100 and rr <= 1e-9, (its, rr)
    phi = dp.get_potential()
    assert np.isfinite(phi).all() and abs(phi.mean()) < 1e-12 * np.abs(phi).max()
    _destroy(hip_lib, dp)
    assert hip_lib.knpemi_last_error() == mark
    dp = _problem(M)
    L.check(hip_lib.knpemi_dg_set_distributed(dp.h, None, None, None, None, None))
    _destroy(hip_lib, dp)
    assert hip_lib.knpemi_last_error() == mark
    Dev().free()                                                    # (the device is still in order)
