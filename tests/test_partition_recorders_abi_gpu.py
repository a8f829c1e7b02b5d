"""GPU tests of knpemi_flux_set_partitioned and knpemi_exchange_set_partitioned in one process: no communicator, a no-op
callback serves as the all-reduce hook, so a record is launch, (nothing), combine.

What is compared with what.  The kernel evaluates an item's term with its own arithmetic (cofactors and fused
multiply-adds), IonFluxes.compute_host with numpy's (an LU solve): the two agree to helpers.TOL, as in test_flux_gpu.py
and test_exchange_gpu.py, never bit for bit.  Bit for bit -- and within the derived bound for sums -- is what the device
gives against ITSELF, the plain recorder on the same handle, whose per-item terms are the same bits:
  * mask of all items, world 1: the row IS the plain row, sums included (the fold takes the same workgroup order and the
    combine adds the one slot to 0);
  * masks of every third item, offsets 0, 1, 2: the three maxima maximise to the plain maximum bit for bit; the three
    sums add up to the plain sum within 2 n 2^-53 sum |term| (n numbers added in two orders, each within
    (n - 1) 2^-53 sum |term| of the exact sum; sum |term| from the host's per-item fields times volumes / areas); each
    row equals compute_host(recorded=mask) to TOL;
  * a mask that is zero on one watch: that watch's columns are exactly 0, the others the plain row's bits;
  * the per-item fields equal the plain record's bit for bit under every mask, the masked-out items included."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import exchange_cases as xc
import test_partition_fluxes_host as ph
from helpers import TOL
from knpemi import IonFluxes, exchange, fluxes
from knpemi import _lib as L

pytestmark = pytest.mark.gpu

SETUPS = ("2d", "tet", "hex", "three")
KINDS = ("flux", "exchange")
NOOP = L.ALLREDUCE_FN(lambda ctx, n: 0)


@functools.lru_cache(maxsize=None)
def _hip():
    """The HIP runtime the library has loaded (its path from the process's map), for the exchange buffer."""
    with open("/proc/self/maps") as maps:
        path = next(line.split()[-1] for line in maps if "libamdhip64.so" in line)
    hip = C.CDLL(path)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


class DeviceBuffer:
    """n doubles of device memory, filled with 7 (knpemi_*_set_partitioned must zero them)."""

    def __init__(self, n):
        self.n, self.ptr, self.free = n, C.c_void_p(), _hip().hipFree
        assert _hip().hipMalloc(C.byref(self.ptr), 8 * n) == 0
        fill = np.full(n, 7.0)
        assert _hip().hipMemcpy(self.ptr, fill.ctypes.data, 8 * n, 1) == 0      # host to device

    def data_ptr(self):
        return self.ptr.value

    def host(self):
        out = np.empty(self.n)
        assert _hip().hipMemcpy(out.ctypes.data, self.ptr, 8 * self.n, 2) == 0      # device to host
        return out

    def __del__(self):
        self.free(self.ptr)


class Recorder:
    """One recorder kind on a handle, through the C ABI."""

    def __init__(self, kind, s, dp):
        self.kind, self.s, self.dp, self.lib = kind, s, dp, dp.lib
        if kind == "flux":
            self.rec = IonFluxes(s.subdomain_list, s.ion_list, s.physical_parameters)
            for tag in s.subdomain_list:
                self.rec.watch(tag)
            self.count = self.rec.n_cells
        else:
            self.rec = xc.exchange(s)
            self.count = self.rec.n_facets
        self.tags = list(self.rec.watched)
        self.sub = np.array([dp.sub_index[t] for t in self.tags], np.int32)
        self.mask = np.array([self.rec.mask(t) for t in self.tags], np.int32)
        self.n_cols = self.rec.n_cols
        self.rec._dev = (dp.lib, dp.h, dict(dp.sub_index))      # fields() reads whichever table the handle holds
        self.xbuf = None

    def fn(self, what):
        return getattr(self.lib, f"knpemi_{self.kind}_{what}")

    def set_plain(self, capacity=4):
        return self.fn("set")(self.dp.h, len(self.tags), L.iptr(self.sub), L.iptr(self.mask), capacity)

    def set_part(self, recorded, rank=0, world=1, capacity=4, hook=NOOP, xbuf=True):
        """recorded: {tag: bool per item} or None (a null mask)."""
        old, self.xbuf = self.xbuf, DeviceBuffer(world * self.n_cols)
        self.dp.sync()                      # the table that refers to the old buffer may have a record in flight
        mask = None if recorded is None else np.ascontiguousarray(
            np.concatenate([recorded[t] for t in self.tags]).astype(np.uint8))
        rc = self.fn("set_partitioned")(
            self.dp.h, len(self.tags), L.iptr(self.sub), L.iptr(self.mask), capacity,
            None if mask is None else mask.ctypes.data_as(L.c_u8_p), rank, world,
            self.xbuf.data_ptr() if xbuf else None, C.cast(hook, C.c_void_p) if hook is not None else None, None)
        self.old = old                      # a refused call leaves the table on the old buffer: keep it
        return rc

    def record(self, fields=1):
        return self.fn("record")(self.dp.h, fields)

    def read(self, k, reset=0):
        buf = np.full((max(k, 1), self.n_cols), np.nan)
        rows, over = C.c_int64(), C.c_int64()
        L.check(self.fn("read")(self.dp.h, k, L.dptr(buf), C.byref(rows), C.byref(over), reset))
        return buf, rows.value, over.value

    def fields(self):
        return {t: self.rec.fields(t) for t in self.tags}

    def one(self, recorded, **kw):
        """(row, fields) of one partitioned record with this mask."""
        L.check(self.set_part(recorded, **kw))
        L.check(self.record(1))
        f = self.fields()
        buf, rows, over = self.read(1)
        assert rows == 1 and over == 0
        return buf[0], f

    def masks(self, what):
        n = {t: self.count(t) for t in self.tags}
        if what == "all":
            return {t: np.ones(n[t], bool) for t in self.tags}
        if what == "zero_last":       # all-zero on the last watch
            return {t: np.full(n[t], t != self.tags[-1]) for t in self.tags}
        return {t: np.arange(n[t]) % 3 == what for t in self.tags}

    def host(self, recorded=None):
        if self.kind == "flux":
            tags = list(self.s.subdomain_list)
            phi = {t: self.s.phi[t].x._a for t in tags}
            c = {t: [f.x._a for f in self.s.c_prev[t]] + [self.s.ion_list[-1][f"c_{t}"].x._a] for t in tags}
            return self.rec.compute_host(phi, c, recorded=recorded)
        return self.rec.compute_host(recorded=recorded, **xc.host_state(self.s))

    def host_err(self, row, recorded):
        """Largest error of a device row against compute_host(recorded=...), every column relative to its scale."""
        f, want = self.host(recorded)
        if self.kind == "exchange":
            # the scale of the whole watch: a third of the facets cancels no better than all of them
            _, whole = self.host()
            return max(abs(row[j] - want[key]) / xc.column_scale(self.rec, whole, f, key)
                       for j, (key, _) in enumerate(self.rec.columns()))
        worst, j = 0.0, 0
        _, whole = self.host()
        for key, w in self.rec.columns():
            a = np.atleast_1d(np.asarray(want[key], np.float64))
            scale = np.abs(np.atleast_1d(np.asarray(whole[key], np.float64))).max()
            worst = max(worst, float(np.abs(row[j:j + w] - a).max() / scale))
            j += w
        return worst


@functools.lru_cache(maxsize=None)
def _handle(name):
    from knpemi.stepper import DeviceStepper
    s = xc.build(name)
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev)
    L.check(st.dp.lib.knpemi_assemble_knp(st.dp.h, 0))      # the splitting scheme the exchange records with
    return s, st


@functools.lru_cache(maxsize=None)
def _plain(name, kind):
    """(recorder, row, fields) of the plain recorder's one record."""
    s, st = _handle(name)
    R = Recorder(kind, s, st.dp)
    L.check(R.set_plain())
    L.check(R.record(1))
    f = R.fields()
    buf, rows, over = R.read(1)
    assert rows == 1 and over == 0
    return R, buf[0], f


def _same_fields(a, b):
    for t in a:
        assert set(a[t]) == set(b[t])
        for k in a[t]:
            assert np.array_equal(a[t][k], b[t][k]), (t, k)


def _column_watch(R):
    """(key, first scalar column, width, watch tag) of every column."""
    out, j = [], 0
    for key, w in R.rec.columns():
        out.append((key, j, w, int(key.split("/")[0])))
        j += w
    return out


def test_setups_cover_the_workgroup_cases(hip_lib):
    """Chunk sizes from the library (kn_flux_chunk, kn_exchange_chunk): every 3-D set-up has a watch that spans several
    workgroups, and each recorder has a watch of several workgroups with a partly filled last one (cells: 13440 =
    52 x 256 + 128 on the tetrahedra; facets: 124 = 3 x 32 + 28 in 2-D; the 3-D membranes fill their workgroups)."""
    for kind, chunk in (("flux", fluxes.chunk()), ("exchange", exchange.chunk())):
        counts = {name: [_plain(name, kind)[0].count(t) for t in _plain(name, kind)[0].tags] for name in SETUPS}
        print(kind, "chunk", chunk, "items", counts)
        for name in ("tet", "hex", "three"):
            assert any(n > 2 * chunk for n in counts[name]), (kind, name, counts[name], chunk)
        assert any(n > 2 * chunk and n % chunk for c in counts.values() for n in c), (kind, counts, chunk)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", SETUPS)
def test_world_one_with_arbitrary_masks(hip_lib, name, kind):
    R, plain_row, plain_f = _plain(name, kind)
    is_max = R.rec.max_columns()
    row, f = R.one(R.masks("all"))
    assert np.array_equal(row, plain_row)
    _same_fields(f, plain_f)
    thirds = []
    for j in range(3):
        row, f = R.one(R.masks(j))
        _same_fields(f, plain_f)
        err = R.host_err(row, R.masks(j))
        print(name, kind, "third", j, "error against compute_host(recorded=mask)", err)
        assert err < TOL
        thirds.append(row)
    thirds = np.array(thirds)
    assert np.all(thirds[:, is_max] <= plain_row[is_max])
    assert np.array_equal(thirds[:, is_max].max(axis=0), plain_row[is_max])
    host_f, _ = R.host()
    nothing = types.SimpleNamespace(watched={})
    terms = ph.sum_abs_terms(R.rec if kind == "flux" else nothing, R.rec if kind == "exchange" else nothing, R.s,
                             host_f, host_f)
    worst = 0.0
    for key, j, w, tag in _column_watch(R):
        if is_max[j]:
            continue
        bound = 2.0 * R.count(tag) * ph.U * np.atleast_1d(terms[key])
        diff = np.abs(thirds[:, j:j + w].sum(axis=0) - plain_row[j:j + w])
        worst = max(worst, float((diff / bound).max()))
        assert np.all(diff <= bound), (key, diff, bound)
    print(name, kind, "largest |sum of the thirds - plain sum| / bound:", worst)
    row, f = R.one(R.masks("zero_last"))
    _same_fields(f, plain_f)
    for key, j, w, tag in _column_watch(R):
        if tag == R.tags[-1]:
            assert not row[j:j + w].any(), key
        else:
            assert np.array_equal(row[j:j + w], plain_row[j:j + w]), key


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ("2d", "three"))
def test_rank_one_of_two_writes_the_second_half(hip_lib, name, kind):
    R, _, plain_f = _plain(name, kind)
    want, _ = R.one(R.masks(1))
    row, f = R.one(R.masks(1), rank=1, world=2)
    _same_fields(f, plain_f)
    R.dp.sync()
    x = R.xbuf.host()
    n = R.n_cols
    assert x.shape == (2 * n,) and not x[:n].any()
    assert np.array_equal(x[n:], want) and np.array_equal(row, want)
    # rank 0 of two: the first half, and the other half is left zero for the next sum
    row, _ = R.one(R.masks(1), rank=0, world=2)
    R.dp.sync()
    x = R.xbuf.host()
    assert np.array_equal(x[:n], want) and not x[n:].any() and np.array_equal(row, want)


@pytest.mark.parametrize("kind", KINDS)
def test_capacity_reset_and_clear(hip_lib, kind):
    R, plain_row, _ = _plain("2d", kind)
    L.check(R.set_plain(capacity=1))
    L.check(R.record(0))
    L.check(R.record(0))
    _, rows0, over0 = R.read(1)
    L.check(R.set_part(R.masks("all"), capacity=1))
    L.check(R.record(0))
    L.check(R.record(0))
    buf, rows, over = R.read(1)
    assert (rows, over) == (rows0, over0) == (1, 1) and np.array_equal(buf[0], plain_row)
    # a new series: the counters and the fields are forgotten, the table and the mask stay
    L.check(R.set_part(R.masks(0), capacity=3))
    L.check(R.record(1))
    first, _, _ = R.read(1)
    L.check(R.fn("reset")(R.dp.h))
    assert R.read(0)[1:] == (0, 0)
    with pytest.raises(L.KnpemiError, match="no record with fields"):
        R.fields()
    L.check(R.record(1))
    L.check(R.record(0))
    buf, rows, over = R.read(2, reset=1)
    assert (rows, over) == (2, 0) and np.array_equal(buf[0], first[0]) and np.array_equal(buf[1], first[0])
    assert R.read(0)[1:] == (0, 0)
    R.fields()
    L.check(R.fn("clear")(R.dp.h))
    assert R.record(0) == L.EINVAL and R.fn("reset")(R.dp.h) == L.EINVAL
    assert R.fn("read")(R.dp.h, 0, None, None, None, 0) == L.EINVAL


@pytest.mark.parametrize("kind", KINDS)
def test_bad_arguments_leave_the_table_alone(hip_lib, kind):
    R, plain_row, _ = _plain("2d", kind)
    L.check(R.set_part(R.masks("all"), capacity=8))
    L.check(R.record(0))
    keep = R.xbuf                                      # the buffer of the table that stays
    lib = R.lib
    m = R.masks("all")
    assert R.set_part(None) == L.EINVAL and b"mask" in lib.knpemi_last_error()
    assert R.set_part(m, rank=1, world=1) == L.EINVAL and b"rank" in lib.knpemi_last_error()
    assert R.set_part(m, rank=-1, world=2) == L.EINVAL and R.set_part(m, rank=0, world=0) == L.EINVAL
    assert R.set_part(m, hook=None) == L.EINVAL and b"no all-reduce hook" in lib.knpemi_last_error()
    assert R.set_part(m, xbuf=False) == L.EINVAL and b"exchange buffer" in lib.knpemi_last_error()
    assert R.set_part(m, capacity=0) == L.EINVAL
    assert R.fn("set_partitioned")(None, 1, None, None, 1, None, 0, 1, None, None, None) == L.EINVAL
    R.xbuf = keep
    L.check(R.record(0))
    buf, rows, over = R.read(2)
    assert (rows, over) == (2, 0) and np.array_equal(buf[1], plain_row)
    # in partitioned mode a watch without items is refused only by the plain call
    L.check(R.fn("clear")(R.dp.h))
