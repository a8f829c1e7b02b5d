"""GPU tests of what the recorders share behind the C ABI (csrc/knpemi_record.hip), on the 2-D set-up of
test_partition_recorders_abi_gpu.py and its handle.

The install rule of knpemi_*_set: a call that is refused leaves the previous recorder in place, and that recorder still
records.  Each case sets a valid table, records, has a second set refused by the validation, records again on unchanged
fields and reads back: the series recorders hold two rows of the same bits, the events and the maps show both records
(the second one completes a statistic that needs the state the first one left).  The refusal after a failed allocation
takes the same path behind the build step and is not provoked here.

The rank slots of a partitioned record: observables with world = 1 and a no-op all-reduce hook give the plain recorder's
row bit for bit -- every observable's fold takes the same workgroup order, and the combine folds the one slot from the op's
identity.  (The fluxes' and the exchange's same case: test_partition_recorders_abi_gpu.test_world_one_with_arbitrary_masks.)"""
import ctypes as C

import numpy as np
import pytest

import test_partition_recorders_abi_gpu as pr
from knpemi import _lib as L
from knpemi.events import MembraneEvents
from knpemi.maps import FieldMaps
from test_observables_gpu import _observables

pytestmark = pytest.mark.gpu


def _refused(lib, rc, text):
    assert rc == L.EINVAL and text in lib.knpemi_last_error(), (rc, lib.knpemi_last_error())


class _Observe:
    """The observables of test_observables_gpu.py on a handle, through the C ABI."""

    def __init__(self, s, dp):
        self.dp, self.lib, self.obs = dp, dp.lib, _observables(s)
        self.n = len(self.obs.items)
        self.spec, self.ptr, self.idx, self.w, self.denom = self.obs.table(dp.sub_index)

    def args(self, n=None, idx=None, capacity=4):
        return (self.dp.h, self.n if n is None else n, L.iptr(self.spec.ravel()), self.ptr.ctypes.data_as(C.POINTER(C.c_int64)),
                L.iptr(self.idx if idx is None else idx), L.dptr(self.w), L.dptr(self.denom), capacity)

    def set_part(self, xbuf, rank=0, world=1, **kw):
        return self.lib.knpemi_observe_set_partitioned(*self.args(**kw), rank, world, xbuf.data_ptr(),
                                                       C.cast(pr.NOOP, C.c_void_p), None)

    def read(self, k, reset=0):
        buf = np.full((max(k, 1), self.n), np.nan)
        rows, over = C.c_int64(), C.c_int64()
        L.check(self.lib.knpemi_observe_read(self.dp.h, k, L.dptr(buf), C.byref(rows), C.byref(over), reset))
        return buf, rows.value, over.value


def test_observables_refused_set_and_world_one_slots(hip_lib):
    s, st = pr._handle("2d")
    O = _Observe(s, st.dp)
    lib, h = O.lib, st.dp.h
    L.check(lib.knpemi_observe_set(*O.args()))
    L.check(lib.knpemi_observe_record(h))
    first, rows, _ = O.read(1)
    assert rows == 1 and np.isfinite(first[0]).all()
    beyond = O.idx.copy()
    beyond[-1] = 1 << 30
    _refused(lib, lib.knpemi_observe_set(*O.args(capacity=0)), b"must be positive")
    _refused(lib, lib.knpemi_observe_set(*O.args(idx=beyond)), b"index out of range")
    xbuf = pr.DeviceBuffer(O.n)
    _refused(lib, O.set_part(xbuf, rank=1, world=1), b"bad rank / world")
    _refused(lib, O.set_part(xbuf, idx=beyond), b"index out of range")
    L.check(lib.knpemi_observe_record(h))
    buf, rows, over = O.read(2, reset=1)
    assert (rows, over) == (2, 0) and np.array_equal(buf[0], first[0]) and np.array_equal(buf[1], first[0])
    # partitioned, one rank: the buffer is zeroed at the set-up, the row is the plain row, the slots hold the partial sums
    L.check(O.set_part(xbuf))
    st.dp.sync()
    assert not xbuf.host().any()
    L.check(lib.knpemi_observe_record(h))
    buf, rows, over = O.read(1)
    assert (rows, over) == (1, 0) and np.array_equal(buf[0], first[0])
    sums = np.array([o.op == L.OBS_SUM for o in O.obs.items])
    assert np.array_equal(xbuf.host()[~sums], first[0][~sums])
    assert np.array_equal(xbuf.host()[sums] / O.denom[sums], first[0][sums])
    # a refused partitioned set leaves the partitioned table and its buffer in place
    _refused(lib, O.set_part(pr.DeviceBuffer(O.n), capacity=0), b"must be positive")
    L.check(lib.knpemi_observe_record(h))
    buf, rows, over = O.read(2)
    assert (rows, over) == (2, 0) and np.array_equal(buf[1], first[0])
    L.check(lib.knpemi_observe_clear(h))
    st.dp.sync()


@pytest.mark.parametrize("kind", pr.KINDS)
def test_watched_refused_set_keeps_the_table_recording(hip_lib, kind):
    s, st = pr._handle("2d")
    _, plain_row, _ = pr._plain("2d", kind)
    R = pr.Recorder(kind, s, st.dp)
    L.check(R.set_plain(capacity=4))
    L.check(R.record(0))
    zero = np.zeros(1, np.int32)
    _refused(R.lib, R.fn("set")(st.dp.h, 1, L.iptr(R.sub[:1]), L.iptr(zero), 4), b"empty ion mask")
    _refused(R.lib, R.set_plain(capacity=0), b"capacity must be positive")
    L.check(R.record(0))
    buf, rows, over = R.read(2)
    assert (rows, over) == (2, 0) and np.array_equal(buf[0], plain_row) and np.array_equal(buf[1], plain_row)
    L.check(R.fn("clear")(st.dp.h))


def test_events_refused_set_keeps_the_state_of_the_first_record(hip_lib):
    s, st = pr._handle("2d")
    dp, lib = st.dp, st.lib
    ev = MembraneEvents(s.subdomain_list)
    ev.watch(1, 0.0, reset=-0.5, keep=2)
    nq = ev.n_q[1]
    before = s.phi_M_prev[1].x._a.copy()
    ev._attach(lib, dp.h, dp.sub_index)
    dp.push_array(L.F_PHI_M, dp.sub_index[1], 0, np.full(nq, -1.0))
    L.check(lib.knpemi_events_record(dp.h, 1.0))
    ecs = np.zeros(1, np.int32)
    _refused(lib, lib.knpemi_events_set(dp.h, 1, L.iptr(ecs), L.dptr(np.zeros(1)), None, 2), b"bad sub-domain index")
    assert lib.knpemi_events_set(dp.h, 1, L.iptr(np.ones(1, np.int32)), L.dptr(np.zeros(1)), None, -1) == L.EINVAL
    # the crossing between the two records: armed by the first one, at the middle of the interval
    dp.push_array(L.F_PHI_M, dp.sub_index[1], 0, np.full(nq, 1.0))
    L.check(lib.knpemi_events_record(dp.h, 2.0))
    m = ev.maps(1)
    assert (m["count"] == 1).all() and (m["t_first"] == 1.5).all() and (m["v_peak"] == 1.0).all()
    assert lib.knpemi_events_record(dp.h, 2.0) == L.EINVAL          # the clock of the table that stayed
    L.check(lib.knpemi_events_clear(dp.h))
    dp.push_array(L.F_PHI_M, dp.sub_index[1], 0, before)


def test_maps_refused_set_keeps_the_state_of_the_first_record(hip_lib):
    s, st = pr._handle("2d")
    dp, lib = st.dp, st.lib
    fm = FieldMaps(s.subdomain_list, s.ion_list)
    fm.watch("phi", "phi", tag=0, stats=("peak",))
    fm._attach(dp, 4)
    before = s.phi[0].x._a.copy()
    a = np.linspace(-1.0, 1.0, before.shape[0])
    dp.push_array(L.F_PHI, dp.sub_index[0], 0, a)
    L.check(lib.knpemi_maps_record(dp.h, 1.0))
    unknown = np.array([99, 0, 0, 1], np.int32)
    _refused(lib, lib.knpemi_maps_set(dp.h, 1, L.iptr(unknown), None, None, 4), b"unknown field")
    _refused(lib, lib.knpemi_maps_set(dp.h, 0, L.iptr(unknown), None, None, 4), b"watches")
    dp.push_array(L.F_PHI, dp.sub_index[0], 0, -a)
    L.check(lib.knpemi_maps_record(dp.h, 2.0))
    m = fm.maps("phi")
    assert np.array_equal(m["v_max"], np.abs(a)) and np.array_equal(m["t_max"], np.where(-a > a, 2.0, 1.0))
    assert lib.knpemi_maps_record(dp.h, 2.0) == L.EINVAL            # the clock of the table that stayed
    L.check(lib.knpemi_maps_clear(dp.h))
    dp.push_array(L.F_PHI, dp.sub_index[0], 0, before)
