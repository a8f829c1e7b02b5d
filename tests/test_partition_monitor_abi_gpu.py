"""GPU tests of knpemi_monitor_set_partitioned and knpemi_maps_set_partitioned in one process (world 1, no communicator, a
no-op callback as the all-reduce hook: a record is launch, (nothing), combine), as test_partition_recorders_abi_gpu.py
tests their siblings: with all the weights on the one rank the partitioned row IS the plain row bit for bit -- the fold
takes the same workgroup order and the combine adds the one slot to the identity; an average is divided by the sum it is
given -- also when the global sum of weights differs from the library's own sum of the local ones in its last bits, in either
direction (the caller adds in another order); and the argument refusals of the two entry points, which leave the
previous table recording."""
import contextlib
import ctypes as C
import io
import types

import numpy as np
import pytest

import exchange_cases as xc
from test_partition_recorders_abi_gpu import NOOP, DeviceBuffer
from knpemi import FieldMaps, MembraneMonitor
from knpemi import _lib as L

pytestmark = pytest.mark.gpu

HOOK = C.cast(NOOP, C.c_void_p)


def _stepper(s):
    from knpemi.stepper import DeviceStepper
    with contextlib.redirect_stdout(io.StringIO()):
        st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev)
        for tag in list(s.subdomain_list)[1:]:
            for mm in s.subdomain_list[tag]["mem_models"]:
                st.add_membrane_model(mm["ode"], {}, None)
    return st


def _captured(rec, dp, name):
    """The arguments `rec._attach` passes to knpemi_<name> (the call itself is not made)."""
    box = {}

    def fake(*args):
        box["args"] = args
        return L.OK
    proxy = types.SimpleNamespace(h=dp.h, sub_index=dp.sub_index, device=dp.device, lib=types.SimpleNamespace(**{name: fake}))
    rec._attach(proxy, 8)
    rec._dev = None
    return box["args"]


def _monitor(s):
    mon = MembraneMonitor(s.subdomain_list, s.ion_list, ft=s.ft)
    for tag in (1, 2):
        mon.watch(tag)
        mem = s.subdomain_list[tag]["mesh_mem"]
        mon.point(f"p{tag}", tag, np.array([0.5, 0.3, 0.2]) @ np.asarray(mem.x)[np.asarray(mem.cells)[5]])
        for op in ("integral", "average", "min", "max"):
            mon.reduce(f"{op}{tag}", tag, op=op)
    return mon


def _rows(lib, h, read, n_cols, n):
    buf, rows, over = np.empty((n, n_cols)), C.c_int64(), C.c_int64()
    L.check(read(h, n, L.dptr(buf), C.byref(rows), C.byref(over), 1))
    assert (rows.value, over.value) == (n, 0)
    return buf


def test_monitor_world_one_is_the_plain_row_and_refusals(hip_lib):
    s = xc.build("three")
    st = _stepper(s)
    lib, h = st.lib, st.dp.h
    mon = _monitor(s)
    args = _captured(mon, st.dp, "knpemi_monitor_set")
    n_cols = mon.n_cols
    L.check(lib.knpemi_monitor_set(*args))
    for t in (1e-4, 2e-4):
        L.check(lib.knpemi_monitor_record(h, t, 0))
    plain = _rows(lib, h, lib.knpemi_monitor_read, n_cols, 2)
    assert np.isfinite(plain).all()
    wsum = np.array([mon.weights(*key).sum() for key in mon.watched])
    xbuf = DeviceBuffer(n_cols)
    tail = (0, 1, xbuf.data_ptr(), HOOK, None)
    # the global sums as numpy adds them, and one unit in the last place to either side of them
    for w in (wsum, np.nextafter(wsum, 0.0), np.nextafter(wsum, 1.0)):
        L.check(lib.knpemi_monitor_set_partitioned(*args, L.dptr(np.ascontiguousarray(w)), *tail))
        for t in (1e-4, 2e-4):
            L.check(lib.knpemi_monitor_record(h, t, 0))
        got = _rows(lib, h, lib.knpemi_monitor_read, n_cols, 2)
        avg = np.array([kind == L.MON_AVERAGE for _, kind, *_ in mon._cols])
        assert np.array_equal(got[:, ~avg], plain[:, ~avg])
        # (the divisor differs from the library's own sequential sum of the weights by n roundings at most)
        assert np.all(np.abs(got[:, avg] - plain[:, avg]) <= 4 * 2.0 ** -52 * mon.n_dofs(1) * np.abs(plain[:, avg]))
    # refusals: each leaves the table above recording
    good = L.dptr(np.ascontiguousarray(wsum))
    bad = [((*args, None, *tail), "global weight sums"),
           ((*args, L.dptr(np.array([np.nan, 1.0])), *tail), "negative or not finite"),
           ((*args, L.dptr(np.array([-1.0, 1.0])), *tail), "negative or not finite"),
           ((*args, good, 1, 1, xbuf.data_ptr(), HOOK, None), "bad rank / world"),
           ((*args, good, 0, 0, xbuf.data_ptr(), HOOK, None), "bad rank / world"),
           ((*args, good, 0, 1, None, HOOK, None), "exchange buffer is required"),
           ((*args, good, 0, 1, xbuf.data_ptr(), None, None), "no all-reduce hook and no library communicator"),
           ((*args[:5], 0, None, 0, None, None, None, 8, good, *tail), "needs a column")]
    for call, match in bad:
        with pytest.raises(L.KnpemiError, match=match):
            L.check(lib.knpemi_monitor_set_partitioned(*call))
    L.check(lib.knpemi_monitor_record(h, 3e-4, 0))
    assert _rows(lib, h, lib.knpemi_monitor_read, n_cols, 1).shape == (1, n_cols)
    L.check(lib.knpemi_monitor_clear(h))
    with pytest.raises(L.KnpemiError, match="no monitors set"):
        L.check(lib.knpemi_monitor_record(h, 4e-4, 0))


def test_maps_world_one_is_the_plain_row_and_refusals(hip_lib):
    s = xc.build("three")
    st = _stepper(s)
    lib, h = st.lib, st.dp.h

    def maps(series=True):
        fm = FieldMaps(s.subdomain_list, s.ion_list)
        fm.watch("K_ecs", "c", tag=0, ion="K", threshold=float(np.median(s.c[0][0].x._a)), series=series)
        fm.watch("phi_M", "phi_M", tag=2, threshold=float(np.median(s.phi_M_prev[2].x._a)), series=series)
        return fm
    fm = maps()
    args = _captured(fm, st.dp, "knpemi_maps_set")
    L.check(lib.knpemi_maps_set(*args))
    for t in (1e-4, 2e-4):
        L.check(lib.knpemi_maps_record(h, t))
    plain = _rows(lib, h, lib.knpemi_maps_series_read, 4, 2)
    assert plain[:, 1].min() > 0 and plain[:, 3].min() > 0
    n_items = fm.watches["K_ecs"].n + fm.watches["phi_M"].n
    own = np.ones(n_items, np.uint8)
    xbuf = DeviceBuffer(4)
    tail = (0, 1, xbuf.data_ptr(), HOOK, None)
    u8 = lambda a: a.ctypes.data_as(L.c_u8_p)      # noqa: E731
    L.check(lib.knpemi_maps_set_partitioned(*args, u8(own), *tail))
    for t in (1e-4, 2e-4):
        L.check(lib.knpemi_maps_record(h, t))
    got = _rows(lib, h, lib.knpemi_maps_series_read, 4, 2)
    assert np.array_equal(got, plain)
    # n counts the owned items only, the measure every item with a weight
    half = own.copy()
    half[::2] = 0
    L.check(lib.knpemi_maps_set_partitioned(*args, u8(half), *tail))
    L.check(lib.knpemi_maps_record(h, 1e-4))
    row = _rows(lib, h, lib.knpemi_maps_series_read, 4, 1)[0]
    assert row[0] == plain[0, 0] and row[2] == plain[0, 2] and 0 < row[1] < plain[0, 1] and 0 < row[3] < plain[0, 3]
    bad = [((*args, None, *tail), "owned mask is required"),
           ((*args, u8(own), 2, 2, xbuf.data_ptr(), HOOK, None), "bad rank / world"),
           ((*args, u8(own), 0, 1, None, HOOK, None), "exchange buffer is required"),
           ((*args, u8(own), 0, 1, xbuf.data_ptr(), None, None), "no all-reduce hook and no library communicator"),
           ((*_captured(maps(series=False), st.dp, "knpemi_maps_set"), u8(own), *tail), "no watch has a series")]
    for call, match in bad:
        with pytest.raises(L.KnpemiError, match=match):
            L.check(lib.knpemi_maps_set_partitioned(*call))
    L.check(lib.knpemi_maps_record(h, 2e-4))      # the table above still records
    assert _rows(lib, h, lib.knpemi_maps_series_read, 4, 1).shape == (1, 4)
