"""GPU tests of the field snapshots (knpemi_snapshot_*, DeviceStepper.snapshot) against the numpy restatement
`Snapshots.frame_host`: every watch of a frame bit for bit (NaN positions equal), the layout, selections, the ring, a run
against downloads of an identical run, the attach rules, every refusal, and the driver's `--snapshots`."""
import contextlib
import ctypes as C
import importlib.util
import io
import os

import numpy as np
import pytest

from knpemi import _lib as L
from knpemi.snapshots import MemorySink, Snapshots

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PROBLEMS = {}
# what a conversion to float must get right: NaN, signed zeros, a double denormal (-> 0), a float denormal, ties to even in
# both directions, a value just above a tie, overflow to +-inf, the first integer a float cannot hold
SPECIAL = np.array([np.nan, 0.0, -0.0, 5e-324, 1e-40, 1.0 + 2.0 ** -24, 1.0 + 3.0 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -40,
                    1e39, -1e39, 16777217.0, -1e-46])


def _values(n, seed):
    """n distinct doubles: SPECIAL first, then seeded values of many magnitudes."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n) + seed
    m = min(n, SPECIAL.size)
    v[:m] = SPECIAL[:m]
    return v


def _models(s):
    """[(tag, model index, MembraneModel)] of the set-up."""
    return [(tag, j, mm["ode"]) for tag, sd in s.subdomain_list.items() if tag > 0
            for j, mm in enumerate(sd.get("mem_models", []))]


def _plant(s, dp, seed=0):
    """Distinct synthetic values in every field and state table, on the host objects and on the device."""
    n_solved = len(s.ion_list) - 1
    for tag in s.subdomain_list:
        sub = dp.sub_index[tag]
        seed += 1
        s.phi[tag].x.array[:] = _values(s.phi[tag].x._a.shape[0], seed)
        dp.push_array(L.F_PHI, sub, 0, s.phi[tag].x._a)
        for k in range(n_solved):
            for f, field in ((s.c[tag][k], L.F_C), (s.c_prev[tag][k], L.F_C_PREV)):
                seed += 1
                f.x.array[:] = _values(f.x._a.shape[0], seed)
                dp.push_array(field, sub, k, f.x._a)
        seed += 1
        f = s.ion_list[-1][f"c_{tag}"]
        f.x.array[:] = _values(f.x._a.shape[0], seed)
        dp.push_array(L.F_C_ELIM, sub, 0, f.x._a)
        if tag > 0:
            seed += 1
            s.phi_M_prev[tag].x.array[:] = _values(s.phi_M_prev[tag].x._a.shape[0], seed)
            dp.push_array(L.F_PHI_M, sub, 0, s.phi_M_prev[tag].x._a)
    for tag, j, m in _models(s):
        for k, ion in enumerate(s.ion_list):
            seed += 1
            f = s.subdomain_list[tag]["mem_models"][j]["I_ch_k"][ion["name"]]
            f.x.array[:] = _values(f.x._a.shape[0], seed)
            dp.push_array(L.F_I_CH, dp.sub_index[tag], j * L.MAX_IONS + k, f.x._a)
        for c in range(m.states.shape[1]):
            seed += 1
            m.states[:, c] = _values(m.states.shape[0], seed)
        st, pa = np.ascontiguousarray(m.states), np.ascontiguousarray(m.parameters)
        L.check(dp.lib.knpemi_ode_set_tables(dp.h, m._sub, m._model, L.dptr(st), L.dptr(pa)))


def _problem(kind):
    """(set-up, device problem) with planted values, built once per kind."""
    if kind not in _PROBLEMS:
        from helpers import Setup
        with contextlib.redirect_stdout(io.StringIO()):
            if kind == "three":
                from test_observables_gpu import _problem as three
                s = three("three", 0)[0]
            else:
                s = Setup("2d", 1) if kind == "2d" else Setup("tet", 0)
        dp = s.a_emi.dp
        _plant(s, dp)
        _PROBLEMS[kind] = (s, dp)
    return _PROBLEMS[kind]


def _snap(s, **kw):
    return Snapshots(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list, **kw)


def _host(s):
    return s.phi, s.c, s.c_prev, s.phi_M_prev


def _take(dp, snap, wait=1):
    """(status, t, seq, frame) of knpemi_snapshot_take, the frame read through the layout the library reported."""
    watches, nbytes = snap._layout
    buf = np.full(nbytes, 0xA5, np.uint8)
    t, seq = C.c_double(-1.0), C.c_int64(-1)
    rc = dp.lib.knpemi_snapshot_take(dp.h, wait, buf.ctypes.data_as(C.c_void_p), nbytes, C.byref(t), C.byref(seq))
    if rc != L.OK:
        assert (buf == 0xA5).all() and t.value == -1.0 and seq.value == -1      # nothing touched
        return rc, None, None, None
    return rc, t.value, seq.value, {name: np.frombuffer(buf, dt, count=n, offset=o) for name, dt, o, n in watches}


def _same(got, want):
    """Every watch bit for bit; NaNs at the same places (a NaN's payload is the converter's)."""
    assert list(got) == list(want)
    for name, a in want.items():
        b = got[name]
        assert b.dtype == a.dtype and b.shape == a.shape, name
        bits = np.uint64 if a.dtype == np.float64 else np.uint32
        nan = np.isnan(a)
        assert np.array_equal(np.isnan(b), nan), name
        assert np.array_equal(b.view(bits)[~nan], a.view(bits)[~nan]), name


def _layout_ok(dp, snap):
    watches, nbytes = snap._layout
    end = 0
    for name, dt, off, n in watches:
        assert off % L.SNAPSHOT_ALIGN == 0 and off >= end and n == snap._items(snap.watches[name]).size, name
        end = off + n * np.dtype(dt).itemsize
    assert nbytes >= end
    only = C.c_int64()
    L.check(dp.lib.knpemi_snapshot_layout(dp.h, None, None, C.byref(only)))
    assert only.value == nbytes


def _define(snap, s, case):
    cells = [t for t in s.subdomain_list if t > 0]
    if case == "results":
        snap.watch_results()
    elif case == "mixed":          # float and double watches alternate in one space: the offsets need padding
        for tag in s.subdomain_list:
            snap.watch(f"phi4_{tag}", "phi", tag, dtype="f4")
            snap.watch(f"K_{tag}", "c", tag, ion="K")
            snap.watch(f"Na4_{tag}", "c", tag, ion="Na", dtype="f4")
            snap.watch(f"Cl4_{tag}", "c", tag, ion="Cl", dtype="f4")
            snap.watch(f"phi_{tag}", "phi", tag)
        for tag in cells:
            snap.watch(f"phi_M4_{tag}", "phi_M", tag, dtype="f4")
            snap.watch(f"phi_M_{tag}", "phi_M", tag)
    elif case == "membrane":       # I_ch and state watches
        for tag, j, m in _models(s):
            for ion in s.ion_list:
                snap.watch(f"I_{ion['name']}_{tag}_{j}", "I_ch", tag, ion=ion["name"], model=j)
            for c in range(m.states.shape[1]):
                snap.watch(f"y{c}_{tag}_{j}", "state", tag, model=j, state=c, dtype="f4" if c % 2 else "f8")
    else:                          # a record-resident and a dense watch in one space
        for tag in s.subdomain_list:
            snap.watch(f"Kp_{tag}", "c_prev", tag, ion="K")
            snap.watch(f"K_{tag}", "c", tag, ion="K")
            snap.watch(f"Clp4_{tag}", "c_prev", tag, ion=1, dtype="f4")
            snap.watch(f"Na_{tag}", "c", tag, ion="Na")
            snap.watch(f"Cl_{tag}", "c", tag, ion="Cl", dtype="f4")
    return snap


@pytest.mark.parametrize("case", ["results", "mixed", "membrane", "record_and_dense"])
@pytest.mark.parametrize("kind", ["2d", "tet", "three"])
def test_kernel_matches_the_restatement(hip_lib, kind, case):
    s, dp = _problem(kind)
    snap = _define(_snap(s), s, case)
    snap._attach(dp, 2)
    try:
        _layout_ok(dp, snap)
        if case == "mixed":        # a float watch that does not fill its last 256 bytes is followed by padding
            watches, _ = snap._layout
            assert any(o2 > o1 + n1 * np.dtype(d1).itemsize for (_, d1, o1, n1), (_, _, o2, _) in zip(watches, watches[1:]))
        L.check(dp.lib.knpemi_snapshot_record(dp.h, 0.125))
        rc, t, seq, frame = _take(dp, snap)
        assert (rc, t, seq) == (L.OK, 0.125, 0)
        want = snap.frame_host(*_host(s))
        _same(frame, want)
        specials = [a for a in want.values() if a.dtype == np.float32]
        if specials:               # the conditions of the test, on the reference: the conversions that can go wrong
            a = specials[0]
            assert np.isnan(a[0]) and a[3] == 0.0 and 0.0 < a[4] < np.finfo(np.float32).tiny and a[5] == 1.0
            assert a[6] == np.float32(1.0 + 2.0 ** -22) and a[7] > 1.0 and np.isinf(a[8]) and a[10] == 16777216.0
            assert np.signbit(a[2]) and not np.signbit(a[1]) and np.signbit(a[11]) and a[11] == 0.0
        print(f"{kind} {case}: {len(want)} watches, {snap._layout[1]} bytes per frame")
    finally:
        L.check(dp.lib.knpemi_snapshot_clear(dp.h))
        snap._detach()


@pytest.mark.parametrize("kind", ["tet", "three"])
def test_selections(hip_lib, kind):
    """Lists of 1 item, 257 items and all items on a bulk and on a membrane space; the other spaces of the launch stay
    unselected."""
    s, dp = _problem(kind)
    rng = np.random.default_rng(3)
    n0, nq = int(dp.n_vert[0]), int(dp.n_q[1])
    assert n0 > 257 and nq > 257 and n0 % 256 and nq % 256
    for membrane, n in ((False, n0), (True, nq)):
        for m in (1, 257, n):
            idx = np.sort(rng.choice(n, size=m, replace=False))
            snap = _define(_snap(s), s, "mixed")
            snap.watch("I_K", "I_ch", 1, ion="K", dtype="f4")
            snap.select(1 if membrane else 0, membrane=membrane, indices=idx)
            snap._attach(dp, 1)
            try:
                _layout_ok(dp, snap)
                L.check(dp.lib.knpemi_snapshot_record(dp.h, 1.0))
                rc, _, _, frame = _take(dp, snap)
                assert rc == L.OK
                want = snap.frame_host(*_host(s))
                picked = "phi_M_1" if membrane else "K_0"
                assert want[picked].shape == (m,) and want["phi_1"].shape == (int(dp.n_vert[1]),)
                assert want["phi_M_1" if not membrane else "K_0"].shape == ((nq,) if not membrane else (n0,))
                assert np.array_equal(snap.locations(picked),
                                      np.asarray(snap._mesh(1 if membrane else 0, membrane).x)[idx])
                _same(frame, want)
            finally:
                L.check(dp.lib.knpemi_snapshot_clear(dp.h))
                snap._detach()


def _constant(s, dp, v):
    s.phi[0].x.array[:] = v
    dp.push_array(L.F_PHI, 0, 0, s.phi[0].x._a)


def test_ring(hip_lib):
    s, dp = _problem("2d")
    lib, h = dp.lib, dp.h
    keep = s.phi[0].x._a.copy()
    snap = _snap(s)
    snap.watch("phi_0", "phi", 0)
    snap.watch("K4_1", "c", 1, ion="K", dtype="f4")
    try:
        assert lib.knpemi_snapshot_pending(h) == 0
        snap._attach(dp, 1)
        # depth 1: the second record is refused and changes nothing
        assert _take(dp, snap, wait=0)[0] == 1 and _take(dp, snap, wait=1)[0] == 1      # nothing in flight: "none"
        _constant(s, dp, 1.5)
        L.check(lib.knpemi_snapshot_record(h, 0.5))
        first = snap.frame_host(*_host(s))
        _constant(s, dp, 2.5)
        assert lib.knpemi_snapshot_record(h, 0.75) == L.EBUSY and b"in flight" in lib.knpemi_last_error()
        assert lib.knpemi_snapshot_pending(h) == 1
        rc, t, seq, frame = _take(dp, snap)
        assert (rc, t, seq) == (L.OK, 0.5, 0) and lib.knpemi_snapshot_pending(h) == 0
        _same(frame, first)
        L.check(lib.knpemi_snapshot_record(h, 0.75))       # the slot is free again
        rc, t, seq, frame = _take(dp, snap)
        assert (rc, t, seq) == (L.OK, 0.75, 1) and np.all(frame["phi_0"] == 2.5)
        with pytest.raises(L.KnpemiError) as e:            # the status has a place in the Python layer
            _constant(s, dp, 0.0)
            L.check(lib.knpemi_snapshot_record(h, 1.0))
            L.check(lib.knpemi_snapshot_record(h, 1.0))
        assert e.value.code == L.EBUSY
        L.check(lib.knpemi_snapshot_clear(h))
        snap._detach()

        # depth 2, five records with the takes interleaved: seq and t in order, each frame the field at its record
        snap._attach(dp, 2)
        got, k = [], 0
        for step in ("r", "r", "t", "r", "t", "t", "r", "r", "t", "t"):
            if step == "r":
                _constant(s, dp, 10.0 + k)
                L.check(lib.knpemi_snapshot_record(h, 0.25 * k))
                k += 1
                assert lib.knpemi_snapshot_pending(h) == k - len(got)
            else:
                rc, t, seq, frame = _take(dp, snap)
                assert rc == L.OK
                got.append((t, seq, frame))
        assert k == 5 and [(t, q) for t, q, _ in got] == [(0.25 * j, j) for j in range(5)]
        for j, (_, _, frame) in enumerate(got):
            assert np.all(frame["phi_0"] == 10.0 + j) and frame["phi_0"].shape == keep.shape
        assert lib.knpemi_snapshot_pending(h) == 0 and _take(dp, snap, wait=0)[0] == 1
        # a poll never hands out a frame twice, whether it finds the copy done or still running
        L.check(lib.knpemi_snapshot_record(h, 2.0))
        rc = _take(dp, snap, wait=0)[0]
        assert rc in (L.OK, L.EBUSY)
        assert lib.knpemi_snapshot_pending(h) == (0 if rc == L.OK else 1)
        # reset with frames in flight
        _constant(s, dp, 20.0)
        L.check(lib.knpemi_snapshot_record(h, 3.0))
        assert lib.knpemi_snapshot_pending(h) >= 1
        L.check(lib.knpemi_snapshot_reset(h))
        assert lib.knpemi_snapshot_pending(h) == 0 and _take(dp, snap)[0] == 1
        _constant(s, dp, 21.0)
        L.check(lib.knpemi_snapshot_record(h, 0.0))
        rc, t, seq, frame = _take(dp, snap)
        assert (rc, t, seq) == (L.OK, 0.0, 0) and np.all(frame["phi_0"] == 21.0)
        _same(frame, snap.frame_host(*_host(s)))
        # a wrong buffer
        L.check(lib.knpemi_snapshot_record(h, 1.0))
        buf = np.empty(snap._layout[1] + 8, np.uint8)
        assert lib.knpemi_snapshot_take(h, 1, buf.ctypes.data_as(C.c_void_p), buf.size, None, None) == L.EINVAL
        assert lib.knpemi_snapshot_take(h, 1, None, snap._layout[1], None, None) == L.EINVAL
        assert lib.knpemi_snapshot_record(h, float("nan")) == L.EINVAL and lib.knpemi_snapshot_pending(h) == 1
    finally:
        lib.knpemi_snapshot_clear(h)
        snap._detach()
        s.phi[0].x.array[:] = keep
        dp.push_array(L.F_PHI, 0, 0, keep)
    assert lib.knpemi_snapshot_record(h, 1.0) == L.EINVAL and lib.knpemi_snapshot_reset(h) == L.EINVAL
    assert lib.knpemi_snapshot_layout(h, None, None, None) == L.EINVAL and lib.knpemi_snapshot_pending(h) == 0
    assert lib.knpemi_snapshot_take(h, 0, buf.ctypes.data_as(C.c_void_p), 8, None, None) == L.EINVAL


def test_arguments(hip_lib):
    """Every refusal of knpemi_snapshot_set; each leaves the previous table recording."""
    s, dp = _problem("2d")
    lib, h = dp.lib, dp.h
    n_sub, K = len(s.subdomain_list), len(s.ion_list)
    n0, nq = int(dp.n_vert[0]), int(dp.n_q[1])
    n_states = _models(s)[0][2].states.shape[1]
    snap = _snap(s)
    snap.watch("phi_0", "phi", 0)
    snap.watch("phi_M_1", "phi_M", 1, dtype="f4")
    snap._attach(dp, 2)
    p64 = C.POINTER(C.c_int64)

    def set_(spec, sel=(), depth=2, handle=h):
        spec = np.ascontiguousarray(spec, np.int32).reshape(-1, 4)
        space = np.array([sp for sp, _ in sel], np.int32)
        off = np.concatenate([[0], np.cumsum([len(i) for _, i in sel])]).astype(np.int64)
        idx = np.ascontiguousarray(np.concatenate([i for _, i in sel]) if sel else np.zeros(0), np.int32)
        return lib.knpemi_snapshot_set(handle, spec.shape[0], L.iptr(spec.ravel()), len(sel), L.iptr(space) if sel else None,
                                       off.ctypes.data_as(p64) if sel else None,
                                       L.iptr(idx) if sel and idx.size else L.iptr(np.zeros(1, np.int32)) if sel else None, depth)
    ok, mem = [L.F_PHI, 0, 0, 0], [L.F_PHI_M, 1, 0, 0]
    refused = [
        lib.knpemi_snapshot_set(h, 1, None, 0, None, None, None, 2),
        lib.knpemi_snapshot_set(h, 1, L.iptr(np.array(ok, np.int32)), 1, None, None, None, 2),
        set_(np.zeros((0, 4))), set_([ok] * (L.SNAPSHOT_MAX_WATCH + 1)),
        set_([99, 0, 0, 0]), set_([L.F_SOURCE, 0, 0, 0]), set_([-1, 0, 0, 0]),                      # unknown field
        set_([L.F_PHI, n_sub, 0, 0]), set_([L.F_PHI, -1, 0, 0]),                                    # sub
        set_([L.F_C, 0, K - 1, 0]), set_([L.F_C, 0, -1, 0]), set_([L.F_C_PREV, 0, K - 1, 0]),      # idx
        set_([L.F_I_CH, 1, -1, 0]), set_([L.F_I_CH, 1, K, 0]), set_([L.F_I_CH, 1, L.MAX_IONS, 0]),  # ion, model slot
        set_([L.F_ODE_STATE, 1, n_states, 0]), set_([L.F_ODE_STATE, 1, -1, 0]),
        set_([L.F_ODE_STATE, 1, L.SNAPSHOT_STATE_STRIDE, 0]), set_([L.F_ODE_STATE, n_sub, 0, 0]),
        set_([L.F_PHI_M, 0, 0, 0]), set_([L.F_I_CH, 0, 0, 0]), set_([L.F_ODE_STATE, 0, 0, 0]),      # ... on the ECS
        set_([ok, mem, ok]),                                                                       # listed twice
        set_(ok, depth=0), set_(ok, depth=-1),
        set_([L.F_PHI, 0, 0, 2]),                                                                   # unknown flag
        set_(ok, sel=[(0, [2, 1])]), set_(ok, sel=[(0, [1, 1])]), set_(ok, sel=[(0, [0, n0])]),     # unsorted, repeated, range
        set_(ok, sel=[(0, [-1, 0])]), set_(ok, sel=[(0, [])]),
        set_([ok, mem], sel=[(0, [1]), (0, [2])]),                                                  # two for one space
        set_(ok, sel=[(1, [0])]), set_(ok, sel=[(L.MAX_SUB + 1, [0])]), set_(ok, sel=[(2 * L.MAX_SUB, [0])]),
        set_(mem, sel=[(L.MAX_SUB + 1, [nq])]),
    ]
    assert refused == [L.EINVAL] * len(refused)
    assert set_([ok, mem, ok]) == L.EINVAL and b"twice" in lib.knpemi_last_error()
    assert set_([L.F_PHI_M, 0, 0, 0]) == L.EINVAL and b"membrane" in lib.knpemi_last_error()
    ode = C.c_void_p()
    L.check(lib.knpemi_ode_create(dp.device, 1, L.iptr(np.array([8], np.int32)), C.byref(ode)))
    assert set_(ok, handle=ode) == L.EINVAL and b"has no fields" in lib.knpemi_last_error()
    lib.knpemi_destroy(ode)
    # ... so the table set before them still records, with its layout
    _layout_ok(dp, snap)
    L.check(lib.knpemi_snapshot_record(h, 0.5))
    rc, t, seq, frame = _take(dp, snap)
    assert (rc, t, seq) == (L.OK, 0.5, 0)
    _same(frame, snap.frame_host(*_host(s)))
    # accepted: the same field in both widths, a state, the largest table; a new table replaces the old one
    assert set_([[L.F_PHI, 0, 0, 0], [L.F_PHI, 0, 0, L.SNAPSHOT_F32], [L.F_ODE_STATE, 1, n_states - 1, 0]],
                sel=[(L.MAX_SUB + 1, [nq - 1])]) == L.OK
    big = [[L.F_PHI, 0, 0, w] for w in (0, 1)] + [[L.F_C, s_, k, w] for s_ in range(n_sub) for k in range(K - 1) for w in (0, 1)]
    assert set_(big) == L.OK and lib.knpemi_snapshot_pending(h) == 0
    L.check(lib.knpemi_snapshot_clear(h))
    snap._detach()


def test_stepper_frames_equal_downloads_of_an_identical_run(hip_lib):
    """Six steps of the 2d r = 1 problem with device solves, snapshot(every=2, depth=2), writer thread: the frames of
    steps 2, 4 and 6 equal, bit for bit, the fields a second identical run downloads at those steps (extrapolate_guess off:
    the extrapolated guess carries the solutions of the last steps across reset())."""
    from test_events_gpu import _stepper, _steps
    s, st, _ = _stepper(extrapolate_guess=False)
    sink = MemorySink()
    snap = _snap(s, sink=sink)
    snap.watch_results()
    snap.watch("Kp_0", "c_prev", 0, ion="K")
    snap.watch("I_Na", "I_ch", 1, ion="Na")
    snap.watch("gate", "state", 1, state=1)
    snap.watch("V4", "state", 1, state=0, dtype="f4")
    st.snapshot(snap, every=2, depth=2, t0=0.5)
    # the attach rules
    with pytest.raises(RuntimeError, match="already"):
        st.snapshot(_define(_snap(s), s, "results"))
    with pytest.raises(RuntimeError, match="attached"):
        snap.watch("late", "phi", 0)
    with pytest.raises(RuntimeError, match="attached"):
        snap.select(0, indices=[0])
    _steps(st, 6)
    snap.flush()
    first = list(sink.frames)
    assert snap.frames == 3 and [(t, k) for t, k, _ in first] == [(0.5 + k * st.dt, k) for k in (2, 4, 6)]
    assert snap.stalls == 0 and st.dp.lib.knpemi_snapshot_pending(st.dp.h) == 0
    # reset() discards a frame in flight and restarts the counters; the sink is untouched
    _steps(st, 2)
    assert st.dp.lib.knpemi_snapshot_pending(st.dp.h) == 1
    st.reset()
    assert st.dp.lib.knpemi_snapshot_pending(st.dp.h) == 0 and snap.frames == 0 and snap.stalls == 0
    assert len(sink.frames) == 3
    seen = []

    def after(k):
        if k % 2 == 0:
            st.download()
            seen.append(snap.frame_host(*_host(s)))
    _steps(st, 6, after)
    snap.flush()
    assert len(seen) == 3 and len(sink.frames) == 6 and snap.frames == 3
    for (_, _, a), (_, _, b), want in zip(first, sink.frames[3:], seen):
        _same(a, want)
        _same(b, want)
    assert not np.array_equal(first[0][2]["phi_M_1"], first[2][2]["phi_M_1"])      # the run moves
    assert not np.array_equal(first[0][2]["K_0"], first[2][2]["K_0"]) and np.ptp(first[2][2]["gate"]) > 0
    snap.close()


def test_a_full_ring_waits_for_the_oldest_frame_alone(hip_lib):
    """depth 1 and a record at every step: every tick but the first finds its slot in flight or just copied; no frame is
    lost or reordered, and a stall is counted exactly when the record had to wait."""
    from test_events_gpu import _stepper, _steps
    s, st, _ = _stepper()
    sink = MemorySink()
    snap = _snap(s, sink=sink, writer="inline")
    snap.watch("phi_M_1", "phi_M", 1)
    st.snapshot(snap, every=1, depth=1)
    _steps(st, 5)
    assert snap.frames + st.dp.lib.knpemi_snapshot_pending(st.dp.h) == 5 and 0 <= snap.stalls <= 4
    snap.flush()
    assert [k for _, k, _ in sink.frames] == [1, 2, 3, 4, 5] and snap.frames == 5
    st.download()
    assert np.array_equal(sink.frames[-1][2]["phi_M_1"], s.phi_M_prev[1].x._a)
    snap.close()


def test_attach_rules(hip_lib):
    from test_events_gpu import _stepper
    s, st, _ = _stepper()
    snap = _define(_snap(s), s, "results")
    for kw in (dict(every=0), dict(every=-2), dict(depth=0), dict(depth=-1)):
        with pytest.raises(ValueError):
            st.snapshot(snap, **kw)
    with pytest.raises(ValueError, match="nothing"):
        st.snapshot(_snap(s))
    assert "snapshot" not in st.taps and st.dp.lib.knpemi_snapshot_pending(st.dp.h) == 0
    st.snapshot(snap)
    with pytest.raises(RuntimeError, match="already"):       # a second snapshot() on the stepper
        st.snapshot(_define(_snap(s), s, "results"))
    s2, st2, _ = _stepper()
    with pytest.raises(RuntimeError, match="already"):       # a Snapshots object that is attached already
        st2.snapshot(snap)
    snap.close()


def test_driver_snapshots_write_the_files_of_the_default(hip_lib, tmp_path):
    """The stim driver, 6 steps on its smallest mesh: the host loop with --snapshots writes the step_*.npz of the default
    path, key for key and bit for bit, and the XDMF series byte for byte; device-resident, the saved fields are those the
    default path downloads."""
    spec = importlib.util.spec_from_file_location("run_stim_duration", os.path.join(
        ROOT, "examples", "local_astrocyte_depolarization", "run_stim_duration.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    cfg = drv.load_config("baseline")
    cfg.update(delay=0.2, period=0.6, pulse_width=0.3, end_time=5.0, save_frequency=4, f_value=97)
    out = {}
    for name, kw in (("host", dict()), ("host_snap", dict(snapshots=True)),
                     ("dev", dict(device_resident=True, extrapolate_guess=False)),
                     ("dev_snap", dict(device_resident=True, extrapolate_guess=False, snapshots=True))):
        d = tmp_path / name
        with contextlib.redirect_stdout(io.StringIO()):
            p, hist = drv.solve_system(dict(cfg), n_steps=6, outdir=str(d), quiet=True, xdmf=True, **kw)
        out[name] = (d, p, hist)
    for a, b in (("host", "host_snap"), ("dev", "dev_snap")):
        da, db = out[a][0], out[b][0]
        assert sorted(os.listdir(da)) == sorted(os.listdir(db))
        assert [f for f in sorted(os.listdir(da)) if f.endswith(".npz")] == ["step_000000.npz", "step_000004.npz", "step_000005.npz"]
        from test_snapshots_host import _same_series
        assert _same_series(da, db) >= 3 * (3 * 3 + 2)
        for f in sorted(os.listdir(da)):
            if f.endswith(".npz"):
                with np.load(da / f) as fa, np.load(db / f) as fb:
                    assert fa.files == fb.files
                    for key in fa.files:
                        assert fa[key].dtype == fb[key].dtype and fa[key].tobytes() == fb[key].tobytes(), (f, key)
        ha, hb = out[a][2], out[b][2]
        for key in ("t", "source", "phi_M_neuron", "phi_M_glia", "K_ecs_max", "its_emi", "its_knp"):
            assert ha[key] == hb[key], key
        pa, pb = out[a][1], out[b][1]
        for tag in (1, 2):                                   # the one download at the end brings the final state
            assert np.array_equal(pa.phi_M_prev[tag].x._a, pb.phi_M_prev[tag].x._a)
