"""GPU tests of the field snapshots of a DG run (csrc/kernels_dg_snapshot.hip, knpemi_dg_snapshot_*): the frames against
`DGSnapshots.frame_host` fed by the `get_*` downloads -- the numpy restatement over the download path the handle had
before, never the pack kernel -- bit for bit; the ring; a whole run of the driver; refusals and recovery."""
import ctypes as C
import functools

import numpy as np
import pytest

from knpemi import _lib as L

pytestmark = pytest.mark.gpu

P64 = C.POINTER(C.c_int64)
ZS = [1.0, -1.0, 2.0, -1.0]


def _mesh(case):
    from knpemi.fem import create_box, create_unit_square
    from knpemi.fem.idealized import _tag
    if case == "fan":                                  # Delaunay mesh with fan vertices of valence 12 and more
        from unstructured_meshes import fan_mesh
        return fan_mesh(2)
    if case == "tri":
        mesh = create_unit_square(None, 8, 8)
    else:
        mesh = create_box(None, [np.zeros(3), np.ones(3)], (4, 4, 4), "tetrahedron" if case == "tet" else "hexahedron")
    d = mesh.x.shape[1]
    ct, ft = _tag(mesh, [([0.25] * d, [0.75] * d)], [1], full_facet_tags=False)
    if case == "hex":                                  # general trilinear cells: the interior vertices moved
        rng = np.random.default_rng(5)
        inner = np.all((mesh.x > 1e-9) & (mesh.x < 1 - 1e-9), axis=1)
        mesh.x[inner] += (0.18 / 4) * (rng.random((inner.sum(), 3)) - 0.5)
    return mesh, ct, ft


def _problem(case, K, bind=True, seed=1):
    """A DGProblem with a random, non-smooth state -- every coincident dof differs -- and a random ODE table."""
    import knpemi_oracle as ko
    from knpemi.dg import DGProblem
    mesh, ct, ft = _mesh(case)
    dp = DGProblem(mesh, ct, ft, [0, 1], [1], n_ions=K)
    rng = np.random.default_rng(seed)
    shape, mshape = (dp.n_cells, dp.nv), (dp.nmf, dp.nf)
    ions = [dict(name=f"i{k}", z=ZS[k], D=[1.0 + 0.3 * k, 0.6 + 0.2 * k]) for k in range(K)]
    dp.set_params(dict(dt=0.05, F=1.3, psi=0.8, C_M=0.7), ions)
    for k in range(K):
        dp.set_concentration(k, 2.0 + k + rng.standard_normal(shape))
        dp.set_channel_current(k, 0.3 * rng.standard_normal(mshape))
    dp.set_potential(0.1 + rng.standard_normal(shape))
    dp.set_membrane_potential(0.2 + 0.1 * rng.standard_normal(mshape))
    if bind:
        m = ko.MODELS["hh_si"]
        n_p = len(m["params"])
        dp.ode_bind(L.MODEL_HH_SI, rng.random((dp.nmf * dp.nf, len(m["states"]))), np.array(m["params"], float),
                    [(3 * k + j) % n_p for k in range(K) for j in range(3)], m["V"])
    return (mesh, ct, ft), dp


def _snapshots(meshdata, K, sink=None):
    from knpemi.dg_snapshots import DGSnapshots
    return DGSnapshots(*meshdata, [0, 1], [1], [f"i{k}" for k in range(K)], sink=sink, writer="inline")


def _watch_everything(snap, K, states=True):
    """Every quantity in every form as float64; phi, the eliminated ion, phi_M and a state also as float32."""
    for form in ("broken", "cell_mean", "vertex"):
        for tag in (0, 1):
            snap.watch(f"phi_{tag}_{form}", "phi", tag, form=form)
            for k in range(K):
                snap.watch(f"c{k}_{tag}_{form}", "c", tag, ion=k, form=form)
            snap.watch(f"phi_{tag}_{form}_f4", "phi", tag, form=form, dtype="f4")
            snap.watch(f"c{K - 1}_{tag}_{form}_f4", "c", tag, ion=K - 1, form=form, dtype="f4")
        if form == "cell_mean":
            continue
        snap.watch(f"phi_M_{form}", "phi_M", 1, form=form)
        snap.watch(f"phi_M_{form}_f4", "phi_M", 1, form=form, dtype="f4")
        for k in range(K):
            snap.watch(f"I{k}_{form}", "I_ch", 1, ion=k, form=form)
        if states:
            snap.watch(f"s0_{form}", "state", 1, state=0, form=form)
            snap.watch(f"s2_{form}_f4", "state", 1, state=2, form=form, dtype="f4")


def _downloads(dp, states=True):
    """What the handle offered before: one blocking download per field."""
    return dict(phi=dp.get_potential(), c=[dp.get_concentration(k) for k in range(dp.K)],
                phi_M=dp.get_membrane_potential(), I_ch=[dp.get_channel_current(k) for k in range(dp.K)],
                states=dp.ode_tables()[0] if states else None)


def _same_bytes(got, want):
    assert list(got) == list(want)
    for name in want:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        assert np.array_equal(got[name].view(np.uint8), want[name].view(np.uint8)), name


@functools.lru_cache(maxsize=None)
def _recorded(case, K, selection):
    """(snap, the frame the device packed, the restatement of the downloads), computed once per case."""
    from knpemi.dg_snapshots import MemorySink
    meshdata, dp = _problem(case, K)
    mem = MemorySink()
    snap = _snapshots(meshdata, K, mem)
    _watch_everything(snap, K)
    if selection:
        for tag in (0, 1):
            for form in ("broken", "cell_mean", "vertex"):
                n = snap.space(tag, form).n
                snap.select(tag, form, indices=np.unique(np.r_[0, np.arange(1, n, 3), n - 1]))
        snap.select(1, "broken", indices=np.arange(0, snap.nq, 2), membrane=True)
        snap.select(1, "vertex", box=([0.0] * meshdata[0].x.shape[1], [0.6] * meshdata[0].x.shape[1]), membrane=True)
    dp.snapshot(snap, depth=2)
    dp.record(1.0)
    snap.flush()
    want = snap.frame_host(**_downloads(dp))
    assert len(mem.frames) == 1 and mem.frames[0][:2] == (1.0, 1)
    return snap, mem.frames[0][2], want, dp


@pytest.mark.parametrize("case,K,selection", [("tri", 3, False), ("tri", 4, False), ("tet", 3, False), ("tet", 4, False),
                                              ("hex", 3, False), ("fan", 3, False), ("tri", 3, True)])
def test_frames_are_bit_identical_to_the_restatement(hip_lib, case, K, selection):
    snap, got, want, dp = _recorded(case, K, selection)
    _same_bytes(got, want)
    # the case is what it claims to be: spaces below and above one workgroup with a partial last one, coincident dofs that
    # differ, a high-valence vertex on the fan mesh
    n = {name: a.shape[0] for name, a in want.items()}
    if case == "tri" and not selection:
        assert n["phi_0_broken"] == 288 and n["phi_1_broken"] == 96 and n["phi_0_cell_mean"] == 96
    S = snap.space(0, "vertex")
    valence = np.diff(S.vptr)
    phi = dp.get_potential().ravel()
    assert all(len(set(phi[S.vdof[S.vptr[i]:S.vptr[i + 1]]])) == valence[i] for i in range(S.n))
    assert valence.max() >= (12 if case == "fan" else 2)
    # the eliminated ion is not a copy of another slot, and the means differ from any single dof
    last = f"c{K - 1}_0_broken"
    assert all(not np.array_equal(want[last], want[f"c{k}_0_broken"]) for k in range(K - 1))
    shared = (valence > 1)[snap._items(snap.watches["phi_0_vertex"])]
    assert shared.any() and not np.any(np.isin(want["phi_0_vertex"][shared], phi))


def test_layout_and_alignment_on_the_device(hip_lib):
    snap, got, want, dp = _recorded("tri", 3, True)
    watches, nbytes = snap._layout
    assert (watches, nbytes) == snap.layout_host() and all(off % L.SNAPSHOT_ALIGN == 0 for _, _, off, _ in watches)
    assert [w[3] for w in watches] == [want[w[0]].shape[0] for w in watches]


def _raw_set(dp, snap, depth, spec=None, space=None):
    sp, spc, list_off, lst, sel_space, sel_off, sel_idx = snap.table()
    sp = sp if spec is None else np.ascontiguousarray(spec, np.int32)
    spc = spc if space is None else np.ascontiguousarray(space, np.int32)
    m = len(sel_space)
    return dp.lib.knpemi_dg_snapshot_set(dp.h, sp.shape[0], L.iptr(sp.ravel()), spc.shape[0], L.iptr(spc.ravel()),
                                         list_off.ctypes.data_as(P64), L.iptr(lst), m, L.iptr(sel_space) if m else None,
                                         sel_off.ctypes.data_as(P64) if m else None, L.iptr(sel_idx) if m else None, depth)


def _error():
    return L.load().knpemi_last_error().decode()


def test_ring(hip_lib):
    meshdata, dp = _problem("tri", 3)
    snap = _snapshots(meshdata, 3)
    snap.watch("phi", "phi", 0, form="vertex")
    snap.watch("pm", "phi_M", 1)
    lib, h = dp.lib, dp.h
    assert lib.knpemi_dg_snapshot_pending(h) == 0
    assert _raw_set(dp, snap, 2) == L.OK
    off, cnt, nbytes = np.zeros(2, np.int64), np.zeros(2, np.int64), C.c_int64()
    L.check(lib.knpemi_dg_snapshot_layout(h, off.ctypes.data_as(P64), cnt.ctypes.data_as(P64), C.byref(nbytes)))
    buf = np.zeros(nbytes.value, np.uint8)
    t, seq = C.c_double(), C.c_int64()
    take = lambda wait=1: lib.knpemi_dg_snapshot_take(h, wait, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(t), C.byref(seq))
    assert take() == 1                                      # nothing in flight
    fields = []
    for k, time in enumerate((0.5, 1.0)):
        dp.set_potential(np.full((dp.n_cells, dp.nv), 10.0 + k))
        fields.append(snap.frame_host(phi=dp.get_potential(), phi_M=dp.get_membrane_potential()))
        assert lib.knpemi_dg_snapshot_record(h, time) == L.OK
    assert lib.knpemi_dg_snapshot_pending(h) == 2
    assert lib.knpemi_dg_snapshot_record(h, 1.5) == L.EBUSY and "in flight" in _error()
    assert lib.knpemi_dg_snapshot_pending(h) == 2           # nothing enqueued
    for k, time in enumerate((0.5, 1.0)):
        assert take() == L.OK and (t.value, seq.value) == (time, k)
        phi = np.frombuffer(buf, np.float64, count=int(cnt[0]), offset=int(off[0]))
        assert np.array_equal(phi, fields[k]["phi"]) and np.all(phi == 10.0 + k)
        assert np.array_equal(np.frombuffer(buf, np.float64, count=int(cnt[1]), offset=int(off[1])), fields[k]["pm"])
    assert take() == 1 and lib.knpemi_dg_snapshot_pending(h) == 0
    assert lib.knpemi_dg_snapshot_take(h, 1, buf.ctypes.data_as(C.c_void_p), buf.size - 8, None, None) == 1
    # the refused record left the clock where it was: 1.5 is accepted now, an earlier time is not
    assert lib.knpemi_dg_snapshot_record(h, 1.0) == L.EINVAL and "greater than the previous" in _error()
    assert lib.knpemi_dg_snapshot_record(h, 1.5) == L.OK
    assert lib.knpemi_dg_snapshot_take(h, 1, buf.ctypes.data_as(C.c_void_p), buf.size - 8, None, None) == L.EINVAL
    assert lib.knpemi_dg_snapshot_pending(h) == 1
    # after a reset the sequence and the clock restart, the frame in flight is dropped
    L.check(lib.knpemi_dg_snapshot_reset(h))
    assert lib.knpemi_dg_snapshot_pending(h) == 0 and take() == 1
    assert lib.knpemi_dg_snapshot_record(h, 0.25) == L.OK and take() == L.OK and (t.value, seq.value) == (0.25, 0)
    L.check(lib.knpemi_dg_snapshot_clear(h))
    assert lib.knpemi_dg_snapshot_record(h, 2.0) == L.EINVAL and "knpemi_dg_snapshot_set" in _error()


def _run(steps, **kw):
    import run_2D_dg
    run = run_2D_dg.DGRun(1, **kw)
    marks = []
    for k in range(steps):
        run.step()
        if (k + 1) % 5 == 0:
            marks.append((run.time, k + 1, _downloads(run.dp)))
    return run, marks


def test_whole_run_of_the_driver(hip_lib):
    """20 steps saving every fifth: the four frames are the restatement of the downloads a second, identical run takes at
    those steps, and saving changes nothing of the run."""
    from knpemi.dg_snapshots import MemorySink
    mem = MemorySink()
    run, _ = _run(20, snapshots=True, save_every=5, sinks=[mem])
    run.snap.flush()
    plain, marks = _run(20)
    assert [(t, k) for t, k, _ in mem.frames] == [(t, k) for t, k, _ in marks] and len(marks) == 4
    assert run.snap.frames == 4 and run.snap.stalls == 0
    for (_, _, frame), (_, _, d) in zip(mem.frames, marks):
        _same_bytes(frame, run.snap.frame_host(**d))
    assert list(mem.frames[0][2]) == ["phi_0", "K_0", "Cl_0", "Na_0", "phi_1", "K_1", "Cl_1", "Na_1", "phi_M_1"]
    a, b = _downloads(run.dp), marks[-1][2]
    for key in ("phi", "phi_M", "states"):
        assert np.array_equal(a[key], b[key]), key
    for key in ("c", "I_ch"):
        assert all(np.array_equal(x, y) for x, y in zip(a[key], b[key])), key
    assert np.array_equal(run.dp.ode_tables()[1], plain.dp.ode_tables()[1]) and run.iterations == plain.iterations
    # reset_recorders rewinds the ring: the next frame is record 5 of a new series
    run.dp.reset_recorders()
    for _ in range(5):
        run.dp.record(run.time + 1.0 + _)
    run.save()
    assert mem.frames[-1][1] == 5 and run.snap.frames == 1


def test_refusals_and_recovery(hip_lib):
    from knpemi.dg import DGSlab
    from knpemi.dg_snapshots import MemorySink
    meshdata, dp = _problem("tri", 3, bind=False)
    lib, h = dp.lib, dp.h
    assert lib.knpemi_dg_snapshot_record(h, 1.0) == L.EINVAL and "no snapshots set" in _error()      # record before set
    mem = MemorySink()
    snap = _snapshots(meshdata, 3, mem)
    _watch_everything(snap, 3, states=False)
    with pytest.raises(ValueError, match="no sub-domain with tag 7"):
        snap.watch("x", "phi", 7)
    with pytest.raises(ValueError, match="unknown ion"):
        snap.watch("x", "c", 0, ion=3)
    # a state watch before knpemi_dg_ode_bind, refused by name; these snapshots stay unattached
    st = _snapshots(meshdata, 3)
    st.watch("s", "state", 1, state=0)
    with pytest.raises(L.KnpemiError, match="knpemi_dg_ode_bind"):
        dp.snapshot(st)
    assert st._dev is None and not dp.taps
    dp.snapshot(snap, depth=2)
    with pytest.raises(RuntimeError, match="takes field snapshots already"):
        dp.snapshot(_snapshots(meshdata, 3))
    with pytest.raises(RuntimeError, match="attached"):
        snap.watch("late", "phi", 0)
    with pytest.raises(NotImplementedError, match="DGSlab.snapshot"):
        DGSlab.snapshot(object(), snap)
    # refused sets, each by name; the recorder installed above stays
    spec, space = snap.table()[:2]

    def refused(text, spec=spec, space=space, depth=2):
        assert _raw_set(dp, snap, depth, spec, space) == L.EINVAL and text in _error(), _error()
    bad = spec.copy(); bad[0, 1] = 5
    refused("unknown tag", bad)
    bad = spec.copy(); bad[1, 2] = 3
    refused("ion index out of range", bad)
    bad = spec.copy(); bad[0, 0] = L.DG_ODE_STATE; bad[0, 3] = L.DG_SNAP_BROKEN
    refused("knpemi_dg_ode_bind", bad)
    bad = spec.copy(); bad[0, 0] = L.DG_JUMP
    refused("unknown quantity", bad)
    bad = spec.copy(); bad[0, 3] = 9
    refused("unknown tag or form", bad)
    bad = spec.copy(); bad[0, 4] = 2
    refused("dtype", bad)
    bad = spec.copy(); bad[1] = bad[0]
    refused("listed twice", bad)
    bad = space.copy(); bad[0, 3] += 1
    refused("one entry per item", space=bad)
    bad = space.copy(); bad[0, 1] = 2
    refused("unknown tag", space=bad)
    refused("depth", depth=0)
    lst = snap.table()[3]
    keep = lst[0]
    snap.space(0, "broken").src[0] = dp.n                  # a dof past the end: refused before anything is uploaded
    refused("out of range")
    snap.space(0, "broken").src[0] = keep
    dp.record(1.0)
    snap.flush()
    assert len(mem.frames) == 1
    _same_bytes(mem.frames[0][2], snap.frame_host(**_downloads(dp, states=False)))
    with pytest.raises(L.KnpemiError, match="greater than the previous"):
        dp.record(1.0)
    # the handle assembles and solves as before
    dp.assemble_emi()
    its, rr = dp.solve_emi(rtol=1e-9)
    assert 0 < its < 200 and rr < 1e-9
    dp.record(2.0)
    snap.close()
    assert len(mem.frames) == 2 and mem.frames[1][:2] == (2.0, 3)
    # before knpemi_dg_set_params a record is refused by name
    from knpemi.dg import DGProblem
    fresh = DGProblem(*meshdata, [0, 1], [1])
    s2 = _snapshots(meshdata, 3)
    s2.watch("phi", "phi", 0)
    fresh.snapshot(s2)
    with pytest.raises(L.KnpemiError, match="knpemi_dg_set_params"):
        fresh.record(1.0)
