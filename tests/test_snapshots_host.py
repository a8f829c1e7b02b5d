"""CPU tests of the field snapshots (knpemi.snapshots): the frames of the numpy restatement `record_host`, selections, the
sinks against the driver's own writers, and the writer thread.  (The driver's host loop builds a device problem, so its
`--snapshots` comparison lives with the GPU tests.)"""
import importlib.util
import os
import threading

import numpy as np
import pytest

from knpemi import _lib as L
from knpemi.snapshots import MemorySink, NpzSink, Snapshots, XdmfSink

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "local_astrocyte_depolarization", "run_stim_duration.py")


@pytest.fixture(scope="module")
def s():
    from helpers import Setup
    s = Setup("2d", 1, build_forms=False)
    s.perturb()
    return s


@pytest.fixture(scope="module")
def drv():
    spec = importlib.util.spec_from_file_location("run_stim_duration", DRIVER)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _snap(s, **kw):
    return Snapshots(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list, **kw)


def _host(s):
    return s.phi, s.c, s.c_prev, s.phi_M_prev


def _results(s):
    """What write_results saves, from the host Functions."""
    out = {}
    for tag in s.subdomain_list:
        out[f"phi_{tag}"] = s.phi[tag].x._a
        for k, ion in enumerate(s.ion_list[:-1]):
            out[f"{ion['name']}_{tag}"] = s.c[tag][k].x._a
        out[f"{s.ion_list[-1]['name']}_{tag}"] = s.ion_list[-1][f"c_{tag}"].x._a
        if tag > 0:
            out[f"phi_M_{tag}"] = s.phi_M_prev[tag].x._a
    return out


def _same_series(a, b):
    """The XDMF files of two directories byte for byte, and every dataset they name in the HDF5 files array for array
    (the HDF5 container itself carries modification times)."""
    import re
    from knpemi.fem.hdf5 import File
    names = sorted(f for f in os.listdir(a) if not f.endswith(".npz"))
    assert names == sorted(f for f in os.listdir(b) if not f.endswith(".npz")) and any(f.endswith(".xdmf") for f in names)
    n = 0
    for f in names:
        if not f.endswith(".xdmf"):
            continue
        text = (a / f).read_bytes()
        assert text == (b / f).read_bytes(), f
        with File(str(a / f)[:-5] + ".h5") as ha, File(str(b / f)[:-5] + ".h5") as hb:
            for path in sorted(set(re.findall(r"\.h5:(/[^<\s]+)", text.decode()))):
                x, y = ha.read(path), hb.read(path)
                assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (f, path)
                n += 1
    return n


@pytest.mark.parametrize("dtype", ["f8", "f4"])
def test_frames_of_record_host(s, dtype):
    sink = MemorySink()
    snap = _snap(s, sink=sink, writer="inline")
    snap.watch_results(dtype=dtype)
    snap.watch("K_prev_1", "c_prev", 1, ion="K", dtype=dtype)
    snap.watch("I_Na", "I_ch", 1, ion=2, dtype=dtype)
    snap.watch("gate", "state", 1, model=0, state=1, dtype=dtype)
    frame = snap.record_host(0.25, 7, *_host(s))
    want = _results(s)
    want["K_prev_1"] = s.c_prev[1][0].x._a
    want["I_Na"] = s.mem_models[0]["I_ch_k"]["Na"].x._a
    want["gate"] = s.mem_models[0]["ode"].states[:, 1]
    assert list(frame) == list(want) and len(want) == 4 + 5 + 3
    np_t = np.float64 if dtype == "f8" else np.float32
    for name, a in want.items():
        assert frame[name].dtype == np_t and frame[name].shape == a.shape, name
        assert frame[name].tobytes() == np.asarray(a, np.float64).astype(np_t).tobytes(), name
        assert not np.shares_memory(frame[name], a), name
    assert np.ptp(want["K_0"]) > 0 and np.ptp(want["phi_M_1"]) > 0
    assert sink.frames == [(0.25, 7, frame)] and snap.frames == 1 and snap.stalls == 0
    # the arguments I_ch and states replace the models' own
    nq = s.mem_models[0]["ode"].nodes
    other = snap.frame_host(*_host(s), I_ch={1: [{"Na": np.arange(float(nq))}]},
                            states={(1, 0): np.tile(np.arange(4.0), (nq, 1))})
    assert np.array_equal(other["I_Na"], np.arange(nq)) and np.all(other["gate"] == 1.0)
    snap.close()


def test_definitions_are_checked(s):
    snap = _snap(s)
    snap.watch("a", "phi", 0)
    for args, kw in ((("a", "phi", 1), {}), (("b", "phi", 0), {}), (("b", "rho", 0), {}), (("b", "phi", 5), {}),
                     (("b", "phi_M", 0), {}), (("b", "c", 0), dict(ion="Ca")), (("b", "c", 0), dict(ion=3)),
                     (("b", "c_prev", 0), dict(ion="Na")), (("b", "phi", 0), dict(dtype="f2")),
                     (("b", "state", 1), {}), (("b", "I_ch", 1), dict(ion="K", model=1))):
        with pytest.raises(ValueError):
            snap.watch(*args, **kw)
    snap.watch("b", "phi", 0, dtype="f4")          # the same field in another width is another watch
    with pytest.raises(ValueError, match="nothing"):
        _snap(s).record_host(0.0, 0, *_host(s))
    with pytest.raises(ValueError):
        _snap(s, writer="process")


def test_selections(s):
    x0 = np.asarray(s.subdomain_list[0]["mesh_sub"].x)
    xm = np.asarray(s.subdomain_list[1]["mesh_mem"].x)
    lo, hi = x0.min(axis=0), x0.max(axis=0)
    box = (lo + 0.25 * (hi - lo), lo + 0.5 * (hi - lo))
    inside = np.flatnonzero(np.all((x0 >= box[0]) & (x0 <= box[1]), axis=1))
    assert 0 < inside.size < x0.shape[0]
    snap = _snap(s, writer="inline")
    snap.watch_results()
    snap.watch("K4", "c", 0, ion="K", dtype="f4")
    snap.select(0, box=box)
    mem = np.array([0, 3, xm.shape[0] - 1])
    snap.select(1, membrane=True, indices=mem)
    frame = snap.record_host(0.0, 0, *_host(s))
    want = _results(s)
    for name in ("phi_0", "K_0", "Cl_0", "Na_0"):
        assert np.array_equal(frame[name], want[name][inside]), name
        assert np.array_equal(snap.locations(name), x0[inside])
    assert frame["K4"].tobytes() == want["K_0"][inside].astype(np.float32).tobytes()
    assert np.array_equal(frame["phi_M_1"], want["phi_M_1"][mem]) and np.array_equal(snap.locations("phi_M_1"), xm[mem])
    for name in ("phi_1", "K_1"):                       # the bulk space of the cell carries no selection
        assert np.array_equal(frame[name], want[name])
        assert np.array_equal(snap.locations(name), np.asarray(s.subdomain_list[1]["mesh_sub"].x))
    # a box on a lower-dimensional corner: the closed box keeps the vertices on its faces
    corner = _snap(s)
    corner.watch("phi", "phi", 0)
    corner.select(0, box=(lo, lo))
    assert corner.locations("phi").shape[0] >= 1 and np.all(corner.locations("phi") == lo)
    # refusals
    n = x0.shape[0]
    for kw in (dict(box=(hi + 1.0, hi + 2.0)), dict(indices=[]), dict(indices=[3, 2]), dict(indices=[2, 2]),
               dict(indices=[0, n]), dict(indices=[-1, 0]), dict(), dict(indices=[1], box=box), dict(indices=[0.5])):
        with pytest.raises(ValueError):
            _snap(s).select(0, **kw)
    with pytest.raises(ValueError, match="already"):
        snap.select(0, indices=[1])
    with pytest.raises(ValueError):
        _snap(s).select(0, membrane=True, indices=[0])
    # the table of knpemi_snapshot_set: spaces in the library's numbering, the lists end to end
    spec, sel_space, sel_off, sel_idx = snap.table({0: 0, 1: 1})
    assert spec.shape == (10, 4) and spec.dtype == np.int32 and spec[-1].tolist() == [L.F_C, 0, 0, L.SNAPSHOT_F32]
    assert sel_space.tolist() == [0, L.MAX_SUB + 1] and sel_off.tolist() == [0, inside.size, inside.size + 3]
    assert np.array_equal(sel_idx, np.concatenate([inside, mem]))
    snap.close()


def test_npz_sink_writes_the_files_of_write_results(s, drv, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    snap = _snap(s, sink=NpzSink(str(b), compressed=True))
    snap.watch_results()
    for k, t in ((0, 0.1), (5, 0.6)):
        s.phi[0].x.array[:] = s.phi[0].x._a + 0.5 * k
        drv.write_results(s, str(a), k, t)
        snap.record_host(t, k, *_host(s))
    snap.flush()
    assert snap.frames == 2 and sorted(os.listdir(a)) == sorted(os.listdir(b)) == ["step_000000.npz", "step_000005.npz"]
    for name in os.listdir(a):
        with np.load(a / name) as fa, np.load(b / name) as fb:
            assert fa.files == fb.files
            for key in fa.files:
                assert fa[key].dtype == fb[key].dtype and fa[key].shape == fb[key].shape, key
                assert fa[key].tobytes() == fb[key].tobytes(), key
    snap.close()


def test_xdmf_sink(s, drv, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    ref = drv.XdmfResults(s, str(a))
    snap = _snap(s, sink=XdmfSink(s, str(b)))
    snap.watch_results()
    for t in (0.1, 0.2):
        ref.write(s, t)
        snap.record_host(t, 0, *_host(s))
    ref.close()
    snap.close()
    assert _same_series(a, b) >= 2 * (2 + 3 + 1)       # two steps of phi, the solved ions of two sub-domains, phi_M
    # a selected or a float32 watch cannot feed the series
    for spoil in ("f4", "select", "missing"):
        d = tmp_path / spoil
        d.mkdir()
        sink = XdmfSink(s, str(d))
        snap = _snap(s, sink=sink)
        if spoil == "missing":
            snap.watch("phi_0", "phi", 0)
        else:
            snap.watch_results(dtype="f4" if spoil == "f4" else "f8")
        if spoil == "select":
            snap.select(1, membrane=True, indices=[0, 1])
        with pytest.raises(ValueError, match="XdmfSink"):
            snap.record_host(0.0, 0, *_host(s))
        sink.close()


def test_writer_thread_keeps_the_order_and_surfaces_errors(s):
    seen, threads = [], set()

    gate = threading.Event()

    def slow(t, k, frame):                              # holds frame 0 until the queue behind it is full
        threads.add(threading.get_ident())
        if k == 0:
            assert gate.wait(timeout=30)
        seen.append((t, k, float(frame["phi_0"][0])))
    snap = _snap(s, sink=slow)
    snap.depth = 2
    snap.watch("phi_0", "phi", 0)
    base = s.phi[0].x._a.copy()
    for k in range(8):                                  # more frames than the queue holds: put blocks, nothing is dropped
        s.phi[0].x.array[:] = base + k
        if k == 3:
            assert snap._w.q.full() and seen == [] and snap.frames == 0
            gate.set()
        snap.record_host(0.1 * k, k, *_host(s))
    snap.flush()
    s.phi[0].x.array[:] = base
    assert seen == [(0.1 * k, k, base[0] + k) for k in range(8)] and snap.frames == 8
    assert threads == {snap._w.thread.ident} and threading.get_ident() not in threads
    assert snap._w.q.empty() and snap._w.q.unfinished_tasks == 0
    snap.close()
    assert snap.frames == 8

    # a sink that raises on frame 2: the error reaches the stepping thread at the next record or at flush()
    def bad(t, k, frame):
        if k == 2:
            raise OSError("disk full")
        seen.append(k)
    for how in ("record", "flush"):
        del seen[:]
        snap = _snap(s, sink=bad)
        snap.watch("phi_0", "phi", 0)
        for k in range(3):
            snap.record_host(0.0, k, *_host(s))
        with pytest.raises(OSError, match="disk full"):
            if how == "flush":
                snap.flush()
            else:
                snap._w.q.join()
                snap.record_host(0.0, 3, *_host(s))
        assert seen == [0, 1] and snap.frames == 2
        snap.flush()                                    # the error was raised once; the queue is empty
        assert snap._w.q.unfinished_tasks == 0
        snap.close()
    # inline: the sink runs on the caller's thread and raises there
    snap = _snap(s, sink=bad, writer="inline")
    snap.watch("phi_0", "phi", 0)
    snap.record_host(0.0, 0, *_host(s))
    with pytest.raises(OSError):
        snap.record_host(0.0, 2, *_host(s))
    snap.close()


def test_abi_table_and_constants(hip_lib):
    header = open(os.path.join(ROOT, "include", "knpemi_hip.h")).read()
    import re
    consts = dict(re.findall(r"#define\s+KNPEMI_([A-Z_0-9]+)\s+\(?(-?\d+)\)?", header))
    for name in ("F_ODE_STATE", "SNAPSHOT_MAX_WATCH", "SNAPSHOT_STATE_STRIDE", "SNAPSHOT_F32", "SNAPSHOT_ALIGN", "EBUSY",
                 "K_SNAPSHOT"):
        assert int(consts[name]) == getattr(L, name), name
    assert int(consts["N_KERNELS"]) == len(L.KERNEL_NAMES) and L.KERNEL_NAMES[L.K_SNAPSHOT] == "snapshot_pack_kernel"
    for name in ("set", "layout", "record", "take", "pending", "reset", "clear"):
        assert f"knpemi_snapshot_{name}" in L.SIGNATURES and hasattr(hip_lib, f"knpemi_snapshot_{name}")
    # without a handle every entry point refuses (pending counts nothing)
    assert hip_lib.knpemi_snapshot_record(None, 0.0) == L.EINVAL and hip_lib.knpemi_snapshot_reset(None) == L.EINVAL
    assert hip_lib.knpemi_snapshot_take(None, 0, None, 0, None, None) == L.EINVAL
    assert hip_lib.knpemi_snapshot_pending(None) == 0 and hip_lib.knpemi_snapshot_clear(None) == L.EINVAL
    import knpemi
    assert knpemi.Snapshots is Snapshots and "Snapshots" in knpemi.__all__
