"""Field snapshots: the watched fields of a device-resident run, packed into one frame on the device, copied out by a
stream of its own and written off the stepping thread.

The reference's astrocyte study writes every field every `save_frequency` steps
(`examples/local_astrocyte_depolarization/run_stim_duration.py:52-90, 446-460, 487-494`: `results_sub_<tag>.xdmf`,
`results_mem_<tag>.xdmf` and the ADIOS2 checkpoints).  With the fields resident on the device that meant
`DeviceStepper.download()` -- one strided gather and one blocking copy per field, every ODE table too -- and then the
compression and the XDMF writes on the stepping thread while the GPU idles.  Here every `every`-th step ONE launch packs
the watched fields into a contiguous frame (csrc/kernels_snapshot.hip), a copy stream takes the frame to pinned host
memory, and a writer thread hands it to the sinks; the main stream never waits for the host and no frame is dropped or
overwritten.

    snap = Snapshots(mesh, ct, ft, subdomain_list, ion_list, sink=NpzSink(outdir))
    snap.watch_results()                                   # what the driver's write_results saves, under its keys
    snap.watch("m_gate", "state", tag=1, model=0, state=0, dtype="f4")
    snap.select(0, box=(lo, hi))                           # the ECS watches store the vertices inside the box only
    stepper.snapshot(snap, every=5, depth=4, t0=0.0)       # ... stepper.step() ...
    snap.flush()                                           # every frame recorded so far has reached the sinks
    snap.close()

A watch is a quantity -- "phi", "c" (any ion, the eliminated one included), "c_prev", "phi_M", "I_ch", "state" (a
component of a membrane model's state table) -- of sub-domain `tag`, stored as float64 ("f8", bit for bit) or as float32
("f4": `np.float32(v)`, round to nearest even).  Watches group by space: the vertices of the sub-mesh, or the membrane
dofs of cell `tag` for phi_M, I_ch and states.  A space may carry a selection (an ascending list of distinct items, or a
box); every watch of the space then stores only those items, in list order.  A frame is the dictionary {name: array}; a
sink is any callable `sink(t, k, frame)` and gets the frames in record order.

The ring.  The device keeps `depth` slots (a device frame, a pinned host frame, an event each).  One tick of the
stepper's tap takes every frame whose copy is done (a poll, no wait) and queues it to the writer, records, and when the
ring is full waits for the oldest frame alone (`stalls` counts these) and records again.  The writer is one daemon
thread behind a queue of `depth` frames; when the queue is full the stepping thread blocks there (back-pressure, never a
drop; `waits` counts these).  An exception in a sink is kept and raised on the stepping thread at the next tick or
`flush()`.

`record_host` is the numpy restatement: the same frame dictionary from host `Function`s into the same sinks.  Host loops
save through it, and it is the reference of the device tests.

Cell-partitioned runs need no communication: every rank snapshots its local items.  `select_owned(halo)` sets the
selection of every watched space to the items this rank owns and `global_ids(name, halo)` numbers them globally, so the
ranks' files can be merged.
"""
from __future__ import annotations

import ctypes as C
import os
import queue
import threading
import types

import numpy as np

from . import _lib as L
from .recording import nodal_values as _values

QUANTITIES = ("phi", "c", "c_prev", "phi_M", "I_ch", "state")
MEMBRANE = ("phi_M", "I_ch", "state")
DTYPES = {"f8": np.float64, "f4": np.float32}
_BUSY = object()


class _Watch:
    __slots__ = ("name", "quantity", "tag", "ion", "model", "state", "dtype")

    @property
    def membrane(self):
        return self.quantity in MEMBRANE

    @property
    def space(self):
        return (self.tag, self.membrane)


class _Nodal:
    """What `XDMFFile.write_function` reads of a Function: its name and nodal array."""

    def __init__(self, name, a):
        self.name, self.x = name, types.SimpleNamespace(_a=a, array=a)


# -- sinks -------------------------------------------------------------------------------------------------
class MemorySink:
    """Keeps every frame: `frames` is the list of (t, k, {name: array})."""

    def __init__(self):
        self.frames = []

    def __call__(self, t, k, frame):
        self.frames.append((t, k, frame))


class NpzSink:
    """`step_%06d.npz` (step k + k_offset) with `t` and the watches under their names: with `watch_results()` the files the
    driver's `write_results` writes, array for array."""

    def __init__(self, outdir, compressed=True, k_offset=0):
        self.outdir, self.compressed, self.k_offset = outdir, bool(compressed), int(k_offset)
        os.makedirs(outdir, exist_ok=True)

    def __call__(self, t, k, frame):
        save = np.savez_compressed if self.compressed else np.savez
        save(os.path.join(self.outdir, f"step_{k + self.k_offset:06d}.npz"), t=t, **frame)


class XdmfSink:
    """The `results_sub_<tag>.xdmf` / `results_mem_<tag>.xdmf` time series the driver's `XdmfResults` writes
    (run_stim_duration.py:52-90, 446-460 of the reference), through `knpemi.fem.XDMFFile`, from the frames of
    `watch_results()`.  p: anything with `subdomain_list`, `ion_list`, `phi`, `c` and `phi_M_prev` (the written Functions
    give the names).  Needs the unselected "f8" watches phi_<tag>, <solved ion>_<tag>, phi_M_<tag>: ValueError otherwise."""

    def __init__(self, p, outdir):
        from .fem import XDMFFile
        self.p, self.sub, self.mem = p, {}, {}
        for tag, sd in p.subdomain_list.items():
            self.sub[tag] = XDMFFile(None, os.path.join(outdir, f"results_sub_{tag}.xdmf"), "w")
            self.sub[tag].write_mesh(sd["mesh_sub"])
            if tag > 0:
                self.mem[tag] = XDMFFile(None, os.path.join(outdir, f"results_mem_{tag}.xdmf"), "w")
                self.mem[tag].write_mesh(sd["mesh_mem"])

    def _written(self):
        """[(file, Function name, watch name, number of values)] in the order `XdmfResults.write` writes."""
        p, out = self.p, []
        for tag, sd in p.subdomain_list.items():
            n = int(sd["mesh_sub"].num_vertices)
            out.append((self.sub[tag], p.phi[tag].name, f"phi_{tag}", n))
            for ion, f in zip(p.ion_list[:-1], p.c[tag]):
                out.append((self.sub[tag], f.name, f"{ion['name']}_{tag}", n))
            if tag > 0:
                out.append((self.mem[tag], p.phi_M_prev[tag].name, f"phi_M_{tag}", int(sd["mesh_mem"].num_vertices)))
        return out

    def check(self, snap):
        for _, _, name, _ in self._written():
            w = snap.watches.get(name)
            if w is None:
                raise ValueError(f"XdmfSink: no watch {name!r} (Snapshots.watch_results defines the written functions)")
            if w.dtype != "f8":
                raise ValueError(f"XdmfSink: watch {name!r} is stored as float32; the XDMF series needs 'f8'")
            if w.space in snap.selections:
                raise ValueError(f"XdmfSink: watch {name!r} stores a selection; the XDMF series needs every item")

    def __call__(self, t, k, frame):
        for f, fname, name, n in self._written():
            a = frame[name]
            if a.dtype != np.float64 or a.shape != (n,):
                raise ValueError(f"XdmfSink: watch {name!r} does not hold the {n} float64 values of its function")
            f.write_function(_Nodal(fname, a), t)

    def close(self):
        for f in list(self.sub.values()) + list(self.mem.values()):
            f.close()


# -- the writer ----------------------------------------------------------------------------------------------
class _Writer:
    """Hands (t, k, frame) to the sinks in the order of `put`: on a daemon thread behind a queue of `depth` items, or
    (threaded=False) on the caller's thread.  The first exception of a sink is kept, the frames behind it are not
    delivered, and `check` raises it on the caller's thread."""

    def __init__(self, sinks, depth, threaded):
        self.sinks, self.error, self.delivered = sinks, None, 0
        self.waits = 0                    # puts that found the queue full
        self.q = self.thread = None
        if threaded:
            self.q = queue.Queue(maxsize=max(int(depth), 1))
            self.thread = threading.Thread(target=self._run, name="knpemi-snapshots", daemon=True)
            self.thread.start()

    def _deliver(self, item):
        if self.error is not None:
            return
        try:
            for s in self.sinks:
                s(*item)
            self.delivered += 1
        except BaseException as e:      # noqa: BLE001 -- kept for the stepping thread
            self.error = e

    def _run(self):
        while True:
            item = self.q.get()
            try:
                if item is None:
                    return
                self._deliver(item)
            finally:
                self.q.task_done()

    def check(self):
        if self.error is not None:
            e, self.error = self.error, None
            raise e

    def put(self, item):
        self.check()
        if self.q is None:
            self._deliver(item)
            self.check()
        else:
            if self.q.full():
                self.waits += 1
            self.q.put(item)      # blocks while the queue is full: back-pressure

    def drain(self):
        if self.q is not None:
            self.q.join()
        self.check()

    def close(self):
        if self.thread is not None:
            self.q.put(None)
            self.thread.join()
            self.q = self.thread = None


class Snapshots:
    _ABI = "knpemi_snapshot_"             # the entry points of the ring: knpemi.dg_snapshots.DGSnapshots names the DG handle's

    def _abi(self, name):
        return getattr(self._dev[0], self._ABI + name)

    def __init__(self, mesh, ct, ft, subdomain_list, ion_list, sink=None, writer="thread"):
        """sink: a callable `sink(t, k, frame)` or a list of them (`add_sink` adds more); writer: "thread" (one daemon
        thread behind a bounded queue) or "inline" (the sinks run on the stepping thread)."""
        if writer not in ("thread", "inline"):
            raise ValueError("writer must be 'thread' or 'inline'")
        self.mesh, self.ct, self.ft = mesh, ct, ft
        self.subdomain_list, self.ion_list = subdomain_list, ion_list
        self.tags = list(subdomain_list.keys())
        self.ion_names = [ion["name"] for ion in ion_list]
        self.watches = {}                 # name -> _Watch, in the order of the frame
        self.selections = {}              # (tag, membrane) -> ascending int32 item indices
        self.sinks = [] if sink is None else (list(sink) if isinstance(sink, (list, tuple)) else [sink])
        self.writer = writer
        self.stalls = 0
        self.depth = 4
        self._delivered = 0               # frames delivered by a writer that is closed
        self._w = None                    # the _Writer, started by the first frame or the attach
        self._dev = None                  # (lib, handle) once attached
        self._drain = None                # `flush` while attached (DeviceStepper._attach asks)
        self._layout = None               # [(name, dtype, byte offset, items)], frame bytes
        self._ks = []                     # step numbers of the frames in flight, oldest first
        self._t_of = {}                   # step -> the time `retime` gave its frame

    # -- definition ------------------------------------------------------------------------------------
    def _defining(self):
        if self._dev is not None:
            raise RuntimeError("these snapshots are attached to a device problem: define watches and selections before "
                               "snapshot()")

    def _models(self, tag):
        return self.subdomain_list[tag].get("mem_models", [])

    def watch(self, name, quantity, tag, ion=None, model=None, state=None, dtype="f8"):
        """Watch `quantity` on sub-domain `tag`: "phi"; "c" or "c_prev" of `ion` (name or index; "c" of the eliminated ion
        is its `c_<tag>`, "c_prev" exists for the solved ions); "phi_M"; "I_ch" of `ion` of membrane model `model`
        (default 0); "state": component `state` (index, or a name the model's `state_indices` knows) of the state table
        of membrane model `model`.  dtype: "f8" stores the doubles, "f4" `np.float32` of them."""
        self._defining()
        if name in self.watches:
            raise ValueError(f"watch {name!r} defined twice")
        if quantity not in QUANTITIES:
            raise ValueError(f"quantity must be one of {QUANTITIES}")
        if tag not in self.subdomain_list:
            raise ValueError(f"no sub-domain with tag {tag}")
        if dtype not in DTYPES:
            raise ValueError("dtype must be 'f8' or 'f4'")
        if len(self.watches) == L.SNAPSHOT_MAX_WATCH:
            raise ValueError(f"at most {L.SNAPSHOT_MAX_WATCH} watches")
        w = _Watch()
        w.name, w.quantity, w.tag, w.dtype = name, quantity, tag, dtype
        w.ion = w.model = w.state = None
        if w.membrane and tag == 0:
            raise ValueError("the ECS (tag 0) has no membrane: give the tag of a cell")
        if quantity in ("c", "c_prev", "I_ch"):
            k = self.ion_names.index(ion) if ion in self.ion_names else ion
            if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 0 <= k < len(self.ion_names):
                raise ValueError(f"unknown ion {ion!r} (ions: {self.ion_names})")
            if quantity == "c_prev" and k == len(self.ion_names) - 1:
                raise ValueError("c_prev exists for the solved ions; watch 'c' of the eliminated one")
            w.ion = int(k)
        if quantity in ("I_ch", "state"):
            w.model = 0 if model is None else int(model)
            if not 0 <= w.model < max(len(self._models(tag)), 1) or w.model >= L.MAX_MODELS:
                raise ValueError(f"sub-domain {tag} has no membrane model {w.model}")
        if quantity == "state":
            if isinstance(state, str):
                state = self._models(tag)[w.model]["ode"].ode.state_indices(state)
            if state is None or not 0 <= int(state) < L.SNAPSHOT_STATE_STRIDE:
                raise ValueError("a state watch needs state=: the component of the model's state table")
            w.state = int(state)
        for o in self.watches.values():
            if (o.quantity, o.tag, o.ion, o.model, o.state, o.dtype) == (quantity, tag, w.ion, w.model, w.state, dtype):
                raise ValueError(f"watch {name!r} repeats watch {o.name!r}")
        self.watches[name] = w

    def watch_results(self, dtype="f8"):
        """Exactly what the driver's `write_results` saves, under its keys: phi_<tag>, <ion>_<tag> of every ion (the
        solver's c; the eliminated ion's c_<tag>) and phi_M_<tag> of every cell."""
        for tag in self.subdomain_list:
            self.watch(f"phi_{tag}", "phi", tag, dtype=dtype)
            for name in self.ion_names:
                self.watch(f"{name}_{tag}", "c", tag, ion=name, dtype=dtype)
            if tag > 0:
                self.watch(f"phi_M_{tag}", "phi_M", tag, dtype=dtype)

    def _mesh(self, tag, membrane):
        return self.subdomain_list[tag]["mesh_mem" if membrane else "mesh_sub"]

    def _n_space(self, tag, membrane):
        return int(self._mesh(tag, membrane).num_vertices)

    def select(self, tag, membrane=False, box=None, indices=None):
        """The selection of a space -- the vertices of sub-domain `tag`, or with membrane=True the membrane dofs of cell
        `tag`: every watch of the space stores only these items, in ascending order.  box=(lo, hi): the items whose
        coordinates lie in the closed box; indices: ascending distinct item indices.  ValueError for an empty, unsorted,
        repeated or out-of-range selection and for a second selection of one space."""
        self._defining()
        if tag not in self.subdomain_list or (membrane and tag == 0):
            raise ValueError(f"no such space: tag {tag}, membrane={membrane}")
        if (box is None) == (indices is None):
            raise ValueError("give box=(lo, hi) or indices=")
        if (tag, bool(membrane)) in self.selections:
            raise ValueError(f"the space (tag {tag}, membrane={bool(membrane)}) has a selection already")
        n = self._n_space(tag, membrane)
        if box is not None:
            x = np.asarray(self._mesh(tag, membrane).x, np.float64)
            lo, hi = (np.asarray(b, np.float64) for b in box)
            idx = np.flatnonzero(np.all((x >= lo) & (x <= hi), axis=1))
        else:
            idx = np.asarray(indices)
            if idx.ndim != 1 or (idx.size and not np.issubdtype(idx.dtype, np.integer)):
                raise ValueError("indices must be a list of integers")
        if idx.size == 0:
            raise ValueError("empty selection")
        if idx.min() < 0 or idx.max() >= n:
            raise ValueError(f"selection index out of range (the space has {n} items)")
        if np.any(np.diff(idx) <= 0):
            raise ValueError("selection indices must be ascending and distinct")
        self.selections[(tag, bool(membrane))] = np.ascontiguousarray(idx, np.int32)

    def _items(self, w):
        """The item indices watch w stores."""
        sel = self.selections.get(w.space)
        return np.arange(self._n_space(*w.space), dtype=np.int32) if sel is None else sel

    def _check(self, name):
        if name not in self.watches:
            raise ValueError(f"no watch {name!r}")
        return self.watches[name]

    def locations(self, name):
        """(n, gdim) coordinates of the stored items of watch `name`, in the order of its array."""
        w = self._check(name)
        return np.array(self._mesh(*w.space).x, np.float64)[self._items(w)]

    # -- cell partitions ---------------------------------------------------------------------------------
    def _owners(self, w, halo):
        mem = w.membrane
        own = np.asarray(halo.vertex_owner("mem" if mem else "bulk"))
        off = total = 0
        for tag in self.subdomain_list:
            if mem and tag == 0:
                continue
            if tag == w.tag:
                off = total
            total += self._n_space(tag, mem)
        if own.shape[0] != total:
            raise ValueError("the halo does not number the items of these sub-domains")
        return own[off:off + self._n_space(*w.space)]

    def select_owned(self, halo):
        """The selection of every watched space becomes the items this rank owns (`halo.vertex_owner("bulk")` /
        `("mem")`, as `FieldMaps.maps(halo=)` decides): the union of the ranks' frames is the global field, every item
        once.  Replaces earlier selections of those spaces; ValueError when the rank owns no item of a watched space."""
        self._defining()
        for w in self.watches.values():
            mine = np.flatnonzero(self._owners(w, halo) == int(halo.rank))
            if mine.size == 0:
                raise ValueError(f"rank {halo.rank} owns no item of the space of watch {w.name!r}")
            self.selections[w.space] = np.ascontiguousarray(mine, np.int32)

    def global_ids(self, name, halo):
        """The global numbers (vertices of the whole mesh) of the stored items of watch `name` on this rank."""
        w = self._check(name)
        s = self.tags.index(w.tag)
        return np.asarray(halo.keys["mem" if w.membrane else "bulk"][s][0], np.int64)[self._items(w)]

    # -- sinks and the writer ------------------------------------------------------------------------------
    def add_sink(self, sink):
        if self._w is not None:
            raise RuntimeError("the writer runs already: add every sink before the first frame")
        self.sinks.append(sink)

    def _open(self, depth=None):
        if self._w is None:
            if not self.watches:
                raise ValueError("nothing is watched")
            for s in self.sinks:
                if hasattr(s, "check"):
                    s.check(self)
            self._w = _Writer(self.sinks, self.depth if depth is None else depth, self.writer == "thread")
        return self._w

    @property
    def frames(self):
        """Frames delivered to the sinks."""
        return self._delivered if self._w is None else self._w.delivered

    @property
    def waits(self):
        """How often the stepping thread found the writer's queue full and had to wait there (back-pressure)."""
        return 0 if self._w is None else self._w.waits

    # -- host restatement --------------------------------------------------------------------------------
    def _sample(self, w, phi, c, c_prev, phi_M_prev, I_ch, states):
        if w.quantity == "phi":
            return _values(phi[w.tag])
        if w.quantity == "phi_M":
            return _values(phi_M_prev[w.tag])
        if w.quantity == "c":
            last = w.ion == len(self.ion_names) - 1
            return _values(self.ion_list[-1][f"c_{w.tag}"] if last else c[w.tag][w.ion])
        if w.quantity == "c_prev":
            return _values(c_prev[w.tag][w.ion])
        if w.quantity == "I_ch":
            if I_ch is not None:
                return _values(I_ch[w.tag][w.model][self.ion_names[w.ion]])
            return _values(self._models(w.tag)[w.model]["I_ch_k"][self.ion_names[w.ion]])
        table = states[(w.tag, w.model)] if states is not None else self._models(w.tag)[w.model]["ode"].states
        return np.asarray(table, np.float64)[:, w.state]

    def frame_host(self, phi, c, c_prev, phi_M_prev, I_ch=None, states=None):
        """{name: array} of every watch from host data, as the device packs it: the stored items, float64 as they are or
        `np.float32` of them."""
        out = {}
        for name, w in self.watches.items():
            v = self._sample(w, phi, c, c_prev, phi_M_prev, I_ch, states)
            if v.shape != (self._n_space(*w.space),):
                raise ValueError(f"watch {name!r}: {v.shape[0]} values for {self._n_space(*w.space)} items")
            sel = self.selections.get(w.space)
            v = v.copy() if sel is None else v[sel]
            with np.errstate(over="ignore", invalid="ignore"):      # beyond the floats' range: +-inf, as the device stores
                out[name] = v.astype(np.float32) if w.dtype == "f4" else v
        return out

    def record_host(self, t, k, phi, c, c_prev, phi_M_prev, I_ch=None, states=None):
        """One frame at time t of step k from host data -- phi[tag], c[tag][j] and c_prev[tag][j] (solved ions; the
        eliminated one is read from ion_list[-1]["c_<tag>"]), phi_M_prev[tag] are `Function`s or arrays; I_ch[tag][model]
        [ion name] and states[(tag, model)] ([dofs][components]) default to those of subdomain_list[tag]["mem_models"] --
        into the sinks, through the writer.  The numpy restatement of the device path: host loops save with it, and it is
        the reference of the device tests.  Returns the frame."""
        frame = self.frame_host(phi, c, c_prev, phi_M_prev, I_ch, states)
        self._open().put((float(t), int(k), frame))
        return frame

    # -- the device ring -----------------------------------------------------------------------------------
    def _field(self, w):
        """(field id, index) of knpemi_snapshot_set."""
        if w.quantity == "phi":
            return L.F_PHI, 0
        if w.quantity == "phi_M":
            return L.F_PHI_M, 0
        if w.quantity == "c":
            return (L.F_C, w.ion) if w.ion < len(self.ion_names) - 1 else (L.F_C_ELIM, 0)
        if w.quantity == "c_prev":
            return L.F_C_PREV, w.ion
        if w.quantity == "I_ch":
            return L.F_I_CH, w.model * L.MAX_IONS + w.ion
        return L.F_ODE_STATE, w.model * L.SNAPSHOT_STATE_STRIDE + w.state

    def table(self, sub_index):
        """(spec [n][4] int32, sel_space [m] int32, sel_off [m + 1] int64, sel_idx int32) of knpemi_snapshot_set; only the
        selections of watched spaces are passed."""
        ws = list(self.watches.values())
        spec = np.array([[self._field(w)[0], sub_index[w.tag], self._field(w)[1], L.SNAPSHOT_F32 if w.dtype == "f4" else 0]
                         for w in ws], np.int32).reshape(-1, 4)
        spaces = [sp for sp in dict.fromkeys(w.space for w in ws) if sp in self.selections]
        sel_space = np.array([sub_index[tag] + (L.MAX_SUB if mem else 0) for tag, mem in spaces], np.int32)
        lists = [self.selections[sp] for sp in spaces]
        sel_off = np.concatenate([[0], np.cumsum([len(a) for a in lists])]).astype(np.int64)
        sel_idx = np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0), np.int32)
        return spec, sel_space, sel_off, sel_idx

    def _attach(self, dp, depth):
        if self._dev is not None:
            raise RuntimeError("these snapshots are attached to a device problem already")
        if not self.watches:
            raise ValueError("nothing is watched")
        if depth < 1:
            raise ValueError("depth must be positive")
        spec, sel_space, sel_off, sel_idx = self.table(dp.sub_index)
        n, m = spec.shape[0], len(sel_space)
        self._open(depth)
        L.check(dp.lib.knpemi_snapshot_set(
            dp.h, n, L.iptr(spec.ravel()), m, L.iptr(sel_space) if m else None,
            sel_off.ctypes.data_as(C.POINTER(C.c_int64)) if m else None, L.iptr(sel_idx) if m else None, int(depth)))
        off, cnt, nbytes = np.zeros(n, np.int64), np.zeros(n, np.int64), C.c_int64()
        p64 = C.POINTER(C.c_int64)
        L.check(dp.lib.knpemi_snapshot_layout(dp.h, off.ctypes.data_as(p64), cnt.ctypes.data_as(p64), C.byref(nbytes)))
        self._layout = ([(w.name, DTYPES[w.dtype], int(o), int(c)) for w, o, c in zip(self.watches.values(), off, cnt)],
                        int(nbytes.value))
        self._dev, self.depth, self._drain = (dp.lib, dp.h), int(depth), self.flush
        self._ks, self.stalls = [], 0

    def _detach(self):
        self._dev = self._drain = self._layout = None

    def retime(self, k, t):
        """The frame of step k, when it is recorded, carries t instead of the tap's t0 + k dt: a driver that accumulates
        its time (t += dt) names its files by that clock."""
        self._t_of[int(k)] = float(t)

    def _take(self, wait):
        """The oldest frame in flight as (t, k, frame); None with nothing in flight, _BUSY while its copy runs."""
        lib, h = self._dev
        watches, nbytes = self._layout
        buf = np.empty(nbytes, np.uint8)      # a buffer of its own per frame: the writer's queue holds views of it
        t, seq = C.c_double(), C.c_int64()
        rc = self._abi("take")(h, 1 if wait else 0, buf.ctypes.data_as(C.c_void_p), nbytes, C.byref(t), C.byref(seq))
        if rc == 1:
            return None
        if rc == L.EBUSY:
            return _BUSY
        L.check(rc)
        frame = {name: np.frombuffer(buf, dt, count=n, offset=o) for name, dt, o, n in watches}
        k = self._ks.pop(0)
        return self._t_of.pop(k, t.value), k, frame

    def _tick(self, t, k):
        """One tick of the stepper's tap: queue every frame that is ready, record, and with a full ring wait for the oldest
        frame alone and record again."""
        lib, h = self._dev
        self._w.check()
        while True:
            r = self._take(False)
            if r is None or r is _BUSY:
                break
            self._w.put(r)
        record = self._abi("record")
        rc = record(h, float(t))
        if rc == L.EBUSY:
            self._w.put(self._take(True))
            self.stalls += 1
            rc = record(h, float(t))
        if rc == L.OK:
            self._ks.append(int(k))
        return rc

    def _rewind(self):
        """A new run: frames in flight are discarded, the frames already queued reach the sinks, the counters restart."""
        lib, h = self._dev
        L.check(self._abi("reset")(h))
        self._ks, self._t_of = [], {}
        self._w.drain()
        self._w.delivered = self._w.waits = 0
        self.stalls = 0

    def flush(self):
        """Take every frame in flight, waiting for each frame's copy, and wait until the writer has handed all of them to
        the sinks; raises what a sink raised."""
        if self._w is None:
            return
        while self._dev is not None:
            r = self._take(True)
            if r is None:
                break
            self._w.put(r)
        self._w.drain()

    def close(self):
        """`flush`, stop the writer thread and close the sinks that have a `close`."""
        try:
            self.flush()
        finally:
            if self._w is not None:
                self._w.close()
                self._delivered, self._w = self._w.delivered, None
            for s in self.sinks:
                if hasattr(s, "close"):
                    s.close()
