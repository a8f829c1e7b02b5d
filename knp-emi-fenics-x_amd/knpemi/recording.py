"""What the on-device recorders share on the host: `RowSeries`, the times and rows of a series (`Observables`,
`IonFluxes`, `MembraneExchange`); `WatchedIons`, the (tag, ions, current) watches of the last two and their tables on a
cell partition; `Tap`, one recorder attached to a `DeviceStepper` (`MembraneEvents` too).

Cell-partitioned runs of `WatchedIons`.  A rank's local mesh holds its cells and a ghost layer, so a sum over the local
items (the cells of a sub-domain, the membrane facets of a cell) would count the ghosts twice.  `partition` gives every
item one recorder with the rule of `Observables.partition` -- the lowest owner among the item's vertices -- as a byte mask
per watch.  The record kernel writes the per-item fields of every local item and keeps the unrecorded ones out of its
sums and maxima; the ranks' partial rows are summed on the device slot by slot (an exact all-gather) and folded in rank
order, sums summed and maxima maximised from 0 (`combine_partials`), so every rank appends the same row.

`MembraneMonitor` and the series of `FieldMaps` follow the same rule through their weights (`item_owners`,
`recorded_items`): a rank integrates its dof (item) weights over the facets (cells) it records, so its partial sums need no
mask; `combine_partials` folds their rows too, with the recorder's own `column_folds()`.

The drain rule: rows collect in a device buffer of `capacity` rows; the host keeps the time of every row it has
enqueued and moves the buffer into the series (one synchronisation) whenever it holds `capacity` of them and when
`series()` is called.  The device must then hold exactly the rows enqueued: a different count, or a row dropped for want
of room, is a RuntimeError.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

CURRENT_BIT = 0x100


def lib_int(name):
    """The int a parameterless accessor of the library returns (kn_flux_chunk, ...)."""
    fn = getattr(L.load(), name)
    fn.restype, fn.argtypes = C.c_int, []
    return int(fn())


def nodal_values(u, n=None):
    """The nodal array of a `Function`, the array itself, or a constant spread over n values."""
    x = getattr(u, "x", None)
    if x is not None:
        a = getattr(x, "_a", None)
        return np.asarray(x.array if a is None else a, np.float64)
    a = np.asarray(u, np.float64)
    return np.full(n, float(a)) if a.ndim == 0 and n is not None else a


def gather_objects(obj):
    """[obj of every rank]: the default `gather` of a recorder's `partition` (torch.distributed.all_gather_object)."""
    import torch.distributed as dist
    out = [None] * dist.get_world_size()
    dist.all_gather_object(out, obj)
    return out


def agree_across_ranks(allr, fields, who, advice):
    """ValueError unless the gathered dictionaries `allr` (one per rank) hold the same `fields`."""
    for r, other in enumerate(allr):
        for what in fields:
            if other[what] != allr[0][what]:
                raise ValueError(f"{who} differ between ranks: {what} of rank {r} is {other[what]!r}, of rank 0 "
                                 f"{allr[0][what]!r} ({advice})")


def rank_slots(dp, halo, world, n_cols):
    """The exchange buffer of a partitioned recorder, a device tensor of [world][n_cols] doubles: the library's
    communicator sums it when the halo runs on it, else the halo's all-reduce (gloo or torch RCCL).  Returns the last
    three arguments of knpemi_*_set_partitioned (xbuf_dev, allreduce, ctx) and the objects the handle then refers to
    (keep them alive while it records)."""
    import torch
    xbuf = torch.zeros(world * n_cols, dtype=torch.float64, device=torch.device("cuda", dp.device))
    cb = None if halo.library_comm else halo.allreduce_callback(xbuf)
    return (xbuf.data_ptr(), C.cast(cb, C.c_void_p) if cb is not None else None, None), (xbuf, cb)


class RowSeries:
    """Times and rows of a recorder whose row has the columns `columns()`: [(key, width)] in the device's order."""

    def _init_series(self):
        self._t, self._rows = [], []
        self._drain = None                # set by the stepper's tap: moves device rows into _t / _rows

    def columns(self):
        raise NotImplementedError

    @property
    def n_cols(self):
        return sum(w for _, w in self.columns())

    def _append_rows(self, times, rows):
        self._t.extend(float(t) for t in times)
        self._rows.extend(np.asarray(rows, np.float64).reshape(len(times), self.n_cols))

    def clear(self):
        self._t, self._rows = [], []

    def series(self):
        """{"t": (n,), key: (n,) or (n, width) for every column of `columns()`}; drains the device buffer of an attached
        stepper first (one synchronisation)."""
        if self._drain is not None:
            self._drain()
        rows = np.array(self._rows, np.float64).reshape(len(self._rows), self.n_cols)
        out, j = {"t": np.array(self._t, np.float64)}, 0
        for key, w in self.columns():
            out[key] = rows[:, j:j + w].copy() if w > 1 else rows[:, j].copy()
            j += w
        return out

    def row_vector(self, row):
        """A row dictionary {key: (width,) array or float} as the flat row of the device buffer."""
        return np.concatenate([np.atleast_1d(np.asarray(row[key], np.float64)) for key, _ in self.columns()])

    def save(self, path):
        """.npz of `series()`."""
        np.savez(path, **self.series())


class WatchedIons(RowSeries):
    """Watches {tag: (ion indices, current)}, set on the device by `knpemi_<_NAME>_set`, the per-item fields read by
    `knpemi_<_NAME>_fields`.  `_WATCH` and `_SELF`: what a watch and the recorder are called in messages."""
    _NAME = _WATCH = _SELF = None

    def _init_watched(self, ion_list):
        self._init_series()
        self.ion_list = ion_list
        self.names = [ion["name"] for ion in ion_list]
        self.K = len(ion_list)
        self.z = [float(ion["z"]) for ion in ion_list]
        self.watched = {}                 # tag -> (ion indices, current)
        self._dev = None                  # (lib, handle, {tag: sub-domain index}) once attached

    def _watch_ions(self, tag, ions, current):
        if tag in self.watched:
            raise ValueError(f"{self._WATCH} {tag} is watched already")
        if ions is None:
            ions = range(self.K)
        idx = sorted({self.names.index(i) if isinstance(i, str) else int(i) for i in ions})
        if any(not 0 <= k < self.K for k in idx):
            raise ValueError("ion index out of range")
        if not idx and not current:
            raise ValueError("nothing to watch: no ion and no current")
        self.watched[tag] = (idx, bool(current))

    def _check_watched(self, tag):
        if tag not in self.watched:
            raise ValueError(f"{self._WATCH} {tag} is not watched")

    def mask(self, tag):
        """Bits 0 .. K-1: the watched ions of `tag`, bit 8: the current (columns)."""
        idx, cur = self.watched[tag]
        return sum(1 << k for k in idx) | (CURRENT_BIT if cur else 0)

    def max_columns(self):
        """Per scalar column of the row: True where it is a maximum (from 0), False where a sum."""
        return np.zeros(self.n_cols, bool)

    def _item_owners(self, halo):
        """{tag: (item mesh, owner rank of every vertex of it)} of the watches on this rank of a partition; the mesh is
        None where the rank holds no item of the watch."""
        raise NotImplementedError

    def partition(self, halo, gather=None, every=1, capacity=1024):
        """The recorded masks of this rank of a cell-partitioned run, set in `self._ptab`: {"rank", "world", "recorded":
        {tag: bool per local item}}.  An item is recorded by the lowest owner among its vertices
        (`halo.vertex_owner`), as `Observables.partition` decides.  halo: the rank's `knpemi.fem.distributed.Halo`
        with its plans built; gather(obj) -> [obj of every rank] (default: `gather_objects`).
        Collective: every rank calls it once with the same watches, ion masks, every and capacity, or every rank raises
        ValueError."""
        if not self.watched:
            raise ValueError(f"no {self._WATCH} is watched")
        rank = int(halo.rank)
        recorded = {}
        for tag, (mesh, ow) in self._item_owners(halo).items():
            recorded[tag] = recorded_items(mesh, ow, rank)
        mine = dict(watches=[(t, self.mask(t)) for t in self.watched], every=int(every), capacity=int(capacity))
        allr = (gather or gather_objects)(mine)
        agree_across_ranks(allr, ("watches", "every", "capacity"), f"{self._NAME} recorders",
                           f"every rank must watch the same {self._WATCH}s with the same ions in the same order and pass "
                           "the same every and capacity")
        self._ptab = dict(rank=rank, world=len(allr), recorded=recorded)
        return self._ptab

    def recorded_mask(self):
        """The masks of `partition`, concatenated in watch order: one uint8 per local item."""
        rec = self._ptab["recorded"]
        return np.ascontiguousarray(np.concatenate([rec[t] for t in self.watched]).astype(np.uint8))

    def _attach(self, dp, capacity, halo=None, every=1):
        """knpemi_<_NAME>_set, or with a halo `partition` and knpemi_<_NAME>_set_partitioned (`rank_slots`).  Returns the
        objects the handle refers to (keep them alive while it records)."""
        if self._dev is not None:
            raise RuntimeError(f"{self._SELF} attached to a device problem already")
        if not self.watched:
            raise ValueError(f"no {self._WATCH} is watched")
        tags = list(self.watched)
        sub = np.array([dp.sub_index[t] for t in tags], np.int32)
        mask = np.array([self.mask(t) for t in tags], np.int32)
        keep = None
        if halo is None:
            L.check(getattr(dp.lib, f"knpemi_{self._NAME}_set")(dp.h, len(tags), L.iptr(sub), L.iptr(mask), int(capacity)))
        else:
            self.partition(halo, None, every, capacity)
            rec = self.recorded_mask()
            rec = rec if rec.size else np.zeros(1, np.uint8)      # a rank without items still passes a mask
            world = self._ptab["world"]
            slots, keep = rank_slots(dp, halo, world, self.n_cols)
            L.check(getattr(dp.lib, f"knpemi_{self._NAME}_set_partitioned")(
                dp.h, len(tags), L.iptr(sub), L.iptr(mask), int(capacity), rec.ctypes.data_as(L.c_u8_p),
                self._ptab["rank"], world, *slots))
        self._dev = (dp.lib, dp.h, dict(dp.sub_index))
        return keep

    def _recorded_of(self, tag, halo, n):
        """The "recorded" entry of fields(tag, halo=halo): this rank's mask over the n local items."""
        ptab = getattr(self, "_ptab", None)
        if ptab is None:
            raise RuntimeError(f"fields(halo=...): {self._SELF} not partitioned (attach with halo=, or call partition)")
        if int(halo.rank) != ptab["rank"] or ptab["recorded"][tag].shape[0] != n:
            raise ValueError("fields(halo=...): not the halo of this recorder's partition")
        return ptab["recorded"][tag].copy()

    def _getter(self, tag, shape, where):
        """get(ion, part) -> the array of `shape` that knpemi_<_NAME>_fields holds for watch `tag`."""
        self._check_watched(tag)
        if self._dev is None:
            raise RuntimeError(f"fields(): not attached to a device problem ({where}); compute_host evaluates host data")
        lib, h, sub_index = self._dev
        fields = getattr(lib, f"knpemi_{self._NAME}_fields")

        def get(ion, part):
            buf = np.empty(shape, np.float64)
            L.check(fields(h, sub_index[tag], ion, part, L.dptr(buf), buf.size))
            return buf
        return get


def item_owners(meshes, halo, kind, message):
    """{tag: owner rank of every vertex of meshes[tag]} on this rank of a cell partition, read off the halo's plans
    (`Halo.vertex_owner(kind)`) without communication.  meshes: {tag: mesh or None} in the device's numbering -- kind
    "bulk": the sub-meshes of the sub-domains in their order; "mem": the membrane meshes of the cells in theirs.
    ValueError(message) when the halo numbers another set of vertices."""
    own, out, off = np.asarray(halo.vertex_owner(kind)), {}, 0
    for tag, mesh in meshes.items():
        n = 0 if mesh is None else int(mesh.x.shape[0])
        out[tag] = own[off:off + n]
        off += n
    if off != own.shape[0]:
        raise ValueError(message)
    return out


def membrane_meshes(subdomain_list):
    """{tag: membrane mesh or None} of the cells (every sub-domain but the first, the ECS) in their order."""
    return {tag: subdomain_list[tag].get("mesh_mem") for tag in list(subdomain_list)[1:]}


def recorded_items(mesh, owner, rank):
    """One bool per cell (membrane facet) of `mesh`: this rank records it -- the lowest owner among its vertices."""
    if mesh is None or np.asarray(mesh.cells).shape[0] == 0:
        return np.zeros(0, bool)
    return owner[np.asarray(mesh.cells)].min(axis=1) == rank


# how record_combine_kernel folds a column over the ranks: a sum from 0, a maximum from 0 (the fluxes' norms), or the
# monitors' minimum from +inf and maximum from -inf
FOLD_SUM, FOLD_MAX0, FOLD_MIN, FOLD_MAX = 0, 1, 2, 3


def combine_partials(rec, rows_by_rank):
    """The row of a partitioned run from the ranks' partial rows (one per rank in rank order: `compute_host(recorded=...)`
    through `row_vector`, `MembraneMonitor.evaluate_partial_host`, `FieldMaps.series_partial_host`), folded as
    record_combine_kernel does, in rank order.  A recorder with `column_folds()` -> (FOLD_* per column, divisors or None)
    says how; without it `rec.max_columns()` are maxima from 0 and the other columns sums.  Minimum and maximum keep a NaN
    of either side."""
    rows = np.asarray(rows_by_rank, np.float64)
    folds = getattr(rec, "column_folds", None)
    if folds is None:
        how, denom = np.where(rec.max_columns(), FOLD_MAX0, FOLD_SUM), None
    else:
        how, denom = folds()
        how = np.asarray(how)
    out = np.where(how == FOLD_MIN, np.inf, np.where(how == FOLD_MAX, -np.inf, 0.0))
    with np.errstate(invalid="ignore"):
        for r in range(rows.shape[0]):
            x = rows[r]
            lo = np.where((out < x) | (out != out), out, x)
            hi = np.where((out > x) | (out != out), out, x)
            out = np.where(how == FOLD_SUM, out + x, np.where(how == FOLD_MIN, lo, hi))
        if denom is not None:
            out = np.where(how == FOLD_SUM, out / np.asarray(denom, np.float64), out)
    return out


class Tap:
    """One recorder attached to a stepper.  `tick(k, dt)` records when k + offset is a multiple of `every`, at the time
    t0 + (k + offset) dt: offset 0 at the end of step k (counted from 1), 1 inside step k (counted from 0) for a row that
    carries the time of the step's end.  record(t, fields) enqueues the launch; read(n, buf) -> (rows, dropped) fills buf
    with the device's first n rows and starts its buffer over (None: no series); rewind() starts a new series on the
    device.  `enabled` and `fields` may be switched between steps (tools/recorder_cost.py).

    halo: the halo the recorder was attached with, or None; partition_refusal: the NotImplementedError text of a
    partitioned step (`DeviceStepper.step(halo)`) with another halo than that, None for a recorder that needs no halo;
    keep: what the handle refers to while the recorder is attached (the exchange buffer, the all-reduce callback)."""

    def __init__(self, target, label, every, record, t0=0.0, offset=0, capacity=None, read=None, n_cols=0, rewind=None,
                 fields=False, halo=None, partition_refusal=None, keep=None):
        self.target, self.label, self.every, self.t0, self.offset = target, label, int(every), float(t0), int(offset)
        self.record, self.read, self.rewind = record, read, rewind
        self.halo, self.partition_refusal, self.keep = halo, partition_refusal, keep
        self.capacity, self.n_cols = capacity if capacity is None else int(capacity), int(n_cols)
        self.enabled, self.fields = True, bool(fields)
        self.pending = []                 # times of the rows the device holds
        if read is not None:
            target.clear()
            target._drain = self.drain

    def refuse_partitioned(self, halo):
        """NotImplementedError when the steps run with `halo` and this recorder cannot record them."""
        if halo is not None and halo is not self.halo and self.partition_refusal is not None:
            raise NotImplementedError(self.partition_refusal)

    def tick(self, k, dt):
        self.tick_at(k, self.t0 + (k + self.offset) * dt)

    def tick_at(self, k, t):
        """`tick` for a caller that keeps the clock itself (`DGProblem.record(t)`): record k is due as above, at time t."""
        if not self.enabled or (k + self.offset) % self.every:
            return
        self.record(t, 1 if self.fields else 0)
        if self.read is not None:
            self.pending.append(t)
            if len(self.pending) == self.capacity:
                self.drain()

    def drain(self):
        """Move the device rows into the host series; the device must hold exactly the rows enqueued."""
        n = len(self.pending)
        buf = np.empty((max(n, 1), self.n_cols), np.float64)
        rows, over = self.read(n, buf)
        if rows != n or over != 0:
            raise RuntimeError(f"{self.label}: the device holds {rows} row(s) (+{over} dropped), the host enqueued {n}")
        self.target._append_rows(self.pending, buf[:n])
        self.pending = []

    def reset(self):
        """A new series (new maps): on the device, in the pending list and in the target."""
        if self.rewind is not None:
            self.rewind()
        self.pending = []
        if self.read is not None:
            self.target.clear()
