"""What the on-device recorders share on the host: `RowSeries`, the times and rows of a series (`Observables`,
`IonFluxes`, `MembraneExchange`); `WatchedIons`, the (tag, ions, current) watches of the last two; `Tap`, one recorder
attached to a `DeviceStepper` (`MembraneEvents` too).

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

    def _attach(self, dp, capacity):
        if self._dev is not None:
            raise RuntimeError(f"{self._SELF} attached to a device problem already")
        if not self.watched:
            raise ValueError(f"no {self._WATCH} is watched")
        tags = list(self.watched)
        sub = np.array([dp.sub_index[t] for t in tags], np.int32)
        mask = np.array([self.mask(t) for t in tags], np.int32)
        L.check(getattr(dp.lib, f"knpemi_{self._NAME}_set")(dp.h, len(tags), L.iptr(sub), L.iptr(mask), int(capacity)))
        self._dev = (dp.lib, dp.h, dict(dp.sub_index))

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


class Tap:
    """One recorder attached to a stepper.  `tick(k, dt)` records when k + offset is a multiple of `every`, at the time
    t0 + (k + offset) dt: offset 0 at the end of step k (counted from 1), 1 inside step k (counted from 0) for a row that
    carries the time of the step's end.  record(t, fields) enqueues the launch; read(n, buf) -> (rows, dropped) fills buf
    with the device's first n rows and starts its buffer over (None: no series); rewind() starts a new series on the
    device.  `enabled` and `fields` may be switched between steps (tools/*_cost.py)."""

    def __init__(self, target, label, every, record, t0=0.0, offset=0, capacity=None, read=None, n_cols=0, rewind=None,
                 fields=False):
        self.target, self.label, self.every, self.t0, self.offset = target, label, int(every), float(t0), int(offset)
        self.record, self.read, self.rewind = record, read, rewind
        self.capacity, self.n_cols = capacity if capacity is None else int(capacity), int(n_cols)
        self.enabled, self.fields = True, bool(fields)
        self.pending = []                 # times of the rows the device holds
        if read is not None:
            target.clear()
            target._drain = self.drain

    def tick(self, k, dt):
        if not self.enabled or (k + self.offset) % self.every:
            return
        t = self.t0 + (k + self.offset) * dt
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
