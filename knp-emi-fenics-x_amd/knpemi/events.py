"""Membrane events: per membrane dof, when phi_M crossed a threshold, how often, and how far it rose.

The reference's users find out whether and when a cell fired by checkpointing every field at every step and
post-processing the checkpoints on the host (`examples/idealized_geometries/run_3D.py:57-60, 376`,
`make_figures.py:67-89`).  `Observables` records a few scalars per step and cannot say anything per membrane dof; an
activation map, a spike count per dof or a conduction velocity needs the whole phi_M array at every step.  Here every
membrane dof of a watched cell keeps a few words of state on the device, one launch behind the end-of-step update
advances them (csrc/kernels_events.hip, `DeviceStepper.detect`), and the host reads the maps only when asked.

    ev = MembraneEvents(subdomain_list)
    ev.watch(tag=1, threshold=-20e-3, reset=-40e-3, keep=8)
    stepper.detect(ev, every=1, t0=0.0)                   # ... stepper.step() ...
    m = ev.maps(1)                                        # count, t_first, t_last, v_peak, t_peak, times
    ev.conduction_velocity(1, origin=x0)

One record at time t with sample v = phi_M[q] (t_prev: the time of the previous record), the same on the device and
in `record_host`:

  * first record after set-up or reset: v_prev <- v, armed <- (v < threshold), v_peak <- v, t_peak <- t; no crossing
    can be counted;
  * later records, in this order (a non-finite v only replaces v_prev):
      1. if not armed and v < reset: armed;
      2. if armed and v >= threshold (v == threshold counts): a crossing at
         t_c = t_prev + (t - t_prev) * ((threshold - v_prev) / (v - v_prev)); count += 1, t_last <- t_c, t_first <- t_c
         at the first one, t_c goes to slot (count - 1) % keep of the dof's ring; disarmed;
      3. if v > v_peak (strictly): v_peak <- v, t_peak <- t;
      4. v_prev <- v.

`reset < threshold` is a hysteresis: after a crossing the dof must fall below `reset` before the next one counts, so
a dip that stays above `reset` is not counted twice.  `keep` bounds only how many crossing TIMES a dof remembers (the
latest `keep`, at most 64); `count`, `t_first` and `t_last` are exact however often it fires.

Stand-alone membrane models (`MembraneModel` on an `OdeProblem`): `MembraneEvents({tag: n_dofs})` and
`model.detect(ev)`; every `step` / `step_lsoda` then records at the model's new time.  `advance` and `steady_state`
run many steps inside one launch without writing phi_M: nothing is recorded during them.

Cell-partitioned runs need no communication: ghost membrane dofs are integrated redundantly with identical bits, so
every rank's events of a dof are those of the single-rank run.  `maps(tag, halo=halo)` returns the dofs this rank owns
(`Halo.vertex_owner("mem")`) with their locations; the union over the ranks is the global map.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L
from .recording import nodal_values as _values

MAP_KEYS = ("count", "t_first", "t_last", "v_peak", "t_peak", "times")


def ring_to_times(ring, count):
    """(n_q, keep) crossing times, oldest first and NaN padded, from the ring [keep][n_q] in slot order: crossing n
    (1-based) sits in slot (n - 1) % keep, so with m = min(count, keep) remembered crossings column j < m holds
    crossing count - m + 1 + j."""
    keep, nq = ring.shape
    times = np.full((nq, keep), np.nan)
    if keep == 0:
        return times
    m = np.minimum(count, keep)
    j = np.arange(keep)[None, :]
    slot = (count[:, None] - m[:, None] + j) % keep
    val = ring[slot, np.arange(nq)[:, None]]
    have = j < m[:, None]
    times[have] = val[have]
    return times


def conduction_velocity(x, t_first, origin):
    """Least-squares slope of the distance from `origin` against the activation time over the dofs that fired
    (finite t_first): (speed, rms of the residual distances, number of dofs used).  ValueError with fewer than 3
    fired dofs, or when they all fired at the same time."""
    x = np.asarray(x, np.float64)
    t = np.asarray(t_first, np.float64)
    use = np.isfinite(t)
    n = int(use.sum())
    if n < 3:
        raise ValueError(f"conduction velocity needs at least 3 fired dofs, {n} fired")
    d = np.linalg.norm(x[use] - np.asarray(origin, np.float64).ravel()[None, :x.shape[1]], axis=1)
    t = t[use]
    tm, dm = t.mean(), d.mean()
    tt = t - tm
    den = np.dot(tt, tt)
    if not den > 0.0:
        raise ValueError("conduction velocity: every fired dof has the same activation time")
    speed = np.dot(tt, d - dm) / den
    res = d - (dm + speed * tt)
    return float(speed), float(np.sqrt(np.mean(res * res))), n


class MembraneEvents:
    def __init__(self, subdomain_list):
        """subdomain_list: the problem's sub-domain dictionary (cells carry their membrane mesh in "mesh_mem"), or
        {tag: number of dofs} for membrane models without a mesh."""
        self.n_q, self._x = {}, {}
        for tag, sd in subdomain_list.items():
            if isinstance(sd, (int, np.integer)):
                self.n_q[tag] = int(sd)
            elif tag != 0 and "mesh_mem" in sd:
                self.n_q[tag] = int(sd["mesh_mem"].num_vertices)
                self._x[tag] = sd["mesh_mem"].x
        self.tags = list(self.n_q)          # the order of the concatenated membrane dofs
        self.watched = {}                   # tag -> (threshold, reset)
        self.keep = None
        self._dev = None                    # (lib, handle, {tag: sub-domain index}) once attached
        self._host = None                   # state of record_host
        self._t_prev = None

    # -- definition ------------------------------------------------------------------------------------
    def watch(self, tag, threshold, reset=None, keep=0):
        """Watch the membrane of cell `tag`: upward crossings of `threshold`, re-armed below `reset` (default: the
        threshold), the latest `keep` crossing times kept per dof (one ring length for all watched cells)."""
        if self._dev is not None:
            raise RuntimeError("events are attached to a device problem: watch every cell before detect()")
        if tag not in self.n_q:
            raise ValueError(f"no cell with tag {tag} (the ECS, tag 0, has no membrane)")
        if tag in self.watched:
            raise ValueError(f"cell {tag} is watched already")
        threshold = float(threshold)
        reset = threshold if reset is None else float(reset)
        if not reset <= threshold:
            raise ValueError("reset must not exceed the threshold")
        keep = int(keep)
        if not 0 <= keep <= L.EVENTS_MAX_KEEP:
            raise ValueError(f"keep must be in 0..{L.EVENTS_MAX_KEEP}")
        if self.keep is not None and keep != self.keep:
            raise ValueError(f"one ring length for all watched cells: keep is {self.keep} already")
        self.keep = keep
        self.watched[tag] = (threshold, reset)
        self._host = None

    def _check_watched(self, tag):
        if tag not in self.watched:
            raise ValueError(f"cell {tag} is not watched")

    # -- the device table (knpemi_events_set) ----------------------------------------------------------
    def _attach(self, lib, h, sub_index):
        if self._dev is not None:
            raise RuntimeError("these events are attached to a device problem already")
        if not self.watched:
            raise ValueError("no cell is watched")
        tags = list(self.watched)
        sub = np.array([sub_index[t] for t in tags], np.int32)
        thr = np.array([self.watched[t][0] for t in tags], np.float64)
        rst = np.array([self.watched[t][1] for t in tags], np.float64)
        L.check(lib.knpemi_events_set(h, len(tags), L.iptr(sub), L.dptr(thr), L.dptr(rst), int(self.keep)))
        self._dev = (lib, h, dict(sub_index))

    def _detach(self):
        self._dev = None

    def _read_device(self, tag):
        lib, h, sub_index = self._dev
        n = self.n_q[tag]
        count = np.zeros(n, np.int32)
        out = [np.empty(n) for _ in range(4)]
        ring = np.empty((self.keep, n))
        L.check(lib.knpemi_events_read(h, sub_index[tag], L.iptr(count), *(L.dptr(a) for a in out), L.dptr(ring)))
        return dict(count=count, t_first=out[0], t_last=out[1], v_peak=out[2], t_peak=out[3], ring=ring)

    # -- host restatement --------------------------------------------------------------------------------
    def _fresh(self, n):
        nan = lambda: np.full(n, np.nan)      # noqa: E731
        return dict(v_prev=nan(), armed=np.zeros(n, np.uint8), count=np.zeros(n, np.int32), t_first=nan(), t_last=nan(),
                    v_peak=nan(), t_peak=nan(), ring=np.full((self.keep, n), np.nan))

    def reset_host(self):
        """The host state back to "before the first record"."""
        self._host, self._t_prev = None, None

    def record_host(self, t, phi_M_prev):
        """One record at time t from host arrays: phi_M_prev[tag] is a `Function` or an array over the membrane dofs
        of every watched cell.  The numpy restatement of the device kernel (the module docstring's rules); host
        drivers record with it, and it is the reference of the device tests."""
        t = float(t)
        if not self.watched:
            raise ValueError("no cell is watched")
        if not np.isfinite(t) or (self._t_prev is not None and not t > self._t_prev):
            raise ValueError("record_host: t must be finite and greater than the previous record's")
        first = self._host is None
        if first:
            self._host = {tag: self._fresh(self.n_q[tag]) for tag in self.watched}
        for tag, (thr, rst) in self.watched.items():
            S = self._host[tag]
            v = _values(phi_M_prev[tag])
            if v.shape != (self.n_q[tag],):
                raise ValueError(f"phi_M of cell {tag}: {v.shape[0]} values for {self.n_q[tag]} membrane dofs")
            if first:
                S["v_prev"] = v.copy()
                S["armed"] = (v < thr).astype(np.uint8)
                S["v_peak"] = v.copy()
                S["t_peak"] = np.full(v.shape, t)
                continue
            vp = S["v_prev"]
            fin = np.isfinite(v)
            armed = S["armed"].astype(bool)
            armed |= fin & ~armed & (v < rst)
            with np.errstate(invalid="ignore"):
                cross = fin & armed & (v >= thr)
                q = np.flatnonzero(cross)
                tc = self._t_prev + (t - self._t_prev) * ((thr - vp[q]) / (v[q] - vp[q]))
            S["count"][q] += 1
            S["t_last"][q] = tc
            one = S["count"][q] == 1
            S["t_first"][q[one]] = tc[one]
            if self.keep:
                S["ring"][(S["count"][q] - 1) % self.keep, q] = tc
            armed[q] = False
            S["armed"] = armed.astype(np.uint8)
            with np.errstate(invalid="ignore"):
                up = fin & (v > S["v_peak"])
            S["v_peak"][up] = v[up]
            S["t_peak"][up] = t
            S["v_prev"] = v.copy()
        self._t_prev = t

    # -- output --------------------------------------------------------------------------------------------
    def locations(self, tag):
        """(n_q, gdim) coordinates of the membrane dofs of cell `tag`, in the order of phi_M_prev[tag].x.array."""
        if tag not in self._x:
            raise ValueError(f"the dofs of cell {tag} have no coordinates (events built from dof counts)")
        return np.array(self._x[tag], np.float64)

    def maps(self, tag, halo=None):
        """{"count" (n_q,) int32, "t_first", "t_last", "v_peak", "t_peak" (n_q,), "times" (n_q, keep) oldest first and
        NaN padded, "locations" (n_q, gdim) where the dofs have coordinates}: the device state of an attached stepper
        or model (one synchronisation), else the state of `record_host`.
        halo: on a cell-partitioned problem, only the membrane dofs this rank owns (`Halo.vertex_owner("mem")`); the
        union of the ranks' maps is the global one."""
        self._check_watched(tag)
        if self._dev is not None:
            S = self._read_device(tag)
        elif self._host is not None:
            S = self._host[tag]
        else:
            S = self._fresh(self.n_q[tag])
        out = {k: np.array(S[k]) for k in MAP_KEYS[:-1]}
        out["times"] = ring_to_times(S["ring"], S["count"])
        if tag in self._x:
            out["locations"] = self.locations(tag)
        if halo is not None:
            own = np.asarray(halo.vertex_owner("mem"))
            off = 0
            for other in self.tags:
                if other == tag:
                    break
                off += self.n_q[other]
            if own.shape[0] != sum(self.n_q.values()):
                raise ValueError("events: the halo does not number the membrane dofs of these sub-domains")
            mine = own[off:off + self.n_q[tag]] == int(halo.rank)
            out = {k: v[mine] for k, v in out.items()}
        return out

    def fired(self, tag, halo=None):
        """Boolean mask: the dof crossed the threshold at least once."""
        return self.maps(tag, halo)["count"] > 0

    def firing_rate(self, tag, t_start, t_end, halo=None):
        """Crossings per unit time of every dof in [t_start, t_end].  A dof remembers its latest `keep` crossing times
        only: when it fired more often, the window is counted from `times` if it does not begin before the oldest
        remembered crossing, from `count` if it covers [t_first, t_last], and is NaN otherwise (the crossings in
        between are not known one by one)."""
        if not t_end > t_start:
            raise ValueError("t_end must be greater than t_start")
        m = self.maps(tag, halo)
        count, times = m["count"], m["times"]
        with np.errstate(invalid="ignore"):
            n = ((times >= t_start) & (times <= t_end)).sum(axis=1).astype(np.float64)
            forgot = count > self.keep
            oldest = times[:, 0] if self.keep else np.full(count.shape, np.nan)
            whole = (m["t_first"] >= t_start) & (m["t_last"] <= t_end)
            n[forgot] = np.where(whole[forgot], count[forgot], np.where(oldest[forgot] <= t_start, n[forgot], np.nan))
        return n / (t_end - t_start)

    def conduction_velocity(self, tag, origin, halo=None, maps=None):
        """Least-squares slope of the distance from `origin` against `t_first` over the fired dofs of cell `tag`:
        (speed, rms of the residual distances, number of dofs used); ValueError with fewer than 3 fired dofs.
        maps: a map with "t_first" and "locations" to use instead of this object's (the union over the ranks of a
        partitioned run)."""
        m = self.maps(tag, halo) if maps is None else maps
        if "locations" not in m:
            raise ValueError(f"the dofs of cell {tag} have no coordinates")
        return conduction_velocity(m["locations"], m["t_first"], origin)

    def save(self, path, halo=None):
        """.npz with "<tag>/<map>" for every watched cell and map ("<tag>/locations" included)."""
        out = {}
        for tag in self.watched:
            for k, v in self.maps(tag, halo).items():
                out[f"{tag}/{k}"] = v
        np.savez(path, **out)

    def summary(self, tag, origin=None, halo=None):
        """One line for a driver's log: fired dofs, first / last activation, conduction velocity from `origin`."""
        m = self.maps(tag, halo)
        fired = m["count"] > 0
        line = f"cell {tag}: {int(fired.sum())} of {fired.shape[0]} membrane dofs fired"
        if fired.any():
            line += f", activation {np.nanmin(m['t_first']):.6g} .. {np.nanmax(m['t_last']):.6g}"
        if origin is not None and "locations" in m:
            try:
                c, rms, n = conduction_velocity(m["locations"], m["t_first"], origin)
                line += f", conduction velocity {c:.6g} (residual rms {rms:.3g}, {n} dofs)"
            except ValueError as e:
                line += f", no conduction velocity ({e})"
        return line
