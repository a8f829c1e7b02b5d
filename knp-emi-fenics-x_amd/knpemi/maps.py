"""Field maps: per vertex of a bulk field, or per membrane dof, the running peak, trough, time integral, arrival time,
exposure and excess over a level, kept on the device over a whole run.

The reference's astrocyte study normalises the glial membrane potential in space by its maximum and its minimum over
the run (`examples/local_astrocyte_depolarization/results/compare_1D_3D.py:89-105`, `compare_tort.py:114-130`,
`make_figures.py:336-352`) and plots ECS concentrations in space at chosen times (`make_figures.py:135`); its users get
such maps by checkpointing every field at every step and post-processing on the host.  Here every item of a watch keeps
its statistics on the device, one launch behind the end-of-step update advances them (csrc/kernels_maps.hip,
`DeviceStepper.track`), and the host reads the maps only when asked.

    fm = FieldMaps(subdomain_list, ion_list)
    fm.watch("K_ecs", "c", tag=0, ion="K", threshold=8.0, stats=("peak", "integral", "threshold"), series=True)
    fm.watch("phi_glia", "phi_M", tag=2, stats=("peak", "trough"))
    fm.watch("dc_shift", "phi", tag=0, threshold=-5.0, below=True)      # stats default: all that apply
    stepper.track(fm, every=1, capacity=1024, t0=0.0)                    # ... stepper.step() ...
    fm.maps("K_ecs")          # v_max, t_max, integral, count, t_arrival, exposure, excess, locations
    fm.series()               # t, K_ecs/measure, K_ecs/n

The rules (csrc/kernels_maps.hip and include/knpemi_hip.h state the same).  A watch is a field (`phi`, `c` of an ion,
`phi_M`) of a sub-domain `tag`, an optional `threshold` thr, a direction s = +1 ("beyond" = at or above) or -1
(`below=True`: at or below) and a selection of the statistics `peak`, `trough`, `integral`, `threshold`.  Its items are
the vertices of the sub-mesh, or the membrane dofs of cell `tag` for `phi_M`.  State per item after set-up or reset:
v_prev, v_max, t_max, v_min, t_min, t_arrival NaN; integral, exposure, excess and count (int32) 0.  One record at time
t (previous record's time t_prev, D = t - t_prev) with sample v, in this order:

  * v not finite: v_prev <- v.  Nothing else changes.
  * v_prev not finite (the first record, or the record after a non-finite sample): no interval is accounted for; peak
    and trough as in step 3; with the threshold statistic and s (v - thr) >= 0: count += 1, t_arrival <- t when
    count == 1 (a field already beyond the level counts as arrived at the first sight of it); v_prev <- v.
  * otherwise, with a = s (v_prev - thr), b = s (v - thr):
      1. integral += 0.5 D (v_prev + v)   (trapezoid);
      2. with theta = a / (a - b) where used:
           onset (a < 0 <= b): t_c = t_prev + D theta; count += 1; t_arrival <- t_c when count == 1;
             exposure += (1 - theta) D; excess += 0.5 (1 - theta) D b;
           stays beyond (a >= 0 and b >= 0): exposure += D; excess += 0.5 D (a + b);
           offset (a >= 0 > b): exposure += theta D; excess += 0.5 theta D a;
      3. not (v <= v_max) -> v_max <- v, t_max <- t.  not (v >= v_min) -> v_min <- v, t_min <- t;
      4. v_prev <- v.

A statistic that is not selected keeps its initial value and costs no memory traffic.  A watch with `series=True`
(needs the threshold statistic) contributes two columns per record: `<name>/measure`, the sum of the lumped nodal
measures (`fem.probe.integral_weights`) of the items with s (v - thr) >= 0 -- the volume, area or length beyond the
level -- and `<name>/n`, their number.

Cell-partitioned runs.  The per-item maps need no communication: ghost values are current after the bulk halo exchange
and ghost membrane dofs are integrated redundantly with identical bits.  `maps(name, halo=halo)` returns the items this
rank owns; the union over the ranks is the global map.  A series would sum ghosts too, so it is recorded with
`stepper.track(fm, halo=halo)` (`partition`): `measure` uses item weights lumped from the cells (phi_M: membrane facets)
the rank records -- the lowest owner among a cell's vertices, the rule of `Observables.partition` -- `n` counts the items
the rank owns, and both columns are summed over the ranks on the device at every record, so every rank holds the global
row (`n` exactly, `measure` to rounding).  Attached without a halo, `step(halo)` refuses a `FieldMaps` with a series.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .events import conduction_velocity
from .fem.probe import integral_weights
from .recording import (RowSeries, agree_across_ranks, gather_objects, item_owners, membrane_meshes,
                        nodal_values as _values, rank_slots, recorded_items)

STATS = ("peak", "trough", "integral", "threshold")
STAT_BITS = dict(peak=L.MAPS_PEAK, trough=L.MAPS_TROUGH, integral=L.MAPS_INTEGRAL, threshold=L.MAPS_THRESHOLD)
# the maps of every statistic, with the `which` of knpemi_maps_read
STAT_MAPS = dict(peak=(("v_max", L.MAP_V_MAX), ("t_max", L.MAP_T_MAX)), trough=(("v_min", L.MAP_V_MIN), ("t_min", L.MAP_T_MIN)),
                 integral=(("integral", L.MAP_INTEGRAL),),
                 threshold=(("count", L.MAP_COUNT), ("t_arrival", L.MAP_T_ARRIVAL), ("exposure", L.MAP_EXPOSURE),
                            ("excess", L.MAP_EXCESS)))
NAN_MAPS = ("v_max", "t_max", "v_min", "t_min", "t_arrival")


class _Watch:
    __slots__ = ("name", "quantity", "tag", "ion", "thr", "sgn", "stats", "series", "n", "w")

    @property
    def flags(self):
        return (sum(STAT_BITS[s] for s in self.stats) | (L.MAPS_SERIES if self.series else 0)
                | (L.MAPS_BELOW if self.sgn < 0 else 0))


class FieldMaps(RowSeries):
    def __init__(self, subdomain_list, ion_list):
        self.subdomain_list, self.ion_list = subdomain_list, ion_list
        self.tags = list(subdomain_list.keys())
        self.ion_names = [ion["name"] for ion in ion_list]
        self.watches = {}                 # name -> _Watch, in the order of the device table
        self._init_series()
        self._dev = None                  # (lib, handle) once attached
        self._host = None                 # state of record_host
        self._t_prev = None
        self._sums = None                 # per watch and statistic, the sums of |increment| of record_host

    # -- definition ------------------------------------------------------------------------------------
    def watch(self, name, quantity, tag, ion=None, threshold=None, below=False, stats=None, series=False):
        """Watch `quantity` ("phi", "c" with `ion`, or "phi_M") on sub-domain `tag` (phi_M: the membrane of cell `tag`).
        stats: a selection of "peak", "trough", "integral", "threshold" (default: all that apply -- the last one with a
        threshold only); below: beyond the level means at or below it; series: the measure of the region beyond the level
        and its number of items as two columns of the series."""
        if self._dev is not None:
            raise RuntimeError("these maps are attached to a device problem: define every watch before track()")
        if name in self.watches:
            raise ValueError(f"watch {name!r} defined twice")
        if tag not in self.subdomain_list:
            raise ValueError(f"no sub-domain with tag {tag}")
        if quantity == "c":
            if ion not in self.ion_names:
                raise ValueError(f"unknown ion {ion!r} (ions: {self.ion_names})")
        elif quantity == "phi_M":
            if tag == 0:
                raise ValueError("the ECS (tag 0) has no membrane: give the tag of a cell")
        elif quantity != "phi":
            raise ValueError("quantity must be 'phi', 'c' or 'phi_M'")
        if stats is None:
            stats = STATS if threshold is not None else STATS[:3]
        stats = tuple(s for s in STATS if s in set(stats)) if set(stats) <= set(STATS) else None
        if not stats:
            raise ValueError(f"stats must be a non-empty selection of {STATS}")
        if "threshold" in stats:
            if threshold is None or not np.isfinite(float(threshold)):
                raise ValueError("the threshold statistic needs a finite threshold")
        elif below or series:
            raise ValueError("below and series need the threshold statistic")
        if len(self.watches) == L.MAPS_MAX_WATCH:
            raise ValueError(f"at most {L.MAPS_MAX_WATCH} watches")
        if sum(1 for o in self.watches.values() if (o.quantity == "phi_M") == (quantity == "phi_M") and o.tag == tag) \
                == L.MAPS_MAX_PER_SPACE:
            raise ValueError(f"at most {L.MAPS_MAX_PER_SPACE} watches on one space")
        w = _Watch()
        w.name, w.quantity, w.tag, w.ion = name, quantity, tag, ion
        w.thr = float(threshold) if "threshold" in stats else 0.0
        w.sgn = -1.0 if below else 1.0
        w.stats, w.series = stats, bool(series)
        mesh = self._mesh(w)
        w.n = int(mesh.num_vertices)
        w.w = integral_weights(mesh) if series else None
        for o in self.watches.values():
            if (o.quantity, o.tag, o.ion, o.flags, o.thr) == (quantity, tag, ion, w.flags, w.thr):
                raise ValueError(f"watch {name!r} repeats watch {o.name!r}")
        self.watches[name] = w
        self._host = None

    def _mesh(self, w):
        return self.subdomain_list[w.tag]["mesh_mem" if w.quantity == "phi_M" else "mesh_sub"]

    def _check(self, name):
        if name not in self.watches:
            raise ValueError(f"no watch {name!r}")
        return self.watches[name]

    def _field(self, w):
        """(field id, index) on the device: a solved ion's new c, the eliminated one's c_<tag> (Observables._ion_field)."""
        if w.quantity == "phi":
            return L.F_PHI, 0
        if w.quantity == "phi_M":
            return L.F_PHI_M, 0
        k = self.ion_names.index(w.ion)
        return (L.F_C, k) if k < len(self.ion_names) - 1 else (L.F_C_ELIM, 0)

    @property
    def has_series(self):
        return any(w.series for w in self.watches.values())

    def columns(self):
        """[(key, 1)] of the series row: measure and n of every series watch, in watch order."""
        return [(f"{w.name}/{c}", 1) for w in self.watches.values() if w.series for c in ("measure", "n")]

    # -- the device table (knpemi_maps_set) ----------------------------------------------------------------
    def table(self, sub_index):
        """(spec [n][4] int32, threshold [n], concatenated weights of the series watches or None) of knpemi_maps_set."""
        ws = list(self.watches.values())
        spec = np.array([[*self._field(w)[:1], sub_index[w.tag], self._field(w)[1], w.flags] for w in ws], np.int32)
        thr = np.array([w.thr for w in ws], np.float64)
        wt = [w.w for w in ws if w.series]
        return spec.reshape(-1, 4), thr, np.ascontiguousarray(np.concatenate(wt)) if wt else None

    def _attach(self, dp, capacity, halo=None, every=1):
        """knpemi_maps_set on the device problem dp, or with a halo (and a series watch) `partition` and
        knpemi_maps_set_partitioned (`rank_slots`).  Returns the objects the handle refers to (keep them alive while it
        records)."""
        if self._dev is not None:
            raise RuntimeError("these maps are attached to a device problem already")
        if not self.watches:
            raise ValueError("nothing is watched")
        spec, thr, wt = self.table(dp.sub_index)
        keep = None
        if halo is None:
            L.check(dp.lib.knpemi_maps_set(dp.h, spec.shape[0], L.iptr(spec.ravel()), L.dptr(thr),
                                           L.dptr(wt) if wt is not None else None, int(capacity)))
        else:
            tab = self.partition(halo, None, every, capacity)
            names = [n for n, w in self.watches.items() if w.series]
            wt = np.ascontiguousarray(np.concatenate([tab["weights"][n] for n in names]), np.float64)
            own = np.ascontiguousarray(np.concatenate([tab["owned"][n] for n in names]).astype(np.uint8))
            wt, own = (wt, own) if wt.size else (np.zeros(1), np.zeros(1, np.uint8))      # a rank without items
            slots, keep = rank_slots(dp, halo, tab["world"], self.n_cols)
            L.check(dp.lib.knpemi_maps_set_partitioned(dp.h, spec.shape[0], L.iptr(spec.ravel()), L.dptr(thr), L.dptr(wt),
                                                       int(capacity), own.ctypes.data_as(L.c_u8_p), tab["rank"],
                                                       tab["world"], *slots))
        self._dev = (dp.lib, dp.h)
        return keep

    # -- cell-partitioned runs: the series ---------------------------------------------------------------
    def partition(self, halo, gather=None, every=1, capacity=1024):
        """The series tables of this rank of a cell-partitioned run, set in `self._ptab`: {"rank", "world", "weights":
        {name: item weights lumped from the cells (phi_M: membrane facets) this rank records}, "owned": {name: bool per
        item}} for every series watch.  A cell is recorded by the lowest owner among its vertices (the rule of
        `Observables.partition`), so the ranks' measures add up to the global one; n counts the items a rank owns.  halo:
        the rank's `knpemi.fem.distributed.Halo` with its plans built; gather(obj) -> [obj of every rank] (default:
        `recording.gather_objects`).  Collective: every rank calls it once with the same watches, every and capacity, or
        every rank raises ValueError."""
        if not self.has_series:
            raise ValueError("no watch has a series: the maps of a partitioned run need no partition")
        rank = int(halo.rank)
        message = "maps: the halo does not number the items of these sub-domains"
        series = [w for w in self.watches.values() if w.series]
        bulk = item_owners({t: sd["mesh_sub"] for t, sd in self.subdomain_list.items()}, halo, "bulk", message) \
            if any(w.quantity != "phi_M" for w in series) else {}
        mem = item_owners(membrane_meshes(self.subdomain_list), halo, "mem", message) \
            if any(w.quantity == "phi_M" for w in series) else {}
        weights, owned = {}, {}
        for name, w in self.watches.items():
            if not w.series:
                continue
            owner = (mem if w.quantity == "phi_M" else bulk)[w.tag]
            mesh = self._mesh(w)
            weights[name] = integral_weights(mesh, cell_mask=recorded_items(mesh, owner, rank)) if w.n else np.zeros(0)
            owned[name] = owner == rank
        mine = dict(watches=[(w.name, w.quantity, w.tag, w.ion, w.thr, w.sgn, w.stats, w.series) for w in self.watches.values()],
                    every=int(every), capacity=int(capacity))
        allr = (gather or gather_objects)(mine)
        agree_across_ranks(allr, ("watches", "every", "capacity"), "field maps",
                           "every rank must define the same watches in the same order and pass the same every and capacity")
        self._ptab = dict(rank=rank, world=len(allr), weights=weights, owned=owned)
        return self._ptab

    def max_columns(self):
        """Per column of the series row: every one is a sum (`recording.combine_partials`)."""
        return np.zeros(self.n_cols, bool)

    def series_partial_host(self, phi, c, phi_M_prev):
        """This rank's slot row of the series of a partitioned run (after `partition`) from host data, as the record
        kernel writes it: per series watch the rank's weights summed over the items beyond the level, and the number of
        such items the rank owns."""
        row = []
        for name, w in self.watches.items():
            if not w.series:
                continue
            v = self._sample(w, phi, c, phi_M_prev)
            with np.errstate(invalid="ignore"):
                beyond = np.isfinite(v) & (w.sgn * (v - w.thr) >= 0.0)
            row += [float(np.sum(self._ptab["weights"][name][beyond])), float((beyond & self._ptab["owned"][name]).sum())]
        return np.array(row)

    def _detach(self):
        self._dev = None

    def _read_device(self, w):
        lib, h = self._dev
        j = list(self.watches).index(w.name)
        out = {}
        for s in w.stats:
            for key, which in STAT_MAPS[s]:
                a = np.empty(w.n, np.int32 if key == "count" else np.float64)
                L.check(lib.knpemi_maps_read(h, j, which, a.ctypes.data_as(C.c_void_p), a.size))
                out[key] = a
        return out

    # -- host restatement --------------------------------------------------------------------------------
    @staticmethod
    def _fresh(n):
        S = {k: np.full(n, np.nan) for k in NAN_MAPS + ("v_prev",)}
        S.update({k: np.zeros(n) for k in ("integral", "exposure", "excess")})
        S["count"] = np.zeros(n, np.int32)
        return S

    def reset_host(self):
        """The host state back to "before the first record"; the host series is emptied."""
        self._host, self._t_prev, self._sums = None, None, None
        if self._dev is None:
            self.clear()

    def _sample(self, w, phi, c, phi_M_prev):
        if w.quantity == "phi":
            u = phi[w.tag]
        elif w.quantity == "phi_M":
            u = phi_M_prev[w.tag]
        else:
            k = self.ion_names.index(w.ion)
            u = c[w.tag][k] if k < len(self.ion_names) - 1 else self.ion_list[-1][f"c_{w.tag}"]
        v = _values(u)
        if v.shape != (w.n,):
            raise ValueError(f"watch {w.name!r}: {v.shape[0]} values for {w.n} items")
        return v

    def record_host(self, t, phi, c, phi_M_prev):
        """One record at time t from host data: phi[tag], c[tag][k] (solved ions; the eliminated one is read from
        ion_list[-1]["c_<tag>"]) and phi_M_prev[tag] are `Function`s or arrays.  The numpy restatement of the device
        kernel (the module docstring's rules), series row included; host drivers record with it, and it is the reference
        of the device tests.  `increment_sums(name)` accumulates the sum of |increment| of every accumulated statistic."""
        t = float(t)
        if not self.watches:
            raise ValueError("nothing is watched")
        if not np.isfinite(t) or (self._t_prev is not None and not t > self._t_prev):
            raise ValueError("record_host: t must be finite and greater than the previous record's")
        if self._host is None:
            self._host = {n: self._fresh(w.n) for n, w in self.watches.items()}
            self._sums = {n: {k: np.zeros(w.n) for k in ("integral", "exposure", "excess")} for n, w in self.watches.items()}
        t_prev = t if self._t_prev is None else self._t_prev
        dt = t - t_prev
        row = []
        for name, w in self.watches.items():
            S, A = self._host[name], self._sums[name]
            v = self._sample(w, phi, c, phi_M_prev)
            vp = S["v_prev"]
            thr, s = w.thr, w.sgn
            with np.errstate(invalid="ignore", divide="ignore"):
                fin = np.isfinite(v)
                later = fin & np.isfinite(vp)            # an interval is accounted for
                b = s * (v - thr)
                a = s * (vp - thr)
                if "integral" in w.stats:
                    q = np.flatnonzero(later)
                    inc = 0.5 * dt * (vp[q] + v[q])
                    S["integral"][q] += inc
                    A["integral"][q] += np.abs(inc)
                if "threshold" in w.stats:
                    seen = fin & ~later & (b >= 0.0)
                    onset = later & (a < 0.0) & (b >= 0.0)
                    stay = later & (a >= 0.0) & (b >= 0.0)
                    offset = later & (a >= 0.0) & (b < 0.0)
                    th = a / (a - b)
                    S["count"][seen | onset] += 1
                    one = S["count"] == 1
                    S["t_arrival"][seen & one] = t
                    q = np.flatnonzero(onset & one)
                    S["t_arrival"][q] = t_prev + dt * th[q]
                    for q, e_inc, x_inc in ((onset, (1.0 - th) * dt, 0.5 * (1.0 - th) * dt * b), (stay, np.full(w.n, dt), 0.5 * dt * (a + b)),
                                            (offset, th * dt, 0.5 * th * dt * a)):
                        S["exposure"][q] += e_inc[q]
                        S["excess"][q] += x_inc[q]
                        A["exposure"][q] += np.abs(e_inc[q])
                        A["excess"][q] += np.abs(x_inc[q])
                if "peak" in w.stats:
                    up = fin & ~(v <= S["v_max"])
                    S["v_max"][up] = v[up]
                    S["t_max"][up] = t
                if "trough" in w.stats:
                    dn = fin & ~(v >= S["v_min"])
                    S["v_min"][dn] = v[dn]
                    S["t_min"][dn] = t
                S["v_prev"] = v.copy()
                if w.series:
                    beyond = fin & (b >= 0.0)
                    row += [float(np.sum(w.w[beyond])), float(beyond.sum())]
        self._t_prev = t
        if row and self._dev is None:
            self._t.append(t)
            self._rows.append(np.array(row))
        return np.array(row)

    def increment_sums(self, name):
        """{"integral", "exposure", "excess": per item, the sum over the records of `record_host` of |increment|}: the scale
        of the rounding error of the accumulated statistics."""
        self._check(name)
        return {k: v.copy() for k, v in self._sums[name].items()}

    # -- output --------------------------------------------------------------------------------------------
    def locations(self, name):
        """(n, gdim) coordinates of the items of watch `name`, in the order of the field's nodal array."""
        return np.array(self._mesh(self._check(name)).x, np.float64)

    def maps(self, name, halo=None):
        """{map: (n,) array} of the selected statistics of watch `name` -- peak: "v_max", "t_max"; trough: "v_min",
        "t_min"; integral: "integral"; threshold: "count" (int32), "t_arrival", "exposure", "excess" -- and "locations"
        (n, gdim): the device state of an attached stepper (one synchronisation), else the state of `record_host`.
        halo: on a cell-partitioned problem, only the items this rank owns (`Halo.vertex_owner("bulk")` / `("mem")`);
        the union of the ranks' maps is the global one."""
        w = self._check(name)
        if self._dev is not None:
            S = self._read_device(w)
        else:
            S = self._host[name] if self._host is not None else self._fresh(w.n)
        out = {key: np.array(S[key]) for s in w.stats for key, _ in STAT_MAPS[s]}
        out["locations"] = self.locations(name)
        if halo is not None:
            mem = w.quantity == "phi_M"
            own = np.asarray(halo.vertex_owner("mem" if mem else "bulk"))
            off = total = 0
            for tag, sd in self.subdomain_list.items():
                if mem and tag == 0:
                    continue
                n = int(sd["mesh_mem" if mem else "mesh_sub"].num_vertices)
                if tag == w.tag:
                    off = total
                total += n
            if own.shape[0] != total:
                raise ValueError("maps: the halo does not number the items of these sub-domains")
            mine = own[off:off + w.n] == int(halo.rank)
            out = {k: v[mine] for k, v in out.items()}
        return out

    def front_speed(self, name, origin, halo=None, maps=None):
        """Least-squares slope of the distance from `origin` against `t_arrival` over the items the front reached:
        (speed, rms of the residual distances, number of items used); ValueError with fewer than 3.  maps: a map with
        "t_arrival" and "locations" to use instead (the union over the ranks of a partitioned run)."""
        m = self.maps(name, halo) if maps is None else maps
        if "t_arrival" not in m:
            raise ValueError(f"watch {name!r} has no threshold statistic")
        return conduction_velocity(m["locations"], m["t_arrival"], origin)

    def functions(self, name):
        """{map: `Function` on the watch's sub-mesh (membrane mesh)} of every map of `name`, for XdmfFile.write_function."""
        from .fem.function import Function, functionspace
        w = self._check(name)
        V = functionspace(self._mesh(w))
        out = {}
        for key, a in self.maps(name).items():
            if key == "locations":
                continue
            f = Function(V, name=f"{name}_{key}")
            f.x.array[:] = a
            out[key] = f
        return out

    def save(self, path, halo=None):
        """.npz with "<name>/<map>" for every watch and map ("<name>/locations" included) and, with a series watch,
        the series ("t", "<name>/measure", "<name>/n")."""
        out = {f"{n}/{k}": v for n in self.watches for k, v in self.maps(n, halo).items()}
        if self.has_series:
            out.update(self.series())
        np.savez(path, **out)

    def summary(self, name):
        """One line for a driver's log."""
        w, m = self._check(name), self.maps(name)
        what = w.quantity if w.ion is None else f"{w.quantity}[{w.ion}]"
        line = f"{name} ({what} on {w.tag}, {w.n} items):"
        if "peak" in w.stats and np.isfinite(m["v_max"]).any():
            line += f" peak {np.nanmin(m['v_max']):.6g} .. {np.nanmax(m['v_max']):.6g}"
        if "trough" in w.stats and np.isfinite(m["v_min"]).any():
            line += f" trough {np.nanmin(m['v_min']):.6g} .. {np.nanmax(m['v_min']):.6g}"
        if "threshold" in w.stats:
            hit = m["count"] > 0
            line += f" {int(hit.sum())} {'below' if w.sgn < 0 else 'beyond'} {w.thr:.6g}"
            if hit.any():
                line += f", arrival {np.nanmin(m['t_arrival']):.6g} .. {np.nanmax(m['t_arrival']):.6g}"
                line += f", longest exposure {m['exposure'].max():.6g}"
        return line
