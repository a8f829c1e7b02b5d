"""What the field-map tests share (test_maps_host.py, test_maps_gpu.py, tools/check_partition_maps.py): the watch
configurations of the kernel test, the synthetic samples with their planted items, and the comparison of a device map
with the host restatement `FieldMaps.record_host`.

Tolerances, from the formulas (eps = 2^-52, n = number of records, D = t - t_prev of the record concerned):
  count, v_max, t_max, v_min, t_min and the NaN pattern of every array: equal -- copies of inputs and integer counts, and
    the comparisons s (v - thr) >= 0 see identical operands;
  t_arrival: within 8 eps max(|t|, D), the bound tests/test_events_gpu.py derives for the same formula;
  integral, exposure, excess: within (8 + n) eps S, S the sum over the records of |increment| of that item and statistic
    (`FieldMaps.increment_sums`): an increment has at most six roundings, and every accumulation rounds once on either side;
  <name>/n: equal;  <name>/measure: within 2 N 2^-53 sum |term| over the N items summed (a changed order of summation).
"""
import contextlib
import io

import numpy as np

from knpemi import _lib as L
from knpemi.maps import FieldMaps

EPS = 2.0 ** -52
N_REC = 40
LEVEL = 0.2                      # of the sinusoids A sin(...), A in [0.5, 1.5]

# name -> [(watch name, quantity, tag, ion, keyword arguments)] on a problem with the cells `cells`; at most two series
# watches each.  "four": four watches of one space, phi and every ion, the eliminated one (Na) included.
ALL = ("peak", "trough", "integral", "threshold")


def config(name, cells):
    if name == "one_c":
        return [("K_ecs", "c", 0, "K", dict(threshold=LEVEL, stats=ALL, series=True))]
    if name == "four":
        return [("phi_ecs", "phi", 0, None, dict(stats=("peak", "trough"))),
                ("K_ecs", "c", 0, "K", dict(threshold=LEVEL, stats=ALL, series=True)),
                ("Cl_ecs", "c", 0, "Cl", dict(threshold=-LEVEL, below=True, stats=("integral", "threshold"), series=True)),
                ("Na_ecs", "c", 0, "Na", dict(threshold=LEVEL, stats=("peak", "threshold")))]
    if name == "phi_M":
        return [(f"phi_M_{t}", "phi_M", t, None, dict(threshold=LEVEL if t == cells[0] else -LEVEL, below=t != cells[0],
                                                      series=True)) for t in cells]
    if name == "bulk_and_membrane":
        return [("K_ics", "c", cells[-1], "K", dict(threshold=LEVEL, stats=("trough", "threshold"), series=True)),
                ("Na_ics", "c", cells[-1], "Na", dict(stats=("integral",))),
                ("phi_M", "phi_M", cells[-1], None, dict(threshold=LEVEL, series=True))]
    raise ValueError(name)


def field_maps(s, watches):
    fm = FieldMaps(s.subdomain_list, [dict(ion) for ion in s.ion_list])      # Play.host sets the eliminated ion's entry
    for name, quantity, tag, ion, kw in watches:
        fm.watch(name, quantity, tag, ion=ion, **kw)
    return fm


def host_setup(kind):
    """The sub-domains and ions of the three problems of the kernel test, without device forms."""
    import exchange_cases
    return exchange_cases.build(kind, forms=False)


def record_times(rng, n=N_REC):
    return np.cumsum(rng.uniform(0.4e-3, 1.6e-3, n))             # non-uniform


def samples(rng, n_items, t, thr, sgn):
    """[n_t][n_items]: A_i sin(2 pi f_i t_k + p_i), and the planted items 0 .. 4 (relative to the level thr, "beyond" in
    direction sgn): constant exactly at the level; touching it at exactly one record; up once and staying; one NaN sample;
    never reaching it."""
    assert n_items >= 8
    A = rng.uniform(0.5, 1.5, n_items)
    f = rng.uniform(50.0, 400.0, n_items)
    ph = rng.uniform(0.0, 2.0 * np.pi, n_items)
    v = A[None, :] * np.sin(2.0 * np.pi * f[None, :] * t[:, None] + ph[None, :])
    v[:, 0] = thr
    v[:, 1] = thr - sgn * 0.3
    v[17, 1] = thr
    v[:, 2] = thr - sgn * 0.4
    v[8:, 2] = thr + sgn * 0.4
    v[11, 3] = np.nan
    v[:, 4] = 0.1 * np.sin(2.0 * np.pi * f[4] * t + ph[4]) + thr - sgn * 0.2
    return v


class Play:
    """The samples of every watched field of `fm`, and the host view record_host takes of record k."""

    def __init__(self, fm, rng, t):
        self.fm, self.t = fm, t
        self.v = {}                       # (quantity, tag, ion) -> [n_t][n]
        for w in fm.watches.values():
            key = (w.quantity, w.tag, w.ion)
            if key not in self.v:         # the planted items follow the level of the field's first watch
                self.v[key] = samples(rng, w.n, t, w.thr, w.sgn)

    def host(self, k):
        """(phi, c, phi_M_prev) of record k: {tag: array} each, c[tag][ion index]; the eliminated ion goes through
        ion_list[-1]["c_<tag>"] as in the drivers."""
        fm = self.fm
        phi, c, phi_M = {}, {}, {}
        for (quantity, tag, ion), v in self.v.items():
            if quantity == "phi":
                phi[tag] = v[k]
            elif quantity == "phi_M":
                phi_M[tag] = v[k]
            else:
                j = fm.ion_names.index(ion)
                if j == len(fm.ion_names) - 1:
                    fm.ion_list[-1][f"c_{tag}"] = v[k]
                else:
                    c.setdefault(tag, {})[j] = v[k]
        return phi, c, phi_M

    def push(self, dp, k):
        """Record k's samples into the device fields."""
        fm = self.fm
        for (quantity, tag, ion), v in self.v.items():
            s = dp.sub_index[tag]
            if quantity == "phi":
                dp.push_array(L.F_PHI, s, 0, v[k])
            elif quantity == "phi_M":
                dp.push_array(L.F_PHI_M, s, 0, v[k])
            else:
                j = fm.ion_names.index(ion)
                if j == len(fm.ion_names) - 1:
                    dp.push_array(L.F_C_ELIM, s, 0, v[k])
                else:
                    dp.push_array(L.F_C, s, j, v[k])


def check_conditions(fm, play, rows):
    """The conditions of the kernel test, on the host reference after all records."""
    n_t = len(play.t)
    first = {}
    for name, w in fm.watches.items():
        first.setdefault((w.quantity, w.tag, w.ion), name)
    for name, w in fm.watches.items():
        if "threshold" not in w.stats:
            continue
        count = fm.maps(name)["count"]
        assert (count >= 2).mean() >= 0.25 and (count == 0).any(), name
        if first[(w.quantity, w.tag, w.ion)] == name:
            m = fm.maps(name)
            assert count[0] == 1 and m["t_arrival"][0] == play.t[0] and m["exposure"][0] > 0 and m["excess"][0] == 0
            assert count[1] == 1 and count[2] == 1 and count[4] == 0, (name, count[:5])
            assert play.t[16] < m["t_arrival"][1] <= play.t[17] and play.t[7] < m["t_arrival"][2] < play.t[8]
    j = 0
    for name, w in fm.watches.items():
        if not w.series:
            continue
        measure = rows[:, j]
        inside = (measure > 0) & (measure < w.w.sum() * (1 - 1e-12))
        assert inside.sum() >= n_t // 2, (name, int(inside.sum()))
        j += 2


def time_tol(ref, t):
    """8 eps max(|t_k|, t_k - t_(k-1)) for every arrival time in `ref`, t_k being the record that found it (the first
    record at or after it)."""
    t = np.asarray(t)
    k = np.clip(np.searchsorted(t, np.nan_to_num(ref, nan=t[0])), 1, len(t) - 1)
    return 8.0 * EPS * np.maximum(np.abs(t[k]), t[k] - t[k - 1])


def compare(dev, ref, sums, t, n_rec=None):
    """A device map against the host map of the same watch; sums: `increment_sums` of the host; t: the record times.
    Returns the largest |dev - ref| / S over the accumulated statistics (0 when they agree bit for bit)."""
    n_rec = len(t) if n_rec is None else n_rec
    assert set(dev) == set(ref)
    worst = 0.0
    for key in ref:
        a, b = dev[key], ref[key]
        assert a.shape == b.shape and a.dtype == b.dtype, key
        if key in ("count", "v_max", "t_max", "v_min", "t_min", "locations"):
            assert np.array_equal(a, b, equal_nan=key != "count"), key
        elif key == "t_arrival":
            assert np.array_equal(np.isnan(a), np.isnan(b)), key
            ok = ~np.isnan(b)
            assert (np.abs(a - b)[ok] <= time_tol(b, t)[ok]).all(), (key, np.nanmax(np.abs(a - b)))
        else:
            S = sums[key]
            assert np.isfinite(a).all() and (np.abs(a - b) <= (8 + n_rec) * EPS * S).all(), \
                (key, float(np.max(np.abs(a - b) / np.maximum(S, 1e-300))))
            worst = max(worst, float(np.max(np.abs(a - b) / np.maximum(S, 1e-300))))
    return worst


def series_terms(fm, play, k):
    """Per series column of record k: (N, sum |term|) of the measure's sum, for its tolerance."""
    out = []
    for w in fm.watches.values():
        if w.series:
            v = play.v[(w.quantity, w.tag, w.ion)][k]
            with np.errstate(invalid="ignore"):
                beyond = w.sgn * (v - w.thr) >= 0.0
            out.append((int(beyond.sum()), float(np.abs(w.w[beyond]).sum())))
    return out


def compare_series(fm, dev_rows, ref_rows, terms):
    """Device rows against the rows of record_host: n equal, measure within 2 N 2^-53 sum |term|; terms[k]: `series_terms`
    (or the same from the fields of record k)."""
    dev_rows, ref_rows = np.asarray(dev_rows), np.asarray(ref_rows)
    assert dev_rows.shape == ref_rows.shape
    for k in range(ref_rows.shape[0]):
        for j, (N, S) in enumerate(terms[k]):
            assert dev_rows[k, 2 * j + 1] == ref_rows[k, 2 * j + 1] == N
            assert abs(dev_rows[k, 2 * j] - ref_rows[k, 2 * j]) <= 2.0 * N * 2.0 ** -53 * S, (k, j)


def quiet():
    return contextlib.redirect_stdout(io.StringIO())
