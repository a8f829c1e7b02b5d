"""CPU tests of the field maps (knpemi.maps.FieldMaps): the numpy restatement `record_host` against hand-computed values
and against independent exact integrals, the definitions, the owned selection, the front speed, the generator of the
kernel test's samples, the driver flag and the ABI table."""
import ctypes as C
import importlib.util
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import maps_cases as mc
from knpemi.maps import FieldMaps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


class _Mesh:
    """n vertices on a line, as the sub-mesh of a watch: what FieldMaps reads of a mesh without a series."""

    def __init__(self, n):
        self.num_vertices, self.x = n, np.arange(float(n))[:, None]


def _line(n=3):
    subs = {0: dict(mesh_sub=_Mesh(n)), 1: dict(mesh_sub=_Mesh(n), mesh_mem=_Mesh(n))}
    ions = [dict(name="K"), dict(name="Cl"), dict(name="Na")]
    return subs, ions


T = [0.0, 1.0, 2.0, 4.0]
# item 0: onset, stay, offset;  item 1: exactly at the level at first sight, stays at it, leaves, comes back;
# item 2: beyond at the first record, a NaN sample in the middle
V = np.array([[0.0, 2.0, 2.0, 0.0], [1.0, 1.0, 0.5, 3.0], [2.0, NAN, 0.0, 2.0]]).T
WANT = dict(count=[1, 2, 2], t_arrival=[0.5, 0.0, 0.0], exposure=[2.5, 2.6, 1.0], excess=[1.75, 1.6, 0.5],
            integral=[5.0, 5.25, 2.0], v_max=[2.0, 3.0, 2.0], t_max=[1.0, 4.0, 0.0], v_min=[0.0, 0.5, 0.0],
            t_min=[0.0, 2.0, 2.0])


def _play(fm, v):
    for k, t in enumerate(T):
        fm.record_host(t, {0: v[k]}, {}, {})


def test_record_host_against_hand_computed_values():
    subs, ions = _line()
    fm = FieldMaps(subs, ions)
    fm.watch("up", "phi", tag=0, threshold=1.0)
    _play(fm, V)
    m = fm.maps("up")
    assert set(m) == set(WANT) | {"locations"} and m["count"].dtype == np.int32
    for key, want in WANT.items():
        assert np.allclose(m[key], want, rtol=4e-16, atol=0), (key, m[key])
    # below=True, mirrored: the same counts, times, exposure and excess; values and integral with the other sign
    fm = FieldMaps(subs, ions)
    fm.watch("down", "phi", tag=0, threshold=-1.0, below=True)
    _play(fm, -V)
    m = fm.maps("down")
    for key in ("count", "t_arrival", "exposure", "excess"):
        assert np.allclose(m[key], WANT[key], rtol=4e-16, atol=0), key
    assert np.array_equal(m["v_min"], -np.array(WANT["v_max"])) and np.array_equal(m["t_min"], WANT["t_max"])
    assert np.array_equal(m["v_max"], -np.array(WANT["v_min"])) and np.array_equal(m["t_max"], WANT["t_min"])
    assert np.allclose(m["integral"], -np.array(WANT["integral"]), rtol=4e-16)
    # times must increase
    with pytest.raises(ValueError, match="greater"):
        fm.record_host(4.0, {0: V[0]}, {}, {})


def _exact(t, v, thr, s):
    """(integral, exposure, excess) of the piecewise-linear interpolant of one item's finite samples, in exact rational
    arithmetic, segment by segment; a segment with a non-finite end is skipped."""
    integral = exposure = excess = Fraction(0)
    for k in range(1, len(t)):
        if not (np.isfinite(v[k - 1]) and np.isfinite(v[k])):
            continue
        d = Fraction(t[k]) - Fraction(t[k - 1])
        a, b = s * (Fraction(v[k - 1]) - Fraction(thr)), s * (Fraction(v[k]) - Fraction(thr))
        integral += d * (Fraction(v[k - 1]) + Fraction(v[k])) / 2
        if a >= 0 and b >= 0:
            exposure += d
            excess += d * (a + b) / 2
        elif a < 0 <= b or b < 0 <= a:           # one zero of the interpolant, at the fraction z of the segment
            z = a / (a - b)
            part, top = (1 - z, b) if b >= 0 else (z, a)
            exposure += d * part
            excess += d * part * top / 2
    return float(integral), float(exposure), float(excess)


@pytest.mark.parametrize("below", [False, True])
def test_integral_exposure_and_excess_are_the_exact_integrals_of_the_interpolant(below):
    rng = np.random.default_rng(11)
    t = mc.record_times(rng)
    subs, ions = _line(24)
    s = -1.0 if below else 1.0
    thr = s * mc.LEVEL
    v = mc.samples(rng, 24, t, thr, s)
    fm = FieldMaps(subs, ions)
    fm.watch("w", "c", tag=1, ion="Cl", threshold=thr, below=below)
    for k in range(len(t)):
        fm.record_host(t[k], {}, {1: {1: v[k]}}, {})
    m, S = fm.maps("w"), fm.increment_sums("w")
    trapz = getattr(np, "trapezoid", None) or np.trapz
    for i in range(24):
        want = _exact(t, v[:, i], thr, s)
        for key, x in zip(("integral", "exposure", "excess"), want):
            assert abs(m[key][i] - x) <= (8 + len(t)) * mc.EPS * S[key][i], (key, i)
        if np.isfinite(v[:, i]).all():
            assert abs(m["integral"][i] - trapz(v[:, i], t)) <= (8 + len(t)) * mc.EPS * S["integral"][i]
    assert np.isfinite(v[:, 3]).sum() == len(t) - 1 and m["integral"][3] != 0.0      # the NaN item skips two segments
    # peak and trough: the extreme finite samples and the time of their first occurrence
    assert np.array_equal(m["v_max"], np.nanmax(v, axis=0)) and np.array_equal(m["v_min"], np.nanmin(v, axis=0))
    assert np.array_equal(m["t_max"], t[np.nanargmax(v, axis=0)]) and np.array_equal(m["t_min"], t[np.nanargmin(v, axis=0)])


def test_measure_is_the_lumped_measure_of_the_region_beyond_the_level():
    from knpemi.fem.probe import integral_weights
    s = mc.host_setup("2d")
    fm = FieldMaps(s.subdomain_list, s.ion_list)
    fm.watch("K", "c", tag=0, ion="K", threshold=0.3, series=True)
    fm.watch("phi_M", "phi_M", tag=1, threshold=-0.1, below=True, series=True)
    assert fm.columns() == [("K/measure", 1), ("K/n", 1), ("phi_M/measure", 1), ("phi_M/n", 1)]
    sub, mem = s.subdomain_list[0]["mesh_sub"], s.subdomain_list[1]["mesh_mem"]
    w0, w1 = integral_weights(sub), integral_weights(mem)
    rng = np.random.default_rng(2)
    for k in range(3):
        a, b = rng.uniform(0, 1, sub.num_vertices), rng.uniform(-1, 1, mem.num_vertices)
        a[0] = 0.3                                   # exactly at the level: beyond
        fm.record_host(float(k), {}, {0: {0: a}}, {1: b})
        row = fm.series()
        assert row["t"].shape == (k + 1,)
        assert row["K/measure"][k] == w0[a >= 0.3].sum() and row["K/n"][k] == (a >= 0.3).sum() and a[0] >= 0.3
        assert row["phi_M/measure"][k] == w1[b <= -0.1].sum() and row["phi_M/n"][k] == (b <= -0.1).sum()
    assert 0 < row["K/measure"][-1] < w0.sum() and abs(w1.sum() - 2 * (60e-6 + 2e-6)) < 1e-12      # the perimeter


def test_unselected_statistics_keep_their_initial_values():
    subs, ions = _line()
    fm = FieldMaps(subs, ions)
    fm.watch("peak", "phi", tag=0, stats=("peak",))
    fm.watch("rest", "phi", tag=0, threshold=1.0, stats=("trough", "integral", "threshold"))
    _play(fm, V)
    assert set(fm.maps("peak")) == {"v_max", "t_max", "locations"}
    assert set(fm.maps("rest")) == set(WANT) - {"v_max", "t_max"} | {"locations"}
    S = fm._host["peak"]
    assert np.isnan(S["v_min"]).all() and np.isnan(S["t_min"]).all() and np.isnan(S["t_arrival"]).all()
    assert not S["integral"].any() and not S["exposure"].any() and not S["excess"].any() and not S["count"].any()
    S = fm._host["rest"]
    assert np.isnan(S["v_max"]).all() and np.isnan(S["t_max"]).all()
    assert np.array_equal(fm.maps("peak")["v_max"], WANT["v_max"]) and np.allclose(fm.maps("rest")["excess"], WANT["excess"])
    # before any record, and after reset_host: the initial state
    fm.reset_host()
    m = fm.maps("rest")
    assert np.isnan(m["v_min"]).all() and np.isnan(m["t_arrival"]).all() and not m["count"].any() and not m["integral"].any()


def test_definition_errors():
    subs, ions = _line()
    fm = FieldMaps(subs, ions)
    fm.watch("a", "phi", tag=0)
    for kw, match in ((dict(name="a", quantity="phi", tag=0), "twice"), (dict(name="b", quantity="phi", tag=7), "no sub-domain"),
                      (dict(name="b", quantity="c", tag=0, ion="Ca"), "unknown ion"),
                      (dict(name="b", quantity="phi_M", tag=0), "no membrane"),
                      (dict(name="b", quantity="J", tag=0), "quantity"),
                      (dict(name="b", quantity="phi", tag=0, stats=("peak", "median")), "stats"),
                      (dict(name="b", quantity="phi", tag=0, stats=()), "stats"),
                      (dict(name="b", quantity="phi", tag=0, stats=("threshold",)), "finite threshold"),
                      (dict(name="b", quantity="phi", tag=0, threshold=NAN), "finite threshold"),
                      (dict(name="b", quantity="phi", tag=0, below=True), "need the threshold"),
                      (dict(name="b", quantity="phi", tag=0, series=True), "need the threshold"),
                      (dict(name="b", quantity="phi", tag=0, threshold=1.0, stats=("peak",), series=True), "need the threshold"),
                      (dict(name="b", quantity="phi", tag=0), "repeats")):
        with pytest.raises(ValueError, match=match):
            fm.watch(**kw)
    assert list(fm.watches) == ["a"] and fm.watches["a"].stats == ("peak", "trough", "integral")      # no level: no threshold
    fm.watch("lvl", "phi", tag=0, threshold=0.0)
    assert fm.watches["lvl"].stats == mc.ALL and not fm.has_series and fm.columns() == []
    for j in range(6):
        fm.watch(f"w{j}", "c", tag=0, ion="K", threshold=float(j))
    with pytest.raises(ValueError, match="one space"):
        fm.watch("ninth", "phi", tag=0, threshold=9.0)
    fm.watch("mem", "phi_M", tag=1)                      # another space
    with pytest.raises(ValueError, match="no watch"):
        fm.maps("nothing")
    with pytest.raises(ValueError, match="4 values for 3 items"):
        fm.record_host(0.0, {0: np.zeros(4)}, {0: {0: np.zeros(3)}}, {1: np.zeros(3)})
    spec, thr, wt = fm.table({0: 0, 1: 1})
    from knpemi import _lib as L
    assert spec.shape == (9, 4) and wt is None and spec[0].tolist() == [L.F_PHI, 0, 0, 7]
    assert spec[2].tolist() == [L.F_C, 0, 0, 15] and spec[8].tolist() == [L.F_PHI_M, 1, 0, 7] and thr[3] == 1.0


def test_maps_of_a_halo_selects_the_owned_items(tmp_path):
    subs, ions = _line(5)
    subs[2] = dict(mesh_sub=_Mesh(4), mesh_mem=_Mesh(6))
    fm = FieldMaps(subs, ions)
    fm.watch("bulk", "c", tag=1, ion="Na", stats=("peak",))
    fm.watch("mem", "phi_M", tag=2, stats=("trough",))
    ions[-1]["c_1"] = np.arange(5.0)
    fm.record_host(0.5, {}, {}, {2: np.arange(6.0)})

    class Halo:
        rank = 1
        owner = dict(bulk=np.array([0] * 5 + [1, 0, 1, 1, 0] + [0] * 4), mem=np.array([1] * 5 + [0, 1, 1, 0, 0, 1]))

        def vertex_owner(self, kind):
            return self.owner[kind]
    m = fm.maps("bulk", halo=Halo())
    assert np.array_equal(m["v_max"], [0.0, 2.0, 3.0]) and np.array_equal(m["locations"][:, 0], [0.0, 2.0, 3.0])
    m = fm.maps("mem", halo=Halo())
    assert np.array_equal(m["v_min"], [1.0, 2.0, 5.0]) and np.array_equal(m["t_min"], [0.5] * 3)
    Halo.owner["bulk"] = np.zeros(3)
    with pytest.raises(ValueError, match="does not number"):
        fm.maps("bulk", halo=Halo())
    # save: every map of every watch; no series without a series watch
    fm.save(tmp_path / "m.npz")
    z = np.load(tmp_path / "m.npz")
    assert set(z.files) == {"bulk/v_max", "bulk/t_max", "bulk/locations", "mem/v_min", "mem/t_min", "mem/locations"}
    assert "peak 0 .. 4" in fm.summary("bulk")


def test_front_speed_recovers_a_planted_plane_front():
    """v = g(c t - x.d) with g = tanh(. / l) rises through the level 0 when the plane x.d = c t passes.  The recorder finds
    the zero of the linear interpolant in time between two records D apart.  The interpolant is off by at most
    D^2 max|v_tt| / 8 = D^2 c^2 M2 / 8 (M2 = max |g''| = 4 / (3 sqrt 3 l^2)), and v crosses the level with the slope
    c g' >= c m1, m1 = min g' over the |xi| <= c D a crossing segment spans, so every arrival time is off by at most
    delta = D^2 c M2 / (8 m1).  The distances are c t_true + const exactly, so the least-squares slope against the recorded
    times is off by at most c delta / std(t_arrival) (Cauchy-Schwarz on the covariance of the times and their errors)."""
    s = mc.host_setup("2d")
    fm = FieldMaps(s.subdomain_list, s.ion_list)
    fm.watch("front", "c", tag=0, ion="K", threshold=0.0, stats=("threshold",))
    x = fm.locations("front")
    d = np.array([1.0, 0.0])
    xi = x @ d - (x @ d).min()
    n, D = 64, 1.0e-3
    c = xi.max() / ((n - 8) * D)
    ell = 4.0 * c * D
    t = D * np.arange(n)
    v = np.tanh((c * (t[:, None] - 3.0 * D) - xi[None, :]) / ell)
    for k in range(n):
        fm.record_host(t[k], {}, {0: {0: v[k]}}, {})
    m = fm.maps("front")
    assert (m["count"] == 1).all() and (m["t_arrival"] > t[0]).all()
    M2, m1 = 4.0 / (3.0 * np.sqrt(3.0) * ell ** 2), 1.0 / (ell * np.cosh(c * D / ell) ** 2)
    # the condition on the host data: the second differences of the samples stay within the bound on v_tt they stand for
    assert np.abs(v[2:] - 2.0 * v[1:-1] + v[:-2]).max() <= (c * D) ** 2 * M2 * (1 + 1e-12)
    delta = D ** 2 * c * M2 / (8.0 * m1)
    assert np.abs(m["t_arrival"] - (3.0 * D + xi / c)).max() <= delta
    # distances along d: the coordinate of every vertex on the line through the origin
    line = dict(t_arrival=m["t_arrival"], locations=xi[:, None])
    speed, rms, used = fm.front_speed("front", [0.0], maps=line)
    bound = c * delta / np.std(m["t_arrival"])
    assert used == x.shape[0] and abs(speed - c) <= bound and bound <= 2e-3 * c, (speed, c, bound)
    # from a point origin on the axis far behind the front the Euclidean distances are those up to h^2 / (2 R)
    R = 1.0e3 * xi.max()
    far = np.array([(x @ d).min() - R, x[:, 1].mean()])
    speed2, _, _ = fm.front_speed("front", far)
    assert abs(speed2 - c) <= bound + c * np.ptp(x[:, 1]) ** 2 / (2.0 * R) / (np.std(m["t_arrival"]) * c)
    with pytest.raises(ValueError, match="no threshold"):
        fm.front_speed("front", far, maps=dict(locations=x))
    f = fm.functions("front")
    assert set(f) == {"count", "t_arrival", "exposure", "excess"} and f["t_arrival"].function_space.mesh is s.subdomain_list[0]["mesh_sub"]
    assert np.array_equal(f["t_arrival"].x._a, m["t_arrival"])


CASES = [(kind, name) for kind in ("2d", "tet", "three") for name in ("one_c", "four", "phi_M", "bulk_and_membrane")]


@pytest.mark.parametrize("kind,name", CASES, ids=[f"{k}-{n}" for k, n in CASES])
def test_the_synthetic_samples_meet_the_conditions_of_the_kernel_test(kind, name):
    s = mc.host_setup(kind)
    cells = tuple(list(s.subdomain_list)[1:])
    fm = mc.field_maps(s, mc.config(name, cells))
    rng = np.random.default_rng(5)
    t = mc.record_times(rng)
    play = mc.Play(fm, rng, t)
    rows = np.array([fm.record_host(t[k], *play.host(k)) for k in range(len(t))])
    mc.check_conditions(fm, play, rows)
    assert rows.shape == (len(t), fm.n_cols) and fm.n_cols == 2 * sum(w.series for w in fm.watches.values()) <= 4
    assert np.array_equal(fm.series()["t"], t)
    # the comparison accepts the reference itself, and refuses a map that is off by more than its tolerance
    for wname in fm.watches:
        m, S = fm.maps(wname), fm.increment_sums(wname)
        assert mc.compare(m, m, S, t) == 0.0
        if "exposure" in m:
            bad = {k: v.copy() for k, v in m.items()}
            bad["exposure"][6] += 60.0 * mc.EPS * S["exposure"][6]
            with pytest.raises(AssertionError):
                mc.compare(bad, m, S, t)


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_drivers_parse_the_maps_flag():
    run_2d = _load("idealized_geometries/run_2D.py", "run_2D_maps")
    a = run_2d.build_parser().parse_args(["--maps", "m.npz", "--maps-threshold", "3.5"])
    kw = run_2d.recorder_arguments(a)
    assert kw["maps"] == "m.npz" and kw["maps_threshold"] == 3.5
    a = run_2d.build_parser(res=0, steps=20).parse_args([])
    assert a.maps is None and a.maps_threshold is None and (a.res, a.steps) == (0, 20)
    src = open(os.path.join(ROOT, "examples", "idealized_geometries", "run_3D.py")).read()
    assert "build_parser(" in src and "recorder_arguments(a)" in src
    stim = _load("local_astrocyte_depolarization/run_stim_duration.py", "run_stim_maps")
    a = stim.build_parser().parse_args(["--maps", "m.npz"])
    assert a.maps == "m.npz" and a.maps_threshold is None
    # the watches of the drivers
    s = mc.host_setup("2d")
    fm = run_2d.field_maps(s, 3.4)
    assert list(fm.watches) == ["K_ecs", "phi_M_1"] and fm.watches["K_ecs"].stats == ("peak", "integral", "threshold")
    assert fm.watches["phi_M_1"].stats == ("peak", "trough") and fm.columns() == [("K_ecs/measure", 1), ("K_ecs/n", 1)]


NAMES = ("knpemi_maps_set", "knpemi_maps_record", "knpemi_maps_read", "knpemi_maps_series_read", "knpemi_maps_reset",
         "knpemi_maps_clear")


def test_maps_abi_is_declared_exported_and_bound(hip_lib):
    from knpemi import _lib as L
    header = open(os.path.join(ROOT, "include", "knpemi_hip.h")).read()
    ctype_of = {"knpemi_handle*": C.c_void_p, "int": C.c_int, "double": C.c_double, "const int32_t*": L.c_int_p,
                "const double*": L.c_dbl_p, "double*": L.c_dbl_p, "void*": C.c_void_p, "size_t": C.c_size_t,
                "int64_t*": C.POINTER(C.c_int64)}
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in knpemi_hip.h"
        params = [" ".join(p.split()[:-1]) for p in m.group(1).replace("\n", " ").split(",")]
        assert hasattr(hip_lib, name), f"{name} is not exported"
        res, args = L.SIGNATURES[name]
        assert res is C.c_int and args == [ctype_of[p] for p in params], (name, params)
    consts = dict(re.findall(r"#define\s+KNPEMI_(MAPS?_[A-Z_]+)\s+(\d+)", header))
    assert len(consts) == 17
    for key, val in consts.items():
        assert getattr(L, key) == int(val), key
    # the rules are stated in the header, the kernel file and the Python module
    kernel = open(os.path.join(ROOT, "knp-emi-fenics-x_amd", "csrc", "kernels_maps.hip")).read()
    import knpemi.maps
    for text in (header, kernel, knpemi.maps.__doc__):
        flat = " ".join(w for w in text.split() if w not in ("*", "//"))
        for rule in ("theta = a / (a - b)", "0.5 (1 - theta) D b", "0.5 theta D a", "0.5 D (a + b)", "0.5 D (v_prev + v)"):
            assert rule in flat, rule
    # a null handle is refused before anything touches a device
    assert hip_lib.knpemi_maps_record(None, 0.0) == L.EINVAL and hip_lib.knpemi_maps_set(None, 0, None, None, None, 0) == L.EINVAL
    assert hip_lib.knpemi_maps_read(None, 0, 0, None, 0) == L.EINVAL and hip_lib.knpemi_maps_reset(None) == L.EINVAL
    assert hip_lib.knpemi_maps_series_read(None, 0, None, None, None, 0) == L.EINVAL and hip_lib.knpemi_maps_clear(None) == L.EINVAL
