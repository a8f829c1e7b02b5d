"""GPU tests of the ion fluxes (knpemi_flux_*, csrc/kernels_flux.hip, DeviceStepper.fluxes) against the numpy restatement
IonFluxes.compute_host, which tests/test_flux_host.py pins to the definitions and to the oracle's operators.  TOL is
relative to the largest magnitude of the compared component over the sub-domain; every watched set includes the
eliminated ion."""
import contextlib
import ctypes as C
import functools
import io

import numpy as np
import pytest

import unstructured_meshes as um
from helpers import TOL, Setup
from knpemi import IonFluxes, fluxes
from knpemi import _lib as L

pytestmark = pytest.mark.gpu

# "2d_r3" and "mms44": the sizes at which the fold of the workgroup partials takes another path (see
# test_setups_cover_the_workgroup_cases)
SETUPS = ("2d", "2d_r3", "mms44", "tet", "hex", "three", "jittered", "fan3d")


def _stepper(s, **kw):
    from knpemi.stepper import DeviceStepper
    return DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev, **kw)


def _build(name):
    with contextlib.redirect_stdout(io.StringIO()):
        if name == "three":
            from knpemi.fem import make_mesh_3D
            from test_gpu_parity import _custom_problem
            mesh, ct, ft = make_mesh_3D(0, "tetrahedron", axon_tags=(1, 1, 2, 2))
            return _custom_problem(mesh, ct, ft, {1: [(1, "hh_si")], 2: [(2, "glial")]})       # perturbed already
        if name in ("jittered", "fan3d"):
            data = um.jittered_tet_box() if name == "jittered" else um.fan_mesh(3)
            s = Setup("tet", 0, mesh_data=data)
        elif name == "2d_r3":
            s = Setup("2d", 3)
        elif name == "mms44":
            from knpemi.fem import make_mesh_mms
            s = Setup("2d", 1, mesh_data=make_mesh_mms(44))
        else:
            s = Setup(name, {"2d": 1, "tet": 0, "hex": 0}[name])
        s.perturb()
    return s


def _host_state(s):
    """phi and the K concentrations the device records hold: c_prev of the solved ions, the eliminated ion's c."""
    tags = list(s.subdomain_list)
    return ({t: s.phi[t].x._a for t in tags},
            {t: [f.x._a for f in s.c_prev[t]] + [s.ion_list[-1][f"c_{t}"].x._a] for t in tags})


def _rel(got, want):
    scale = np.abs(want).max(axis=0)
    return float((np.abs(got - want).max(axis=0) / np.where(scale > 0, scale, 1.0)).max())


def _row_err(fl, dev, row):
    """Largest error of a device row against a row dictionary of compute_host, every key relative to the key's largest
    component."""
    worst, j = 0.0, 0
    for key, w in fl.columns():
        want = np.atleast_1d(np.asarray(row[key], np.float64))
        worst = max(worst, float(np.abs(dev[j:j + w] - want).max() / np.abs(want).max()))
        j += w
    return worst


def _read(dp, n_cols, k, reset=0):
    buf = np.full((max(k, 1), n_cols), np.nan)
    rows, over = C.c_int64(), C.c_int64()
    L.check(dp.lib.knpemi_flux_read(dp.h, k, L.dptr(buf), C.byref(rows), C.byref(over), reset))
    return buf, rows.value, over.value


@functools.lru_cache(maxsize=None)
def _recorded(name):
    """(set-up, fluxes watching everything, device fields of one record, the record's row)."""
    s = _build(name)
    st = _stepper(s)
    fl = IonFluxes(s.subdomain_list, s.ion_list, s.physical_parameters)
    for tag in s.subdomain_list:
        fl.watch(tag)
    st.fluxes(fl, fields=True)
    dp = st.dp
    L.check(dp.lib.knpemi_flux_record(dp.h, 1))
    dev = {tag: fl.fields(tag) for tag in s.subdomain_list}
    buf, rows, over = _read(dp, fl.n_cols, 1, reset=1)
    assert rows == 1 and over == 0
    return s, st, fl, dev, buf[0]


@pytest.mark.parametrize("name", SETUPS)
def test_fields_and_row_match_the_restatement(hip_lib, name):
    s, st, fl, dev, row = _recorded(name)
    fields, want = fl.compute_host(*_host_state(s))
    worst = 0.0
    for tag in s.subdomain_list:
        assert set(dev[tag]) == set(fields[tag])
        for key in fields[tag]:
            assert dev[tag][key].shape == (fl.n_cells(tag), s.mesh.gdim)
            worst = max(worst, _rel(dev[tag][key], fields[tag][key]))
    e_row = _row_err(fl, row, want)
    print(name, "fields", worst, "row", e_row)
    assert worst < TOL and e_row < TOL
    if name == "tet":       # the lattice path of the row kernels; the flux kernel reads the same records
        flags = C.c_int(-1)
        L.check(st.dp.lib.knpemi_debug_geometry(st.dp.h, C.byref(flags)))
        assert flags.value & 1


def test_setups_cover_the_workgroup_cases(hip_lib):
    """From the cell counts and the kernel's cells per workgroup: one watched sub-domain spans several workgroups, one
    fits in a single workgroup, one has a partial last wave.  From the workgroup counts and the depth of the fold of the
    partials (fluxes.fold_depth() loads in flight, then one by one): one watch has exactly `depth` workgroups, one
    fewer, and one more than `depth` with a remainder."""
    chunk, depth = fluxes.chunk(), fluxes.fold_depth()
    counts = []
    for name in ("2d", "2d_r3", "mms44", "tet"):
        s, _, fl, _, _ = _recorded(name)
        counts += [fl.n_cells(t) for t in s.subdomain_list]
    assert any(n > 2 * chunk for n in counts) and any(n <= chunk for n in counts) and any(n % 64 for n in counts)
    assert any(n > chunk and n % chunk for n in counts)
    groups = [-(-n // chunk) for n in counts]
    print("cells", counts, "workgroups", groups, "depth", depth)
    assert any(g == depth for g in groups) and any(g < depth for g in groups)
    assert any(g > depth and g % depth for g in groups)
    # the counts of the set-ups themselves
    s, _, fl, _, _ = _recorded("2d_r3")
    assert [-(-fl.n_cells(t) // chunk) for t in s.subdomain_list] == [4096 // 256, 3840 // 256]
    s, _, fl, _, _ = _recorded("tet")
    assert [-(-fl.n_cells(t) // chunk) for t in s.subdomain_list] == [-(-13440 // 256), -(-2112 // 256)]


def _ion_count_problem(K):
    """The 2D r = 1 mesh with K ions, fields pushed as arrays (no forms needed): K = 4 uses slot 3 of the record."""
    from helpers import C_M, FARADAY, PSI, make_mesh
    from knpemi.device import DeviceProblem
    from knpemi.fem import Constant, extract_submesh
    spec = {2: [("K", 1.0, 1.96e-9), ("Na", 1.0, 1.33e-9)],
            4: [("K", 1.0, 1.96e-9), ("Cl", -1.0, 2.03e-9), ("Ca", 2.0, 0.71e-9), ("Na", 1.0, 1.33e-9)]}[K]
    mesh, ct, ft = make_mesh("2d", 1)
    subs = {}
    for t in (0, 1):
        sm, e2p, v2p, _, _ = extract_submesh(mesh, ct, t)
        subs[t] = dict(tag=t, name=f"sub{t}", mesh_sub=sm, sub_to_parent=e2p, sub_vertex_to_parent=v2p)
    g, g2p, _, _, _ = extract_submesh(mesh, ft, [1])
    subs[1].update(mesh_mem=g, mem_to_parent=g2p, membrane_tags=[1])
    pp = {'F': Constant(mesh, FARADAY), 'psi': Constant(mesh, PSI), 'C_M': Constant(mesh, C_M)}
    ions = [dict(name=n, z=z, D={0: Constant(None, D), 1: Constant(None, 1.1 * D)}) for n, z, D in spec]
    dp = DeviceProblem(mesh, ct, ft, subs, ions)
    return dp, subs, ions, pp


@pytest.mark.parametrize("K", [2, 4])
def test_ion_counts_other_than_three(hip_lib, K):
    dp, subs, ions, pp = _ion_count_problem(K)
    dp.set_params(pp, ions, 1e-4)
    rng = np.random.default_rng(5)
    phi, c = {}, {}
    for t, sd in subs.items():
        n, s = sd["mesh_sub"].x.shape[0], dp.sub_index[t]
        phi[t] = 1e-3 * rng.uniform(-1, 1, n)
        c[t] = [(10.0 + 30.0 * k) * (1.0 + 1e-2 * rng.uniform(-1, 1, n)) for k in range(K)]
        dp.push_array(L.F_PHI, s, 0, phi[t])
        for k in range(K - 1):
            dp.push_array(L.F_C_PREV, s, k, c[t][k])
        dp.push_array(L.F_C_ELIM, s, 0, c[t][K - 1])
    fl = IonFluxes(subs, ions, pp)
    for t in subs:
        fl.watch(t)
    fl._attach(dp, 4)
    L.check(dp.lib.knpemi_flux_record(dp.h, 1))
    fields, want = fl.compute_host(phi, c)
    worst = 0.0
    for t in subs:
        dev = fl.fields(t)
        assert set(dev) == {f"{i['name']}/{p}" for i in ions for p in fluxes.PARTS} | {"current", "current/diffusive", "current/drift"}
        for key in fields[t]:
            worst = max(worst, _rel(dev[key], fields[t][key]))
    buf, rows, over = _read(dp, fl.n_cols, 1)
    e_row = _row_err(fl, buf[0], want)
    print(K, "fields", worst, "row", e_row)
    assert rows == 1 and worst < TOL and e_row < TOL


def test_masks_and_bad_arguments(hip_lib):
    s = _build("2d")
    st = _stepper(s)
    dp, lib = st.dp, st.lib
    phi, c = _host_state(s)
    # one cell, one ion (the eliminated one), no current: the row has exactly those columns
    fl = IonFluxes(s.subdomain_list, s.ion_list, s.physical_parameters)
    fl.watch(1, ions=["Na"], current=False)
    assert fl.mask(1) == 0b100 and fl.n_cols == 5
    fl._attach(dp, 4)
    L.check(lib.knpemi_flux_record(dp.h, 1))
    buf, rows, over = _read(dp, 5, 1)
    fields, want = fl.compute_host(phi, c)
    assert rows == 1 and _row_err(fl, buf[0], want) < TOL
    dev = fl.fields(1)
    assert set(dev) == {"Na/diffusive", "Na/drift"}
    assert max(_rel(dev[k], fields[1][k]) for k in dev) < TOL
    nc = {t: fl.n_cells(t) for t in (0, 1)}
    out = np.empty(2 * nc[0])

    def fields_rc(sub, ion, part, n):
        rc = lib.knpemi_flux_fields(dp.h, sub, ion, part, L.dptr(out), n)
        return rc
    assert fields_rc(0, 2, 0, 2 * nc[0]) == L.EINVAL and b"not watched" in lib.knpemi_last_error()      # sub-domain
    assert fields_rc(1, 0, 0, 2 * nc[1]) == L.EINVAL and b"not watched" in lib.knpemi_last_error()      # ion
    assert fields_rc(1, -1, 0, 2 * nc[1]) == L.EINVAL and b"current" in lib.knpemi_last_error()
    assert fields_rc(1, 2, 2, 2 * nc[1]) == L.EINVAL
    assert fields_rc(1, 2, 0, nc[1]) == L.EINVAL
    assert fields_rc(5, 2, 0, 2 * nc[1]) == L.EINVAL
    with pytest.raises(ValueError):
        fl.fields(0)
    # a new series forgets the fields; a record without fields does not bring them back
    L.check(lib.knpemi_flux_reset(dp.h))
    L.check(lib.knpemi_flux_record(dp.h, 0))
    assert fields_rc(1, 2, 0, 2 * nc[1]) == L.EINVAL and b"no record with fields" in lib.knpemi_last_error()

    def set_rc(sub, mask, capacity=4):
        sub, mask = np.array(sub, np.int32), np.array(mask, np.int32)
        return lib.knpemi_flux_set(dp.h, len(sub), L.iptr(sub), L.iptr(mask), capacity)
    assert set_rc([2], [1]) == L.EINVAL and set_rc([-1], [1]) == L.EINVAL                 # bad sub-domain
    assert set_rc([0, 0], [1, 1]) == L.EINVAL
    assert set_rc([0], [0]) == L.EINVAL and b"empty" in lib.knpemi_last_error()
    assert set_rc([0], [0b1000]) == L.EINVAL and set_rc([0], [0x200]) == L.EINVAL        # bits at or above K = 3
    assert set_rc([0], [1], capacity=0) == L.EINVAL
    assert lib.knpemi_flux_set(dp.h, 1, None, None, 4) == L.EINVAL
    # the refused calls left the table alone
    L.check(lib.knpemi_flux_record(dp.h, 0))
    assert _read(dp, 5, 0)[1] == 2
    L.check(lib.knpemi_flux_clear(dp.h))
    assert lib.knpemi_flux_record(dp.h, 0) == L.EINVAL and lib.knpemi_flux_reset(dp.h) == L.EINVAL
    assert lib.knpemi_flux_read(dp.h, 0, None, None, None, 0) == L.EINVAL
    assert fields_rc(1, 2, 0, 2 * nc[1]) == L.EINVAL
    assert lib.knpemi_flux_record(None, 0) == L.EINVAL
    # parameters not yet set
    dp2, subs, ions, pp = _ion_count_problem(2)
    fl2 = IonFluxes(subs, ions, pp)
    fl2.watch(0)
    fl2._attach(dp2, 2)
    assert dp2.lib.knpemi_flux_record(dp2.h, 0) == L.EINVAL and b"knpemi_set_params" in lib.knpemi_last_error()


def test_series_buffer(hip_lib):
    s = _build("tet")
    st = _stepper(s)
    dp, lib = st.dp, st.lib
    fl = IonFluxes(s.subdomain_list, s.ion_list, s.physical_parameters)
    for tag in s.subdomain_list:
        fl.watch(tag)
    fl._attach(dp, 2)
    n = fl.n_cols
    _, want = fl.compute_host(*_host_state(s))
    L.check(lib.knpemi_flux_record(dp.h, 0))
    L.check(lib.knpemi_flux_record(dp.h, 1))
    first, rows, over = _read(dp, n, 2)
    assert rows == 2 and over == 0
    assert _row_err(fl, first[0], want) < TOL
    # the same state twice, once with the fields and once without: the same bits
    assert np.array_equal(first[0], first[1])
    # a third record finds the buffer full: nothing is written, the row is counted as dropped
    L.check(lib.knpemi_flux_record(dp.h, 0))
    after, rows, over = _read(dp, n, 3)
    assert rows == 2 and over == 1
    assert np.array_equal(after[:2], first) and np.isnan(after[2]).all()
    # read(reset=1) starts over
    _, rows, over = _read(dp, n, 0, reset=1)
    assert rows == 2 and over == 1
    assert _read(dp, n, 0)[1:] == (0, 0)
    L.check(lib.knpemi_flux_record(dp.h, 0))
    again, rows, over = _read(dp, n, 2)
    assert rows == 1 and over == 0 and np.array_equal(again[0], first[0]) and np.isnan(again[1]).all()


def _stepper_run(with_fluxes, steps=6, every=2, t0=0.25):
    with contextlib.redirect_stdout(io.StringIO()):
        s = Setup("2d", 1, g_syn=10.0)
    for t in s.subdomain_list:          # the solves start from c = c_prev
        for k in range(2):
            s.c[t][k].x.array[:] = s.c_prev[t][k].x._a
    st = _stepper(s, device_solves=(1e-9, 1e-10))
    st.add_membrane_model(s.mem_models[0]["ode"], s.stim_params["stimulus"], s.stim_params["stimulus_locator"])
    fl, ref = None, []
    if with_fluxes:
        fl = IonFluxes(s.subdomain_list, s.ion_list, s.physical_parameters)
        for tag in s.subdomain_list:
            fl.watch(tag)
        st.fluxes(fl, every=every, capacity=2, t0=t0, fields=True)
    with contextlib.redirect_stdout(io.StringIO()):
        for k in range(steps):
            st.step()
            if with_fluxes and (k + 1) % every == 0:
                st.download()
                ref.append(fl.compute_host(*_host_state(s)))
        st.download()
    phi, c = _host_state(s)
    state = [phi[t].copy() for t in phi] + [a.copy() for t in c for a in c[t]] + [s.phi_M_prev[1].x._a.copy()]
    return s, st, fl, ref, state


def test_stepper_records_behind_the_update(hip_lib):
    s, st, fl, ref, state = _stepper_run(True)
    ser = fl.series()
    dt = float(s.dt)
    assert ser["t"].shape == (3,) and np.allclose(ser["t"], 0.25 + np.array([2, 4, 6]) * dt, rtol=1e-14, atol=0)
    assert set(ser) == {"t"} | {k for k, _ in fl.columns()}
    worst = 0.0
    for i, (_, want) in enumerate(ref):
        for key, w in fl.columns():
            assert ser[key].shape == ((3, 2) if w > 1 else (3,))
            x = np.atleast_1d(np.asarray(want[key]))
            worst = max(worst, float(np.abs(np.atleast_1d(ser[key][i]) - x).max() / np.abs(x).max()))
    # the fields of the latest record are those of the state after step six
    fields = ref[-1][0]
    for tag in s.subdomain_list:
        dev = fl.fields(tag)
        worst = max(worst, max(_rel(dev[k], fields[tag][k]) for k in dev))
    print("stepper: largest relative error", worst)
    assert worst < TOL
    assert np.ptp(ser["0/K/max"]) > 0                      # the fields move
    # nothing attached: the same run ends in the same bits
    plain = _stepper_run(False)[4]
    assert len(plain) == len(state) and all(np.array_equal(a, b) for a, b in zip(state, plain))
    # reset() empties the series
    with contextlib.redirect_stdout(io.StringIO()):
        st.reset()
    assert fl.series()["t"].shape == (0,)
    with pytest.raises(L.KnpemiError):
        fl.fields(0)
    with contextlib.redirect_stdout(io.StringIO()):
        st.step()
        st.step()
    again = fl.series()
    assert again["t"].shape == (1,) and again["t"][0] == 0.25 + 2 * dt
    with pytest.raises(NotImplementedError, match="partitioned"):
        st.step(halo=object())
