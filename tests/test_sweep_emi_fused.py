"""The membrane sweep and the potential system's matrix in one launch (knpemi_ode_step_emi, csrc/kernels_sweep_emi.hip).

The fused launch reorders nothing inside either half: a sweep workgroup runs the body of ode_step_kernel, a row workgroup
the body of emi_rows_v2.  So every comparison here is bit for bit -- fused (DeviceStepper(overlap=True), one model)
against the plain sequence (overlap=False) -- and the bound is zero: A_emi, P_emi, b_emi after the Robin launch, the ODE
tables, phi_M, I_ch, and the sweep's counters.  The meshes are the smallest on which the fused grid's indexing can go
wrong (test_meshes_cover_the_index_cases says which mesh covers what); the fallbacks must decline and change nothing."""
import contextlib
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- no GPU -----------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound(hip_lib):
    from knpemi import _lib as L
    header = open(os.path.join(ROOT, "include", "knpemi_hip.h")).read()
    ctype_of = {"knpemi_handle*": C.c_void_p, "int": C.c_int, "double": C.c_double, "const int32_t*": L.c_int_p,
                "int*": C.POINTER(C.c_int)}
    name = "knpemi_ode_step_emi"
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in knpemi_hip.h"
    params = [" ".join(p.split()[:-1]) for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 12 and params[-1] == "int*" and params[-2] == "int"
    assert hasattr(hip_lib, name), f"{name} is not exported"
    res, args = L.SIGNATURES[name]
    assert res is C.c_int and args == [ctype_of[p] for p in params], (name, params)
    fn = getattr(hip_lib, name)
    assert fn.restype is C.c_int and list(fn.argtypes) == args
    # the arguments of knpemi_ode_step, then the assembly's flags and the answer
    res0, args0 = L.SIGNATURES["knpemi_ode_step"]
    assert args[:len(args0)] == args0
    # a null handle is refused before anything touches a device
    fused = C.c_int(7)
    assert fn(None, 1, 0, 0.0, 1e-4, 1e-8, 1e-10, 0, None, 0, 0, C.byref(fused)) == L.EINVAL


# ---- GPU --------------------------------------------------------------------------------------------------------
def _box(n, lo, hi, size, cell="tetrahedron"):
    from knpemi.fem import CellType, create_box
    from knpemi.fem.idealized import _tag
    mesh = create_box(None, [np.zeros(3), np.array(size)], n, getattr(CellType, cell))
    ct, ft = _tag(mesh, [(lo, hi)], [1])
    return mesh, ct, ft


# name -> mesh of Setup("tet", 0, mesh_data=...) (None: the r = 0 box of the idealized geometry, four axons)
MESHES = {
    "tet_r0": None,
    # one hexahedron of cell, split into six tetrahedra: 8 membrane dofs
    "one_cell": ((4, 3, 3), [1e-6, 1e-6, 1e-6], [2e-6, 2e-6, 2e-6], [4e-6, 3e-6, 3e-6]),
    # a bar of ten: 44 membrane dofs
    "bar": ((12, 3, 3), [1e-6, 1e-6, 1e-6], [11e-6, 2e-6, 2e-6], [12e-6, 3e-6, 3e-6]),
}


def _setup(mesh, model_source=False):
    from helpers import Setup
    with contextlib.redirect_stdout(io.StringIO()):
        data = None if MESHES[mesh] is None else _box(*MESHES[mesh])
        s = Setup("tet", 0, g_syn=10.0, mesh_data=data, build_forms=False)
        if model_source:      # the same model, bound from HIP source (test_rtc_models.py)
            from test_rtc_models import HH_SI_SOURCE
            ode = s.mem_models[0]['ode']
            shipped = ode.ode

            class _Plug:
                __name__ = "mm_hh_user"
                RHS_HIP = HH_SI_SOURCE
                init_state_values = staticmethod(shipped.init_state_values)
                init_parameter_values = staticmethod(shipped.init_parameter_values)
                state_indices = staticmethod(shipped.state_indices)
                parameter_indices = staticmethod(shipped.parameter_indices)
            ode.ode = _Plug
        s.build_forms()
    return s


def _sensible_fields(s):
    """Perturbed fields, "solutions" close to them (no solves between the steps: c and phi are held, as in
    test_gpu_parity.test_device_stepper_matches_dropin_path)."""
    s.perturb()
    for t in s.subdomain_list:
        for k in range(2):
            s.c[t][k].x.array[:] = s.c_prev[t][k].x._a * 1.001
    s.phi[1].x.array[:] += -0.0744


def _layout(dp):
    from knpemi import _lib as L
    out = (C.c_int * 9)()
    L.check(dp.lib.knpemi_debug_layout(dp.h, out, 9))
    return list(out)


def _run(s, overlap, splitting=True, want_p=1, steps=3, **kw):
    """`steps` steps of the device stepper; everything the fused launch and its neighbours write."""
    from knpemi import _lib as L
    from knpemi.stepper import DeviceStepper
    for f in (s.a_emi, s.a_knp):
        f.shared['splitting_scheme'] = splitting
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev,
                       overlap=overlap, **kw)
    if not want_p:
        st.flags_emi &= ~L.WANT_P
    ode = s.mem_models[0]['ode']
    st.add_membrane_model(ode, s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
    fused = []
    for _ in range(steps):
        st.step()
        fused.append(st.last_fused)
    dp = st.dp
    out = {"A_emi": dp.csr(L.A_EMI).data.copy(), "b_emi": dp.rhs(L.B_EMI).copy()}
    if want_p:
        out["P_emi"] = dp.csr(L.P_EMI).data.copy()
    nr, ns, nf = C.c_int64(), C.c_int64(), C.c_int32()
    L.check(dp.lib.knpemi_ode_stats(dp.h, ode._sub, ode._model, C.byref(nr), C.byref(ns), C.byref(nf)))
    assert nf.value == 0
    st.download()
    out.update(states=ode.states.copy(), parameters=ode.parameters.copy(), phi_M=s.phi_M_prev[1].x._a.copy())
    for name, f in s.mem_models[0]['I_ch_k'].items():
        out["I_ch_" + name] = f.x._a.copy()
    info = dict(fused=fused, nfe=nr.value, nst=ns.value, nq=ode.nodes, layout=_layout(dp))
    return out, info


def _assert_same_bits(got, want):
    assert got.keys() == want.keys()
    for k in want:
        assert got[k].shape == want[k].shape and np.all(np.isfinite(want[k])), k
        assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), k


_PLAIN = {}


def _plain(mesh, splitting, want_p, general):
    """The plain sequence's results, computed once per case and left unchanged."""
    key = (mesh, splitting, want_p, general)
    if key not in _PLAIN:
        s = _setup(mesh)
        _sensible_fields(s)
        _PLAIN[key] = _run(s, overlap=False, splitting=splitting, want_p=want_p)
        for a in _PLAIN[key][0].values():
            a.setflags(write=False)
    return _PLAIN[key]


@pytest.mark.gpu
@pytest.mark.parametrize("general", [False, True], ids=["lattice", "general"])
@pytest.mark.parametrize("splitting,want_p", [(True, 1), (False, 1), (True, 0), (False, 0)])
def test_fused_launch_matches_the_plain_sequence_bit_for_bit(hip_lib, monkeypatch, splitting, want_p, general):
    """tet_r0, HH, 3 steps: both splitting modes, with and without the preconditioner matrix, lattice and general
    tetrahedra (KNPEMI_TET_NOT_UNIFORM=1 before knpemi_create)."""
    if general:
        monkeypatch.setenv("KNPEMI_TET_NOT_UNIFORM", "1")
    want, ref = _plain("tet_r0", splitting, want_p, general)
    s = _setup("tet_r0")
    _sensible_fields(s)
    got, info = _run(s, overlap=True, splitting=splitting, want_p=want_p)
    assert info["fused"] == [1, 1, 1] and ref["fused"] == [None, None, None]
    geometry = C.c_int(-1)
    from knpemi import _lib as L
    L.check(hip_lib.knpemi_debug_geometry(s.a_emi.dp.h, C.byref(geometry)))
    assert bool(geometry.value & 1) == (not general)
    _assert_same_bits(got, want)
    assert (info["nfe"], info["nst"]) == (ref["nfe"], ref["nst"]) and info["nfe"] > 2 * 3 * info["nq"]
    # the results are not trivially equal: the steps moved the state, the matrix is there
    assert np.abs(got["A_emi"]).max() > 0 and np.ptp(got["phi_M"]) > 0 and np.abs(got["b_emi"]).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("mesh", ["one_cell", "bar"])
def test_fused_launch_on_the_smallest_meshes(hip_lib, mesh):
    want, ref = _plain(mesh, True, 1, False)
    s = _setup(mesh)
    _sensible_fields(s)
    got, info = _run(s, overlap=True)
    assert info["fused"] == [1, 1, 1]
    _assert_same_bits(got, want)
    assert (info["nfe"], info["nst"]) == (ref["nfe"], ref["nst"])


@pytest.mark.gpu
def test_meshes_cover_the_index_cases(hip_lib):
    """What the three meshes are there for, read from the problems themselves: HH runs 16 dofs per wave, a sweep
    workgroup per wave, the fused grid pads the sweep to a multiple of 8 workgroups and puts the row blocks behind."""
    nq, nblocks = {}, {}
    for mesh in MESHES:
        _, ref = _plain(mesh, True, 1, False)
        nq[mesh], nblocks[mesh] = ref["nq"], ref["layout"][8]
    sweep = {m: -(-n // 16) for m, n in nq.items()}
    assert any(n % 16 for n in nq.values())                       # a partial last wave
    assert nq["tet_r0"] % 16 and sweep["tet_r0"] % 8 and sweep["tet_r0"] > 8    # ... and padding workgroups, several rounds of 8
    assert nq["one_cell"] < 16 and sweep["one_cell"] == 1         # one sweep workgroup, seven of padding
    assert 1 < sweep["bar"] < 8
    assert any(n % 8 for n in nblocks.values()) and min(nblocks.values()) < 8 < max(nblocks.values())
    assert nblocks["one_cell"] % 8 and nblocks["bar"] % 8


def _declines(s, **kw):
    got, info = _run(s, overlap=True, **kw)
    assert info["fused"][0] == 0, info["fused"]                   # asked once, declined; the stream schedule takes over
    assert all(f is None for f in info["fused"][1:])
    return got, info


@pytest.mark.gpu
def test_hexahedra_take_the_plain_path(hip_lib):
    from helpers import Setup
    res = []
    for overlap in (False, True):
        with contextlib.redirect_stdout(io.StringIO()):
            s = Setup("hex", 0, g_syn=10.0)
        _sensible_fields(s)
        res.append(_run(s, overlap=overlap) if not overlap else _declines(s))
    _assert_same_bits(res[1][0], res[0][0])
    assert (res[1][1]["nfe"], res[1][1]["nst"]) == (res[0][1]["nfe"], res[0][1]["nst"])


@pytest.mark.gpu
def test_a_model_bound_from_source_takes_the_plain_path(hip_lib):
    res = []
    for overlap in (False, True):
        s = _setup("bar", model_source=True)
        _sensible_fields(s)
        res.append(_run(s, overlap=overlap) if not overlap else _declines(s))
    _assert_same_bits(res[1][0], res[0][0])
    assert (res[1][1]["nfe"], res[1][1]["nst"]) == (res[0][1]["nfe"], res[0][1]["nst"])


@pytest.mark.gpu
def test_a_fixed_step_integrator_takes_the_plain_path(hip_lib):
    res = []
    for overlap in (False, True):
        s = _setup("bar")
        _sensible_fields(s)
        kw = dict(ode_method="rk4", ode_substeps=25)
        res.append(_run(s, overlap=overlap, **kw) if not overlap else _declines(s, **kw))
    _assert_same_bits(res[1][0], res[0][0])


@pytest.mark.gpu
def test_phase_stamps_take_the_plain_path(hip_lib, monkeypatch):
    """KNPEMI_ODE_STAMPS asks for the diagnostic build of the sweep, which the fused kernel does not have."""
    want, ref = _plain("bar", True, 1, False)
    monkeypatch.setenv("KNPEMI_ODE_STAMPS", "1")
    s = _setup("bar")
    _sensible_fields(s)
    got, info = _declines(s)
    _assert_same_bits(got, want)
    assert (info["nfe"], info["nst"]) == (ref["nfe"], ref["nst"])


@pytest.mark.gpu
def test_the_environment_switch_disables_the_fused_launch(hip_lib, monkeypatch):
    want, _ = _plain("bar", True, 1, False)
    monkeypatch.setenv("KNPEMI_FUSED_SWEEP", "0")
    s = _setup("bar")
    _sensible_fields(s)
    got, _ = _declines(s)
    _assert_same_bits(got, want)


@pytest.mark.gpu
def test_two_models_on_one_handle_take_the_plain_path(hip_lib):
    """The stepper does not ask with two models; the entry point itself declines and runs the two launches."""
    from knpemi import _lib as L
    from knpemi.fem import make_mesh_3D
    from knpemi.stepper import DeviceStepper
    from test_gpu_parity import _custom_problem
    res = []
    for entry in (False, True):
        with contextlib.redirect_stdout(io.StringIO()):
            mesh, ct, ft = make_mesh_3D(0, "tetrahedron", axon_tags=(1, 1, 2, 2))
            s = _custom_problem(mesh, ct, ft, {1: [(1, "hh_si")], 2: [(2, "glial")]})       # perturbed already
        for t in s.subdomain_list:     # "solutions" the end-of-step update can take: c close to c_prev, the cells near rest
            for k in range(2):
                s.c[t][k].x.array[:] = s.c_prev[t][k].x._a * 1.001
            if t > 0:
                s.phi[t].x.array[:] += -0.0744
        st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev,
                           overlap=False)
        models = [s.subdomain_list[t]['mem_models'][0]['ode'] for t in (1, 2)]
        for m in models:
            st.add_membrane_model(m)
        st.step()                      # everything is on the device; st.last_fused is None: two models, not asked
        assert st.last_fused is None
        dp, lib, m = st.dp, st.lib, models[0]
        flags = L.ODE_SET_TRACES | L.ODE_SET_V
        args = (dp.h, m._sub, m._model, float(m.time), st.dt, m.rtol, m.atol, flags, L.iptr(m._ion_param), int(m.V_index))
        if entry:
            fused = C.c_int(-1)
            L.check(lib.knpemi_ode_step_emi(*args, st.flags_emi, C.byref(fused)))
            assert fused.value == 0
        else:
            L.check(lib.knpemi_ode_step(*args))
            L.check(lib.knpemi_assemble_emi(dp.h, st.flags_emi | L.SKIP_MEMBRANE_RHS))
        L.check(lib.knpemi_assemble_emi_membrane_rhs(dp.h, st.flags_emi))
        out = {"A_emi": dp.csr(L.A_EMI).data.copy(), "P_emi": dp.csr(L.P_EMI).data.copy(), "b_emi": dp.rhs(L.B_EMI).copy()}
        st.download()
        out.update(states=m.states.copy(), parameters=m.parameters.copy(), phi_M=s.phi_M_prev[1].x._a.copy())
        res.append(out)
    _assert_same_bits(res[1], res[0])
