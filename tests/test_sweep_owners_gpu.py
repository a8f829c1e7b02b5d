"""The two owners of a membrane ODE sweep -- the DG handle (knpemi_dg_ode_*: the membrane nodes of the broken space) and
the handle of knpemi_ode_create (knpemi_ode_*: membrane models on their own) -- run one sweep: the same tables give the
same bits and the same counters, and the binds of both refuse the same mistakes under their own names.

Mesh: dg_cases.make_mesh(2, 5, membrane=True): 50 triangles, 4 membrane facets, 8 membrane nodes.  M = 4, the smallest
mesh with membrane facets (tests/test_dg_vec_index_gpu.py), has 16 nodes, exactly one full wave of the HH sweep (4 lanes
per dof, 16 dofs per wave); with 8 the last (only) wave of either model is partial."""
import ctypes as C

import numpy as np
import pytest

import dg_cases
import knpemi_oracle as ko
from knpemi import _lib as L

pytestmark = pytest.mark.gpu

M_MESH = 5
NAMES = ["Na", "K", "Cl"]
# oracle name -> (library id, Cm, psi, {ion: (ECS, intracellular)}): SI units for hh_si, mV / ms / mM for the glial model
CASES = {
    "hh_si": (L.MODEL_HH_SI, 0.02, 96485.0 / (8.314 * 300.0), dict(Na=(100.0, 12.0), K=(4.0, 125.0), Cl=(104.0, 137.0))),
    "glial": (L.MODEL_GLIAL, 1.0, 1.0 / 26.64, dict(Na=(144.6, 15.5), K=(3.09, 99.3), Cl=(133.7, 5.2))),
}


def _dg_problem():
    from knpemi.dg import DGProblem
    mesh, ct, mem_facets, mem_tags = dg_cases.make_mesh(2, M_MESH, True)
    ft = np.zeros(len(mesh.facets), np.int32)                       # dense facet tags from the membrane's facet list
    key = {tuple(sorted(f)): i for i, f in enumerate(mesh.facets.tolist())}
    for f, t in zip(mem_facets.tolist(), mem_tags):
        ft[key[tuple(sorted(f))]] = t
    dp = DGProblem(mesh, ct, ft, [0, 1], [1])
    assert dp.nmf == len(mem_facets) > 0
    return dp


def _tables(name, nq):
    """State and parameter tables of model `name`, every dof a little different from every other, and the columns the DG
    bind wants: [ECS trace, intracellular trace, channel current] per ion, and V."""
    _, cm, psi, conc = CASES[name]
    m = ko.MODELS[name]
    ix = m["pidx"]
    prow = np.array(m["params"], float)
    prow[ix["Cm"]], prow[ix["psi"]] = cm, psi
    prow[ix["z_Na"]], prow[ix["z_K"]], prow[ix["z_Cl"]] = 1.0, 1.0, -1.0
    for n in NAMES:
        prow[ix[f"{n}_e"]], prow[ix[f"{n}_i"]] = conc[n]
    q = np.arange(nq, dtype=float)[:, None]
    st = np.array(m["states"], float)[None, :] * (1.0 + 1e-3 * np.cos(q + np.arange(m["n_states"])[None, :]))
    pr = np.tile(prow, (nq, 1))
    for j, n in enumerate(NAMES):
        pr[:, ix[f"{n}_e"]] *= 1.0 + 0.01 * np.sin(q[:, 0] + j)
        pr[:, ix[f"{n}_i"]] *= 1.0 + 0.01 * np.cos(2.0 * q[:, 0] + j)
    assert len({r.tobytes() for r in st}) == nq and len({r.tobytes() for r in pr}) == nq
    ion_param = np.array(sum(([ix[f"{n}_e"], ix[f"{n}_i"], ix[f"I_ch_{n}"]] for n in NAMES), []), np.int32)
    return np.ascontiguousarray(st), np.ascontiguousarray(pr), ion_param, m["V"]


@pytest.mark.parametrize("name", list(CASES))
def test_dg_sweep_and_standalone_sweep_are_one_sweep(hip_lib, name):
    from knpemi.odeSolver import OdeProblem
    dp = _dg_problem()
    nq = dp.nmf * dp.nf
    assert nq % 16 != 0                                             # the last wave is partial
    model_id = CASES[name][0]
    st0, pr0, ion_param, v = _tables(name, nq)
    ns, npar = st0.shape[1], pr0.shape[1]
    dp.ode_bind(model_id, st0, pr0, ion_param, v)
    op = OdeProblem([nq])
    L.check(hip_lib.knpemi_ode_bind(op.h, 1, 0, model_id, ns, npar))
    L.check(hip_lib.knpemi_ode_set_tables(op.h, 1, 0, L.dptr(st0), L.dptr(pr0)))
    t, dt = 0.0, 1e-4
    for step in range(3):
        dp.ode_step(t, dt, set_v=False, set_traces=False)           # no exchange with the PDE fields on either side
        L.check(hip_lib.knpemi_ode_step(op.h, 1, 0, t, dt, 1e-8, 1e-10, 0, L.iptr(ion_param), v))
        t += dt
        st_d, pr_d = dp.ode_tables()
        st_s, pr_s = np.zeros((nq, ns)), np.zeros((nq, npar))
        L.check(hip_lib.knpemi_ode_get_tables(op.h, 1, 0, L.dptr(st_s), L.dptr(pr_s)))
        assert np.array_equal(st_d, st_s) and np.array_equal(pr_d, pr_s), step
        assert np.isfinite(st_d).all() and not np.array_equal(st_d, st0)
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        rc_d = hip_lib.knpemi_dg_ode_stats(dp.h, C.byref(a), C.byref(b), C.byref(c))
        e, f, g = C.c_int64(), C.c_int64(), C.c_int32()
        rc_s = hip_lib.knpemi_ode_stats(op.h, 1, 0, C.byref(e), C.byref(f), C.byref(g))
        print(name, "step", step, "dg", (rc_d, a.value, b.value, c.value), "standalone", (rc_s, e.value, f.value, g.value))
        assert (rc_d, a.value, b.value, c.value) == (rc_s, e.value, f.value, g.value)
        assert rc_d == L.OK and a.value >= b.value >= nq and c.value == 0


def _refused(hip_lib, name, rc):
    assert rc == L.EINVAL, (name, rc)
    msg = hip_lib.knpemi_last_error()
    assert msg.startswith(name.encode() + b":"), (name, msg)


def test_dg_ode_bind_and_siblings_refuse_bad_arguments(hip_lib):
    dp = _dg_problem()
    nq = dp.nmf * dp.nf
    st, pr, ip, v = _tables("hh_si", nq)
    ns, npar = st.shape[1], pr.shape[1]
    out_s, out_p, cnt = np.zeros((nq, ns)), np.zeros((nq, npar)), [C.c_int64() for _ in range(3)]
    # before a bind
    _refused(hip_lib, "knpemi_dg_ode_step", hip_lib.knpemi_dg_ode_step(dp.h, 0.0, 1e-4, 1e-8, 1e-10, 0))
    _refused(hip_lib, "knpemi_dg_ode_get_tables", hip_lib.knpemi_dg_ode_get_tables(dp.h, L.dptr(out_s), L.dptr(out_p)))
    _refused(hip_lib, "knpemi_dg_ode_stats", hip_lib.knpemi_dg_ode_stats(dp.h, *[C.byref(x) for x in cnt]))

    def bind(model_id=L.MODEL_HH_SI, n_states=ns, n_params=npar, ion_param=ip, v_index=v):
        return hip_lib.knpemi_dg_ode_bind(dp.h, model_id, n_states, n_params, L.dptr(st), L.dptr(pr), L.iptr(ion_param), v_index)

    for bad in (-1, 3):
        _refused(hip_lib, "knpemi_dg_ode_bind", bind(model_id=bad))                 # unknown model id
    _refused(hip_lib, "knpemi_dg_ode_bind", bind(n_states=ns + 1))                  # counts that are not the model's
    _refused(hip_lib, "knpemi_dg_ode_bind", bind(n_params=npar + 1))
    _refused(hip_lib, "knpemi_dg_ode_bind", bind(model_id=L.MODEL_GLIAL))           # (hh_si's counts under the glial id)
    for bad in (-1, ns):
        _refused(hip_lib, "knpemi_dg_ode_bind", bind(v_index=bad))
    for pos in (0, len(ip) - 1):
        for bad in (-1, npar):
            wrong = ip.copy()
            wrong[pos] = bad
            _refused(hip_lib, "knpemi_dg_ode_bind", bind(ion_param=wrong))
    # none of the refused binds bound anything
    _refused(hip_lib, "knpemi_dg_ode_step", hip_lib.knpemi_dg_ode_step(dp.h, 0.0, 1e-4, 1e-8, 1e-10, 0))
    assert bind() == L.OK
    _refused(hip_lib, "knpemi_dg_ode_bind", bind())                                 # second bind
    L.check(hip_lib.knpemi_dg_ode_get_tables(dp.h, L.dptr(out_s), L.dptr(out_p)))
    assert np.array_equal(out_s, st) and np.array_equal(out_p, pr)


def test_ode_bind_refuses_wrong_counts_and_a_second_bind(hip_lib):
    from knpemi.odeSolver import OdeProblem
    ids = {"hh_si": L.MODEL_HH_SI, "hh_mv": L.MODEL_HH_MV, "glial": L.MODEL_GLIAL}
    op = OdeProblem([3] * len(ids))
    for i, (name, model_id) in enumerate(ids.items()):
        ns, npar = ko.MODELS[name]["n_states"], ko.MODELS[name]["n_params"]
        for wrong in ((ns + 1, npar), (ns, npar + 1), (ns, npar - 1), (npar, ns)):
            _refused(hip_lib, "knpemi_ode_bind", hip_lib.knpemi_ode_bind(op.h, 1 + i, 0, model_id, *wrong))
        assert hip_lib.knpemi_ode_bind(op.h, 1 + i, 0, model_id, ns, npar) == L.OK
        _refused(hip_lib, "knpemi_ode_bind", hip_lib.knpemi_ode_bind(op.h, 1 + i, 0, model_id, ns, npar))
    _refused(hip_lib, "knpemi_ode_bind", hip_lib.knpemi_ode_bind(op.h, 1, 0, 3, 4, 22))   # unknown model id
