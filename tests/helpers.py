"""Test helpers: the shared driver set-up plus error norms."""
import numpy as np

import adapters
from setup_problem import (C_M, DT, FARADAY, PSI, load_model, make_mesh)  # noqa: F401
from setup_problem import Setup as _Setup


class Setup(_Setup):
    """Driver set-up plus the oracle view of the same problem."""

    def oracle(self):
        return adapters.oracle_problem(self)

    def oracle_fields(self):
        return adapters.oracle_fields(self)


def rel_err(a, b):
    a = np.asarray(a)
    b = np.asarray(b)
    scale = np.abs(b).max()
    return np.abs(a - b).max() / (scale if scale > 0 else 1.0)


def csr_rel_err(A, B):
    """max |A - B| relative to max |B| (patterns may differ by explicit zeros)."""
    D = (A - B).tocoo()
    scale = np.abs(B.data).max() if B.nnz else 1.0
    return (np.abs(D.data).max() if D.nnz else 0.0) / scale


TOL = 1e-10   # stated fp64 tolerance for assembled operators


def assemble_both(s, splitting=True):
    """Both systems through the knpemi API and through the oracle: relative errors of the five assembled objects and the
    objects themselves (A_emi, P_emi, b_emi, A_knp, b_knp)."""
    from knpemi.pdeSolver import create_solver_emi, create_solver_knp
    o, P, params, ions = s.oracle()
    c_all, phi, phiM, mm = s.oracle_fields()
    for f in (s.a_emi, s.a_knp):
        f.shared['splitting_scheme'] = splitting
    emi = create_solver_emi(s.a_emi, s.L_emi, s.phi, s.entity_maps, s.subdomain_list, None,
                            p=s.p_emi, direct=False)
    knp = create_solver_knp(s.a_knp, s.L_knp, s.c, s.entity_maps, s.subdomain_list, None, p=s.p_knp)
    A, b = emi.assemble()
    Ak, bk = knp.assemble()
    Ao, Po, bo = o.assemble_emi(P, params, ions, c_all, phiM, mm, splitting_scheme=splitting)
    Ako, bko = o.assemble_knp(P, params, ions, c_all, phi, phiM, mm, s.dt, splitting_scheme=splitting)
    return dict(A_emi=csr_rel_err(A, Ao), P_emi=csr_rel_err(emi.P, Po), b_emi=rel_err(b, bo),
                A_knp=csr_rel_err(Ak, Ako), b_knp=rel_err(bk, bko)), (A, emi.P, b, Ak, bk)


ION_SPECS = {        # name, valence, c_init outside / inside, D; the last ion is the eliminated one
    2: [("K", 1.0, 3.3, 124.2, 1.96e-9), ("Na", 1.0, 100.7, 12.8, 1.33e-9)],
    3: [("K", 1.0, 3.3, 124.2, 1.96e-9), ("Cl", -1.0, 104.0, 137.0, 2.03e-9), ("Na", 1.0, 100.7, 12.8, 1.33e-9)],
    4: [("K", 1.0, 3.3, 124.2, 1.96e-9), ("Cl", -1.0, 104.0, 137.0, 2.03e-9), ("Ca", 2.0, 1.2, 1e-1, 0.71e-9),
        ("Na", 1.0, 100.7, 12.8, 1.33e-9)]}


def ion_count_problem(mesh_data, n_ions, splitting=True, dt=1e-4):
    """The two-sub-domain problem of the parity tests with `n_ions` species (ION_SPECS) on `mesh_data` = (mesh, ct, ft):
    perturbed fields (seed 11), both systems' forms, and the oracle's view of the same problem.  Returns a namespace with
    the driver's names (mesh, subdomain_list, ion_list, phi, c, c_prev, a_emi, p_emi, L_emi, a_knp, ...) plus `rho` and
    `oracle` = (o, P, params, ions) and `oracle_fields` = (c_all, phi, phiM, mm)."""
    import contextlib
    import io
    import types
    from knpemi import create_functions_emi, create_functions_knp, emi_system, knp_system, set_initial_conditions
    from knpemi.fem import Constant, Function, extract_submesh
    spec = ION_SPECS[n_ions]
    mesh, ct, ft = mesh_data

    class Dummy:        # the forms only read the facet tag of a membrane model (emiWeakForm.py:162)
        tag = 1
    subs = {}
    for t in (0, 1):
        sm, e2p, v2p, _, _ = extract_submesh(mesh, ct, t)
        subs[t] = dict(tag=t, name=f"sub{t}", mesh_sub=sm, sub_to_parent=e2p, sub_vertex_to_parent=v2p)
    g, g2p, _, _, _ = extract_submesh(mesh, ft, [1])
    subs[1].update(mesh_mem=g, mem_to_parent=g2p, membrane_tags=[1])
    rho = {'z': -1, 0: Constant(subs[0]['mesh_sub'], 0.05), 1: Constant(subs[1]['mesh_sub'], 0.2)}
    pp = {'dt': Constant(mesh, dt), 'F': Constant(mesh, FARADAY), 'psi': Constant(mesh, PSI),
          'C_phi': Constant(mesh, C_M / dt), 'C_M': Constant(mesh, C_M), 'rho': rho}
    ions = [dict(name=n, z=z, D={0: Constant(None, D), 1: Constant(None, 1.1 * D)},
                 c_init={0: Constant(None, ce), 1: Constant(None, ci)}) for n, z, ce, ci, D in spec]
    with contextlib.redirect_stdout(io.StringIO()):
        phi, phi_M_prev = create_functions_emi(subs, degree=1)
        c, c_prev = create_functions_knp(subs, ions, degree=1)
        set_initial_conditions(ions, subs, c_prev)
    Q = phi_M_prev[1].function_space
    subs[1]['mem_models'] = [{'ode': Dummy(), 'I_ch_k': {ion['name']: Function(Q, name=f"I_{ion['name']}") for ion in ions}}]
    rng = np.random.default_rng(11)
    for t in (0, 1):
        ions[-1][f'c_{t}'].x.array[:] = spec[-1][2 + t]
        for f in c_prev[t] + [ions[-1][f'c_{t}']]:
            f.x.array[:] *= 1.0 + 1e-2 * rng.uniform(-1, 1, f.x.array.shape[0])
        phi[t].x.array[:] = 1e-3 * rng.uniform(-1, 1, phi[t].x.array.shape[0])
        for f in c[t]:
            f.x.array[:] = rng.uniform(1.0, 100.0, f.x.array.shape[0])
    phi_M_prev[1].x.array[:] = -0.07 + 1e-3 * rng.uniform(-1, 1, phi_M_prev[1].x.array.shape[0])
    for f in subs[1]['mem_models'][0]['I_ch_k'].values():
        f.x.array[:] = 1e-2 * rng.uniform(-1, 1, f.x.array.shape[0])
    a_emi, p_emi, L_emi = emi_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c_prev, dt,
                                     splitting_scheme=splitting)
    a_knp, p_knp, L_knp = knp_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c, c_prev, dt,
                                     splitting_scheme=splitting)
    s = types.SimpleNamespace(mesh=mesh, ct=ct, ft=ft, subdomain_list=subs, ion_list=ions, physical_parameters=pp, dt=dt,
                              phi=phi, phi_M_prev=phi_M_prev, c=c, c_prev=c_prev)
    s.oracle = adapters.oracle_problem(s, {0: [], 1: [1]})
    s.oracle_fields = adapters.oracle_fields(s)
    s.__dict__.update(rho=rho, a_emi=a_emi, p_emi=p_emi, L_emi=L_emi, a_knp=a_knp, p_knp=p_knp, L_knp=L_knp)
    return s


def check_facet_integrals_of_the_write_back_launch(s):
    """KNPEMI_OPT_FOLD_MEMBRANE on the perturbed set-up `s`: b_knp with the membrane-facet integrals formed by the launch
    that writes a potential back equals, bit for bit, the one assembled with the facet kernel as a launch of its own, and
    matches the oracle; the stored integrals are dropped as soon as one of their inputs changes (phi_M here)."""
    import ctypes as C
    from knpemi import _lib as L
    from knpemi.pdeSolver import create_solver_emi, create_solver_knp
    o, P, params, ions = s.oracle()
    emi = create_solver_emi(s.a_emi, s.L_emi, s.phi, s.entity_maps, s.subdomain_list, None, p=s.p_emi, direct=False)
    knp = create_solver_knp(s.a_knp, s.L_knp, s.c, s.entity_maps, s.subdomain_list, None, p=s.p_knp)
    emi.assemble()
    knp.assemble()                              # pushes every field; facet kernel as its own launch
    dp = knp.dp
    ref = dp.rhs(L.B_KNP).copy()
    phi_all = np.concatenate([s.phi[t].x._a for t in s.subdomain_list])
    hip = C.CDLL("libamdhip64.so")
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), C.c_size_t(phi_all.nbytes)) == 0
    assert hip.hipMemcpy(dev, phi_all.ctypes.data_as(C.c_void_p), C.c_size_t(phi_all.nbytes), 1) == 0
    out = {}
    for fold in (1, 0):
        L.check(dp.lib.knpemi_set_option(dp.h, L.OPT_FOLD_MEMBRANE, fold))
        dp.set_rhs(L.B_KNP, np.full(len(ref), np.nan))
        L.check(dp.lib.knpemi_set_solution(dp.h, L.B_EMI, dev, 1))         # paste on the device
        L.check(dp.lib.knpemi_assemble_knp(dp.h, 0))
        out[fold] = dp.rhs(L.B_KNP).copy()
    assert np.array_equal(out[1], out[0]) and np.array_equal(out[1], ref)
    # an input changes after the potential was written back: the stored integrals must not be used
    L.check(dp.lib.knpemi_set_option(dp.h, L.OPT_FOLD_MEMBRANE, 1))
    L.check(dp.lib.knpemi_set_solution(dp.h, L.B_EMI, dev, 1))
    s.phi_M_prev[1].x.array[:] = s.phi_M_prev[1].x._a + 1e-3
    _, fresh = knp.assemble()                   # pushes the new phi_M (knpemi_set_field), then assembles
    c_all, phi, phiM, mm = s.oracle_fields()
    _, bko = o.assemble_knp(P, params, ions, c_all, phi, phiM, mm, s.dt)
    assert rel_err(fresh, bko) < TOL and not np.array_equal(fresh, ref)
    hip.hipFree(dev)
