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
