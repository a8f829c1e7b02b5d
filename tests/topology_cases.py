"""One problem builder for the membrane-topology tests (test_topology_host.py, test_topology_gpu.py), in the style of
exchange_cases.three_problem: test_gpu_parity._custom_problem for any {cell tag: [(facet tag, model)]}, with the same
parameters, seeded perturbation and per-sub-domain D and rho.  A facet tag whose model is None belongs to the membrane mesh
and is integrated by no model.  forms=False builds no device forms, so host tests run without a GPU."""
import contextlib
import io
import types

import numpy as np

import topology_meshes as tm


def problem(mesh_data, cell_specs, forms=True, dt=1e-4):
    from helpers import C_M, FARADAY, PSI, load_model
    from knpemi import (create_functions_emi, create_functions_knp, emi_system, knp_system, set_initial_conditions,
                        setup_membrane_model)
    from knpemi.fem import Constant, extract_submesh
    mesh, ct, ft = mesh_data
    tags = [0] + sorted(cell_specs)
    subs = {}
    for t in tags:
        sm, e2p, v2p, _, _ = extract_submesh(mesh, ct, t)
        subs[t] = dict(tag=t, name=f"sub{t}", mesh_sub=sm, sub_to_parent=e2p, sub_vertex_to_parent=v2p)
        if t > 0:
            mtags = [ftag for ftag, _ in cell_specs[t]]
            g, g2p, _, _, _ = extract_submesh(mesh, ft, mtags)
            subs[t].update(mesh_mem=g, mem_to_parent=g2p, membrane_tags=mtags,
                           ode_models={ftag: load_model(m) for ftag, m in cell_specs[t] if m is not None})
    rho = {'z': -1, **{t: Constant(subs[t]['mesh_sub'], 0.1 * t) for t in tags}}
    pp = {'dt': Constant(mesh, dt), 'F': Constant(mesh, FARADAY), 'psi': Constant(mesh, PSI),
          'C_phi': Constant(mesh, C_M / dt), 'C_M': Constant(mesh, C_M), 'rho': rho}
    init = {"Na": (100.7, 12.8), "K": (3.3, 124.2), "Cl": (104.0, 137.0)}
    Dv = {"Na": 1.33e-9, "K": 1.96e-9, "Cl": 2.03e-9}
    ions = [dict(name=n, z=z, D={t: Constant(None, Dv[n] * (1 + 0.1 * t)) for t in tags},
                 c_init={t: Constant(None, init[n][0 if t == 0 else 1]) for t in tags})
            for n, z in (("K", 1.0), ("Cl", -1.0), ("Na", 1.0))]
    with contextlib.redirect_stdout(io.StringIO()):
        phi, phi_M_prev = create_functions_emi(subs, degree=1)
        c, c_prev = create_functions_knp(subs, ions, degree=1)
        set_initial_conditions(ions, subs, c_prev)
        for t in tags[1:]:
            subs[t]['mem_models'] = setup_membrane_model({'stimulus': {}, 'stimulus_locator': None}, pp,
                                                         subs[t]['ode_models'], ft, phi_M_prev[t].function_space, ions)
    s = types.SimpleNamespace(mesh=mesh, ct=ct, ft=ft, subdomain_list=subs, ion_list=ions, physical_parameters=pp, dt=dt,
                              phi=phi, phi_M_prev=phi_M_prev, c=c, c_prev=c_prev, entity_maps=[], cell_specs=cell_specs)
    if forms:
        with contextlib.redirect_stdout(io.StringIO()):
            s.a_emi, s.p_emi, s.L_emi = emi_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c_prev, dt)
            s.a_knp, s.p_knp, s.L_knp = knp_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c, c_prev, dt)
    rng = np.random.default_rng(7)                          # seeded, physically sensible perturbation
    for t in tags:
        for f in c_prev[t] + [ions[-1][f'c_{t}']]:
            f.x.array[:] *= 1.0 + 1e-3 * rng.uniform(-1, 1, f.x.array.shape[0])
        phi[t].x.array[:] = 1e-3 * rng.uniform(-1, 1, phi[t].x.array.shape[0])
        if t > 0:
            phi_M_prev[t].x.array[:] = -0.07 + 1e-3 * rng.uniform(-1, 1, phi_M_prev[t].x.array.shape[0])
            for mm in subs[t]['mem_models']:
                for f in mm['I_ch_k'].values():
                    f.x.array[:] = 1e-2 * rng.uniform(-1, 1, f.x.array.shape[0])
    return s


def build(kind, case, jittered=False, forms=True):
    """The perturbed problem of tests/topology_meshes.build(kind, case, jittered) with the models of tm.SPECS."""
    return problem(tm.build(kind, case, jittered), tm.SPECS[case], forms=forms)


def oracle_objects(s, splitting=True):
    """(A_emi, P_emi, b_emi, A_knp, b_knp) of the oracle on the set-up `s`."""
    import adapters
    o, P, params, ions = adapters.oracle_problem(s)
    c_all, phi, phiM, mm = adapters.oracle_fields(s)
    return (o.assemble_emi(P, params, ions, c_all, phiM, mm, splitting_scheme=splitting)
            + o.assemble_knp(P, params, ions, c_all, phi, phiM, mm, s.dt, splitting_scheme=splitting))
