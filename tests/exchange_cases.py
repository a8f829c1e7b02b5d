"""Set-ups shared by the membrane-exchange tests (test_exchange_host.py, test_exchange_gpu.py): perturbed problems on
every facet kind, and the host views of their fields that MembraneExchange.compute_host takes."""
import contextlib
import io

import numpy as np

import unstructured_meshes as um
from helpers import Setup
from knpemi import MembraneExchange

# name -> what it adds: "2d" intervals (NF = 2), "tet" triangles on the lattice records (NF = 3), "hex" planar bilinear
# quadrilaterals (NF = 4), "three" two cells with a model each, "jittered" general triangles, "jittered_hex" non-planar
# quadrilaterals
SETUPS = ("2d", "tet", "hex", "three", "jittered", "jittered_hex")


def jittered_hex_box():
    """The hexahedral r = 0 box with every interior vertex moved by up to 10 % of the grid spacing: the membrane facets
    are no longer planar, the surface Jacobian varies over a facet."""
    from knpemi.fem import Mesh, make_mesh_3D, meshtags
    mesh, ct, ft = make_mesh_3D(0, "hexahedron")
    h = np.abs(np.diag(np.asarray(mesh.uniform_cell).reshape(3, 3)))
    lo, hi = mesh.x.min(axis=0), mesh.x.max(axis=0)
    inner = np.all((mesh.x > lo + 0.5 * h) & (mesh.x < hi - 0.5 * h), axis=1)
    rng = np.random.default_rng(3)
    x = mesh.x.copy()
    x[inner] += 0.1 * h * (2.0 * rng.random((int(inner.sum()), 3)) - 1.0)
    m2 = Mesh(x, mesh.cells.copy(), mesh.cell_type)
    return m2, meshtags(m2, m2.tdim, ct.indices, ct.values), meshtags(m2, m2.tdim - 1, ft.indices, ft.values)


def three_problem(forms):
    """ECS + cell 1 (HH) + cell 2 (glial) on the tetrahedral r = 0 box, each cell with its own membrane mesh and model
    and its own diffusion coefficients: the problem of test_flux_gpu._build("three"), i.e. test_gpu_parity._custom_problem
    with {1: [(1, "hh_si")], 2: [(2, "glial")]}, with the same parameters, seed and perturbation.  It is a deliberate
    copy: _custom_problem always builds the device forms, which needs a GPU, and the host tests run this problem without
    one (forms=False); with forms=True it also builds the device forms."""
    from helpers import C_M, FARADAY, PSI, load_model
    from knpemi import (create_functions_emi, create_functions_knp, emi_system, knp_system, set_initial_conditions,
                        setup_membrane_model)
    from knpemi.fem import Constant, extract_submesh, make_mesh_3D
    mesh, ct, ft = make_mesh_3D(0, "tetrahedron", axon_tags=(1, 1, 2, 2))
    dt, models, subs = 1e-4, {1: "hh_si", 2: "glial"}, {}
    for t in (0, 1, 2):
        sm, e2p, v2p, _, _ = extract_submesh(mesh, ct, t)
        subs[t] = dict(tag=t, name=f"sub{t}", mesh_sub=sm, sub_to_parent=e2p, sub_vertex_to_parent=v2p)
        if t > 0:
            g, g2p, _, _, _ = extract_submesh(mesh, ft, [t])
            subs[t].update(mesh_mem=g, mem_to_parent=g2p, membrane_tags=[t], ode_models={t: load_model(models[t])})
    rho = {'z': -1, **{t: Constant(subs[t]['mesh_sub'], 0.1 * t) for t in subs}}
    pp = {'dt': Constant(mesh, dt), 'F': Constant(mesh, FARADAY), 'psi': Constant(mesh, PSI),
          'C_phi': Constant(mesh, C_M / dt), 'C_M': Constant(mesh, C_M), 'rho': rho}
    init = {"Na": (100.7, 12.8), "K": (3.3, 124.2), "Cl": (104.0, 137.0)}
    Dv = {"Na": 1.33e-9, "K": 1.96e-9, "Cl": 2.03e-9}
    ions = [dict(name=n, z=z, D={t: Constant(None, Dv[n] * (1 + 0.1 * t)) for t in subs},
                 c_init={t: Constant(None, init[n][0 if t == 0 else 1]) for t in subs})
            for n, z in (("K", 1.0), ("Cl", -1.0), ("Na", 1.0))]
    phi, phi_M_prev = create_functions_emi(subs, degree=1)
    c, c_prev = create_functions_knp(subs, ions, degree=1)
    set_initial_conditions(ions, subs, c_prev)
    for t in (1, 2):
        subs[t]['mem_models'] = setup_membrane_model({'stimulus': {}, 'stimulus_locator': None}, pp,
                                                     subs[t]['ode_models'], ft, phi_M_prev[t].function_space, ions)
    s = type("S", (), {})()
    s.__dict__.update(mesh=mesh, ct=ct, ft=ft, subdomain_list=subs, ion_list=ions, physical_parameters=pp, dt=dt,
                      phi=phi, phi_M_prev=phi_M_prev, c=c, c_prev=c_prev, entity_maps=[])
    if forms:
        s.a_emi, s.p_emi, s.L_emi = emi_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c_prev, dt)
        s.a_knp, s.p_knp, s.L_knp = knp_system(mesh, ct, ft, pp, ions, subs, phi, phi_M_prev, c, c_prev, dt)
    rng = np.random.default_rng(7)
    for t in subs:
        for f in c_prev[t] + [ions[-1][f'c_{t}']]:
            f.x.array[:] *= 1.0 + 1e-3 * rng.uniform(-1, 1, f.x.array.shape[0])
        phi[t].x.array[:] = 1e-3 * rng.uniform(-1, 1, phi[t].x.array.shape[0])
        if t > 0:
            phi_M_prev[t].x.array[:] = -0.07 + 1e-3 * rng.uniform(-1, 1, phi_M_prev[t].x.array.shape[0])
            for mm in subs[t]['mem_models']:
                for f in mm['I_ch_k'].values():
                    f.x.array[:] = 1e-2 * rng.uniform(-1, 1, f.x.array.shape[0])
    return s


def build(name, r=None, forms=True, **kw):
    """The perturbed set-up `name`; r overrides the refinement level of "2d", "tet" and "hex"; forms=False leaves the
    device forms out (CPU tests)."""
    with contextlib.redirect_stdout(io.StringIO()):
        if name == "three":
            return three_problem(forms)
        if name == "jittered":
            s = Setup("tet", 0, mesh_data=um.jittered_tet_box(), build_forms=forms, **kw)
        elif name == "jittered_hex":
            s = Setup("hex", 0, mesh_data=jittered_hex_box(), build_forms=forms, **kw)
        else:
            s = Setup(name, {"2d": 1, "tet": 0, "hex": 0}[name] if r is None else r, build_forms=forms, **kw)
        s.perturb()
    return s


def exchange(s, watch=True):
    ex = MembraneExchange(s.subdomain_list, s.ion_list, s.physical_parameters, ft=s.ft)
    if watch:
        for tag in list(s.subdomain_list)[1:]:
            ex.watch(tag)
    return ex


def host_state(s):
    """What the exchange record sees, as host arrays: phi, the K concentrations (c_prev of the solved ions, the
    eliminated ion's c), phi_M_prev and I_ch per membrane model."""
    tags = list(s.subdomain_list)
    return dict(
        phi={t: s.phi[t].x._a.copy() for t in tags},
        c_prev={t: [f.x._a.copy() for f in s.c_prev[t]] + [s.ion_list[-1][f"c_{t}"].x._a.copy()] for t in tags},
        phi_M_prev={t: s.phi_M_prev[t].x._a.copy() for t in tags[1:]},
        I_ch={t: [{n: f.x._a.copy() for n, f in mm["I_ch_k"].items()} for mm in s.subdomain_list[t]["mem_models"]]
              for t in tags[1:]},
        dt=float(s.dt))


def column_scale(ex, row, fields, key):
    """The magnitude a column of the series row is compared against: its own, |column|.  Two columns are the exception,
    the totals "<tag>/capacitive" and "<tag>/channel": the capacitive current of a closed cell integrates to zero under the
    splitting scheme (the cell holds no current source), to 1e-9 of its largest per-facet term in the stepper run, and
    the total channel current is a sum of ionic currents of both signs.  There neither the device nor numpy can know the
    sum better than the rounding of its terms, so these two are compared relative to the larger of |column| and the
    largest per-facet integral among their terms.  The flux columns keep |column| whatever their terms do."""
    tag, what = key.split("/", 1)
    f = fields[int(tag)]
    term = 0.0
    if what == "capacitive":
        term = float((f["area"] * np.abs(f["capacitive"])).max())
    elif what == "channel":
        term = max([float((f["area"] * np.abs(f[k])).max()) for k in f if k.endswith("/channel")], default=0.0)
    return max(abs(row[key]), term) or 1.0


def row_err(ex, dev, row, fields):
    """Largest error of a device row against (fields, row) of compute_host, every column relative to `column_scale`."""
    worst = 0.0
    for j, (key, _) in enumerate(ex.columns()):
        worst = max(worst, abs(dev[j] - row[key]) / column_scale(ex, row, fields, key))
    return worst


def fields_err(dev, want):
    """Largest error of the per-facet fields, every component relative to its largest magnitude over the membrane."""
    assert set(dev) == set(want)
    worst = 0.0
    for key in want:
        if key == "facet":
            assert np.array_equal(dev[key], want[key])
            continue
        worst = max(worst, float(np.abs(dev[key] - want[key]).max() / (np.abs(want[key]).max() or 1.0)))
    return worst
