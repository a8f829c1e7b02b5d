"""GPU tests on simplex meshes that are not Kuhn-split boxes (tests/unstructured_meshes.py): the general geometry of the row
kernels on left-handed, arbitrarily ordered and badly shaped cells, rows longer than the 31 entries of the lattice layout,
lanes with more pairs than the prefetch holds, row blocks with more distinct vertices than one staging pass takes,
membrane rows with many general facets, and the DG kernels on the same meshes.  `knpemi_debug_layout` proves in every
test that the mesh reached the code it is there for."""
import ctypes
import functools

import numpy as np
import pytest

import unstructured_meshes as um
from helpers import TOL, Setup, assemble_both, check_facet_integrals_of_the_write_back_launch, csr_rel_err, rel_err
from knpemi import _lib as L

pytestmark = pytest.mark.gpu

KN_PREFETCH = 8        # pairs a lane of the row kernels loads ahead (csrc/knpemi_internal.h)
KN_STAGED = 768        # distinct vertices of a block staged by the batched loads (kernels_assemble.hip: stage_records)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return {"fan2d": lambda: um.fan_mesh(2), "fan3d": lambda: um.fan_mesh(3), "jittered": um.jittered_tet_box}[name]()


def _setup(name, **kw):
    s = Setup("2d" if name == "fan2d" else "tet", 0, mesh_data=_mesh(name), **kw)
    s.perturb()
    return s


def _layout(dp):
    out = (ctypes.c_int * 8)()
    L.check(dp.lib.knpemi_debug_layout(dp.h, out, 8))
    return dict(zip(("longest_row", "lanes_per_row", "pairs_per_lane", "block_vertices", "membrane_entries", "lds_emi",
                     "lds_knp", "longest_laplacian_row"), out))


def _lattice_path(dp):
    flags = ctypes.c_int(-1)
    L.check(dp.lib.knpemi_debug_geometry(dp.h, ctypes.byref(flags)))
    return bool(flags.value & 1)


def _values(a):
    return np.asarray(a.data if hasattr(a, "indptr") else a)


@pytest.mark.parametrize("name", ["fan2d", "fan3d", "jittered"])
@pytest.mark.parametrize("splitting", [True, False])
def test_assembly_matches_oracle_on_unstructured_simplices(hip_lib, name, splitting):
    """All five objects at 1e-10 on the general path.  The jittered box still carries `uniform_cell`: the lattice path
    must be refused on the coordinates.  Layout on the fan meshes (3D / 2D): longest row 47 / 37, 19 / 18 pairs per
    lane at the default 4 / 2 lanes per row (76 / 36 cells at one vertex)."""
    s = _setup(name)
    errs, _ = assemble_both(s, splitting)
    lay = _layout(s.a_emi.dp)
    print(name, splitting, errs, lay)
    assert not _lattice_path(s.a_emi.dp)
    if name == "jittered":
        assert getattr(s.mesh, "uniform_cell", None) is not None
    else:
        assert lay["longest_row"] > 31 and lay["longest_laplacian_row"] > 31
        assert lay["pairs_per_lane"] > KN_PREFETCH
    assert lay["lds_emi"] > 0 and lay["lds_knp"] > 0
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("name,lanes", [("fan3d", (1, 2, 4, 8)), ("fan2d", (1, 2, 4))])
def test_lanes_per_row_agree_on_the_fan_meshes(hip_lib, monkeypatch, name, lanes):
    """KNPEMI_LPR: with one lane per row a lane carries every pair of its row (76 in 3D, 36 in 2D), with eight some lanes
    of a short row carry none.  Every run against the oracle at 1e-10, the runs against each other at 1e-12 of the largest
    entry (the lanes' partial sums are added in another order)."""
    most_cells = um.mesh_statistics(_mesh(name))["most_cells_at_a_submesh_vertex"]
    res = {}
    for lpr in lanes:
        monkeypatch.setenv("KNPEMI_LPR", str(lpr))
        s = _setup(name)
        errs, objs = assemble_both(s)
        lay = _layout(s.a_emi.dp)
        print(name, lpr, errs, lay)
        assert lay["lanes_per_row"] == lpr and lay["pairs_per_lane"] == -(-most_cells // lpr)
        assert lay["pairs_per_lane"] > KN_PREFETCH
        assert max(errs.values()) < TOL, (lpr, errs)
        res[lpr] = [_values(a).copy() for a in objs]
    for lpr in lanes[1:]:
        for a, b in zip(res[lanes[0]], res[lpr]):
            assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max(), lpr


def test_oversized_row_blocks_on_the_shuffled_box(hip_lib, monkeypatch):
    """KNPEMI_BLOCK_CLASSIC=1 on the jittered, shuffled box: 64 consecutive rows of a random numbering touch up to 771
    distinct vertices on the r = 0 box (make_mesh_3D(0, "tetrahedron", l=2); x-fastest numbering: 456), more than the 768
    the batched loads of stage_records take, so its loop for oversized blocks runs (clustered blocks: fewer).  Against the
    oracle, and bit for bit equal to the clustered run."""
    res = {}
    for classic in (False, True):
        if classic:
            monkeypatch.setenv("KNPEMI_BLOCK_CLASSIC", "1")
        else:
            monkeypatch.delenv("KNPEMI_BLOCK_CLASSIC", raising=False)
        s = _setup("jittered")
        errs, objs = assemble_both(s)
        lay = _layout(s.a_emi.dp)
        print("classic" if classic else "clustered", errs, lay)
        assert max(errs.values()) < TOL, errs
        res[classic] = (objs, lay)
    assert res[True][1]["block_vertices"] > KN_STAGED
    for a, b in zip(res[False][0], res[True][0]):
        assert np.array_equal(_values(a), _values(b))


def test_emi_invariants_and_reproducibility_on_the_3d_fan_mesh(hip_lib):
    s = _setup("fan3d")
    _, first = assemble_both(s)
    A = first[0]
    assert np.abs(A @ np.ones(A.shape[0])).max() < 1e-12 * np.abs(A.data).max()
    assert csr_rel_err(A, A.T.tocsr()) < 1e-14
    first = [_values(a).copy() for a in first]
    _, second = assemble_both(s)
    for a, b in zip(first, second):
        assert np.array_equal(a, _values(b))


def test_trace_on_a_jagged_interface_matches_oracle(hip_lib):
    """test_trace_matches_oracle on the 2D fan mesh: 43 membrane vertices on three closed polygons, shuffled numbering."""
    from knpemi import interpolate_to_membrane
    s = _setup("fan2d")
    o, P, params, ions = s.oracle()
    qe, qi = interpolate_to_membrane(s.phi[0], s.phi[1], s.phi_M_prev[1].function_space, s.mesh, s.ct,
                                     s.subdomain_list, 1)
    te, ti = P.trace(1, s.phi[0].x._a, s.phi[1].x._a)
    assert len(te) >= 40 and np.abs(te - ti).max() > 0
    assert np.array_equal(qe.x._a, te) and np.array_equal(qi.x._a, ti)
    assert qe.name == s.phi[0].name


def test_update_pde_on_a_jagged_interface_matches_oracle(hip_lib):
    """test_update_pde_matches_oracle on the 2D fan mesh."""
    from knpemi import update_pde_variables
    s = _setup("fan2d")
    o, P, params, ions = s.oracle()
    c_all, phi, phiM, mm = s.oracle_fields()
    c_new = {t: [f.x._a.copy() for f in s.c[t]] for t in s.subdomain_list}
    s.physical_parameters['rho'][1].value = np.asarray(0.7)
    rho = {'z': -1, 0: 0.0, 1: 0.7}
    update_pde_variables(s.c, s.c_prev, s.phi, s.phi_M_prev, s.physical_parameters, s.ion_list,
                         s.subdomain_list, s.mesh, s.ct)
    o.update_pde_variables(P, ions, rho, c_new, c_all, phi, phiM)
    for t in s.subdomain_list:
        for k in range(2):
            assert np.array_equal(s.c_prev[t][k].x._a, c_all[t][k])
        assert rel_err(s.ion_list[-1][f'c_{t}'].x._a, c_all[t][2]) < 1e-15
    assert rel_err(s.phi_M_prev[1].x._a, phiM[1]) < 1e-15


def test_three_time_steps_on_the_2d_fan_mesh_match_oracle(hip_lib):
    """The loop of test_ten_time_steps_2d_match_oracle on the 2D fan mesh, three steps (the index plumbing of a jagged
    interface is under test, not the integrator): GPU assembly + ODE sweep + direct host solves against the oracle loop,
    the same comparisons at the same tolerances."""
    import driver
    from knpemi import update_ode_variables, update_pde_variables
    from knpemi.pdeSolver import create_solver_emi, create_solver_knp
    s = Setup("2d", 0, g_syn=10.0, mesh_data=_mesh("fan2d"))
    o, P, params, ions = s.oracle()
    c_all, _, _, _ = s.oracle_fields()
    ode = s.mem_models[0]['ode']
    mask = np.array([x[0] < 20e-6 for x in ode.dof_locations])
    assert 0 < mask.sum() < len(mask)
    run = driver.OracleRun(P, params, ions, "hh_si", c_all, ode.states.copy(), ode.parameters.copy(),
                           ode.dof_locations, mask, {o.MODELS["hh_si"]["pidx"]["stim_amplitude"]: 10.0},
                           {'z': -1, 0: 0.0, 1: 0.0})
    emi = create_solver_emi(s.a_emi, s.L_emi, s.phi, s.entity_maps, s.subdomain_list, None, direct=True, p=s.p_emi)
    knp = create_solver_knp(s.a_knp, s.L_knp, s.c, s.entity_maps, s.subdomain_list, None, direct=True, p=s.p_knp)
    for k in range(3):
        update_ode_variables(ode, s.c_prev, s.phi_M_prev[1], s.ion_list, s.subdomain_list, s.mesh, s.ct, 1, k)
        ode.step_lsoda(s.dt, s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
        ode.get_membrane_potential(s.phi_M_prev[1])
        for ion, f in s.mem_models[0]['I_ch_k'].items():
            ode.get_parameter("I_ch_" + ion, f)
        emi.solve()
        knp.solve()
        update_pde_variables(s.c, s.c_prev, s.phi, s.phi_M_prev, s.physical_parameters, s.ion_list,
                             s.subdomain_list, s.mesh, s.ct)
        run.step()
    errs = dict(phiM=rel_err(s.phi_M_prev[1].x._a, run.phiM[1]), states=rel_err(ode.states, run.states))
    x_gpu = np.concatenate([s.phi[0].x._a, s.phi[1].x._a])
    x_ref = np.concatenate([run.phi[0], run.phi[1]])
    errs["phi"] = rel_err(x_gpu - x_gpu.mean(), x_ref - x_ref.mean())
    for t in (0, 1):
        for k in range(3):
            got = s.c_prev[t][k].x._a if k < 2 else s.ion_list[-1][f'c_{t}'].x._a
            errs[f"c{t}{k}"] = rel_err(got, run.c_all[t][k])
    print(errs)
    assert errs["phiM"] < 1e-8 and errs["phi"] < 1e-8 and errs["states"] < 1e-8
    assert max(v for k, v in errs.items() if k.startswith("c")) < 1e-10


def test_facet_integrals_of_the_write_back_launch_on_the_3d_fan_mesh(hip_lib):
    """test_facet_integrals_formed_in_the_potential_write_back_launch on 118 general membrane triangles, up to twelve on
    one membrane vertex."""
    s = _setup("fan3d")
    check_facet_integrals_of_the_write_back_launch(s)
    assert _layout(s.a_emi.dp)["membrane_entries"] >= 5


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("splitting", [True, False])
def test_dg_assembly_matches_oracle_on_the_fan_meshes(hip_lib, dim, splitting):
    """The body of test_dg_assembly_matches_oracle (tests/test_dg_gpu.py) on the committed meshes, K = 3."""
    from knpemi.dg import DGProblem
    import knpemi_dg_oracle as dg
    from test_dg_gpu import _push, _random_state
    K = 3
    mesh, ct, ft = _mesh(f"fan{dim}d")
    dp = DGProblem(mesh, ct, ft, [0, 1], [1], n_ions=K)
    dp.gamma = 7.5
    o = dg.DGOracle(mesh.x, mesh.cells, mesh.cell_type, dp.cell_sub, dp.mem_facets, dp.mem_tags)
    zs = [1.0, -1.0, 2.0, -1.0][:K]
    ions = [dict(name=f"i{k}", z=zs[k], D=[1.0 + 0.3 * k, 0.6 + 0.2 * k]) for k in range(K)]
    params = dict(dt=0.05, F=1.3, psi=0.8, C_M=0.7)
    c_all, phi, phi_M, I_ch, src = _random_state(dp, K, 1)
    _push(dp, params, ions, c_all, phi, phi_M, I_ch, src)
    dp.assemble_emi(splitting)
    dp.assemble_knp(splitting)
    A, b = o.assemble_emi(params, ions, c_all, phi_M, I_ch, splitting_scheme=splitting, gamma=7.5)
    As, bs = o.assemble_knp(params, ions, c_all, phi, phi_M, I_ch, splitting_scheme=splitting, gamma=7.5, f_source=src)
    errs = dict(A_emi=csr_rel_err(dp.matrix(0), A), b_emi=rel_err(dp.rhs(0), b))
    for k in range(K - 1):
        errs[f"A_knp{k}"], errs[f"b_knp{k}"] = csr_rel_err(dp.matrix(1 + k), As[k]), rel_err(dp.rhs(1 + k), bs[k])
    print(dim, splitting, errs)
    assert max(errs.values()) < 1e-10, errs
    # the pattern is the one the header promises: one nv-wide block per cell and facet neighbour, sorted
    assert np.all(np.diff(dp.indptr) % dp.nv == 0)
    for r in (0, dp.n // 2, dp.n - 1):
        cols = dp.indices[dp.indptr[r]:dp.indptr[r + 1]]
        assert np.all(np.diff(cols) > 0) and r in cols


@pytest.mark.parametrize("height", [1.0, 1e-3])
def test_sliver_tetrahedra(hip_lib, height):
    """One ECS and one intracellular tetrahedron on a shared membrane triangle of edge 1 um, apexes at +-height um:
    1 : 1 as the control, 1 : 1000 as the sliver.  The bound is not fixed in advance: the oracle's own rounding
    sensitivity on this mesh (the largest relative difference over the five objects when every cell's vertex list is
    rotated by one) times 100 -- the kernel and the oracle order the cancellation in g0 = -(g1 + g2 + g3) differently --
    and never less than 1e-10.  Measured oracle sensitivity: 7.4e-14 (1 : 1) and 3.1e-13 (1 : 1000), both in b_emi, so the
    bound is 1e-10 on both; the kernel's figures are printed."""
    data = um.sliver_mesh(height)
    sens = max(um.rounding_sensitivity(data).values())
    s = Setup("tet", 0, mesh_data=data)
    s.perturb()
    for splitting in (True, False):
        errs, _ = assemble_both(s, splitting)
        print("sliver", height, "oracle sensitivity", sens, "kernel", errs)
        assert not _lattice_path(s.a_emi.dp)
        assert max(errs.values()) < max(TOL, 100.0 * sens), (sens, errs)


@pytest.mark.parametrize("shift,lattice", [(1e-7, False), (1e-12, True)])
def test_lattice_acceptance_tolerance(hip_lib, shift, lattice):
    """The tet r = 0 box with ONE interior vertex moved by `shift` grid spacings.  1e-7: the mesh is not the grid (the
    shape table would be wrong by a relative 1e-6 or so, four decades above the stated 1e-10): the general kernels must
    run and meet the oracle on the moved mesh.  1e-12: rounding of the coordinates, the lattice path stays."""
    from setup_problem import make_mesh
    mesh, ct, ft = make_mesh("tet", 0)
    h = np.diag(mesh.uniform_cell)
    inner = np.flatnonzero(np.all((mesh.x > 2.5 * h) & (mesh.x < mesh.x.max(axis=0) - 2.5 * h), axis=1))
    v = inner[len(inner) // 2]
    mesh.x[v] += shift * h
    s = Setup("tet", 0, mesh_data=(mesh, ct, ft))
    s.perturb()
    errs, _ = assemble_both(s)
    print(shift, errs, _layout(s.a_emi.dp))
    assert _lattice_path(s.a_emi.dp) == lattice
    assert max(errs.values()) < TOL, errs
