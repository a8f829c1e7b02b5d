"""The facet integrals of b_knp -- stand-alone (knp_membrane_kernel) and in the potential's write-back launch
(emi_writeback_membrane_kernel) -- issue their loads in two batches ahead of the barrier that publishes the quadrature
table: what the thread index addresses, then the facet's data, for every facet; a facet without a model loads with model
slot 0 and drops what it loaded, lanes past the last (facet, side) repeat the last one.  No sum changes, so

  b_knp   with the facet integrals formed by the write-back launch  ==  by the stand-alone facet kernel, bit for bit, and
          both, with A_knp, match the oracle at the tolerance of the parity tests;
  early   knp_membrane_pre_kernel, the two-part form of the same integrals, loads the same way: b_knp formed from its
          parts matches the oracle at that tolerance (its sums are other sums: no bits to compare with the one-part form).

The comparison runs twice and must give the same bits both times.  The set-ups are the smallest that reach the edges of
that code; what each of them contains is asserted from the host tables (test_inputs_reach_the_edges)."""
import contextlib
import ctypes as C
import functools
import io
import os
import re

import numpy as np
import pytest

from helpers import TOL, Setup, csr_rel_err, rel_err
from knpemi import _lib as L
from test_gpu_parity import _custom_problem

pytestmark = pytest.mark.gpu


def _define(header, name):
    """An integer #define of the kernels' sources (the library does not export it)."""
    src = os.path.join(os.path.dirname(os.path.abspath(L.__file__)), os.pardir, "csrc", header)
    with open(src) as f:
        found = re.findall(rf"^\s*#\s*define\s+{name}\s+(\d+)\s*(?://.*)?$", f.read(), re.M)
    assert len(found) == 1, (header, name, found)
    return int(found[0])


MEM_LQ = _define("membrane_facet.h", "KN_MEM_LQ")      # lanes per (facet, side) of the facet kernels
FACET_BLOCK = 256                                      # their workgroup (__launch_bounds__ and launch in kernels_assemble.hip)

NAMES = ("2d", "tet", "hex", "three_subdomains", "unbound_tag", "empty_interface", "fan")


def _build(name):
    if name in ("2d", "tet", "hex"):
        s = Setup(name, 1 if name == "2d" else 0)
        s.perturb()
        return s, None
    if name == "fan":            # a Delaunay mesh whose membrane has vertices of 12, 13 and 15 facets (tests/golden)
        from unstructured_meshes import fan_mesh
        with contextlib.redirect_stdout(io.StringIO()):
            s = Setup("tet", 0, mesh_data=fan_mesh(3))
        s.perturb()
        return s, None
    from knpemi.fem import make_mesh_2D, make_mesh_3D, meshtags
    if name == "three_subdomains":
        mesh, ct, ft = make_mesh_3D(0, "tetrahedron", axon_tags=(1, 1, 2, 2))
        return _custom_problem(mesh, ct, ft, {1: [(1, "hh_si")], 2: [(2, "glial")]}), {0: [], 1: [1], 2: [2]}
    if name == "unbound_tag":    # two tags with a model each, a third one in the membrane space without any
        from unittest import mock
        import knpemi
        mesh, ct, ft = make_mesh_2D(1)
        vals = ft.values.copy()
        mem = np.flatnonzero(vals == 1)
        xm = mesh.x[mesh.facets[ft.indices[mem]]].mean(axis=1)[:, 0]
        vals[mem[xm > 20e-6]] = 6
        vals[mem[xm > 45e-6]] = 7
        make_models = knpemi.setup_membrane_model

        def without_tag_7(stim, pp, ode_models, *args):      # tag 7 stays a membrane tag of the cell; no model is set up for it
            return make_models(stim, pp, {t: m for t, m in ode_models.items() if t != 7}, *args)
        with mock.patch.object(knpemi, "setup_membrane_model", without_tag_7):
            s = _custom_problem(mesh, ct, meshtags(mesh, 1, ft.indices, vals),
                                {1: [(1, "hh_si"), (6, "hh_si"), (7, "hh_si")]})
        assert len(s.subdomain_list[1]['mem_models']) == 2 and s.subdomain_list[1]['membrane_tags'] == [1, 6, 7]
        return s, {0: [], 1: [1, 6, 7]}
    assert name == "empty_interface"
    mesh, ct, ft = make_mesh_2D(0)
    return _custom_problem(mesh, ct, ft, {1: [(1, "hh_si")]}), {0: [], 1: [1]}


class Case:
    """One set-up with both systems assembled once through the solver objects (which upload every field), the oracle's
    objects for it, and the device problem the tests then drive through the C entry points."""

    def __init__(self, name):
        import adapters
        from knpemi.pdeSolver import create_solver_emi, create_solver_knp
        s, subdomains = _build(name)
        self.s = s
        o, P, params, ions = adapters.oracle_problem(s, subdomains) if subdomains else s.oracle()
        c_all, phi, phiM, mm = adapters.oracle_fields(s)
        self.A_knp_oracle, self.b_knp_oracle = o.assemble_knp(P, params, ions, c_all, phi, phiM, mm, s.dt)
        emi = create_solver_emi(s.a_emi, s.L_emi, s.phi, s.entity_maps, s.subdomain_list, None, p=s.p_emi, direct=False)
        knp = create_solver_knp(s.a_knp, s.L_knp, s.c, s.entity_maps, s.subdomain_list, None, p=s.p_knp)
        emi.assemble()
        knp.assemble()
        self.dp = knp.dp
        assert emi.dp is knp.dp
        self.phi_all = np.concatenate([s.phi[t].x._a for t in s.subdomain_list])

    def facet_models(self):
        """Model slot of every membrane facet, -1 without one: the slot of the first model of the facet's cell
        sub-domain that is bound to the facet's tag."""
        dp, out = self.dp, [np.zeros(0, np.int64)]
        for si in range(1, len(dp.tags)):
            tag = dp.flat["facet_tag"][si]
            fm = np.full(tag.shape[0], -1, np.int64)
            for j in reversed(range(int(dp.n_models[si]))):
                fm[tag == int(dp.models[(si, j)]["ode"].tag)] = j
            out.append(fm)
        return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@contextlib.contextmanager
def on_device(a):
    hip = C.CDLL("libamdhip64.so")
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), C.c_size_t(max(a.nbytes, 8))) == 0
    try:
        assert hip.hipMemcpy(dev, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
        yield dev
    finally:
        hip.hipFree(dev)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_inputs_reach_the_edges(hip_lib):
    """What the set-ups contain, from the host tables: launches whose last workgroup has lanes past the last
    (facet, side) and one that ends on a full workgroup, more than one workgroup, facets with NF = 2, 3 and 4 vertices,
    facets without a model beside facets of two models, three sub-domains, a handle without any membrane facet."""
    lanes = {}
    for name in NAMES:
        c = case(name)
        lanes[name] = 2 * int(c.dp.n_facet.sum()) * MEM_LQ
        assert c.facet_models().size == int(c.dp.n_facet.sum()), name
        print(name, "facets", int(c.dp.n_facet.sum()), "lanes", lanes[name], "past the end", -lanes[name] % FACET_BLOCK)
    assert lanes["fan"] % FACET_BLOCK != 0 and lanes["2d"] % FACET_BLOCK != 0
    assert lanes["tet"] % FACET_BLOCK == 0 and lanes["hex"] % FACET_BLOCK == 0   # ... and launches that end on a full workgroup
    assert min(lanes["tet"], lanes["fan"]) > FACET_BLOCK                     # more than one workgroup
    assert [case(n).dp.flat["facet_q"][1].shape[1] for n in ("2d", "tet", "hex")] == [2, 3, 4]
    fm = case("unbound_tag").facet_models()
    assert (fm < 0).any() and (fm == 0).any() and (fm == 1).any()            # fmodel negative on some facets, two slots on others
    assert all((case(n).facet_models() >= 0).all() for n in ("2d", "tet", "hex", "fan"))
    assert len(case("three_subdomains").dp.tags) == 3 and (case("three_subdomains").dp.n_facet[1:] > 0).all()
    assert lanes["empty_interface"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_concentration_system_with_folded_and_stand_alone_facet_integrals(hip_lib, name):
    c = case(name)
    dp = c.dp
    got = []
    with on_device(c.phi_all) as dev:
        for _ in range(2):
            out = {}
            for fold in (1, 0):
                L.check(dp.lib.knpemi_set_option(dp.h, L.OPT_FOLD_MEMBRANE, fold))
                dp.set_rhs(L.B_KNP, np.full(c.b_knp_oracle.size, np.nan))
                L.check(dp.lib.knpemi_set_solution(dp.h, L.B_EMI, dev, 1))     # the write-back launch (fold: with the integrals)
                L.check(dp.lib.knpemi_assemble_knp(dp.h, 0))
                out[fold] = (dp.csr(L.A_KNP), dp.rhs(L.B_KNP).copy())
            L.check(dp.lib.knpemi_set_option(dp.h, L.OPT_FOLD_MEMBRANE, 1))
            for fold in (1, 0):
                errs = (csr_rel_err(out[fold][0], c.A_knp_oracle), rel_err(out[fold][1], c.b_knp_oracle))
                print(name, "fold", fold, "A_knp, b_knp against the oracle:", errs)
                assert max(errs) < TOL, (name, fold, errs)
            assert same_bits(out[1][1], out[0][1]) and same_bits(out[1][0].data, out[0][0].data)
            dp.set_rhs(L.B_KNP, np.full(c.b_knp_oracle.size, np.nan))
            dp.assemble_knp(early_membrane=True)
            early = dp.rhs(L.B_KNP).copy()
            print(name, "early form, b_knp against the oracle:", rel_err(early, c.b_knp_oracle))
            assert rel_err(early, c.b_knp_oracle) < TOL, name
            got.append(out[1] + (early,))
    assert same_bits(got[0][1], got[1][1]) and same_bits(got[0][0].data, got[1][0].data) and same_bits(got[0][2], got[1][2])
