"""CPU tests of the membrane exchange's numpy restatement (knpemi.exchange.MembraneExchange.compute_host), the reference
of the device tests: tied to the oracle's b_knp, to the charge identity, to closed forms on constant fields, and to the
mass budget of one solved step.  TOL is relative to the magnitude of the compared column or component."""
import contextlib
import functools
import io
import os
import re

import numpy as np
import pytest

import adapters
import exchange_cases as xc
from helpers import TOL, Setup
from knpemi import MembraneExchange

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SETUPS = ("2d", "tet", "hex", "three", "jittered")


@functools.lru_cache(maxsize=None)
def _case(name):
    """(set-up, exchange watching every cell, host state)"""
    s = xc.build(name, forms=False)
    return s, xc.exchange(s), xc.host_state(s)


def _abs_flux(fields, key):
    """sum over the facets of |int_facet j dS|: the magnitude a budget defect is measured against."""
    return float((fields["area"] * np.abs(fields[key])).sum())


@pytest.mark.parametrize("splitting", [True, False])
@pytest.mark.parametrize("name", ORACLE_SETUPS)
def test_block_sums_of_the_oracles_membrane_term(name, splitting):
    """b_knp of the oracle with the membrane models minus b_knp without them is the membrane term; the facet functions
    sum to one, so block (tag, k) of it sums to -int j_k^i dS and block (0, k) to +sum_cells int j_k^e dS."""
    s, ex, st = _case(name)
    subdomains = {t: list(sd.get("membrane_tags", [])) for t, sd in s.subdomain_list.items()}
    o, P, params, ions = adapters.oracle_problem(s, subdomains)
    c_all, phi, phiM, mm = adapters.oracle_fields(s)
    _, b = o.assemble_knp(P, params, ions, c_all, phi, phiM, mm, s.dt, splitting_scheme=splitting)
    _, b0 = o.assemble_knp(P, params, ions, c_all, phi, phiM, {t: [] for t in mm}, s.dt, splitting_scheme=splitting)
    d = b - b0
    boff, _ = o.knp_block_offsets(P, len(ions) - 1)
    _, row = ex.compute_host(splitting=splitting, **st)
    worst = 0.0
    for k, ion in enumerate(ions[:-1]):
        into_ecs = 0.0
        for t in P.tags[1:]:
            got, want = d[boff[(t, k)]:boff[(t, k)] + P.N[t]].sum(), -row[f"{t}/{ion['name']}/ics"]
            worst = max(worst, abs(got - want) / abs(want))
            into_ecs += row[f"{t}/{ion['name']}/ecs"]
        got = d[boff[(0, k)]:boff[(0, k)] + P.N[0]].sum()
        worst = max(worst, abs(got - into_ecs) / abs(into_ecs))
    print(name, splitting, "largest relative error", worst)
    assert worst < TOL


@pytest.mark.parametrize("splitting", [True, False])
@pytest.mark.parametrize("name", xc.SETUPS)
def test_charge_identity(name, splitting):
    """sum_k alpha_k = 1: F sum_k z_k j_k = I_cap + (1 - S) I_ch,tot on both sides, and the per-ion channel columns add
    up to the channel column."""
    s, ex, st = _case(name)
    _, row = ex.compute_host(splitting=splitting, **st)
    for tag in ex.watched:
        want = row[f"{tag}/capacitive"] + (0.0 if splitting else 1.0) * row[f"{tag}/channel"]
        for side in ("ecs", "ics"):
            got = ex.F * sum(z * row[f"{tag}/{n}/{side}"] for z, n in zip(ex.z, ex.names))
            assert abs(got - want) < TOL * abs(want), (tag, side)
        chan = sum(row[f"{tag}/{n}/channel"] for n in ex.names)
        scale = max(abs(row[f"{tag}/{n}/channel"]) for n in ex.names)
        assert abs(chan - row[f"{tag}/channel"]) < TOL * scale


def _membrane_area(name):
    """From the box geometry: the 2-D cell is [1, 61] x [1, 3] um, the 3-D cells are four axons of 22 x 0.2 x 0.2 um."""
    if name == "2d":
        return 2.0 * (60e-6 + 2e-6)
    return 4.0 * (4.0 * 22e-6 * 0.2e-6 + 2.0 * 0.2e-6 * 0.2e-6)


@pytest.mark.parametrize("splitting", [True, False])
@pytest.mark.parametrize("name", ["2d", "tet", "hex"])
def test_constant_fields_give_area_times_the_pointwise_formula(name, splitting):
    s, ex, st = _case(name)
    rng = np.random.default_rng(11)
    K, S = ex.K, 1.0 if splitting else 0.0
    phi_v = {0: 1.3e-3, 1: -68.2e-3}
    c_v = {t: [float(v) for v in rng.uniform(5.0, 120.0, K)] for t in (0, 1)}
    I_v = [float(v) for v in rng.uniform(-2e-2, 2e-2, K)]
    pm = -71.0e-3
    n = {t: s.subdomain_list[t]["mesh_sub"].x.shape[0] for t in (0, 1)}
    nq = s.subdomain_list[1]["mesh_mem"].x.shape[0]
    args = dict(phi={t: np.full(n[t], phi_v[t]) for t in (0, 1)},
                c_prev={t: [np.full(n[t], v) for v in c_v[t]] for t in (0, 1)},
                I_ch={1: [{nm: np.full(nq, I_v[k]) for k, nm in enumerate(ex.names)}]}, dt=st["dt"])
    fields, row = ex.compute_host(phi_M_prev={1: np.full(nq, pm)}, splitting=splitting, **args)
    area = _membrane_area(name)
    assert abs(row["1/area"] - area) < 1e-12 * area
    assert abs(fields[1]["area"].sum() - area) < 1e-12 * area
    I_cap = ex.C_M * ((phi_v[1] - phi_v[0]) - pm) / st["dt"]
    I_tot = sum(I_v)
    for k, nm in enumerate(ex.names):
        for t, side in ((0, "ecs"), (1, "ics")):
            asum = sum(ex.D[t][j] * ex.z[j] ** 2 * c_v[t][j] for j in range(K))
            alpha = ex.D[t][k] * ex.z[k] ** 2 * c_v[t][k] / asum
            j = (I_v[k] + alpha * (I_cap - S * I_tot)) / (ex.F * ex.z[k])
            assert abs(row[f"1/{nm}/{side}"] - area * j) < TOL * abs(area * j)
            assert np.abs(fields[1][f"{nm}/{side}"] - j).max() < TOL * abs(j)
        assert abs(row[f"1/{nm}/channel"] - area * I_v[k]) < TOL * abs(area * I_v[k])
    assert abs(row["1/capacitive"] - area * I_cap) < TOL * abs(area * I_cap)
    assert abs(row["1/channel"] - area * I_tot) < TOL * abs(area * I_tot)
    # phi_M = phi_M_prev: no capacitive current, every ion carries its channel current alone (without the splitting)
    _, rest = ex.compute_host(phi_M_prev={1: np.full(nq, phi_v[1] - phi_v[0])}, splitting=splitting, **args)
    assert abs(rest["1/capacitive"]) < TOL * abs(area * I_tot)
    if not splitting:
        for k, nm in enumerate(ex.names):
            want = area * I_v[k] / (ex.F * ex.z[k])
            assert abs(rest[f"1/{nm}/ics"] - want) < TOL * abs(want)


@pytest.mark.parametrize("name", xc.SETUPS)
def test_row_equals_area_weighted_sums_of_the_fields(name):
    s, ex, st = _case(name)
    fields, row = ex.compute_host(**st)
    for tag in ex.watched:
        f = fields[tag]
        assert np.array_equal(f["facet"], np.arange(ex.n_facets(tag)))
        for key in f:
            if key in ("facet", "area"):
                continue
            want = row[f"{tag}/{key}"]
            assert abs((f["area"] * f[key]).sum() - want) < TOL * abs(want), key
        assert abs(f["area"].sum() - row[f"{tag}/area"]) < TOL * row[f"{tag}/area"]
    flat = ex.row_vector(row)
    assert flat.shape == (ex.n_cols,) and ex.n_cols == len(ex.watched) * (3 * ex.K + 3)


def test_facets_without_a_model_contribute_nothing():
    """Cell 1 of the three-sub-domain mesh with the membrane model moved to another facet tag: every facet has
    fmodel = -1."""
    s, ex, st = _case("three")
    models = s.subdomain_list[1]["mem_models"]
    other = type("Ode", (), {"tag": 77})()
    subs = dict(s.subdomain_list)
    subs[1] = dict(subs[1], mem_models=[dict(models[0], ode=other)])
    ex2 = MembraneExchange(subs, s.ion_list, s.physical_parameters, ft=s.ft)
    ex2.watch(1)
    ex2.watch(2)
    fields, row = ex2.compute_host(**st)
    assert all(row[k] == 0.0 for k in row if k.startswith("1/"))
    assert all(not fields[1][k].any() for k in fields[1] if k != "facet")
    _, full = ex.compute_host(**st)
    assert all(row[k] == full[k] for k in row if k.startswith("2/"))


def test_mass_budget_of_one_step():
    """One step of the perturbed 2-D set-up from the oracle's A_knp and b_knp (SciPy LU, the oracle's mass weights
    dt 1^T A_knp): (M_new - M_old) / dt + int j^i dS (cell) and (M_new - M_old) / dt - int j^e dS (ECS) vanish up to
    rounding.  M / dt is 1e4 to 1e5 times the flux here, so the difference of the masses cancels that many digits.
    Measured on the CPU, relative to sum_facets |int_facet j dS|: 1.2e-12 (K, ECS), 5.7e-12 (K, cell), 2.6e-12 (Cl, ECS),
    1.1e-12 (Cl, cell); LU residual 6e-22.  Asserted: 10 x the largest, 5.7e-11, which covers the pivoting of other
    SciPy builds and stays far below the 1e-6 at which the budget would no longer resolve the flux."""
    import scipy.sparse.linalg as spla
    with contextlib.redirect_stdout(io.StringIO()):
        s = Setup("2d", 1, g_syn=10.0, build_forms=False)
        s.perturb()
    ex, st = xc.exchange(s), xc.host_state(s)
    o, P, params, ions = adapters.oracle_problem(s)
    c_all, phi, phiM, mm = adapters.oracle_fields(s)
    A, b = o.assemble_knp(P, params, ions, c_all, phi, phiM, mm, s.dt)
    x = spla.splu(A.tocsc()).solve(b)
    w = s.dt * np.asarray(A.sum(axis=0)).ravel()
    fields, row = ex.compute_host(**st)
    boff, _ = o.knp_block_offsets(P, 2)
    worst = 0.0
    for k, nm in enumerate(("K", "Cl")):
        for t, side, sign in ((0, "ecs", -1.0), (1, "ics", 1.0)):
            sl = slice(boff[(t, k)], boff[(t, k)] + P.N[t])
            defect = (w[sl] @ x[sl] - w[sl] @ c_all[t][k]) / s.dt + sign * row[f"1/{nm}/{side}"]
            rel = abs(defect) / _abs_flux(fields[1], f"{nm}/{side}")
            print(nm, side, "defect", defect, "relative", rel)
            worst = max(worst, rel)
    assert worst < 5.7e-11


def test_watch_arguments_series_amounts_and_budget():
    s, _, st = _case("2d")
    ex = xc.exchange(s, watch=False)
    with pytest.raises(ValueError, match="ECS"):
        ex.watch(0)
    with pytest.raises(ValueError):
        ex.watch(7)
    with pytest.raises(ValueError):
        ex.watch(1, ions=[], current=False)
    with pytest.raises(ValueError):
        ex.watch(1, ions=[3])
    ex.watch(1, ions=["Cl", 0], current=False)
    with pytest.raises(ValueError):
        ex.watch(1)
    assert ex.mask(1) == 0b011
    assert [k for k, _ in ex.columns()] == ["1/K/ecs", "1/K/ics", "1/K/channel", "1/Cl/ecs", "1/Cl/ics", "1/Cl/channel"]
    full = xc.exchange(s)
    assert full.mask(1) == 0x100 | 0b111
    assert [k for k, _ in full.columns()][-3:] == ["1/capacitive", "1/channel", "1/area"]
    dt = st["dt"]
    ex.record_host(dt, **st)
    ex.record_host(2 * dt, **st)
    ser = ex.series()
    _, row = ex.compute_host(**st)
    assert ser["t"].tolist() == [dt, 2 * dt] and set(ser) == {"t"} | set(row)
    assert all(ser[k].shape == (2,) and ser[k][1] == row[k] for k in row)
    am = ex.amounts()
    assert set(am) == {"t", "1/K/ecs", "1/K/ics", "1/Cl/ecs", "1/Cl/ics"}
    assert np.allclose(am["1/K/ics"], dt * row["1/K/ics"] * np.array([1.0, 2.0]), rtol=1e-15, atol=0)
    ex._every = 2
    with pytest.raises(ValueError, match="every"):
        ex.amounts()
    ex._every = 1
    # masses that move exactly as the recorded fluxes say close the budget; the row without M(t - dt) gets NaN
    steps = np.array([1.0, 2.0])
    M = {ex.mass_key(1, n): -dt * steps * row[f"1/{n}/ics"] for n in ("K", "Cl")}
    M.update({ex.mass_key(0, n): dt * steps * row[f"1/{n}/ecs"] for n in ("K", "Cl")})
    bud = ex.budget(dict(t=dt * steps, **M))
    assert set(bud) == {"t", "1/K", "1/Cl", "0/K", "0/Cl"}
    for key, col in (("1/K", "1/K/ics"), ("1/Cl", "1/Cl/ics"), ("0/K", "1/K/ecs"), ("0/Cl", "1/Cl/ecs")):
        assert np.isnan(bud[key][0]) and abs(bud[key][1]) < 1e-12 * abs(row[col]), key
    # the K - 1 solved concentrations with the eliminated ion's from c_elim give the same row
    part = dict(st, c_prev={t: st["c_prev"][t][:2] for t in st["c_prev"]})
    _, row2 = ex.compute_host(c_elim={t: st["c_prev"][t][2] for t in st["c_prev"]}, **part)
    assert row2 == row
    with pytest.raises(ValueError):
        ex.compute_host(st["phi"], st["c_prev"])


def test_abi_declares_and_exports_the_exchange_entries(hip_lib):
    header = open(os.path.join(ROOT, "include", "knpemi_hip.h")).read()
    declared = set(re.findall(r"\bint (knpemi_exchange_[a-z_]+)\s*\(", header))
    assert declared == {"knpemi_exchange_set", "knpemi_exchange_record", "knpemi_exchange_read",
                        "knpemi_exchange_fields", "knpemi_exchange_reset", "knpemi_exchange_clear"}
    for name in declared:
        assert hasattr(hip_lib, name), name
        at = header.index("int " + name + "(")
        assert "knpWeakForm.py:168-214" in header[header.rfind("/*", 0, at):at]
    from knpemi import exchange
    assert exchange.chunk() == 32
