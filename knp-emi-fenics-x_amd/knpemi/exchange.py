"""Membrane ion exchange per cell: how much of every ion crosses a cell's membrane, and the mass budget it closes.

`Observables` records point values and field statistics, `MembraneEvents` the firing of the membranes and `IonFluxes` how
ions move inside a sub-domain.  What crosses the membranes is computed in every step and then discarded: the membrane
term of the KNP right-hand side (`knpWeakForm.py:168-214`) is minus the transmembrane molar flux of each ion, tested
against the facet functions.  Without this module a user downloads phi, every concentration, phi_M and every `I_ch_k`
between the KNP assembly and the end-of-step update and integrates a rational integrand over the facets on the host.
Here one launch directly behind the KNP assembly (csrc/kernels_exchange.hip, `DeviceStepper.exchange`) integrates the
fluxes over the membrane facets of the watched cells from the data the assembly has just read, and appends them to a time
series; the host reads it only when asked.

    ex = MembraneExchange(subdomain_list, ion_list, physical_params)
    ex.watch(tag=1)                                   # every ion and the currents of cell 1
    ex.watch(tag=2, ions=["K"], current=False)
    stepper.exchange(ex, every=1)                     # ... stepper.step() ...
    ser = ex.series()      # "t", "1/K/ecs", "1/K/ics" [mol/s], "1/K/channel" [A], "1/capacitive", "1/channel" [A], "1/area"
    f = ex.fields(1)       # per facet: "K/ecs", "K/ics", "K/channel", "capacitive", "area", "facet" (index into mesh_mem)
    ex.amounts()           # dt * cumulative sums of the molar columns [mol]
    ex.budget(obs.series())

Definitions.  At a point of a membrane facet of cell `tag`, on side s = e (the ECS) or s = i (the cell), for every ion
k = 0 .. K-1, the eliminated one included:

  * j_k^s = (I_ch,k + alpha_k^s (I_cap - S I_ch,tot)) / (F z_k)   [mol / (m^2 s)]
  * I_cap = C_M (phi_M - phi_M_prev) / dt with phi_M = phi_i - phi_e, the jump of the potential just solved for;
  * alpha_k^s = D_k^s z_k^2 c_k^s / sum_j D_j^s z_j^2 c_j^s with c = c_prev on side s (the eliminated ion's c), the
    sum over all K ions;
  * I_ch,tot = sum_j I_ch,j;  S = 1 with the splitting scheme, 0 without.

Sign convention: j and every current are positive OUT of the cell, into the ECS.  Each ion carries its channel current
plus its share alpha of the capacitive current; sum_k alpha_k = 1, so F sum_k z_k j_k^s = I_cap + (1 - S) I_ch,tot on both
sides.  The two sides differ only in alpha: the scheme moves the same charge but not the same ions out of the cell and
into the ECS.

Integrals use the degree-6 facet rule of the assembly (4 Gauss points on intervals, the 12-point rule on triangles, 4 x 4
Gauss with the surface Jacobian per point on bilinear quadrilaterals).  A facet that belongs to no membrane model
contributes nothing; its per-facet values, the area included, are 0.

Series row: per watched (cell, ion) "ecs" = int j_k^e dS, "ics" = int j_k^i dS [mol/s] and "channel" = int I_ch,k dS [A];
with `current=True` "capacitive" = int I_cap dS, "channel" = int I_ch,tot dS [A] and "area", the membrane area.  The time
of a row is the END of the step whose mean rate it is.  `fields` are per-facet means: the facet's integral divided by its
area.

Mass budget.  The facet functions sum to one, so the sum of block (tag, k) of the membrane part of b_knp is
-int j_k^i dS and that of block (0, k) is +sum_cells int j_k^e dS; the row sums of the volume terms of A_knp leave only
the mass term.  The discrete scheme therefore conserves every solved ion exactly, up to the residual of the KNP solve:

    (M_tag,k(t) - M_tag,k(t - dt)) / dt = -int j_k^i dS                              (cells)
    (M_0,k(t)   - M_0,k(t - dt))   / dt = +sum_cells int j_k^e dS  (+ int f_source)   (ECS)

with M = int c dx (`Observables.reduce(op="integral")`).  `budget` returns the defects of these identities.

Cell-partitioned runs (`DeviceStepper.exchange(ex, halo=halo)`, `WatchedIons.partition`): every membrane facet of the
global mesh is recorded by one rank, the lowest owner among its vertices; the facets of a rank's ghost layer get their
per-facet means and enter none of its sums.  Every rank holds the global series, equal to that of one rank holding the
whole mesh up to the order of summation, so `budget` works unchanged with the series of a partitioned `Observables`;
`fields(tag, halo=halo)` returns the means of the local facets with the mask of the ones this rank records.
"""
from __future__ import annotations

import numpy as np

from .fem.function import as_float
from .recording import (CURRENT_BIT, WatchedIons, combine_partials, item_owners, lib_int,  # noqa: F401
                        membrane_meshes, nodal_values as _values)

ION_PARTS = ("ecs", "ics", "channel")


def chunk():
    """Membrane facets per workgroup of the record kernel."""
    return lib_int("kn_exchange_chunk")


def fold_depth():
    """Workgroup partials the record kernel's fold of a column has in flight."""
    return lib_int("kn_exchange_fold_depth")


def facet_rule(nf):
    """(weights (nq,), shape values (nq, nf), reference derivatives (nq, nf, 2) or None) of the degree-6 rule on a facet
    with nf vertices; the weights include the reference measure (1, 1/2, 1)."""
    gx, gw = np.polynomial.legendre.leggauss(4)
    gx, gw = 0.5 * (gx + 1.0), 0.5 * gw
    if nf == 2:
        return gw, np.stack([1.0 - gx, gx], axis=1), None
    if nf == 3:       # 12-point degree-6 symmetric rule (Dunavant)
        w1, b1 = 0.1167862757263793660252896, 0.2492867451709104212916386
        w2, b2 = 0.05084490637020681692093681, 0.0630890144915022283403316
        w3, b3, c3 = 0.08285107561837357519355346, 0.05314504984481694735324967, 0.3103524510337844054166077
        a1, a2, a3 = 1.0 - 2.0 * b1, 1.0 - 2.0 * b2, 1.0 - b3 - c3
        P = [(w1, a1, b1, b1), (w1, b1, a1, b1), (w1, b1, b1, a1), (w2, a2, b2, b2), (w2, b2, a2, b2), (w2, b2, b2, a2),
             (w3, a3, b3, c3), (w3, a3, c3, b3), (w3, b3, a3, c3), (w3, b3, c3, a3), (w3, c3, a3, b3), (w3, c3, b3, a3)]
        P = np.array(P)
        return 0.5 * P[:, 0], P[:, 1:].copy(), None
    if nf != 4:
        raise ValueError("membrane facets are intervals, triangles or quadrilaterals")
    x, y = np.tile(gx, 4), np.repeat(gx, 4)             # vertices in lexicographic order
    N = np.stack([(1 - x) * (1 - y), x * (1 - y), (1 - x) * y, x * y], axis=1)
    dN = np.stack([np.stack([-(1 - y), -(1 - x)], axis=1), np.stack([1 - y, -x], axis=1),
                   np.stack([-y, 1 - x], axis=1), np.stack([y, x], axis=1)], axis=1)
    return np.tile(gw, 4) * np.repeat(gw, 4), N, dN


def facet_weights(X, w, dN):
    """wq (n_facet, nq): quadrature weight times surface Jacobian of the facets with vertex coordinates X (n, nf, gdim)."""
    nf = X.shape[1]
    if nf == 2:
        return w[None, :] * np.linalg.norm(X[:, 1] - X[:, 0], axis=1)[:, None]
    if nf == 3:
        n = np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
        return w[None, :] * np.linalg.norm(n, axis=1)[:, None]          # 2 x area x (weights summing to 1/2)
    u = np.einsum("qb,fbg->fqg", dN[:, :, 0], X)
    v = np.einsum("qb,fbg->fqg", dN[:, :, 1], X)
    return w[None, :] * np.linalg.norm(np.cross(u, v), axis=2)


class MembraneExchange(WatchedIons):
    _NAME, _WATCH, _SELF = "exchange", "cell", "this exchange is"

    def __init__(self, subdomain_list, ion_list, physical_params, ft=None):
        """subdomain_list: the problem's sub-domain dictionary (the ECS, tag 0, first; every cell carries "mesh_sub",
        "mesh_mem" and its "mem_models"); ion_list: the ions in the problem's order, the eliminated one last;
        physical_params: "F" and "C_M" are read.  ft: the facet tags of the parent mesh -- needed by the host
        restatement only where a cell has several membrane models or facets that belong to none: a facet goes to the
        first model whose `ode.tag` is its tag.  Without it every facet of a cell belongs to the cell's first model."""
        self.tags = list(subdomain_list)
        if self.tags[0] != 0:
            raise ValueError("the first sub-domain must be the ECS with tag 0")
        self._init_watched(ion_list)
        self.subdomain_list = subdomain_list
        self.cells = [t for t in self.tags[1:] if "mesh_mem" in subdomain_list[t]]
        self.D = {t: [as_float(ion["D"][t]) for ion in ion_list] for t in self.tags}
        self.F, self.C_M = as_float(physical_params["F"]), as_float(physical_params["C_M"])
        self.ft = ft
        self._geo = {}
        self._dt, self._every = None, 1   # step and record interval of the series (amounts, budget)

    # -- definition ------------------------------------------------------------------------------------
    def watch(self, tag, ions=None, current=True):
        """Watch cell `tag`: the ions named in `ions` (names or indices; None: all, the eliminated one included) and,
        with `current`, the capacitive and the total channel current and the membrane area."""
        if self._dev is not None:
            raise RuntimeError("the exchange is attached to a device problem: watch every cell before exchange()")
        if tag not in self.subdomain_list:
            raise ValueError(f"no sub-domain with tag {tag}")
        if tag not in self.cells:
            raise ValueError("the ECS (tag 0) has no membrane of its own: give the tag of a cell")
        self._watch_ions(tag, ions, current)

    def columns(self):
        """[(key, width)] of the series row in the device's order, every width 1: "<tag>/<ion>/ecs", "<tag>/<ion>/ics"
        [mol/s], "<tag>/<ion>/channel" [A], "<tag>/capacitive", "<tag>/channel" [A] and "<tag>/area"."""
        out = []
        for tag, (idx, cur) in self.watched.items():
            for k in idx:
                out += [(f"{tag}/{self.names[k]}/{p}", 1) for p in ION_PARTS]
            if cur:
                out += [(f"{tag}/capacitive", 1), (f"{tag}/channel", 1), (f"{tag}/area", 1)]
        return out

    def n_facets(self, tag):
        return int(self.subdomain_list[tag]["mesh_mem"].cells.shape[0])

    def _item_owners(self, halo):
        mems = membrane_meshes(self.subdomain_list)
        own = item_owners(mems, halo, "mem", "exchange: the halo does not number the membrane dofs of these cells")
        return {tag: (mems[tag], own[tag]) for tag in mems if tag in self.watched}

    # -- host restatement ----------------------------------------------------------------------------------
    def _geometry(self, tag):
        """Of the membrane of cell `tag`: vertex ids of the facets on the ECS side, the cell side and the membrane mesh,
        the facet table (weights folded into wq), and the model of every facet (-1: none)."""
        if tag not in self._geo:
            sd = self.subdomain_list[tag]
            mem, ecs, ics = sd["mesh_mem"], self.subdomain_list[0]["mesh_sub"], sd["mesh_sub"]
            q = np.asarray(mem.cells)
            pv = np.asarray(mem.parent_vertices)[q]
            e = np.searchsorted(ecs.parent_vertices, pv)
            i = np.searchsorted(ics.parent_vertices, pv)
            w, N, dN = facet_rule(q.shape[1])
            wq = facet_weights(np.asarray(mem.x, np.float64)[q], w, dN)
            models = sd.get("mem_models", [])
            if self.ft is None:
                fmodel = np.full(q.shape[0], 0 if models else -1)
            else:
                ftag = self.ft.dense()[mem.parent_entities]
                fmodel = np.full(q.shape[0], -1)
                for j in reversed(range(len(models))):      # the first model with a given tag wins
                    fmodel[ftag == int(models[j]["ode"].tag)] = j
            self._geo[tag] = (e, i, q, N, wq, fmodel)
        return self._geo[tag]

    def compute_host(self, phi, c_prev, c_elim=None, phi_M_prev=None, I_ch=None, dt=None, splitting=True, recorded=None):
        """(fields, row) from host data, written from the definitions of the module docstring: the numpy restatement of
        the device kernel and the reference of the device tests.  phi[tag]: the potential just solved for, in the ECS
        and in every watched cell; c_prev[tag]: the nodal concentrations, K of them, or the K - 1 solved ones with the
        eliminated ion's taken from c_elim[tag] (default: `ion_list[-1]["c_<tag>"]`); phi_M_prev[tag]: the membrane
        potential after the ODE step; I_ch[tag]: per membrane model of the cell {ion name: channel current on the
        membrane dofs} (default: the `I_ch_k` of `subdomain_list[tag]["mem_models"]`).  `Function`s or arrays.
        fields[tag]: what `fields(tag)` returns; row: the series row as {key: float}.
        recorded: {tag: bool per facet} -- the partial row of one rank of a partition (`partition`): the sums run over
        the recorded facets only; the fields are those of every facet."""
        if dt is None or phi_M_prev is None:
            raise ValueError("compute_host needs phi_M_prev and dt")
        dt, S = as_float(dt), 1.0 if splitting else 0.0

        def conc(tag):
            ck = list(c_prev[tag])
            if len(ck) == self.K - 1:
                ck.append(self.ion_list[-1][f"c_{tag}"] if c_elim is None else c_elim[tag])
            if len(ck) != self.K:
                raise ValueError(f"sub-domain {tag}: {len(ck)} concentrations for {self.K} ions")
            return [_values(u) for u in ck]
        c_e = conc(0)
        phi_e = _values(phi[0])
        fields, row = {}, {}
        for tag, (idx, cur) in self.watched.items():
            e, i, q, N, wq, fmodel = self._geometry(tag)
            rec = slice(None) if recorded is None else np.asarray(recorded[tag], bool)
            at = lambda nodal, ids: np.einsum("qa,fa->fq", N, nodal[ids])      # noqa: E731
            wq = wq * (fmodel >= 0)[:, None]
            area = wq.sum(axis=1)
            c_i = conc(tag)
            nQ = self.subdomain_list[tag]["mesh_mem"].x.shape[0]
            models = self.subdomain_list[tag].get("mem_models", []) if I_ch is None else I_ch[tag]
            Ik = np.zeros((self.K,) + wq.shape)
            for j, mm in enumerate(models):
                sel = fmodel == j
                cur_k = mm["I_ch_k"] if I_ch is None else mm
                for k, name in enumerate(self.names):
                    Ik[k][sel] = at(_values(cur_k[name], nQ), q[sel])
            I_tot = Ik.sum(axis=0)
            I_cap = self.C_M * ((at(_values(phi[tag]), i) - at(phi_e, e)) - at(_values(phi_M_prev[tag]), q)) / dt
            cq_e = [at(c, e) for c in c_e]
            cq_i = [at(c, i) for c in c_i]
            asum_e = sum(self.D[0][k] * self.z[k] ** 2 * cq_e[k] for k in range(self.K))
            asum_i = sum(self.D[tag][k] * self.z[k] ** 2 * cq_i[k] for k in range(self.K))
            inv_area = np.divide(1.0, area, out=np.zeros_like(area), where=area > 0)
            out = {}

            def keep(key, integrand):
                per_facet = (wq * integrand).sum(axis=1)
                out[key] = per_facet * inv_area
                row[f"{tag}/{key}"] = float(per_facet[rec].sum())
            for k in idx:
                n, Fz = self.names[k], self.F * self.z[k]
                a_e = self.D[0][k] * self.z[k] ** 2 * cq_e[k] / asum_e
                a_i = self.D[tag][k] * self.z[k] ** 2 * cq_i[k] / asum_i
                keep(f"{n}/ecs", (Ik[k] + a_e * (I_cap - S * I_tot)) / Fz)
                keep(f"{n}/ics", (Ik[k] + a_i * (I_cap - S * I_tot)) / Fz)
                keep(f"{n}/channel", Ik[k])
            if cur:
                keep("capacitive", I_cap)
                row[f"{tag}/channel"] = float((wq * I_tot)[rec].sum())
                out["area"] = area
                row[f"{tag}/area"] = float(area[rec].sum())
            out["facet"] = np.arange(q.shape[0])
            fields[tag] = out
        return fields, row

    def record_host(self, t, phi, c_prev, c_elim=None, phi_M_prev=None, I_ch=None, dt=None, splitting=True):
        """Append the row of `compute_host` to the series (host drivers): call it between the KNP assembly and the
        end-of-step update, with t the end of the step."""
        self._dt = as_float(dt)
        self._t.append(float(t))
        self._rows.append(self.row_vector(self.compute_host(phi, c_prev, c_elim, phi_M_prev, I_ch, dt, splitting)[1]))

    # -- output --------------------------------------------------------------------------------------------
    def fields(self, tag, halo=None):
        """Per-facet means of the last device record made with fields: "<ion>/ecs", "<ion>/ics", "<ion>/channel" for
        every watched ion, "capacitive" and "area" where the currents are watched, and "facet", the facet's index into
        the cell's `mesh_mem` (one synchronisation).  halo: on a cell-partitioned run the arrays cover this rank's local
        facets, those of the ghost layer included, and "recorded" is the mask of the facets this rank records."""
        self._check_watched(tag)
        nf = self.n_facets(tag)
        get = self._getter(tag, nf, "DeviceStepper.exchange")
        idx, cur = self.watched[tag]
        out = {}
        for k in idx:
            for p, name in enumerate(ION_PARTS):
                out[f"{self.names[k]}/{name}"] = get(k, p)
        if cur:
            out["capacitive"], out["area"] = get(-1, 0), get(-1, 1)
        out["facet"] = np.arange(nf)
        if halo is not None:
            out["recorded"] = self._recorded_of(tag, halo, nf)
        return out

    def amounts(self):
        """{"t", "<tag>/<ion>/ecs", "<tag>/<ion>/ics"}: dt times the cumulative sums of the molar columns -- the amount
        [mol] of the ion that has left the cell (ics) and entered the ECS (ecs) since the series began.  Needs a row for
        every step (every == 1): ValueError otherwise."""
        if self._every != 1:
            raise ValueError("amounts() needs a row for every step (every == 1)")
        ser = self.series()
        if self._dt is None:
            raise ValueError("amounts(): the time step is not known (attach to a stepper or record_host(dt=...))")
        out = {"t": ser["t"]}
        for key, _ in self.columns():
            if key.endswith("/ecs") or key.endswith("/ics"):
                out[key] = self._dt * np.cumsum(ser[key])
        return out

    def mass_key(self, tag, ion):
        """Key under which `budget` looks for int c_ion dx over sub-domain `tag` in an observables series."""
        return f"mass/{tag}/{ion}"

    def observe_masses(self, obs):
        """Define, in the `Observables` obs, the "integral" reduction of every solved ion's c over the ECS and every
        watched cell, under `mass_key`: what `budget` reads."""
        for tag in [0] + list(self.watched):
            for name in self.names[:-1]:
                obs.reduce(self.mass_key(tag, name), "c", tag, "integral", ion=name)

    def budget(self, obs_series):
        """Defects of the mass budget, per row of the series: {"t", "<tag>/<ion>": (M(t) - M(t - dt)) / dt + the ics
        column, for every watched cell and watched solved ion, and "0/<ion>": (M_0(t) - M_0(t - dt)) / dt - the sum of
        the ecs columns, where every cell of the problem watches that ion}.  obs_series: a series of `Observables` that
        holds M = int c dx under `mass_key` (see `observe_masses`) at t and t - dt for every row; a row whose two masses
        are not both there gets NaN.  The ECS identity leaves out a source term f_source.  The defects vanish up to the
        residual of the KNP solve."""
        ser = self.series()
        if self._dt is None:
            raise ValueError("budget(): the time step is not known (attach to a stepper or record_host(dt=...))")
        dt, t = self._dt, ser["t"]
        to = np.asarray(obs_series["t"], np.float64)

        def index(times):
            if to.size == 0:
                return np.full(times.shape, -1)
            j = np.abs(to[None, :] - times[:, None]).argmin(axis=1)
            return np.where(np.abs(to[j] - times) < 1e-6 * dt, j, -1)
        j1, j0 = index(t), index(t - dt)
        ok = (j1 >= 0) & (j0 >= 0)

        def rate(tag, name):
            M = np.asarray(obs_series[self.mass_key(tag, name)], np.float64)
            r = np.full(t.shape, np.nan)
            r[ok] = (M[j1[ok]] - M[j0[ok]]) / dt
            return r
        out = {"t": t}
        for k, name in enumerate(self.names[:-1]):
            cells = [tag for tag, (idx, _) in self.watched.items() if k in idx]
            for tag in cells:
                if self.mass_key(tag, name) in obs_series:
                    out[f"{tag}/{name}"] = rate(tag, name) + ser[f"{tag}/{name}/ics"]
            if set(cells) == set(self.cells) and self.mass_key(0, name) in obs_series:
                out[f"0/{name}"] = rate(0, name) - sum(ser[f"{tag}/{name}/ecs"] for tag in cells)
        return out
