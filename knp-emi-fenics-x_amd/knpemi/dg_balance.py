"""The per-cell ion balance of a DG run (knpemi.dg.DGProblem): facet fluxes and membrane exchange, cell by cell.

The DG counterpart of `knpemi.fluxes.IonFluxes` + `knpemi.exchange.MembraneExchange` + its `budget`, at the resolution
the scheme conserves at.  The reference has no DG code (knpemi/dg.py says what it does have), so there is no reference
interface here either.  Testing the system of solved ion k with the indicator of one cell T leaves

    (m_T,k(new) - m_T,k(old)) / dt + out_T,k = mem_T,k + src_T,k   (+ the cell's share of the solve's residual)

    m_T,k   = int_T c_k
    out_T,k = sum over the interior facets F of T of the numerical outflow, in three parts
                cons  = - int_F {D_k grad c_k} . n_T
                pen   =   int_F (gamma / h_F) {D_k} [c_k]
                drift =   int_F beta_F c_k^up,  beta_F = -z_k psi {D_k grad phi} . n_T, upwind side T when beta_F > 0
    mem_T,k = +/- the integral over the cell's membrane facets of j_k^s of knpemi/exchange.py, positive INTO T
    src_T,k = int_T f_k on ECS cells

because the gradients of a cell's basis sum to zero.  The numerical outflow is antisymmetric between the two cells of a
facet, so the outflows of a sub-domain sum to rounding noise and its mass changes by membrane transfer and sources alone.

    bal = DGIonBalance(mesh, ct, ft, [0, 1], [1], ["Na", "K", "Cl"])
    dp.balance(bal)
    ... dp.assemble_knp(); dp.record_membrane(); dp.solve_knp(update=True); dp.record(t) ...
    bal.series()       # "t", "<sub>/<ion>/mass", ".../outflow", ".../penalty", ".../defect_max",
                       # "<tag>/<ion>/ecs", "<tag>/<ion>/ics", "<tag>/capacitive", "<tag>/channel", "<tag>/area"
    bal.cells()        # {"mem", "cons", "pen", "drift", "m_old", "m_new", "src", "defect"}: (n_cells, K) of the last record
    bal.current()      # F sum_k z_k out_T,k per cell

Two launches per recorded step (csrc/kernels_dg_balance.hip): `record_membrane` between the assembly and the solve of the
concentrations, where the old concentrations, the new potential, the old phi_M and I_ch are on the device, and `record`
at the end of the step.  `evaluate_host` is the numpy restatement the device is tested against: quadrature with every
basis function evaluated through its own cell's map, each facet computed once and handed to its two cells with opposite
signs -- on purpose another route than the kernel's closed forms and facet-aligned frames.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .dg import cell_subdomains, membrane_facets
from .dg_recording import DGTopology, element_integral_weights
from .exchange import facet_rule, facet_weights
from .fem.probe import _G2, _tensor_shape
from .recording import RowSeries

CELL_COLUMNS = ("mem", "cons", "pen", "drift", "m_old", "m_new", "src", "defect")
SUB_COLUMNS = ("mass", "outflow", "penalty", "defect_max")
_FACET_TYPE = {"triangle": "interval", "tetrahedron": "triangle", "hexahedron": "quadrilateral"}


def _hex_ref(local):
    """Reference coordinates of the local vertices `local` (...,) of a hexahedron: bit a is the coordinate along axis a."""
    return np.stack([(local >> a) & 1 for a in range(3)], axis=-1).astype(np.float64)


class DGIonBalance(RowSeries):
    def __init__(self, mesh, ct, ft, subdomain_tags, membrane_tags, ion_names):
        """`mesh`, `ct`, `ft`, `subdomain_tags`, `membrane_tags`: as for `DGProblem`; `ion_names`: the K ions in the
        problem's order, the eliminated one last."""
        if mesh.cell_type not in _FACET_TYPE:
            raise ValueError("the DG variant is built for triangles, tetrahedra and hexahedra")
        self.mesh = mesh
        self.cell_type = mesh.cell_type
        self.cell_sub = cell_subdomains(ct, subdomain_tags)
        self.mem_facets, self.mem_tags = membrane_facets(mesh, ft, membrane_tags)
        self.subdomain_tags = list(subdomain_tags)
        self.membrane_tags = [t for t in membrane_tags if np.any(self.mem_tags == t)]
        self.ion_names = list(ion_names)
        self.K = len(self.ion_names)
        if not 2 <= self.K <= L.MAX_IONS:
            raise ValueError("2 to 4 ionic species are supported")
        if len(self.membrane_tags) > 8:
            raise ValueError("at most 8 membrane tags")
        x = np.asarray(mesh.x, np.float64)
        self.cells_v = np.asarray(mesh.cells, np.int64)
        self.n_cells, self.nv = self.cells_v.shape
        self.nmf, self.nf = self.mem_facets.shape
        self.X = x[self.cells_v]                                      # (n_cells, nv, d)
        self.XM = x[self.mem_facets]                                  # (nmf, nf, d)
        self.gdim = self.X.shape[2]
        index = {t: i for i, t in enumerate(self.membrane_tags)}
        self.facet_tag = np.array([index[t] for t in self.mem_tags], np.int32)
        self._init_series()
        self._topo = self._W = None
        self._dp = None
        self._want_cells = True

    # -- the row ------------------------------------------------------------------------------------------------
    def columns(self):
        out = [(f"{s}/{ion}/{c}", 1) for s in self.subdomain_tags for ion in self.ion_names for c in SUB_COLUMNS]
        for t in self.membrane_tags:
            out += [(f"{t}/{ion}/ecs", 1) for ion in self.ion_names] + [(f"{t}/{ion}/ics", 1) for ion in self.ion_names]
            out += [(f"{t}/capacitive", 1), (f"{t}/channel", 1), (f"{t}/area", 1)]
        return out

    @property
    def topology(self):
        if self._topo is None:
            self._topo = DGTopology(self.cells_v, self.cell_type, self.cell_sub, self.mem_facets)
        return self._topo

    @property
    def weights(self):
        """(n_cells, nv) integrals of the basis functions over their cells."""
        if self._W is None:
            self._W = element_integral_weights(self.X, self.cell_type)
        return self._W

    # -- the device ---------------------------------------------------------------------------------------------
    def _attach(self, dp, capacity, want_cells=True):
        if self._dp is not None:
            raise RuntimeError("this balance is attached to a problem already")
        if dp.n_cells != self.n_cells or dp.nv != self.nv or dp.nmf != self.nmf or dp.K != self.K:
            raise ValueError("this balance was defined on another mesh or for another number of ions")
        ftag = self.facet_tag if self.nmf else np.zeros(1, np.int32)
        L.check(dp.lib.knpemi_dg_balance_set(dp.h, int(capacity), int(bool(want_cells)), len(self.membrane_tags), L.iptr(ftag)))
        self._dp, self._want_cells = dp, bool(want_cells)

    def cells(self):
        """{"mem", "cons", "pen", "drift", "m_old", "m_new", "src", "defect"}: (n_cells, K) arrays of the last record
        (one synchronisation); src and defect are zero for the eliminated ion."""
        if self._dp is None:
            raise RuntimeError("cells(): not attached to a problem (DGProblem.balance); evaluate_host evaluates host data")
        buf = np.empty((self.n_cells, self.K, len(CELL_COLUMNS)))
        L.check(self._dp.lib.knpemi_dg_balance_cells(self._dp.h, L.dptr(buf)))
        return {c: buf[:, :, j].copy() for j, c in enumerate(CELL_COLUMNS)}

    def current(self, cells=None, F=None, z=None):
        """F sum_k z_k out_T,k per cell (n_cells,): the charge leaving the cell through its interior facets per unit time.
        `cells`: a table of `cells()` / `evaluate_host` (default: the last record's); F, z: default the attached problem's
        (`DGProblem.set_params`)."""
        cells = self.cells() if cells is None else cells
        if F is None or z is None:
            if self._dp is None or self._dp.ion_params is None:
                raise RuntimeError("current(): F and z are needed (not attached, or DGProblem.set_params has not been called)")
            F, z = self._dp.ion_params
        out = cells["cons"] + cells["pen"] + cells["drift"]
        return float(F) * out @ np.asarray(z, np.float64)

    # -- host restatement -----------------------------------------------------------------------------------------
    def _fields(self, fs):
        return [np.asarray(f, np.float64).reshape(self.n_cells, self.nv) for f in fs]

    def _interior_points(self):
        """Per interior facet (cT < cN) and point of the facet rule: weight times measure (m, q), T's outward unit normal
        (m, q, d), 1 / h_F (m, q), and of both cells the basis values (m, q, nv) and physical gradients (m, q, nv, d) --
        every one through the cell's own map."""
        topo = self.topology
        cT, cN, lT, lN = topo.cT, topo.cN, topo.lT, topo.lN
        X, nv, d = self.X, self.nv, self.gdim
        if self.cell_type != "hexahedron":
            # affine maps: lambda_j(x) = a0[j] + G[j] . x
            M = np.concatenate([np.ones((self.n_cells, nv, 1)), X], axis=2)
            Minv = np.linalg.inv(M)
            a0, G = Minv[:, 0, :], np.transpose(Minv[:, 1:, :], (0, 2, 1))
            P = np.take_along_axis(X[cT], lT[:, :, None], axis=1)      # (m, nf, d)
            if d == 2:
                fphi = np.stack([1.0 - _G2, _G2], axis=1)
                wq = np.full(2, 0.5)[None, :] * np.linalg.norm(P[:, 1] - P[:, 0], axis=1)[:, None]
            else:
                fphi = np.array([[2 / 3, 1 / 6, 1 / 6], [1 / 6, 2 / 3, 1 / 6], [1 / 6, 1 / 6, 2 / 3]])      # degree 2
                area = 0.5 * np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)
                wq = np.full(3, 1 / 3)[None, :] * area[:, None]
            Xq = np.einsum("qa,mad->mqd", fphi, P)
            nq = Xq.shape[1]
            lam = [a0[c][:, None, :] + np.einsum("mjd,mqd->mqj", G[c], Xq) for c in (cT, cN)]
            grad = [np.repeat(G[c][:, None], nq, axis=1) for c in (cT, cN)]
            gT, gN = G[cT, topo.fT], G[cN, topo.fN]
            nT = -gT / np.linalg.norm(gT, axis=1)[:, None]
            inv_h = 0.5 * (np.linalg.norm(gT, axis=1) + np.linalg.norm(gN, axis=1))
            return wq, np.repeat(nT[:, None], nq, axis=1), np.repeat(inv_h[:, None], nq, axis=1), lam, grad
        st = np.array([[_G2[p & 1], _G2[p >> 1]] for p in range(4)])
        Nf, _ = _tensor_shape(st)                                      # (q, 4): the facet's shape functions in T's positions
        lam, grad, gxi, J = [], [], [], []
        for c, l, f in ((cT, lT, topo.fT), (cN, lN, topo.fN)):
            xi = np.einsum("qa,mad->mqd", Nf, _hex_ref(l))            # the points in the cell's own reference coordinates
            N, G, Jc = self._hex_geom(c, xi)
            lam.append(N)
            grad.append(G)
            J.append(Jc)
            ax = f // 2
            refa = np.array([[(j >> a) & 1 for j in range(8)] for a in range(3)], np.float64)
            gxi.append(np.einsum("mj,mqjd->mqd", refa[ax], G))        # grad xi_normal
        axT = topo.fT // 2
        sd = np.where(topo.fT % 2 == 1, 1.0, -1.0)
        t = [np.stack([J[0][k, :, :, a] for k, a in enumerate(np.where(axT == 0, 1, 0))]),
             np.stack([J[0][k, :, :, a] for k, a in enumerate(np.where(axT == 2, 1, 2))])]
        area = np.linalg.norm(np.cross(t[0], t[1]), axis=2)
        ghT, ghN = np.linalg.norm(gxi[0], axis=2), np.linalg.norm(gxi[1], axis=2)
        nT = sd[:, None, None] * gxi[0] / ghT[:, :, None]
        return 0.25 * area, nT, 0.5 * (ghT + ghN), lam, grad

    def _hex_geom(self, c, xi):
        """Cells c (m,), reference points xi (m, q, 3): basis (m, q, 8), physical gradients (m, q, 8, 3), Jacobians
        J[m, q, g, t] = d x_g / d xi_t."""
        m, q = xi.shape[:2]
        N, dN = _tensor_shape(xi.reshape(m * q, 3))
        N, dN = N.reshape(m, q, 8), dN.reshape(m, q, 8, 3)
        J = np.einsum("mjg,mqjt->mqgt", self.X[c], dN)
        G = np.einsum("mqjt,mqtg->mqjg", dN, np.linalg.inv(J))
        return N, G, J

    def outflow_host(self, params, ions, c_all, phi, gamma):
        """(cons, pen, drift), each (n_cells, K): the three parts of the outflow of every ion through the interior facets
        of every cell, for the concentrations c_all (K fields) and the potential phi."""
        K = self.K
        c_all, (phi,) = self._fields(c_all), self._fields([phi])
        out = np.zeros((3, self.n_cells, K))
        topo = self.topology
        if topo.cT.size == 0:
            return out[0], out[1], out[2]
        cT, cN = topo.cT, topo.cN
        w, n, inv_h, lam, grad = self._interior_points()
        gn = [np.einsum("mqjd,mqd->mqj", g, n) for g in grad]         # normal derivatives of the basis functions
        s = self.cell_sub[cT]
        psi = float(getattr(params["psi"], "value", params["psi"]))
        gp = [np.einsum("mqj,mj->mq", gn[i], phi[c]) for i, c in enumerate((cT, cN))]
        for k, ion in enumerate(ions):
            D = np.asarray([float(ion["D"][i]) for i in range(len(self.subdomain_tags))])
            DT, DN, z = D[s][:, None], D[self.cell_sub[cN]][:, None], float(ion["z"])
            u = c_all[k]
            gc = [np.einsum("mqj,mj->mq", gn[i], u[c]) for i, c in enumerate((cT, cN))]
            tr = [np.einsum("mqj,mj->mq", lam[i], u[c]) for i, c in enumerate((cT, cN))]
            cons = -np.sum(w * 0.5 * (DT * gc[0] + DN * gc[1]), axis=1)
            pen = np.sum(w * gamma * inv_h * 0.5 * (DT + DN) * (tr[0] - tr[1]), axis=1)
            beta = -z * psi * 0.5 * (DT * gp[0] + DN * gp[1])
            drift = np.sum(w * beta * np.where(beta > 0, tr[0], tr[1]), axis=1)
            for j, v in enumerate((cons, pen, drift)):                # antisymmetric: what leaves T enters N
                np.add.at(out[j, :, k], cT, v)
                np.add.at(out[j, :, k], cN, -v)
        return out[0], out[1], out[2]

    def membrane_host(self, params, ions, c_old, phi, phi_M, I_ch, splitting_scheme=True):
        """(mem (n_cells, K), tags (n_tags, 2 K + 3)): the membrane transfer into every cell and per membrane tag the
        integrals of j_k^e (K), j_k^i (K), I_cap, I_ch,tot and the area -- the degree-6 facet rule, the traces through
        the adjacent cells' own maps."""
        K = self.K
        val = lambda v: float(getattr(v, "value", v))
        F, C_M, dt = val(params["F"]), val(params["C_M"]), val(params["dt"])
        mem = np.zeros((self.n_cells, K))
        tags = np.zeros((len(self.membrane_tags), 2 * K + 3))
        if self.nmf == 0:
            return mem, tags
        c_old, (phi,) = self._fields(c_old), self._fields([phi])
        phi_M = np.asarray(phi_M, np.float64).reshape(self.nmf, self.nf)
        I_ch = [np.asarray(i, np.float64).reshape(self.nmf, self.nf) for i in I_ch]
        wts, Nf, dN = facet_rule(self.nf)
        wq = facet_weights(self.XM, wts, dN)                           # (nmf, q)
        topo = self.topology
        sides = []
        for dofs in (topo.dof_e, topo.dof_i):
            c, loc = dofs[:, 0] // self.nv, dofs % self.nv
            if self.cell_type == "hexahedron":
                lam = self._hex_geom(c, np.einsum("qa,mad->mqd", Nf, _hex_ref(loc)))[0]
            else:
                M = np.concatenate([np.ones((len(c), self.nv, 1)), self.X[c]], axis=2)
                Minv = np.linalg.inv(M)
                Xq = np.einsum("qa,mad->mqd", Nf, self.XM)
                lam = Minv[:, 0, :][:, None, :] + np.einsum("mdj,mqd->mqj", Minv[:, 1:, :], Xq)
            sides.append((c, lam))
        at = lambda u, side: np.einsum("mqj,mj->mq", side[1], u[side[0]])
        pm = np.einsum("qa,ma->mq", Nf, phi_M)
        Iq = [np.einsum("qa,ma->mq", Nf, i) for i in I_ch]
        It = sum(Iq)
        icap = C_M * ((at(phi, sides[1]) - at(phi, sides[0])) - pm) / dt
        drive = icap - It if splitting_scheme else icap
        nsub = len(self.subdomain_tags)
        asum = [sum(np.asarray([float(ion["D"][i]) for i in range(nsub)])[self.cell_sub[sd[0]]][:, None] * float(ion["z"]) ** 2
                    * at(c_old[k], sd) for k, ion in enumerate(ions)) for sd in sides]
        for k, ion in enumerate(ions):
            z = float(ion["z"])
            D = np.asarray([float(ion["D"][i]) for i in range(nsub)])
            for side, (sd, sign) in enumerate(zip(sides, (1.0, -1.0))):
                alpha = D[self.cell_sub[sd[0]]][:, None] * z * z * at(c_old[k], sd) / asum[side]
                j = np.sum(wq * (Iq[k] + alpha * drive), axis=1) / (F * z)      # per facet, out of the intracellular cell
                np.add.at(mem[:, k], sd[0], sign * j)
                np.add.at(tags[:, side * K + k], self.facet_tag, j)
        for col, v in enumerate((icap, It, np.ones_like(It))):
            np.add.at(tags[:, 2 * K + col], self.facet_tag, np.sum(wq * v, axis=1))
        return mem, tags

    def evaluate_host(self, params, ions, c_old, c_new, phi, phi_M, I_ch, gamma=10.0, splitting_scheme=True, f_source=None):
        """(cells, row) of one recorded step with numpy.  c_old: the K concentration fields (n_cells, nv) the membrane
        launch sees (before the solve), c_new: those the record sees (after the update), phi the potential of the step,
        phi_M (nmf, nf) the membrane potential of the previous step, I_ch the K channel currents (nmf, nf); f_source:
        {solved ion: (n_cells, nv)} or None.  `cells`: the table of `cells()`; `row`: the series row as a flat array in
        the order of `columns()`."""
        K, W = self.K, self.weights
        val = lambda v: float(getattr(v, "value", v))
        dt = val(params["dt"])
        c_old, c_new = self._fields(c_old), self._fields(c_new)
        cons, pen, drift = self.outflow_host(params, ions, c_new, phi, gamma)
        mem, tags = self.membrane_host(params, ions, c_old, phi, phi_M, I_ch, splitting_scheme)
        m_old = np.stack([np.sum(W * c, axis=1) for c in c_old], axis=1)
        m_new = np.stack([np.sum(W * c, axis=1) for c in c_new], axis=1)
        src = np.zeros((self.n_cells, K))
        for k, f in (f_source or {}).items():
            f = np.asarray(f, np.float64).reshape(self.n_cells, self.nv)
            src[:, k] = np.where(self.cell_sub == 0, np.sum(W * f, axis=1), 0.0)
        defect = (m_new - m_old) / dt + cons + pen + drift - mem - src
        defect[:, K - 1] = 0.0                                         # the eliminated ion has no equation
        cells = dict(mem=mem, cons=cons, pen=pen, drift=drift, m_old=m_old, m_new=m_new, src=src, defect=defect)
        return cells, self.row_of(cells, tags)

    def row_of(self, cells, tags):
        """The series row (flat, in the order of `columns()`) of a cell table and the membrane tags' sums (n_tags, 2 K + 3)."""
        row = []
        out = cells["cons"] + cells["pen"] + cells["drift"]
        for s in range(len(self.subdomain_tags)):
            sel = self.cell_sub == s
            for k in range(self.K):
                row += [cells["m_new"][sel, k].sum(), out[sel, k].sum(), np.abs(cells["pen"][sel, k]).sum(),
                        np.abs(cells["defect"][sel, k]).max(initial=0.0)]
        return np.concatenate([np.array(row, np.float64), np.asarray(tags, np.float64).ravel()])

    def save(self, path):
        """.npz of `series()` and, attached with the cell table and after a record, of the last `cells()` as "cells/<column>"."""
        out = self.series()
        if self._dp is not None and self._want_cells and len(out["t"]):
            out.update({f"cells/{k}": v for k, v in self.cells().items()})
        np.savez(path, **out)
