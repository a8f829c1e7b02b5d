"""Field snapshots of a DG run (knpemi.dg.DGProblem): broken, cell-mean and vertex-averaged frames.

The machinery is that of `knpemi.snapshots`: every `every`-th record ONE launch packs the watched fields
into a contiguous frame on the device (csrc/kernels_dg_snapshot.hip), a copy stream takes the frame to pinned host memory,
and a writer thread hands it to the sinks -- the ring, the writer and the sinks are that module's, imported.  What is new
is the FORM of a watch, because a DG field is broken: a mesh vertex carries one dof per cell that touches it.

    snap = DGSnapshots(mesh, ct, ft, [0, 1], [1], ["K", "Cl", "Na"], sink=NpzSink(outdir))
    snap.watch_results()                                   # phi, every ion per sub-domain, phi_M per membrane tag: "vertex"
    snap.watch("K_jumps", "c", 0, ion="K", form="broken")
    snap.watch("m", "state", 1, state=0, dtype="f4")       # a column of the bound ODE table, per membrane node
    snap.select(0, "vertex", box=(lo, hi))
    dp.snapshot(snap, every=5, depth=4)                    # ... dp.update(c); dp.record(t) ...
    snap.flush(); snap.close()

Forms of a bulk quantity ("phi", or "c" of any ion, the eliminated one included) over the cells of sub-domain `tag`:

  "broken"     one value per dof (cell, local vertex), in the cell order of the sub-domain: the field as it is, jumps and all;
  "cell_mean"  one value per cell: the nodal values summed in local-vertex order 0 .. nv - 1 and divided by nv.  This is the
               NODAL mean.  It is the integral mean of the broken P1 / Q1 function on simplices and on parallelepiped
               hexahedra (where the basis functions have equal integrals); on a general trilinear hexahedron it is not;
  "vertex"     one value per mesh vertex the sub-domain's cells touch, in increasing vertex id: the coincident broken dofs
               summed in increasing dof order and divided by their number -- the layout of the reference's
               `results_sub_<tag>.xdmf` (run_stim_duration.py:52-90), and what a comparison with a conforming run wants.

Membrane quantities ("phi_M", "I_ch" of an ion, "state": a column of the bound ODE table) over the facets tagged with
membrane tag `tag`: "broken" is one value per membrane node (facet, a), "vertex" the mean over the nodes of that tag that
share a mesh vertex, by the same ordering rule (`results_mem_<tag>.xdmf`).

Arithmetic: a sum starts from its first entry, then additions in list order, then one IEEE double division by the count
("broken" divides by nothing); "f4" stores `np.float32(v)`.  `frame_host` restates exactly this in numpy, so a device
frame equals it bit for bit.

A space is (sub-domain or membrane tag, form); a selection belongs to a space and every watch of the space then stores
only the selected items.  The class is constructible without a GPU and without the library.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L
from .dg import cell_subdomains, membrane_facets
# the ring's host side and the writer (`_Writer`, through `Snapshots._open`) are inherited; the sinks are re-exported
from .snapshots import DTYPES, MemorySink, NpzSink, Snapshots, _Nodal      # noqa: F401

QUANTITIES = ("phi", "c", "phi_M", "I_ch", "state")
MEMBRANE = ("phi_M", "I_ch", "state")
FORMS = {"broken": L.DG_SNAP_BROKEN, "cell_mean": L.DG_SNAP_CELL_MEAN, "vertex": L.DG_SNAP_VERTEX}
_FACET_TYPE = {"triangle": "interval", "tetrahedron": "triangle", "hexahedron": "quadrilateral"}


class _Watch:
    __slots__ = ("name", "quantity", "tag", "ion", "state", "form", "dtype")

    @property
    def membrane(self):
        return self.quantity in MEMBRANE

    @property
    def space(self):
        return (self.membrane, self.tag, self.form)


class _Space:
    """The items of a space.  src: the dofs / nodes ("broken") or the cells ("cell_mean"); vptr, vdof: the incidence list
    ("vertex"); x: the coordinates of the items; ids: cells, mesh vertices or (dofs, nodes) the items are."""
    __slots__ = ("form", "n", "src", "vptr", "vdof", "x", "ids")


def ordered_sum(v, ptr, idx):
    """sum_j v[idx[ptr[i] + j]] for every i, the entries added one at a time in list order starting from the first -- the
    order of the device, so the doubles agree bit for bit."""
    cnt = np.diff(ptr)
    first = ptr[:-1]
    s = v[idx[first]].copy()
    for j in range(1, int(cnt.max()) if cnt.size else 0):
        m = cnt > j
        s[m] = s[m] + v[idx[first[m] + j]]
    return s, cnt


def _incidence(vids, entries):
    """(items, vptr, vdof): the distinct ids in increasing order and, per id, its entries in increasing order."""
    order = np.lexsort((entries, vids))
    items, counts = np.unique(vids, return_counts=True)
    vptr = np.zeros(items.shape[0] + 1, np.int32)
    np.cumsum(counts, out=vptr[1:])
    return items, vptr, np.ascontiguousarray(entries[order], np.int32)


class DGSnapshots(Snapshots):
    _ABI = "knpemi_dg_snapshot_"

    def __init__(self, mesh, ct, ft, subdomain_tags, membrane_tags, ion_names, sink=None, writer="thread"):
        """`mesh`, `ct`, `ft`, `subdomain_tags`, `membrane_tags`: as for `DGProblem`; `ion_names`: the K ions in the
        problem's order, the eliminated one last.  sink, writer: as for `knpemi.snapshots.Snapshots`."""
        if mesh.cell_type not in _FACET_TYPE:
            raise ValueError("the DG variant is built for triangles, tetrahedra and hexahedra")
        Snapshots.__init__(self, mesh, ct, ft, {}, [dict(name=n) for n in ion_names], sink=sink, writer=writer)
        self.cell_type, self.facet_type = mesh.cell_type, _FACET_TYPE[mesh.cell_type]
        self.subdomain_tags, self.membrane_tags = list(subdomain_tags), list(membrane_tags)
        self.sub_index = {t: s for s, t in enumerate(self.subdomain_tags)}
        self.mem_index = {t: s for s, t in enumerate(self.membrane_tags)}
        self.cell_sub = cell_subdomains(ct, subdomain_tags)
        self.mem_facets, self.mem_tags = membrane_facets(mesh, ft, membrane_tags)
        self.x = np.asarray(mesh.x, np.float64)
        self.cells = np.asarray(mesh.cells, np.int64)
        self.n_cells, self.nv = self.cells.shape
        self.nmf, self.nf = self.mem_facets.shape
        self.n, self.nq = self.n_cells * self.nv, self.nmf * self.nf
        self.K = len(self.ion_names)
        self._spaces = {}

    # -- spaces ------------------------------------------------------------------------------------------
    def space(self, tag, form, membrane=False):
        """The `_Space` of (sub-domain `tag`, form), or with membrane=True of (membrane tag `tag`, form)."""
        key = (bool(membrane), tag, form)
        if key in self._spaces:
            return self._spaces[key]
        if form not in FORMS:
            raise ValueError(f"form must be one of {tuple(FORMS)}")
        S = _Space()
        S.form = form
        if membrane:
            if tag not in self.mem_index or not np.any(self.mem_tags == tag):
                raise ValueError(f"no membrane facet with tag {tag}")
            if form == "cell_mean":
                raise ValueError("a membrane quantity has no 'cell_mean' form: 'broken' (per membrane node) or 'vertex'")
            ent = np.flatnonzero(self.mem_tags == tag)
            per, verts = self.nf, np.asarray(self.mem_facets, np.int64)[ent]
        else:
            if tag not in self.sub_index:
                raise ValueError(f"no sub-domain with tag {tag}")
            ent = np.flatnonzero(self.cell_sub == self.sub_index[tag])
            if ent.size == 0:
                raise ValueError(f"sub-domain {tag} has no cells")
            per, verts = self.nv, self.cells[ent]
        dofs = (ent[:, None] * per + np.arange(per)[None, :]).ravel()
        S.src = S.vptr = S.vdof = None
        if form == "broken":
            S.src, S.ids, S.x = np.ascontiguousarray(dofs, np.int32), dofs, self.x[verts].reshape(dofs.shape[0], -1)
        elif form == "cell_mean":
            S.src, S.ids, S.x = np.ascontiguousarray(ent, np.int32), ent, self.x[verts].mean(axis=1)
        else:
            S.ids, S.vptr, S.vdof = _incidence(verts.ravel(), dofs)
            S.x = self.x[S.ids]
        S.n = int(S.ids.shape[0])
        self._spaces[key] = S
        return S

    # -- definition --------------------------------------------------------------------------------------
    def watch(self, name, quantity, tag, ion=None, state=None, form="broken", dtype="f8"):
        """Watch `quantity`: "phi" or "c" of `ion` (name or index) over sub-domain `tag`; "phi_M", "I_ch" of `ion` or
        "state" (column `state` of the bound ODE table) over the membrane tagged `tag`.  form: "broken", "cell_mean" (bulk
        only) or "vertex" (the module's docstring); dtype: "f8" stores the doubles, "f4" `np.float32` of them."""
        self._defining()
        if name in self.watches:
            raise ValueError(f"watch {name!r} defined twice")
        if quantity not in QUANTITIES:
            raise ValueError(f"quantity must be one of {QUANTITIES}")
        if dtype not in DTYPES:
            raise ValueError("dtype must be 'f8' or 'f4'")
        if len(self.watches) == L.SNAPSHOT_MAX_WATCH:
            raise ValueError(f"at most {L.SNAPSHOT_MAX_WATCH} watches")
        w = _Watch()
        w.name, w.quantity, w.tag, w.form, w.dtype = name, quantity, tag, form, dtype
        w.ion = w.state = None
        self.space(tag, form, w.membrane)                   # ValueError for an unknown tag or form
        if quantity in ("c", "I_ch"):
            k = self.ion_names.index(ion) if ion in self.ion_names else ion
            if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 0 <= k < self.K:
                raise ValueError(f"unknown ion {ion!r} (ions: {self.ion_names})")
            w.ion = int(k)
        if quantity == "state":
            if state is None or isinstance(state, bool) or not isinstance(state, (int, np.integer)) or state < 0:
                raise ValueError("a state watch needs state=: the column of the bound ODE table")
            w.state = int(state)
        for o in self.watches.values():
            if (o.quantity, o.tag, o.ion, o.state, o.form, o.dtype) == (quantity, tag, w.ion, w.state, form, dtype):
                raise ValueError(f"watch {name!r} repeats watch {o.name!r}")
        if len({o.space for o in self.watches.values()} | {w.space}) > L.DG_SNAPSHOT_MAX_SPACE:
            raise ValueError(f"at most {L.DG_SNAPSHOT_MAX_SPACE} spaces")
        self.watches[name] = w

    def watch_results(self, form="vertex", dtype="f8"):
        """phi_<tag> and <ion>_<tag> of every ion per sub-domain and phi_M_<tag> per membrane tag: with form="vertex" the
        functions of the reference's `results_sub_<tag>.xdmf` / `results_mem_<tag>.xdmf`.  phi_M has no "cell_mean": with
        that form it is stored per membrane node."""
        for tag in self.subdomain_tags:
            self.watch(f"phi_{tag}", "phi", tag, form=form, dtype=dtype)
            for name in self.ion_names:
                self.watch(f"{name}_{tag}", "c", tag, ion=name, form=form, dtype=dtype)
        for tag in self.membrane_tags:
            self.watch(f"phi_M_{tag}", "phi_M", tag, form="broken" if form == "cell_mean" else form, dtype=dtype)

    def select(self, tag, form, box=None, indices=None, membrane=False):
        """The selection of the space (sub-domain `tag`, form), or with membrane=True (membrane tag `tag`, form): every
        watch of the space stores only these items, in ascending order.  box=(lo, hi): the items whose coordinates
        (`locations`: the dof, the cell's vertex centroid, the mesh vertex) lie in the closed box; indices: ascending
        distinct item indices.  ValueError for an empty, unsorted, repeated or out-of-range selection and for a second
        selection of one space."""
        self._defining()
        S = self.space(tag, form, membrane)
        key = (bool(membrane), tag, form)
        if (box is None) == (indices is None):
            raise ValueError("give box=(lo, hi) or indices=")
        if key in self.selections:
            raise ValueError(f"the space (tag {tag}, form {form!r}, membrane={bool(membrane)}) has a selection already")
        if box is not None:
            lo, hi = (np.asarray(b, np.float64) for b in box)
            idx = np.flatnonzero(np.all((S.x >= lo) & (S.x <= hi), axis=1))
        else:
            idx = np.asarray(indices)
            if idx.ndim != 1 or (idx.size and not np.issubdtype(idx.dtype, np.integer)):
                raise ValueError("indices must be a list of integers")
        if idx.size == 0:
            raise ValueError("empty selection")
        if idx.min() < 0 or idx.max() >= S.n:
            raise ValueError(f"selection index out of range (the space has {S.n} items)")
        if np.any(np.diff(idx) <= 0):
            raise ValueError("selection indices must be ascending and distinct")
        self.selections[key] = np.ascontiguousarray(idx, np.int32)

    def _space_of(self, w):
        return self.space(w.tag, w.form, w.membrane)

    def _items(self, w):
        sel = self.selections.get(w.space)
        return np.arange(self._space_of(w).n, dtype=np.int32) if sel is None else sel

    def locations(self, name):
        """(n, gdim) coordinates of the stored items of watch `name`, in the order of its array: the dofs' (nodes')
        vertices ("broken"), the cells' vertex centroids ("cell_mean"), the mesh vertices ("vertex")."""
        w = self._check(name)
        return self._space_of(w).x[self._items(w)]

    def item_ids(self, name):
        """What the stored items of watch `name` are: broken dofs c * nv + j (membrane nodes f * nf + a), cells, or mesh
        vertices."""
        w = self._check(name)
        return np.asarray(self._space_of(w).ids, np.int64)[self._items(w)]

    def select_owned(self, halo):
        raise NotImplementedError("DGSnapshots: snapshots of a cell-partitioned DG run are not built")

    def global_ids(self, name, halo):
        raise NotImplementedError("DGSnapshots: snapshots of a cell-partitioned DG run are not built")

    # -- host restatement ----------------------------------------------------------------------------------
    def _source(self, w, phi, c, phi_M, I_ch, states):
        def need(a, what):
            if a is None:
                raise ValueError(f"watch {w.name!r} needs {what}")
            return a
        if w.quantity == "phi":
            v, n = need(phi, "phi"), self.n
        elif w.quantity == "c":
            v, n = need(c, "c")[w.ion], self.n
        elif w.quantity == "phi_M":
            v, n = need(phi_M, "phi_M"), self.nq
        elif w.quantity == "I_ch":
            v, n = need(I_ch, "I_ch")[w.ion], self.nq
        else:
            table = np.asarray(need(states, "states"), np.float64)
            if table.ndim != 2 or not w.state < table.shape[1]:
                raise ValueError(f"watch {w.name!r}: the state table has no column {w.state}")
            v, n = table[:, w.state], self.nq
        v = np.ascontiguousarray(v, np.float64).reshape(-1)
        if v.shape[0] != n:
            raise ValueError(f"watch {w.name!r}: {v.shape[0]} values for {n} dofs")
        return v

    def _reduce(self, S, v, per):
        if S.form == "broken":
            return v[S.src]
        with np.errstate(over="ignore", invalid="ignore"):
            if S.form == "cell_mean":
                ptr = np.arange(S.n + 1, dtype=np.int64) * per
                idx = (S.src.astype(np.int64)[:, None] * per + np.arange(per)[None, :]).ravel()
                s, cnt = ordered_sum(v, ptr, idx)
            else:
                s, cnt = ordered_sum(v, S.vptr.astype(np.int64), S.vdof)
            return s / cnt.astype(np.float64)

    def frame_host(self, phi=None, c=None, phi_M=None, I_ch=None, states=None):
        """{name: array} of every watch from host data, as the device packs it: phi (n_cells, nv), c the K concentration
        fields (the eliminated ion last), phi_M (nmf, nf), I_ch the K channel currents (nmf, nf), states the ODE table
        (membrane nodes, columns) -- what `get_potential`, `get_concentration(k)`, `get_membrane_potential`,
        `get_channel_current(k)` and `ode_tables()[0]` of a DGProblem return.  Only what a watch needs must be given.  The
        summation order is the device's."""
        out = {}
        for name, w in self.watches.items():
            S = self._space_of(w)
            v = self._reduce(S, self._source(w, phi, c, phi_M, I_ch, states), self.nf if w.membrane else self.nv)
            sel = self.selections.get(w.space)
            v = v.copy() if sel is None else v[sel]
            with np.errstate(over="ignore", invalid="ignore"):      # beyond the floats' range: +-inf, as the device stores
                out[name] = v.astype(np.float32) if w.dtype == "f4" else v
        return out

    def record_host(self, t, k, phi=None, c=None, phi_M=None, I_ch=None, states=None):
        """One frame at time t of record k from host data into the sinks, through the writer; returns the frame."""
        frame = self.frame_host(phi, c, phi_M, I_ch, states)
        self._open().put((float(t), int(k), frame))
        return frame

    def layout_host(self):
        """([(name, dtype, byte offset, items)], frame bytes) as knpemi_dg_snapshot_layout reports them: the watches in
        order, each at a multiple of KNPEMI_SNAPSHOT_ALIGN."""
        out, end = [], 0
        for name, w in self.watches.items():
            off = -(-end // L.SNAPSHOT_ALIGN) * L.SNAPSHOT_ALIGN
            n = int(self._items(w).shape[0])
            end = off + n * (4 if w.dtype == "f4" else 8)
            out.append((name, DTYPES[w.dtype], off, n))
        return out, max(-(-end // L.SNAPSHOT_ALIGN) * L.SNAPSHOT_ALIGN, L.SNAPSHOT_ALIGN)

    # -- the device table ----------------------------------------------------------------------------------
    def _quantity(self, w):
        return {"phi": (L.DG_PHI, 0), "c": (L.DG_C, w.ion), "phi_M": (L.DG_PHI_M, 0), "I_ch": (L.DG_I_CH, w.ion),
                "state": (L.DG_ODE_STATE, w.state)}[w.quantity]

    def table(self):
        """(spec [n][5], space [m][4], list_off [m + 1] int64, list, sel_space, sel_off int64, sel_idx) of
        knpemi_dg_snapshot_set: the watched spaces in the order of their first watch."""
        ws = list(self.watches.values())
        index = lambda w: (self.mem_index if w.membrane else self.sub_index)[w.tag]
        spec = np.array([[self._quantity(w)[0], index(w), self._quantity(w)[1], FORMS[w.form], L.SNAPSHOT_F32 if w.dtype == "f4" else 0]
                         for w in ws], np.int32).reshape(-1, 5)
        first = {}
        for w in ws:
            first.setdefault(w.space, w)
        space, lists = [], []
        for key, w in first.items():
            S = self._space_of(w)
            space.append([1 if w.membrane else 0, index(w), FORMS[w.form], S.n])
            lists.append(S.src if S.form != "vertex" else np.concatenate([S.vptr, S.vdof]).astype(np.int32))
        list_off = np.concatenate([[0], np.cumsum([len(a) for a in lists])]).astype(np.int64)
        keys = list(first)
        sel_keys = [k for k in keys if k in self.selections]
        sel_space = np.array([keys.index(k) for k in sel_keys], np.int32)
        sels = [self.selections[k] for k in sel_keys]
        sel_off = np.concatenate([[0], np.cumsum([len(a) for a in sels])]).astype(np.int64)
        sel_idx = np.ascontiguousarray(np.concatenate(sels) if sels else np.zeros(0), np.int32)
        return (spec, np.array(space, np.int32).reshape(-1, 4), list_off, np.ascontiguousarray(np.concatenate(lists), np.int32),
                sel_space, sel_off, sel_idx)

    def _attach(self, dp, depth):
        if self._dev is not None:
            raise RuntimeError("these snapshots are attached to a device problem already")
        if not self.watches:
            raise ValueError("nothing is watched")
        if depth < 1:
            raise ValueError("depth must be positive")
        if dp.n != self.n or dp.nmf != self.nmf or dp.K != self.K:
            raise ValueError("these snapshots were defined on another mesh or for another number of ions")
        spec, space, list_off, lst, sel_space, sel_off, sel_idx = self.table()
        n, m = spec.shape[0], len(sel_space)
        p64 = C.POINTER(C.c_int64)
        opened = self._w is None
        self._open(depth)
        try:
            L.check(dp.lib.knpemi_dg_snapshot_set(
                dp.h, n, L.iptr(spec.ravel()), space.shape[0], L.iptr(space.ravel()), list_off.ctypes.data_as(p64), L.iptr(lst),
                m, L.iptr(sel_space) if m else None, sel_off.ctypes.data_as(p64) if m else None,
                L.iptr(sel_idx) if m else None, int(depth)))
        except Exception:
            if opened:                  # a refused set leaves these snapshots as they were: defined, not attached
                self._w.close()
                self._w = None
            raise
        off, cnt, nbytes = np.zeros(n, np.int64), np.zeros(n, np.int64), C.c_int64()
        L.check(dp.lib.knpemi_dg_snapshot_layout(dp.h, off.ctypes.data_as(p64), cnt.ctypes.data_as(p64), C.byref(nbytes)))
        self._layout = ([(w.name, DTYPES[w.dtype], int(o), int(c)) for w, o, c in zip(self.watches.values(), off, cnt)],
                        int(nbytes.value))
        if self._layout != self.layout_host():
            raise RuntimeError("DGSnapshots: the device's frame layout is not the host's")
        self._dev, self.depth, self._drain = (dp.lib, dp.h), int(depth), self.flush
        self._ks, self.stalls = [], 0


# -- the XDMF sink ---------------------------------------------------------------------------------------------
class DGXdmfSink:
    """XDMF time series of the frames of a `DGSnapshots`, through `knpemi.fem.XDMFFile`:

      "vertex" watches   `results_sub_<tag>.xdmf` / `results_mem_<tag>.xdmf` -- the sub-mesh of the sub-domain (of the
                         membrane tag) with its vertices in increasing parent id, one temporal collection per watch, named
                         after it: the layout of the reference's files (run_stim_duration.py:52-90, 446-460);
      "broken" watches   `broken_sub_<tag>.xdmf` / `broken_mem_<tag>.xdmf` on the exploded mesh -- points
                         x[cells].reshape(-1, d), cells arange -- so a viewer shows the jumps.

    Needs unselected "f8" watches; a "cell_mean" watch has no nodal file (NpzSink keeps it): ValueError for either."""

    def __init__(self, snap, outdir):
        self.snap, self.outdir, self.files = snap, outdir, {}

    def _mesh(self, w):
        from .fem import Mesh
        snap = self.snap
        S = snap._space_of(w)
        cell_type = snap.facet_type if w.membrane else snap.cell_type
        per = snap.nf if w.membrane else snap.nv
        if w.form == "broken":
            return Mesh(S.x, np.arange(S.n, dtype=np.int32).reshape(-1, per), cell_type)
        ent = snap.mem_facets[snap.mem_tags == w.tag] if w.membrane else snap.cells[snap.cell_sub == snap.sub_index[w.tag]]
        return Mesh(S.x, np.searchsorted(S.ids, np.asarray(ent, np.int64)).astype(np.int32), cell_type)

    def check(self, snap):
        from .fem import XDMFFile
        if snap is not self.snap:
            raise ValueError("DGXdmfSink: made for other snapshots")
        for w in snap.watches.values():
            if w.form == "cell_mean":
                raise ValueError(f"DGXdmfSink: watch {w.name!r} is a cell mean; the XDMF series hold nodal functions")
            if w.dtype != "f8":
                raise ValueError(f"DGXdmfSink: watch {w.name!r} is stored as float32; the XDMF series needs 'f8'")
            if w.space in snap.selections:
                raise ValueError(f"DGXdmfSink: watch {w.name!r} stores a selection; the XDMF series needs every item")
        for w in snap.watches.values():
            if w.space not in self.files:
                stem = ("results" if w.form == "vertex" else "broken") + ("_mem_" if w.membrane else "_sub_") + str(w.tag)
                f = XDMFFile(None, os.path.join(self.outdir, stem + ".xdmf"), "w")
                f.write_mesh(self._mesh(w))
                self.files[w.space] = f

    def __call__(self, t, k, frame):
        for name, w in self.snap.watches.items():
            a = frame[name]
            n = self.snap._space_of(w).n
            if a.dtype != np.float64 or a.shape != (n,):
                raise ValueError(f"DGXdmfSink: watch {name!r} does not hold the {n} float64 values of its function")
            self.files[w.space].write_function(_Nodal(name, a), t)

    def close(self):
        for f in self.files.values():
            f.close()


def read_xdmf_series(path, name):
    """(times [n], values [n][items]) of the temporal collection `name` of an XDMF file written by `DGXdmfSink`, read back
    through `knpemi.fem.XDMFFile`."""
    from .fem import XDMFFile
    f = XDMFFile(None, path, "r")
    try:
        times, values = [], []
        for coll in f._tree.getroot().iter("Grid"):
            if coll.get("Name") == name and coll.get("GridType") == "Collection":
                for g in coll.findall("Grid"):
                    times.append(float(g.find("Time").get("Value")))
                    values.append(np.asarray(f._item(g.find("Attribute")), np.float64).reshape(-1))
        if not times:
            raise KeyError(f"{path}: no temporal collection named {name!r}")
        return np.array(times), np.array(values)
    finally:
        f.close()
