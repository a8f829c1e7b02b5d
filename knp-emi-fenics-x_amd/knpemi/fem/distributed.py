"""Cell partition of an arbitrary mesh over the GPUs of a node, id-keyed halos and distributed linear solves.

The reference lets DOLFINx partition whatever mesh it reads -- the structured boxes as well as the unstructured emimesh
tetrahedra of `examples/local_astrocyte_depolarization/run_stim_duration.py:127-134` -- with
`GhostMode.shared_facet`, updates ghosts with `Function.x.scatter_forward()` and runs its KSP solves on the mesh's
communicator (`src/knpemi/pdeSolver.py:24-35,74-78,99-110`).  Here:

* cells are partitioned by recursive coordinate bisection of their centroids (`rcb_partition`; `slab_partition`
  cuts whole layers along one axis), a vertex belongs to the lowest rank among its cells, and a rank keeps every cell
  that touches a vertex it owns -- so all rows of owned vertices are assembled locally (owner-computes, no matrix
  communication) with the cells in their global order (bit-identical rows);
* `VertexHalo` is the forward halo (owner -> ghost) of the dof fields, keyed by (sub-domain, global vertex id);
* `Halo.enable_solves` hands the library the ownership mask and the two communication steps of a distributed Krylov
  solve (all-reduce of the dot products, halo of a solver vector), both stream-ordered `torch.distributed` calls
  (backend "nccl" = RCCL over xGMI; "gloo" for CPU tests and one-card rehearsals).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .. import _lib as L
from ..recording import gather_objects
from .mesh import MeshTags, extract_submesh, match_facets
from .transport import Transport, cg_endpoint


# ---------------------------------------------------------------------------------------------------------------
# cell partitions
# ---------------------------------------------------------------------------------------------------------------
def rcb_partition(centroids, world):
    """Recursive coordinate bisection: split along the longest axis of the bounding box, proportionally to the
    number of ranks on either side.  Deterministic (ties by cell index)."""
    part = np.zeros(centroids.shape[0], np.int32)

    def split(ids, r0, n):
        if n == 1:
            part[ids] = r0
            return
        x = centroids[ids]
        axis = int(np.argmax(x.max(axis=0) - x.min(axis=0)))
        order = ids[np.lexsort((ids, x[:, axis]))]
        nl = n // 2
        cut = (len(order) * nl) // n
        split(order[:cut], r0, nl)
        split(order[cut:], r0 + nl, n - nl)
    split(np.arange(centroids.shape[0]), 0, world)
    return part


def slab_partition(centroids, world, axis=0):
    """Whole layers of cells along `axis`, as equal as the layer structure allows (the x-slabs of the idealized
    boxes: 2 neighbours per rank, every axon cross-section on one GPU)."""
    x = np.round(centroids[:, axis] / (np.ptp(centroids[:, axis]) + 1e-300) * 1e9).astype(np.int64)
    layers, inv = np.unique(x, return_inverse=True)
    if len(layers) < world:
        raise ValueError("fewer cell layers than ranks")
    cuts = [(len(layers) * r) // world for r in range(world + 1)]
    layer_rank = np.zeros(len(layers), np.int32)
    for r in range(world):
        layer_rank[cuts[r]:cuts[r + 1]] = r
    return layer_rank[inv]


class LocalPart:
    """One rank's share of a partitioned mesh."""

    def __init__(self, mesh, ct, ft, part, rank, world):
        nvpc = mesh.cells.shape[1]
        owner = np.full(mesh.num_vertices, world, np.int32)
        np.minimum.at(owner, mesh.cells.ravel(), np.repeat(part.astype(np.int32), nvpc))
        own_v = owner == rank
        local_cells = np.flatnonzero(own_v[mesh.cells].any(axis=1)).astype(np.int32)
        marker = MeshTags(mesh, mesh.tdim, local_cells, np.ones(len(local_cells), np.int32))
        sub, emap, vmap, _, _ = extract_submesh(mesh, marker, 1)
        self.mesh = sub
        if getattr(mesh, "uniform_cell", None) is not None:
            sub.uniform_cell = mesh.uniform_cell          # cells of a uniform grid stay cells of that grid: the same bits on every rank
        self.rank, self.world = rank, world
        self.cell_global = local_cells
        self.vert_global = vmap.sub_to_parent.astype(np.int64)     # ascending
        self.vert_owner = owner[self.vert_global]
        self.ct = MeshTags(sub, sub.tdim, np.arange(sub.num_cells, dtype=np.int32), ct.dense()[local_cells])
        self.ct.name = getattr(ct, "name", "cell_marker")
        # facet tags: those of the matching global facets, except on facets that are interior globally but lie on
        # the boundary of the local mesh (no vertex of such a facet is owned here, so no owned row needs it -- and a
        # membrane facet must see both of its cells)
        pf = match_facets(mesh, sub, vmap)
        dense = ft.dense(fill=-1)
        tag = np.where(pf >= 0, dense[np.clip(pf, 0, None)], -1)
        sub._build_facets()
        mesh._build_facets()
        cut = (sub._facets["counts"] == 1) & (pf >= 0) & (mesh._facets["counts"][np.clip(pf, 0, None)] == 2)
        tag[cut] = -1
        keep = np.flatnonzero(tag >= 0).astype(np.int32)
        self.ft = MeshTags(sub, sub.tdim - 1, keep, tag[keep])
        self.ft.name = getattr(ft, "name", "facet_marker")


# ---------------------------------------------------------------------------------------------------------------
# halos
# ---------------------------------------------------------------------------------------------------------------
class Halo:
    """Forward (owner -> ghost) halo of one rank.  `plans[kind]` (kind in {'bulk', 'mem'}) maps a label to
    dict(nb=neighbour rank, send=index array, recv=index array) in the global device numbering of the DeviceProblem
    (vertex ids across sub-meshes, Q-dof ids).  What is exchanged is decided here (the plans, the pack / unpack kernels,
    the hooks of the distributed solves); how the packed buffers move between the ranks is the business of `transport`
    (`knpemi.fem.transport.Transport`, bound to the CG handle in `attach`), which also owns the exchange `mode`."""

    supports_solves = False

    def __init__(self):
        self.plans = None
        self.dp = None
        self.transport = None
        self._dev = None
        self.rank = None            # this rank (set by the subclasses)
        self.n_local = None         # {"bulk": local vertex ids, "mem": local membrane dofs} of the device numbering
        self._hook_error = None

    @property
    def mode(self):
        return "not attached" if self.transport is None else self.transport.mode

    @property
    def library_comm(self):
        """The exchange runs on the library's own communicator (which then also sums the recorders' rank slots)."""
        return self.transport is not None and self.transport.library

    # -- host exchange (CPU tests, Vector.scatter_forward): `arr` = [n_global_ids, width] array ------------------
    def forward_host_array(self, kind, arr, dist):
        import torch
        ops, bufs = [], []
        for pl in self.plans[kind].values():
            sb = torch.from_numpy(np.ascontiguousarray(arr[pl["send"]]))
            rb = torch.empty((len(pl["recv"]),) + arr.shape[1:], dtype=torch.float64)
            ops += [dist.P2POp(dist.isend, sb, pl["nb"]), dist.P2POp(dist.irecv, rb, pl["nb"])]
            bufs.append((pl, rb, sb))
        if ops:
            for req in dist.batch_isend_irecv(ops):
                req.wait()
        for pl, rb, _ in bufs:
            arr[pl["recv"]] = rb.numpy()

    # -- device exchange ---------------------------------------------------------------------------------------
    def attach(self, dp):
        self.dp = dp
        self.transport = Transport(cg_endpoint(dp), self)
        self.transport.negotiate()
        self._dev = {}
        for k, kind in enumerate(("bulk", "mem")):
            self._dev[kind] = self.transport.plan(self.plans[kind], int(dp.lib.knpemi_halo_width(dp.h, k)))

    def _exchange(self, kind):
        dp = self.dp
        d = self._dev.get(kind)
        if d is None:
            return
        k = 0 if kind == "bulk" else 1
        L.check(dp.lib.knpemi_halo_pack(dp.h, k, d["send_idx"].data_ptr(), d["send_idx"].numel(),
                                        d["send_buf"].data_ptr()))
        self.transport.transfer(d)
        L.check(dp.lib.knpemi_halo_unpack(dp.h, k, d["recv_idx"].data_ptr(), d["recv_idx"].numel(),
                                          d["recv_buf"].data_ptr()))

    def exchange_bulk(self):
        self._exchange("bulk")

    def exchange_membrane(self):
        self._exchange("mem")

    # -- distributed linear solves ------------------------------------------------------------------------------
    def owned_mask(self):
        """One byte per local vertex (device numbering): 1 = owned.  Every ghost is received from its owner."""
        n = int(self.dp.n_vert.sum())
        own = np.ones(n, np.uint8)
        for pl in self.plans["bulk"].values():
            own[pl["recv"]] = 0
        return own

    def vertex_owner(self, kind="bulk"):
        """Owner rank of every local vertex ("bulk", device numbering) or membrane dof ("mem"), read off the plans
        without communication: an entry is owned here unless a neighbour sends it, and then that neighbour owns it."""
        own = np.full(self.n_local[kind], self.rank, np.int32)
        for pl in self.plans[kind].values():
            own[pl["recv"]] = pl["nb"]
        return own

    def enable_solves(self):
        """knpemi_solve_emi / knpemi_solve_knp on this handle become solves of the GLOBAL systems
        (knpemi_set_distributed): halo'd SpMV, all-reduced dot products, per-rank AMG (block Jacobi)."""
        dp, tr = self.dp, self.transport
        torch, dist, dev = tr.torch, tr.dist, tr.ep.device
        KS = dp.K - 1
        voff, nvs = dp.voff, dp.n_vert

        def knp_index(g):          # (vertex id) -> its KS entries in the block order [sub][ion][vertex]
            g = np.asarray(g, np.int64)
            s = np.searchsorted(voff[1:], g, side="right")
            base = KS * voff[s] + (g - voff[s])
            return np.concatenate([base + k * nvs[s] for k in range(KS)])
        # per neighbour the KS blocks must stay together in the packed buffer: the KNP plan is built from mapped indices
        mapped = {key: dict(nb=pl["nb"], send=knp_index(pl["send"]), recv=knp_index(pl["recv"]))
                  for key, pl in self.plans["bulk"].items()}
        self._vec = {L.B_EMI: tr.plan(self.plans["bulk"], 1), L.B_KNP: tr.plan(mapped, 1)}
        self._red = torch.zeros(8 + 64, dtype=torch.float64, device=dev)    # 8 scalars + the coarse vector
        self._hook_error = None
        own = np.ascontiguousarray(self.owned_mask())
        if tr.library:
            # the solves stay inside the library: its own all-reduce and vector halo are the hooks, the handle the context
            i64 = C.POINTER(C.c_int64)
            for which, d in self._vec.items():
                if d is None:
                    d = dict(send_idx=torch.zeros(0, dtype=torch.int32, device=dev),
                             recv_idx=torch.zeros(0, dtype=torch.int32, device=dev),
                             send_buf=torch.zeros(1, dtype=torch.float64, device=dev),
                             recv_buf=torch.zeros(1, dtype=torch.float64, device=dev),
                             peer=np.zeros(0, np.int32), send_off=np.zeros(0, np.int64), send_cnt=np.zeros(0, np.int64),
                             recv_off=np.zeros(0, np.int64), recv_cnt=np.zeros(0, np.int64))
                    self._vec[which] = d
                L.check(dp.lib.knpemi_comm_set_vector_plan(
                    dp.h, which, d["send_idx"].data_ptr(), d["send_idx"].numel(), d["recv_idx"].data_ptr(),
                    d["recv_idx"].numel(), d["send_buf"].data_ptr(), d["recv_buf"].data_ptr(), len(d["peer"]),
                    L.iptr(d["peer"]), d["send_off"].ctypes.data_as(i64), d["send_cnt"].ctypes.data_as(i64),
                    d["recv_off"].ctypes.data_as(i64), d["recv_cnt"].ctypes.data_as(i64)))
            hooks = (C.cast(dp.lib.knpemi_comm_allreduce_hook, C.c_void_p), C.cast(dp.lib.knpemi_comm_halo_hook, C.c_void_p))
            L.check(dp.lib.knpemi_set_distributed(dp.h, own.ctypes.data_as(L.c_u8_p), self._red.data_ptr(),
                                                  hooks[0], hooks[1], dp.h))
        else:
            self._cb = (self.allreduce_callback(self._red),                 # keep the callbacks alive
                        L.HALO_FN(tr.guarded(lambda ctx, vec, which: self._exchange_vector(vec, which))))
            L.check(dp.lib.knpemi_set_distributed(dp.h, own.ctypes.data_as(L.c_u8_p), self._red.data_ptr(),
                                                  C.cast(self._cb[0], C.c_void_p), C.cast(self._cb[1], C.c_void_p), None))
        if os.environ.get("KNPEMI_NO_COARSE") is None and dist.get_world_size() * len(dp.n_vert) <= 64:
            L.check(dp.lib.knpemi_set_distributed_coarse(dp.h, dist.get_rank(), dist.get_world_size()))
        self.supports_solves = True

    def allreduce_callback(self, buf):
        """knpemi_allreduce_fn summing the first n doubles of the device tensor `buf` over the ranks, as a C function
        pointer (keep the returned callback object alive); a failure is kept in `_hook_error`."""
        return L.ALLREDUCE_FN(self.transport.guarded(lambda ctx, n: self.transport.allreduce(n, buf)))

    def _exchange_vector(self, vec, which):
        dp = self.dp
        d = self._vec[which]
        if d is None:
            return
        L.check(dp.lib.knpemi_vec_gather(dp.h, vec, d["send_idx"].data_ptr(), d["send_idx"].numel(),
                                         d["send_buf"].data_ptr()))
        self.transport.transfer(d)
        L.check(dp.lib.knpemi_vec_scatter(dp.h, vec, d["recv_idx"].data_ptr(), d["recv_idx"].numel(),
                                          d["recv_buf"].data_ptr()))


class VertexHalo(Halo):
    """Halo of a general cell partition, keyed by (sub-domain index, global vertex id)."""

    def __init__(self, local: LocalPart, subdomain_list):
        super().__init__()
        self.local = local
        self.rank = local.rank
        self.keys = {"bulk": {}, "mem": {}}       # kind -> {s: (global ids ascending, owners, device offset)}
        off = qoff = 0
        self.owned_dofs = 0
        for s, (tag, sd) in enumerate(subdomain_list.items()):
            pv = sd["mesh_sub"].parent_vertices
            self.keys["bulk"][s] = (local.vert_global[pv], local.vert_owner[pv], off)
            off += len(pv)
            self.owned_dofs += int((local.vert_owner[pv] == local.rank).sum())
            if tag > 0:
                qv = sd["mesh_mem"].parent_vertices
                self.keys["mem"][s] = (local.vert_global[qv], local.vert_owner[qv], qoff)
                qoff += len(qv)
        self.n_local = {"bulk": off, "mem": qoff}

    def build(self, gather_objects):
        """`gather_objects(obj) -> [obj of rank 0, ..., obj of rank world-1]`."""
        rank = self.local.rank
        needs = {}
        for kind, subs in self.keys.items():
            for s, (gid, owner, _) in subs.items():
                for r in np.unique(owner[owner != rank]):
                    needs.setdefault(int(r), {}).setdefault(kind, {})[s] = gid[owner == r]
        all_needs = gather_objects(needs)
        plans = {"bulk": {}, "mem": {}}
        for kind, subs in self.keys.items():
            nbs = set(r for r, nd in enumerate(all_needs) if rank in nd and kind in nd[rank])
            nbs |= set(r for r in needs if kind in needs[r])
            for nb in sorted(nbs):
                send, recv = [], []
                for s, (gid, owner, off) in sorted(subs.items()):
                    want = all_needs[nb].get(rank, {}).get(kind, {}).get(s)
                    if want is not None and len(want):
                        pos = np.searchsorted(gid, want)
                        if not (np.all(pos < len(gid)) and np.array_equal(gid[pos], want)
                                and np.all(owner[pos] == rank)):
                            raise RuntimeError("halo: a neighbour's ghost is not owned here")
                        send.append(pos + off)
                    mine = needs.get(nb, {}).get(kind, {}).get(s)
                    if mine is not None and len(mine):
                        recv.append(np.searchsorted(gid, mine) + off)
                cat = lambda v: np.concatenate(v).astype(np.int32) if v else np.zeros(0, np.int32)
                plans[kind][nb] = dict(nb=nb, send=cat(send), recv=cat(recv))
        self.plans = plans
        return plans


def make_partitioned_problem(kind, r, rank, world, g_syn=10.0, length=None, method="rcb", gather=None, mesh_data=None):
    """The rank-local driver set-up (examples/idealized_geometries/setup_problem.Setup) of a partitioned idealized
    box: global mesh `make_mesh_3D(r, kind, l=length)` (default length 2 * world: weak scaling), cells partitioned
    with `method` in {"rcb", "slab"}.  `mesh_data` = (mesh, ct, ft): that global mesh instead (the same on every rank)."""
    from setup_problem import Setup
    from .idealized import make_mesh_3D
    cell_type = {"tet": "tetrahedron", "hex": "hexahedron"}[kind]
    l = 2 * world if length is None else int(length)
    mesh, ct, ft = mesh_data if mesh_data is not None else make_mesh_3D(r, cell_type, l=l)
    cent = mesh.x[mesh.cells].mean(axis=1)
    part = rcb_partition(cent, world) if method == "rcb" else slab_partition(cent, world)
    local = LocalPart(mesh, ct, ft, part, rank, world)
    s = Setup(kind, r, g_syn=g_syn, mesh_data=(local.mesh, local.ct, local.ft), build_forms=True)
    s.halo = VertexHalo(local, s.subdomain_list)
    s.halo.build(gather or gather_objects)
    s.owned_dofs = s.halo.owned_dofs
    s.local = local
    s.global_length = l * 16e-6
    s.global_mesh = (mesh, ct, ft)
    return s


def make_partitioned_astro(cfg, rank, world, method="rcb", gather=None):
    """The rank-local set-up of the three-sub-domain driver (ECS + neuron with the HH model + glia with the Kir4.1 / pump
    model, pulsed ECS source: `examples/local_astrocyte_depolarization/run_stim_duration.Problem`) on a cell partition
    of its mesh -- what DOLFINx's MPI partition gives the reference when that driver runs under `mpirun`
    (run_stim_duration.py:127-134,168-211).  Three sub-domain halos, two membrane models (their ghost dofs integrated
    redundantly), the source term evaluated on the local ECS vertices."""
    import run_stim_duration as rsd
    mesh, ct, ft = rsd.read_mesh(cfg)
    cent = mesh.x[mesh.cells].mean(axis=1)
    part = rcb_partition(cent, world) if method == "rcb" else slab_partition(cent, world)
    local = LocalPart(mesh, ct, ft, part, rank, world)
    s = rsd.Problem(cfg, mesh_data=(local.mesh, local.ct, local.ft))
    s.halo = VertexHalo(local, s.subdomain_list)
    s.halo.build(gather or gather_objects)
    s.owned_dofs = s.halo.owned_dofs
    s.local = local
    s.global_length = float(mesh.x[:, 0].max())
    s.global_mesh = (mesh, ct, ft)
    return s
