"""How bytes move between the ranks of a partitioned run: one `Transport` under the CG halo (`knpemi.fem.distributed.Halo`)
and the DG slab (`knpemi.dg.DGSlab`).  It is bound once to an `Endpoint` -- a device handle with its stream, communicator
and sync entry points -- agrees with the other ranks on one of four ways to move a packed buffer (`negotiate`, the only
place where that sequence of collectives is written), lays the buffers out (`plan`) and moves them (`transfer`).  What is
packed into the buffers, and by which kernels, is the business of the halo or slab that owns the transport.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple

import numpy as np

from .. import _lib as L

# lib, handle and torch device of one device problem, and the four entry points that differ between the handles:
# stream(handle) -> hipStream_t, comm_init(handle, rank, world, id, 128), comm_sendrecv(handle, ...), sync()
Endpoint = namedtuple("Endpoint", "lib handle device stream comm_init comm_sendrecv sync")


def cg_endpoint(dp):
    """The handle of a `knpemi.device.DeviceProblem`."""
    import torch
    return Endpoint(dp.lib, dp.h, torch.device("cuda", dp.device), dp.lib.knpemi_stream, dp.lib.knpemi_comm_init,
                    dp.lib.knpemi_comm_sendrecv, dp.sync)


def dg_endpoint(dp):
    """The handle of a `knpemi.dg.DGProblem`."""
    import torch
    return Endpoint(dp.lib, dp.h, torch.device("cuda", dp.device), dp.lib.knpemi_dg_stream, dp.lib.knpemi_dg_comm_init,
                    dp.lib.knpemi_dg_comm_sendrecv, dp.sync)


class Transport:
    """`mode` is chosen ONCE, in `negotiate`, and agreed on by all ranks; a communication error during a run propagates
    (the rank exits non-zero) instead of switching modes under a half-posted batch.
      "library RCCL (<comm_sendrecv>)": RCCL called by the library itself: pack -> ncclSend/ncclRecv group -> unpack on
                                the handle's stream, a few microseconds of host time per exchange instead of ~50 through
                                torch.distributed's Python layer (`library` is True)
      "stream-ordered RCCL":    pack kernel -> send/recv -> unpack kernel on the handle's stream, no host sync
      "host-synchronised RCCL": KNPEMI_HALO_SYNC=1, or torch cannot wrap the handle's stream
      "gloo host-staged":       single-GPU rehearsals and CPU tests
    `owner` is the halo or slab whose `_hook_error` keeps what a `guarded` hook caught."""

    def __init__(self, endpoint, owner):
        import torch
        import torch.distributed as dist
        self.ep, self.owner, self.torch, self.dist = endpoint, owner, torch, dist
        self.mode = "not attached"
        self.library = False
        self._ext = None
        self._stream_ordered = False

    def negotiate(self):
        """Every rank issues the same collectives in the same order, whatever it finds locally: with a backend other than
        gloo and neither KNPEMI_HALO_TORCH nor KNPEMI_HALO_SYNC set (the environment is the same on all ranks), (1) the
        object broadcast of the id box and, unless rank 0 could not draw an id, (2) the MIN-vote after comm_init;
        where the library's communicator is not asked for or not agreed on, (3) the MIN-vote on stream ordering.  A
        rank-local decision that skips or adds one of them deadlocks the others."""
        ep, torch, dist = self.ep, self.torch, self.dist
        stream_ordered = os.environ.get("KNPEMI_HALO_SYNC") is None
        try:
            if ep.device.type != "cuda":
                raise TypeError("a CPU device (host tests) has no stream to wrap")
            self._ext = torch.cuda.ExternalStream(ep.stream(ep.handle), device=ep.device)
        except (RuntimeError, TypeError):
            self._ext, stream_ordered = None, False
        if dist.get_backend() == "gloo":
            self.mode = "gloo host-staged"
        else:
            # first choice: the library's own communicator.  All ranks must agree, so every step of the set-up is voted on.
            # KNPEMI_HALO_SYNC=1 asks for the host-synchronised exchange, which only the torch transport has
            library = os.environ.get("KNPEMI_HALO_TORCH") is None and os.environ.get("KNPEMI_HALO_SYNC") is None
            if library:
                library = self._library_comm_init()
            if library:
                self.mode = f"library RCCL ({ep.comm_sendrecv.__name__})"
                self.library = True
            else:
                self.mode = "stream-ordered RCCL" if self._vote(stream_ordered) else "host-synchronised RCCL"
        self._stream_ordered = self.mode == "stream-ordered RCCL"
        return self.mode

    def _vote(self, ok):
        flag = self.torch.tensor([1 if ok else 0], dtype=self.torch.int32, device=self.ep.device)
        self.dist.all_reduce(flag, op=self.dist.ReduceOp.MIN)
        return bool(int(flag.item()))

    def _library_comm_init(self):
        """Create the library's own RCCL communicator: rank 0 draws the unique id, torch.distributed carries it."""
        ep, dist = self.ep, self.dist
        rank, world = dist.get_rank(), dist.get_world_size()
        buf = C.create_string_buffer(128)
        ok = True
        if rank == 0:
            ok = ep.lib.knpemi_comm_unique_id(buf, 128) == 0
        box = [buf.raw if ok else None]
        dist.broadcast_object_list(box, src=0)
        if box[0] is None:
            return False
        return self._vote(ep.comm_init(ep.handle, rank, world, box[0], 128) == 0)

    def plan(self, plan, w, index_map=None):
        """One packed buffer per direction for `plan` = {label: dict(nb=neighbour rank, send=ids, recv=ids)}, w doubles per
        id (each id standing for the entries `index_map(ids)` where one is given): all neighbours' entries are packed /
        unpacked by a single kernel launch, the point-to-point operations work on slices of it."""
        torch, dev = self.torch, self.ep.device
        sides = list(plan.values())
        if not sides:
            return None
        f = (lambda a: a) if index_map is None else index_map
        send_idx = np.concatenate([f(pl["send"]) for pl in sides]).astype(np.int32)
        recv_idx = np.concatenate([f(pl["recv"]) for pl in sides]).astype(np.int32)
        m = 1 if index_map is None else len(f(np.zeros(1, np.int64)))
        d = dict(send_idx=torch.from_numpy(send_idx).to(dev), recv_idx=torch.from_numpy(recv_idx).to(dev),
                 send_buf=torch.empty(len(send_idx) * w, dtype=torch.float64, device=dev),
                 recv_buf=torch.empty(len(recv_idx) * w, dtype=torch.float64, device=dev), parts=[])
        so = ro = 0
        for pl in sides:
            ns, nr = len(pl["send"]) * w * m, len(pl["recv"]) * w * m
            d["parts"].append((pl["nb"], slice(so, so + ns), slice(ro, ro + nr)))
            so, ro = so + ns, ro + nr
        # the same parts as flat arrays for comm_sendrecv
        d["peer"] = np.array([p[0] for p in d["parts"]], np.int32)
        for key, idx, attr in (("send_off", 1, "start"), ("recv_off", 2, "start")):
            d[key] = np.array([getattr(p[idx], attr) for p in d["parts"]], np.int64)
        d["send_cnt"] = np.array([p[1].stop - p[1].start for p in d["parts"]], np.int64)
        d["recv_cnt"] = np.array([p[2].stop - p[2].start for p in d["parts"]], np.int64)
        return d

    def _wait_for_torch(self):
        if self.ep.device.type == "cuda":
            self.torch.cuda.current_stream().synchronize()

    def transfer(self, d, library=None):
        """send_buf -> neighbours -> recv_buf of a `plan`, ordered on the handle's stream (see `mode`).  library=False
        keeps a buffer off the library's communicator where `mode` is library RCCL: it then moves through
        torch.distributed, host-synchronised."""
        ep, dist, torch = self.ep, self.dist, self.torch
        if self.library if library is None else library:
            i64 = C.POINTER(C.c_int64)
            L.check(ep.comm_sendrecv(
                ep.handle, d["send_buf"].data_ptr(), d["recv_buf"].data_ptr(), len(d["peer"]), L.iptr(d["peer"]),
                d["send_off"].ctypes.data_as(i64), d["send_cnt"].ctypes.data_as(i64),
                d["recv_off"].ctypes.data_as(i64), d["recv_cnt"].ctypes.data_as(i64)))
        elif dist.get_backend() != "gloo":
            ops = []
            for nb, ss, rs in d["parts"]:
                ops += [dist.P2POp(dist.isend, d["send_buf"][ss], nb), dist.P2POp(dist.irecv, d["recv_buf"][rs], nb)]
            if self._stream_ordered:
                # RCCL: torch's current stream is the handle's stream (ExternalStream), so the send/recv kernels are
                # ordered after the pack kernel and `wait()` orders the unpack kernel after them: no host
                # synchronisation anywhere in the exchange (tools/check_async_halo.py rehearses this with real RCCL)
                with torch.cuda.stream(self._ext):
                    for req in dist.batch_isend_irecv(ops):
                        req.wait()
            else:
                ep.sync()                        # packed data is complete before RCCL reads it
                for req in dist.batch_isend_irecv(ops):
                    req.wait()
                torch.cuda.current_stream().synchronize()
        else:                           # single-GPU rehearsal: stage through host memory
            ep.sync()
            sb = d["send_buf"].cpu()
            rb = torch.empty(d["recv_buf"].shape, dtype=torch.float64)
            ops = []
            for nb, ss, rs in d["parts"]:
                ops += [dist.P2POp(dist.isend, sb[ss], nb), dist.P2POp(dist.irecv, rb[rs], nb)]
            for req in dist.batch_isend_irecv(ops):
                req.wait()
            d["recv_buf"].copy_(rb)
            self._wait_for_torch()

    def allreduce(self, n, buf):
        """Sum the first n doubles of the device tensor `buf` over the ranks (through torch.distributed in every mode)."""
        dist, torch = self.dist, self.torch
        if dist.get_backend() == "gloo":
            self.ep.sync()
            host = buf[:n].cpu()
            dist.all_reduce(host)
            buf[:n].copy_(host)
            self._wait_for_torch()
        elif self._stream_ordered:
            with torch.cuda.stream(self._ext):
                dist.all_reduce(buf[:n])
        else:
            self.ep.sync()
            dist.all_reduce(buf[:n])
            torch.cuda.current_stream().synchronize()

    def guarded(self, fn):
        """`fn` as the body of a hook the library calls (wrap the result in L.ALLREDUCE_FN / L.HALO_FN): an exception must
        not propagate through the C frame, so it is kept in the owner's `_hook_error` and reported as a failure."""
        def hook(*args):
            try:
                fn(*args)
                return 0
            except Exception as exc:       # noqa: BLE001
                self.owner._hook_error = exc
                return -1
        return hook
