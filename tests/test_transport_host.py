"""CPU tests of knpemi.fem.transport.Transport, the one transport under the CG halo and the DG slab: the layout of the
packed buffers against hand-written arrays, the gloo host-staged transfer between real ranks on CPU tensors (with
torch.cuda made unusable: on a CPU device that branch must not touch it), and the guarded hooks."""
import os
import sys
import types

import numpy as np
import pytest

from partition_ranks import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 2        # doubles per id in the transfer test


def _transport(owner=None, sync=lambda: None):
    """A transport on a CPU endpoint: no library, no handle, no stream."""
    import torch
    from knpemi.fem.transport import Endpoint, Transport
    return Transport(Endpoint(None, None, torch.device("cpu"), None, None, None, sync), owner)


# a rank with two neighbours: 3 ids sent to and 2 received from rank 0, 1 sent to and 4 received from rank 2
PLAN = dict(low=dict(nb=0, send=np.array([4, 7, 9]), recv=np.array([1, 2])),
            high=dict(nb=2, send=np.array([5]), recv=np.array([10, 11, 12, 13])))


def _knp_index(g):          # KS = 2 entries of every id, 100 apart: per neighbour the blocks stay together
    g = np.asarray(g, np.int64)
    return np.concatenate([g + 100 * k for k in range(2)])


@pytest.mark.parametrize("w,index_map,send_idx,recv_idx,send,recv", [
    (1, None, [4, 7, 9, 5], [1, 2, 10, 11, 12, 13], [(0, 3), (3, 4)], [(0, 2), (2, 6)]),
    (5, None, [4, 7, 9, 5], [1, 2, 10, 11, 12, 13], [(0, 15), (15, 20)], [(0, 10), (10, 30)]),
    (1, _knp_index, [4, 7, 9, 104, 107, 109, 5, 105], [1, 2, 101, 102, 10, 11, 12, 13, 110, 111, 112, 113],
     [(0, 6), (6, 8)], [(0, 4), (4, 12)]),
    (5, _knp_index, [4, 7, 9, 104, 107, 109, 5, 105], [1, 2, 101, 102, 10, 11, 12, 13, 110, 111, 112, 113],
     [(0, 30), (30, 40)], [(0, 20), (20, 60)]),
])
def test_plan_layout(w, index_map, send_idx, recv_idx, send, recv):
    import torch
    d = _transport().plan(PLAN, w, index_map)
    for key, want in (("send_idx", send_idx), ("recv_idx", recv_idx)):
        assert d[key].dtype == torch.int32 and d[key].tolist() == want, key
    assert d["parts"] == [(0, slice(*send[0]), slice(*recv[0])), (2, slice(*send[1]), slice(*recv[1]))]
    assert d["send_buf"].shape == (send[1][1],) and d["recv_buf"].shape == (recv[1][1],)
    assert d["send_buf"].dtype == d["recv_buf"].dtype == torch.float64
    want = dict(peer=[0, 2], send_off=[s[0] for s in send], send_cnt=[s[1] - s[0] for s in send],
                recv_off=[r[0] for r in recv], recv_cnt=[r[1] - r[0] for r in recv])
    for key, v in want.items():
        assert d[key].dtype == (np.int32 if key == "peer" else np.int64) and d[key].tolist() == v, key
    assert _transport().plan({}, w, index_map) is None


def _count(src, dst):
    """Ids that rank src sends to rank dst: different in the two directions and for every pair."""
    return 1 + (2 * src + dst) % 4


def _send_offset(src, dst):
    """Where the slice for dst begins in the packed send buffer of src (neighbours in rank order)."""
    return sum(_count(src, q) * W for q in range(dst) if q != src)


def _transfer_worker(rank, world, port):
    sys.path.insert(0, os.path.join(ROOT, "knp-emi-fenics-x_amd"))
    import torch
    import torch.distributed as dist

    def no_gpu(*a, **k):
        raise AssertionError("torch.cuda used on a CPU device")
    torch.cuda.current_stream = torch.cuda.ExternalStream = torch.cuda.stream = torch.cuda.synchronize = no_gpu
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    synced = []
    tr = _transport(sync=lambda: synced.append(1))
    assert tr.mode == "not attached" and tr.negotiate() == tr.mode == "gloo host-staged" and not tr.library
    others = [q for q in range(world) if q != rank]
    d = tr.plan({q: dict(nb=q, send=np.arange(_count(rank, q)), recv=np.arange(_count(q, rank))) for q in others}, W)
    assert [p[0] for p in d["parts"]] == others
    d["send_buf"].copy_(1000.0 * rank + torch.arange(d["send_buf"].numel(), dtype=torch.float64))
    d["recv_buf"].fill_(-1.0)
    tr.transfer(d)
    assert synced == [1]              # the packed data is complete before it leaves
    for q, _, rs in d["parts"]:
        n = _count(q, rank) * W
        want = 1000.0 * q + _send_offset(q, rank) + torch.arange(n, dtype=torch.float64)
        assert rs.stop - rs.start == n and torch.equal(d["recv_buf"][rs], want), (rank, q, d["recv_buf"][rs], want)
    assert d["parts"][-1][2].stop == d["recv_buf"].numel()
    if world > 2:
        assert d["parts"][1][1].start > 0 and d["parts"][1][2].start > 0
    # the reduction of the solve hooks and the recorders: the first n entries only
    buf = torch.arange(4, dtype=torch.float64) + rank
    tr.allreduce(3, buf)
    tot = sum(range(world))
    assert buf.tolist() == [tot, world + tot, 2 * world + tot, 3.0 + rank]
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_transfer_between_cpu_ranks(world):
    """Every rank is every other rank's neighbour and fills its send buffer with 1000 rank + position: after the transfer
    every slice of the receive buffer holds the neighbour's values of the slice meant for this rank.  With three ranks
    the second neighbour's slices begin at a non-zero offset on both sides."""
    import torch.multiprocessing as mp
    mp.spawn(_transfer_worker, args=(world, free_port()), nprocs=world, join=True)


def test_guarded_hook_keeps_the_exception():
    from knpemi import _lib as L
    owner = types.SimpleNamespace(_hook_error=None)
    tr = _transport(owner)
    seen = []
    assert tr.guarded(lambda ctx, n: seen.append(n))(None, 3) == 0 and seen == [3] and owner._hook_error is None

    def body(ctx, n):
        raise KeyError("in the hook")
    cb = L.ALLREDUCE_FN(tr.guarded(body))           # as the library calls it: nothing crosses the C frame
    assert cb(None, 3) == -1
    assert isinstance(owner._hook_error, KeyError) and "in the hook" in str(owner._hook_error)


def test_halo_keeps_the_error_where_the_stepper_looks():
    """`_hook_error` and `mode` before attach, on the object stepper.py and the rank tools read them from."""
    from knpemi.fem.distributed import Halo
    h = Halo()
    assert h._hook_error is None and h.mode == "not attached" and not h.library_comm
    h.transport = _transport(h)
    assert h.transport.guarded(lambda: 1 / 0)() == -1 and isinstance(h._hook_error, ZeroDivisionError)
