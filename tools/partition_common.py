"""The opening and closing every rank tool (tools/check_partition_*.py, check_dg_partition.py, check_async_halo.py)
shares: the import paths, rank and world size from the environment, the device, the process group, a gather."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in ("knp-emi-fenics-x_amd", os.path.join("examples", "idealized_geometries"), "tools"):
    sys.path.insert(0, os.path.join(ROOT, _p))


def start(backend="gloo", rank=None, world=None, device=0, device_id=True):
    """(rank, world) of this process -- RANK and WORLD_SIZE of the environment unless given -- after
    torch.cuda.set_device(device) and init_process_group(backend) at tcp://MASTER_ADDR:MASTER_PORT.  Every rank uses GPU 0
    by default (one-card rehearsals); "nccl" is bound to the device (device_id) unless told otherwise."""
    rank = int(os.environ.get("RANK", 0)) if rank is None else rank
    world = int(os.environ.get("WORLD_SIZE", 1)) if world is None else world
    torch.cuda.set_device(device)
    addr = f"tcp://{os.environ.get('MASTER_ADDR', '127.0.0.1')}:{os.environ['MASTER_PORT']}"
    kw = dict(device_id=torch.device("cuda", device)) if backend == "nccl" and device_id else {}
    dist.init_process_group(backend, init_method=addr, rank=rank, world_size=world, **kw)
    return rank, world


def gather(obj):
    """[obj of rank 0, ..., obj of rank world - 1] on every rank."""
    out = [None] * dist.get_world_size()
    dist.all_gather_object(out, obj)
    return out


def finish(barrier=True):
    if barrier:
        dist.barrier()
    dist.destroy_process_group()
