"""Field snapshots on a cell-partitioned problem against one rank holding the whole mesh (rehearsal with gloo, 2+ ranks on
one card; started by tests/test_00_partition_snapshots.py):

    torchrun --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29537 tools/check_partition_snapshots.py \\
        --kind tet --method rcb --records 3

Every rank pushes the analytic field of tools/check_partition_maps.py, evaluated at its local vertex (membrane dof)
coordinates, into the watched fields for every record, and snapshots it with `select_owned(halo)`: the frames hold the
items the rank owns.  Every rank hands its frames and their `global_ids` to rank 0.  Their union must hold every item of
the whole mesh exactly once, and, put in the order of the global numbers, equal the frame of one rank holding the whole
mesh bit for bit.
"""
import argparse, contextlib, io
import numpy as np

import partition_common as pc

from check_partition_events import stepper  # noqa: E402
from check_partition_maps import LEVEL, sample  # noqa: E402
from check_partition_steps import init_fields  # noqa: E402

# name -> (quantity, tag, ion, dtype, the level of the analytic field)
WATCHES = {"K_ecs": ("c", 0, "K", "f8", LEVEL["K_ecs"]),            # the solver's c: a dense array
           "phi_ecs": ("phi", 0, None, "f8", LEVEL["phi_ecs"]),      # the vertex records
           "phi_ecs4": ("phi", 0, None, "f4", LEVEL["phi_ecs"]),
           "Na_ics": ("c", 1, "Na", "f8", LEVEL["Na_ics"]),          # the eliminated ion
           "phi_M": ("phi_M", 1, None, "f8", LEVEL["phi_M"])}


def snapshots(s, sink):
    from knpemi.snapshots import Snapshots
    snap = Snapshots(s.mesh, s.ct, s.ft, s.subdomain_list, s.ion_list, sink=sink, writer="inline")
    for name, (quantity, tag, ion, dtype, _) in WATCHES.items():
        snap.watch(name, quantity, tag, ion=ion, dtype=dtype)
    return snap


def record(s, st, halo, L_x, times):
    """[(t, k, frame)] of the records at `times`, and the snapshots."""
    from knpemi import _lib as L
    from knpemi.snapshots import MemorySink
    dp = st.dp
    sink = MemorySink()
    snap = snapshots(s, sink)
    if halo is not None:
        snap.select_owned(halo)
    # the full fields are pushed at the coordinates of every local item; the snapshot stores the selection
    where = {name: np.array(snap._mesh(*snap.watches[name].space).x, np.float64) for name in WATCHES}
    st.snapshot(snap, depth=2)
    for k, t in enumerate(times):
        for name, w in snap.watches.items():
            field, idx = snap._field(w)
            dp.push_array(field, dp.sub_index[w.tag], idx, sample(where[name], L_x, WATCHES[name][4], t))
        L.check(snap._tick(float(t), k + 1))
    snap.flush()
    return sink.frames, snap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="tet")
    ap.add_argument("--method", default="rcb", choices=["slab", "rcb"])
    ap.add_argument("--records", type=int, default=3)
    a = ap.parse_args()
    rank, world = pc.start()
    from knpemi.fem import make_mesh_3D
    from knpemi.fem.distributed import make_partitioned_problem
    from setup_problem import Setup
    gm, gct, gft = make_mesh_3D(0, {"tet": "tetrahedron", "hex": "hexahedron"}[a.kind], l=2 * world)
    with contextlib.redirect_stdout(io.StringIO()):
        s = make_partitioned_problem(a.kind, 0, rank, world, g_syn=10.0, method=a.method)
    L_x = s.global_length
    times = np.cumsum(np.linspace(0.4e-3, 1.1e-3, a.records))
    single = ids1 = None
    if rank == 0:
        with contextlib.redirect_stdout(io.StringIO()):
            g = Setup(a.kind, 0, g_syn=10.0, mesh_data=(gm, gct, gft))
        init_fields(g, L_x)
        single, snap1 = record(g, stepper(g, None), None, L_x, times)
        ids1 = {name: np.asarray(snap1._mesh(*w.space).parent_vertices, np.int64) for name, w in snap1.watches.items()}
    init_fields(s, L_x)
    st = stepper(s, s.halo)
    frames, snap = record(s, st, s.halo, L_x, times)
    ids = {name: snap.global_ids(name, s.halo) for name in snap.watches}
    print(f"rank {rank}: transport {s.halo.mode}, owned items " +
          ", ".join(f"{n} {ids[n].shape[0]} of {snap._n_space(*w.space)}" for n, w in snap.watches.items()), flush=True)
    parts = pc.gather((ids, [(t, k, {n: np.array(v) for n, v in f.items()}) for t, k, f in frames]))
    if rank == 0:
        assert len(single) == a.records
        for j, (t, k, ref) in enumerate(single):
            assert all((p[1][j][0], p[1][j][1]) == (t, k) for p in parts)
            for name, want in ref.items():
                gid = np.concatenate([p[0][name] for p in parts])
                got = np.concatenate([p[1][j][2][name] for p in parts])
                n = want.shape[0]
                assert gid.shape[0] == np.unique(gid).shape[0] == n, \
                    f"{name}: {gid.shape[0]} owned items ({np.unique(gid).shape[0]} distinct) over the ranks, {n} on one rank"
                order, order1 = np.argsort(gid), np.argsort(ids1[name])
                assert np.array_equal(gid[order], ids1[name][order1]), f"{name}: an item no rank owns"
                assert got.dtype == want.dtype and got[order].tobytes() == want[order1].tobytes(), (name, j)
                assert np.ptp(want.astype(np.float64)) > 0, f"{name}: a constant field shows nothing"
        print(f"{len(single)} frames of {list(single[0][2])} compared, "
              f"{[int(v.shape[0]) for v in single[0][2].values()]} items", flush=True)
        print("PARTITION SNAPSHOTS OK", flush=True)
    pc.finish()


if __name__ == "__main__":
    main()
