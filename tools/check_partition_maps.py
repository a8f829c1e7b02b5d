"""Field maps on a cell-partitioned problem against one rank holding the whole mesh (rehearsal with gloo, 2+ ranks on one
card; started by tests/test_00_partition_maps.py):

    torchrun --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29536 tools/check_partition_maps.py \\
        --kind tet --method rcb --records 8

Every rank pushes an analytic field f(x, t_k) = g(x) cos(w t_k) + q(x) sin(w t_k) - 3 u(x) + level (u: x_0 over the length
of the box, so the far end never comes back up to the level), evaluated at its local vertex (membrane dof) coordinates,
into the watched fields for every record and records it (knpemi_maps_record); g and q are polynomials of the coordinates
formed with multiplications and additions only, and the two factors of t_k are scalars, so a vertex gets the same bits on
every rank that holds it.  Every rank hands its owned maps (`FieldMaps.maps(name, halo=halo)`) to rank 0.  Their union,
matched to the single-rank items by the coordinates, must hold every item exactly once, and every map must equal the
single-rank map bit for bit.  A `FieldMaps` with a series watch is refused by `step(halo)`.
"""
import argparse, contextlib, io, math
import numpy as np

import partition_common as pc

from check_partition_events import stepper  # noqa: E402
from check_partition_steps import init_fields  # noqa: E402

LEVEL = {"K_ecs": 3.0, "phi_ecs": 0.0, "Na_ics": 10.0, "phi_M": -0.05}
OMEGA = 2.0 * math.pi * 180.0


def field_maps(s):
    from knpemi import FieldMaps
    fm = FieldMaps(s.subdomain_list, s.ion_list)
    fm.watch("K_ecs", "c", tag=0, ion="K", threshold=LEVEL["K_ecs"])                     # the solver's c: a dense array
    fm.watch("phi_ecs", "phi", tag=0, stats=("peak", "trough"))                          # the vertex records
    fm.watch("Na_ics", "c", tag=1, ion="Na", threshold=LEVEL["Na_ics"], below=True, stats=("integral", "threshold"))
    fm.watch("phi_M", "phi_M", tag=1, threshold=LEVEL["phi_M"])
    return fm


def sample(x, L_x, level, t):
    """f(x, t) at the coordinates x (n, 3)."""
    u = x[:, 0] * (1.0 / L_x)
    v = x[:, 1] * 1.0e6
    w = x[:, 2] * 1.0e6
    g = u * (1.0 - u) * 4.0 + v * w * 0.5
    q = (u * u) * (1.0 + w) - v * 0.25
    scale = 0.1 * (abs(level) or 1.0)
    return (g * (scale * math.cos(OMEGA * t)) + q * (scale * math.sin(OMEGA * t)) - u * (3.0 * scale)) + level


def record(s, st, fm, L_x, times):
    from knpemi import _lib as L
    dp = st.dp
    st.track(fm)
    for t in times:
        for name, w in fm.watches.items():
            field, idx = fm._field(w)
            dp.push_array(field, dp.sub_index[w.tag], idx, sample(fm.locations(name), L_x, LEVEL[name], t))
        L.check(dp.lib.knpemi_maps_record(dp.h, float(t)))
    return fm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="tet")
    ap.add_argument("--method", default="rcb", choices=["slab", "rcb"])
    ap.add_argument("--records", type=int, default=8)
    a = ap.parse_args()
    rank, world = pc.start()
    from knpemi.fem import make_mesh_3D
    from knpemi.fem.distributed import make_partitioned_problem
    from setup_problem import Setup
    gm, gct, gft = make_mesh_3D(0, {"tet": "tetrahedron", "hex": "hexahedron"}[a.kind], l=2 * world)
    with contextlib.redirect_stdout(io.StringIO()):
        s = make_partitioned_problem(a.kind, 0, rank, world, g_syn=10.0, method=a.method)
    L_x = s.global_length
    times = np.cumsum(np.linspace(0.4e-3, 1.1e-3, a.records))          # non-uniform
    single = None
    if rank == 0:
        with contextlib.redirect_stdout(io.StringIO()):
            g = Setup(a.kind, 0, g_syn=10.0, mesh_data=(gm, gct, gft))
        init_fields(g, L_x)
        fm1 = record(g, stepper(g, None), field_maps(g), L_x, times)
        single = {name: fm1.maps(name) for name in fm1.watches}
    init_fields(s, L_x)
    st = stepper(s, s.halo)
    fm = record(s, st, field_maps(s), L_x, times)
    mine = {name: fm.maps(name, halo=s.halo) for name in fm.watches}
    print(f"rank {rank}: transport {s.halo.mode}, owned items " +
          ", ".join(f"{n} {m['locations'].shape[0]} of {fm.watches[n].n}" for n, m in mine.items()), flush=True)
    parts = pc.gather(mine)
    if rank == 0:
        key = lambda x: [r.tobytes() for r in np.ascontiguousarray(x)]      # noqa: E731
        for name, ref in single.items():
            union = {k: np.concatenate([p[name][k] for p in parts]) for k in ref}
            where = {b: i for i, b in enumerate(key(union["locations"]))}
            n = ref["locations"].shape[0]
            assert len(where) == union["locations"].shape[0] == n, \
                f"{name}: {union['locations'].shape[0]} owned items ({len(where)} distinct) over the ranks, {n} on one rank"
            perm = np.array([where[b] for b in key(ref["locations"])])       # KeyError: an item no rank owns
            for k, want in ref.items():
                got = union[k][perm]
                assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=k != "count"), (name, k)
            if "count" in ref:
                c = ref["count"]
                assert c.min() != c.max(), f"{name}: the level separates nothing"
                print(f"{name}: {n} items, counts {int(c.min())} .. {int(c.max())} at {LEVEL[name]!r}, maps compared: {sorted(ref)}")
            else:
                assert np.ptp(ref["v_max"]) > 0
                print(f"{name}: {n} items, maps compared: {sorted(ref)}")
    # a series would sum the ghosts too: partitioned steps refuse it
    from knpemi import FieldMaps, _lib as L
    L.check(st.dp.lib.knpemi_maps_clear(st.dp.h))
    del st.taps["track"]
    fs = FieldMaps(s.subdomain_list, s.ion_list)
    fs.watch("K_ecs", "c", tag=0, ion="K", threshold=LEVEL["K_ecs"], series=True)
    st.track(fs)
    try:
        st.step(s.halo)
    except NotImplementedError as e:
        assert "series" in str(e)
    else:
        raise AssertionError("step(halo) accepted field maps with a series watch")
    if rank == 0:
        print("PARTITION MAPS OK", flush=True)
    pc.finish()


if __name__ == "__main__":
    main()
