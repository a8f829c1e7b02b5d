"""Membrane events on a cell-partitioned run against a single-rank run of the whole mesh (rehearsal with gloo, 2+ ranks
on one card; started by tests/test_00_partition_events.py):

    torchrun --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29535 tools/check_partition_events.py \\
        --kind tet --method rcb --steps 6

Rank 0 first steps the whole mesh, takes the threshold as the midpoint between the smallest initial phi_M and the
largest phi_M any dof reaches, and broadcasts it.  Every rank then steps its part with `DeviceStepper.detect`
(as tools/check_partition_steps.py, without solves: the steps are bit-identical to the single-rank ones) and hands its
owned maps (`MembraneEvents.maps(tag, halo=halo)`) to rank 0.  Their union, matched to the single-rank dofs by the
coordinates, must hold every dof exactly once, and every map must equal the single-rank map bit for bit.
"""
import argparse, contextlib, io
import numpy as np

import torch.distributed as dist

import partition_common as pc

from check_partition_steps import init_fields, membrane_models  # noqa: E402

KEEP = 2


def stepper(s, halo):
    from knpemi.stepper import DeviceStepper
    st = DeviceStepper((s.a_emi, s.p_emi, s.L_emi), (s.a_knp, s.p_knp, s.L_knp), s.c, s.c_prev, s.phi, s.phi_M_prev)
    for _, mm in membrane_models(s):
        st.add_membrane_model(mm['ode'], s.stim_params['stimulus'], s.stim_params['stimulus_locator'])
    if halo is not None:
        halo.attach(st.dp)
        halo.exchange_bulk()
        halo.exchange_membrane()
    return st


def detect(s, st, halo, K, threshold):
    from knpemi import MembraneEvents
    ev = MembraneEvents(s.subdomain_list)
    ev.watch(1, threshold, keep=KEEP)
    st.detect(ev)
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(K):
            st.step(halo)
    return ev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="tet")
    ap.add_argument("--method", default="rcb", choices=["slab", "rcb"])
    ap.add_argument("--steps", type=int, default=6)
    a = ap.parse_args()
    rank, world = pc.start()
    from knpemi.fem import make_mesh_3D
    from knpemi.fem.distributed import make_partitioned_problem
    from setup_problem import Setup
    gm, gct, gft = make_mesh_3D(0, {"tet": "tetrahedron", "hex": "hexahedron"}[a.kind], l=2 * world)
    with contextlib.redirect_stdout(io.StringIO()):
        s = make_partitioned_problem(a.kind, 0, rank, world, g_syn=10.0, method=a.method)
    L_x = s.global_length
    box, single = [None], None
    if rank == 0:
        def whole():      # a fresh single-rank problem at the common start (a download moves the host objects on)
            with contextlib.redirect_stdout(io.StringIO()):
                g = Setup(a.kind, 0, g_syn=10.0, mesh_data=(gm, gct, gft))
            init_fields(g, L_x)
            return g, stepper(g, None)
        g, st1 = whole()
        lo = float(g.phi_M_prev[1].x._a.min())
        hi = -np.inf
        with contextlib.redirect_stdout(io.StringIO()):
            for _ in range(a.steps):
                st1.step()
                st1.download()
                hi = max(hi, float(g.phi_M_prev[1].x._a.max()))
        box[0] = 0.5 * (lo + hi)
        g, st1 = whole()
        single = detect(g, st1, None, a.steps, box[0]).maps(1)
    dist.broadcast_object_list(box, src=0)
    threshold = box[0]
    init_fields(s, L_x)
    ev = detect(s, stepper(s, s.halo), s.halo, a.steps, threshold)
    if getattr(s.halo, "_hook_error", None) is not None:
        raise s.halo._hook_error
    mine = ev.maps(1, halo=s.halo)
    print(f"rank {rank}: transport {s.halo.mode}, {mine['count'].shape[0]} owned of {ev.n_q[1]} local membrane dofs",
          flush=True)
    parts = pc.gather(mine)
    if rank == 0:
        union = {k: np.concatenate([p[k] for p in parts]) for k in single}
        key = lambda x: [r.tobytes() for r in np.ascontiguousarray(x)]      # noqa: E731
        where = {b: i for i, b in enumerate(key(union["locations"]))}
        n = single["count"].shape[0]
        assert len(where) == union["count"].shape[0] == n, \
            f"{union['count'].shape[0]} owned dofs ({len(where)} distinct) over the ranks, {n} on one rank"
        perm = np.array([where[b] for b in key(single["locations"])])       # KeyError: a dof no rank owns
        for k, ref in single.items():
            got = union[k][perm]
            assert got.dtype == ref.dtype and np.array_equal(got, ref, equal_nan=k != "count"), k
        print(f"threshold {threshold!r}: {int((single['count'] > 0).sum())} of {n} dofs fired, v_peak "
              f"{single['v_peak'].min()!r} .. {single['v_peak'].max()!r}")
        print("maps compared:", sorted(single), "records", a.steps)
        print("PARTITION EVENTS OK", flush=True)
    pc.finish()


if __name__ == "__main__":
    main()
