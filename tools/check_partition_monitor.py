"""Membrane monitors and the maps' series on a cell-partitioned run against one rank holding the whole mesh (rehearsal with
gloo, 2+ ranks on one card; started by tests/test_00_partition_monitor.py):

    torchrun --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29537 tools/check_partition_monitor.py \\
        --kind tet --method rcb --records 8

The problem is the two-cell-type box of tests/test_partition_monitor_host.py: cell 1 carries the shipped Hodgkin-Huxley
model, cell 2 examples/benchmark/mm_glial.py, which is bound from source, so its watch runs the hipRTC monitor program.
Both are watched with all quantities, two points each and every reduction of every quantity, attached with
`DeviceStepper.monitor(mon, fields=True, halo=halo)`.

Without --steps the state is analytic: before every record each rank writes c_prev, the eliminated ion's c, the solver's c
and phi_M as polynomials of its local coordinates and of t (test_partition_monitor_host.analytic_state: multiplications
and additions only, so a dof has the same bits wherever it is held; the gates of the state tables likewise, once), and the
taps record.  With --steps N the ranks take N steps of the device-resident stepper instead (LSODA, no solves: the fields
of partitioned and single-rank runs are bit-identical, tools/check_partition_steps.py) and the monitors record after each.

Checks: every rank holds the same series bit for bit; against one rank holding the whole mesh points, minima and maxima
are equal bit for bit, integrals within n 2^-52 sum_q |w_q v_q| and averages within that over the sum of weights plus
2^-52 |average| (test_partition_monitor_host.sum_bound, from the single-rank per-dof values of the same record); the
largest ratio to the bound is printed.  The union of `values(halo=halo)` over the ranks, matched by coordinates, holds
every dof exactly once and equals the single-rank `values()` bit for bit.
Analytic runs also track a `FieldMaps` with a K_ecs and a phi_M series watch and a plain phi_ecs watch
(`track(fm, halo=halo)`): the n columns equal the single-rank counts exactly, the measures lie within
n 2^-52 sum |w_q| over the n items beyond the level, all ranks hold identical bits, and the per-item maps, gathered as
tools/check_partition_maps.py does, equal the single-rank maps bit for bit.
--method rcbz: the cut across z of the host test.  Three ranks: ranks 0 and 2 hold no membrane dof of one of the cells.  Two
ranks: rank 0 records every facet of cell 1 (the global sum of its weights is that rank's sum and zeros) and rank 1 holds no
dof of it.  --method far (three ranks): rank 0 holds ECS cells only, away from every membrane: no membrane dof of any watch,
no record launch, the operations' identities in its slots from the set-up on.
--cost N: afterwards, N records with both taps on, timed on the host between two synchronisations (record launch,
all-reduce through gloo and the host, combine launch, for the monitors and the maps): one JSON line per rank.
"""
import argparse, contextlib, io, json, os, sys, time
import numpy as np

import torch.distributed as dist

import partition_common as pc
sys.path.insert(0, os.path.join(pc.ROOT, "tests"))

from check_partition_events import stepper  # noqa: E402
from check_partition_steps import init_fields  # noqa: E402
import test_partition_monitor_host as tm  # noqa: E402

DT = 1.0e-4


def push_state(s, dp, state):
    """The analytic state into the device fields the recorders read: c_prev and the eliminated ion's c (the vertex
    records), the solver's c (the K_ecs watch of the maps) and phi_M."""
    from knpemi import _lib as L
    n_solved = len(s.ion_list) - 1
    for tag in s.subdomain_list:
        sub = dp.sub_index[tag]
        if dp.n_vert[sub] == 0:
            continue
        for k in range(n_solved):
            dp.push_array(L.F_C_PREV, sub, k, state["c"][tag][k])
            dp.push_array(L.F_C, sub, k, state["c"][tag][k])
        dp.push_array(L.F_C_ELIM, sub, 0, state["c"][tag][n_solved])
        if tag > 0 and state["phi_M"][tag].shape[0]:
            dp.push_array(L.F_PHI_M, sub, 0, state["phi_M"][tag])


def field_maps(s):
    fm = tm.series_maps(s)
    fm.watch("phi_ecs", "phi", tag=0, stats=("peak", "trough"))
    return fm


def run(s, halo, points, L_x, records, steps):
    """The records of one run.  Returns (monitor, series, per-record owned values, maps, maps series, stepper)."""
    from knpemi import MembraneMonitor
    analytic = steps == 0
    if analytic:      # the gates, before the stepper uploads the tables
        for (tag, j), (st_, _) in tm.analytic_state(s, L_x, 0.0)["tables"].items():
            s.subdomain_list[tag]["mem_models"][j]["ode"].states[...] = st_
    else:
        init_fields(s, L_x)
    with contextlib.redirect_stdout(io.StringIO()):
        st = stepper(s, halo)
    mon = tm.define(MembraneMonitor(s.subdomain_list, s.ion_list, ft=s.ft, partitioned=halo is not None), points)
    st.monitor(mon, every=1, capacity=1024, fields=True, halo=halo)
    fm = None
    if analytic:
        fm = field_maps(s)
        st.track(fm, every=1, capacity=1024, halo=halo)
    values = []
    for k in range(steps or records):
        if analytic:
            push_state(s, st.dp, tm.analytic_state(s, L_x, (k + 1) * DT))
            st.taps["monitor"].tick(k + 1, DT)
            st.taps["track"].tick(k + 1, DT)
        else:
            with contextlib.redirect_stdout(io.StringIO()):
                st.step(halo)
        values.append({key: mon.values(*key, halo=halo) for key in mon.watched})
    if halo is not None and getattr(halo, "_hook_error", None) is not None:
        raise halo._hook_error
    return mon, mon.series(), values, fm, fm.series() if analytic else None, st


def key_of(x):
    return [r.tobytes() for r in np.ascontiguousarray(x)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="tet", choices=["tet"])
    ap.add_argument("--method", default="rcb", choices=["rcb", "rcbz", "slab", "far"])
    ap.add_argument("--records", type=int, default=8, help="analytic records (without --steps)")
    ap.add_argument("--steps", type=int, default=0, help="steps of the device-resident stepper instead, one record each")
    ap.add_argument("--length", type=int, default=2, help="length of the box in units of 16 um")
    ap.add_argument("--cost", type=int, default=0, metavar="N", help="time N partitioned records of both taps afterwards")
    a = ap.parse_args()
    rank, world = pc.start()
    gmesh = tm.two_type_mesh(a.length)
    L_x = float(np.ptp(gmesh[0].x[:, 0]))
    g0 = tm.build(gmesh, plug_in=True)
    points = tm.membrane_points(g0)
    s, halo = tm.local_problem(gmesh, a.method, rank, world, pc.gather, forms=True, plug_in=True)
    s.halo = halo
    mon, ser, values, fm, fser, st = run(s, halo, points, L_x, a.records, a.steps)
    n_rec = ser["t"].shape[0]
    assert n_rec == (a.steps or a.records) and len(mon._cols) == mon.n_cols
    nq = {key: mon.n_dofs(key[0]) for key in mon.watched}
    print(f"rank {rank}: transport {halo.mode}, {mon.n_cols} columns, {n_rec} rows, local membrane dofs {nq}, recorded facets "
          f"{ {t: int(r.sum()) for t, r in mon._ptab['recorded'].items()} }, points taken "
          f"{[p for p, r in enumerate(mon._ptab['taker']) if r == rank]}", flush=True)
    empty = [key for key in mon.watched if not mon._ptab["recorded"][key[0]].any()]
    if a.method == "rcbz" and world == 3:
        assert (rank in (0, 2)) == bool(empty), (rank, empty)
    if a.method == "rcbz" and world == 2:      # rank 0 records every facet of cell 1, rank 1 holds no dof of it
        assert (nq[(1, 0)] == 0) == (rank == 1) and (empty == [(1, 0)]) == (rank == 1), (rank, nq, empty)
    if a.method == "far":                      # rank 0 holds no membrane dof at all: no record launch, ever
        assert (sum(nq.values()) == 0) == (rank == 0), (rank, nq)
    for r, other in enumerate(pc.gather((ser, fser))):                 # every rank holds the same (global) series
        for mine, theirs in zip((ser, fser), other):
            for k in mine or {}:
                assert np.array_equal(theirs[k], mine[k], equal_nan=True), ("rank", r, k)
    parts = pc.gather(values[-1])
    map_parts = pc.gather({name: fm.maps(name, halo=halo) for name in fm.watches} if fm is not None else None)
    if rank == 0:
        g = tm.build(gmesh, forms=True, plug_in=True)
        gmon, ref, gvalues, gfm, gfser, _ = run(g, None, points, L_x, a.records, a.steps)
        assert list(ref) == list(ser) and np.array_equal(ref["t"], ser["t"])
        wg = {key: gmon.weights(*key) for key in gmon.watched}
        wsum = {key: float(w.sum()) for key, w in wg.items()}
        worst, exact, summed = 0.0, 0, 0
        for i in range(n_rec):
            bounds = tm.sum_bound(gmon, gvalues[i], wg, wsum)
            got = np.array([ser[k][i] for k, _ in mon.columns()])
            assert np.isfinite(got).all(), [k for (k, _), v in zip(mon.columns(), got) if not np.isfinite(v)]
            worst = max(worst, tm.compare_row(mon, got, {k: ref[k][i] for k in ref if k != "t"}, bounds))
            summed += len(bounds)
            exact += len(got) - len(bounds)
        spread = [k for k, _ in mon.columns() if np.ptp(ref[k]) > 0.0]
        # (stepped without solves, only what depends on phi_M and the gates moves: the concentrations stay)
        assert len(spread) > (0 if a.steps else mon.n_cols // 2), "the state does not move between the records"
        print(f"monitor series: {n_rec} records, {exact} point / min / max values bit for bit, {summed} sums within the "
              f"bound; largest |partitioned - single| / bound: {worst:.3f}", flush=True)
        for key in gmon.watched:
            tag = key[0]
            x = np.array(g.subdomain_list[tag]["mesh_mem"].x, np.float64)
            loc = np.concatenate([p[key]["locations"].reshape(-1, x.shape[1]) for p in parts])
            where = {b: i for i, b in enumerate(key_of(loc))}
            assert len(where) == loc.shape[0] == x.shape[0], \
                f"{key}: {loc.shape[0]} owned dofs ({len(where)} distinct) over the ranks, {x.shape[0]} on one rank"
            perm = np.array([where[b] for b in key_of(x)])                 # KeyError: a dof no rank owns
            for name, want in gvalues[-1][key].items():
                got = np.concatenate([p[key][name] for p in parts])[perm]
                assert np.array_equal(got, want), (key, name)
            print(f"values of slot {key}: {x.shape[0]} dofs, {len(gvalues[-1][key])} quantities bit for bit", flush=True)
        if gfm is not None:
            mworst = 0.0
            for name in ("K_ecs", "phi_M"):
                w = gfm.watches[name]
                n_ref, n_got = gfser[f"{name}/n"], fser[f"{name}/n"]
                assert np.array_equal(n_got, n_ref), (name, n_got, n_ref)
                assert n_ref.min() > 0 and n_ref.max() < w.n and np.ptp(n_ref) > 0, (name, n_ref)
                for i in range(n_rec):
                    state = tm.analytic_state(g, L_x, (i + 1) * DT)
                    v = state["c"][0][0] if name == "K_ecs" else state["phi_M"][2]
                    beyond = v >= tm.LEVEL[name]
                    assert beyond.sum() == n_ref[i]
                    bound = int(beyond.sum()) * tm.EPS * float(w.w[beyond].sum())
                    diff = abs(fser[f"{name}/measure"][i] - gfser[f"{name}/measure"][i])
                    assert diff <= bound, (name, i, diff, bound)
                    mworst = max(mworst, diff / bound)
                print(f"maps series {name}: n {n_ref.astype(int).tolist()} of {w.n} exact", flush=True)
            print(f"maps series: largest |partitioned - single| / bound of a measure: {mworst:.3f}", flush=True)
            for name in gfm.watches:
                want = gfm.maps(name)
                union = {k: np.concatenate([p[name][k] for p in map_parts]) for k in want}
                where = {b: i for i, b in enumerate(key_of(union["locations"]))}
                assert len(where) == union["locations"].shape[0] == want["locations"].shape[0], name
                perm = np.array([where[b] for b in key_of(want["locations"])])
                for k, v in want.items():
                    assert np.array_equal(union[k][perm], v, equal_nan=k != "count"), (name, k)
            print("per-item maps of the same FieldMaps: bit for bit", flush=True)
    if a.cost:
        taps = [st.taps[n] for n in ("monitor", "track") if n in st.taps]
        for tap in taps:
            tap.fields = False
        out = {}
        k0 = (a.steps or a.records) + 1
        for name, some in (("monitor", taps[:1]), ("maps", taps[1:]), ("both", taps)):
            if not some:
                continue
            ms = []
            for w in range(4):                                  # the first window warms up
                st.dp.sync()
                dist.barrier()
                t0 = time.perf_counter()
                for k in range(a.cost):
                    for tap in some:
                        tap.tick(k0, DT)
                    k0 += 1
                st.dp.sync()
                ms.append((time.perf_counter() - t0) * 1e3 / a.cost)
            out[name] = ms[1:]
        for tap in taps:
            tap.drain()
        print(json.dumps(dict(rank=rank, world=world, records=a.cost, us_per_partitioned_record={
            k: [round(x * 1e3, 1) for x in v] for k, v in out.items()})), flush=True)
    if rank == 0:
        print("PARTITION MONITOR OK", flush=True)
    pc.finish()


if __name__ == "__main__":
    main()
