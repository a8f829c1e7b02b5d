"""Stream-ordered halo exchange rehearsal on ONE GPU with real RCCL: a world-size-1 nccl group sends the packed
halo buffer to itself.  Verifies that pack (library stream) -> RCCL send/recv -> unpack (library stream) is correctly
ordered WITHOUT host synchronisation when torch's current stream is the library's stream (ExternalStream)."""
import contextlib, io, os, sys, time
import numpy as np
import torch
import torch.distributed as dist

import partition_common as pc

os.environ.setdefault("MASTER_PORT", "29577")
pc.start("nccl", rank=0, world=1)
from knpemi import _lib as L
from setup_problem import Setup
with contextlib.redirect_stdout(io.StringIO()):
    s = Setup("tet", 0)
dp = s.a_emi.dp
lib = dp.lib
dev = torch.device("cuda", 0)
nv = int(dp.n_vert.sum())
rng = np.random.default_rng(0)
n = 3000
send_idx = torch.from_numpy(rng.choice(nv, n, replace=False).astype(np.int32)).to(dev)
recv_idx = torch.from_numpy(rng.permutation(nv)[:n].astype(np.int32)).to(dev)
w = int(lib.knpemi_halo_width(dp.h, 0))     # doubles per vertex of the bulk halo (c3 c0 c1 c2 phi)
send_buf = torch.empty(n * w, dtype=torch.float64, device=dev)
recv_buf = torch.empty(n * w, dtype=torch.float64, device=dev)
ext = torch.cuda.ExternalStream(lib.knpemi_stream(dp.h), device=dev)


def exchange():
    L.check(lib.knpemi_halo_pack(dp.h, 0, send_idx.data_ptr(), n, send_buf.data_ptr()))
    with torch.cuda.stream(ext):
        for req in dist.batch_isend_irecv([dist.P2POp(dist.isend, send_buf, 0), dist.P2POp(dist.irecv, recv_buf, 0)]):
            req.wait()
    L.check(lib.knpemi_halo_unpack(dp.h, 0, recv_idx.data_ptr(), n, recv_buf.data_ptr()))


phi0 = s.phi[0]
n0 = phi0.x.array.shape[0]
ok = True
t0 = time.perf_counter()
for it in range(300):
    phi0.x.array[:] = float(it) + np.arange(n0) * 1e-6
    dp.push(L.F_PHI, 0, 0, phi0)        # async upload on the library stream
    exchange()
    if it % 50 == 49 or it < 3:
        dp.sync()
        got = recv_buf.cpu().numpy().reshape(n, w)[:, w - 1]
        si = send_idx.cpu().numpy()
        exp = np.where(si < n0, float(it) + si * 1e-6, got)
        good = np.array_equal(got[si < n0], exp[si < n0])
        ok &= bool(good)
        print("iteration", it, "phi column of the received halo correct:", good, flush=True)
dp.sync()
el = time.perf_counter() - t0
print(f"{300 / el:.0f} exchanges/s including upload", "ALL OK" if ok else "MISMATCH")


def exchange_sync():
    L.check(lib.knpemi_halo_pack(dp.h, 0, send_idx.data_ptr(), n, send_buf.data_ptr()))
    dp.sync()
    for req in dist.batch_isend_irecv([dist.P2POp(dist.isend, send_buf, 0), dist.P2POp(dist.irecv, recv_buf, 0)]):
        req.wait()
    torch.cuda.current_stream().synchronize()
    L.check(lib.knpemi_halo_unpack(dp.h, 0, recv_idx.data_ptr(), n, recv_buf.data_ptr()))


for name, fn in (("stream-ordered", exchange), ("host-synchronised", exchange_sync)):
    for _ in range(20):
        fn()
    dp.sync()
    t0 = time.perf_counter()
    for _ in range(500):
        fn()
    dp.sync()
    print(f"{name}: {(time.perf_counter() - t0) / 500 * 1e6:.1f} us per exchange", flush=True)
# the library's own RCCL transport (knpemi_comm_*): same exchange, no torch.distributed in the loop
import ctypes as C
idbuf = C.create_string_buffer(128)
L.check(lib.knpemi_comm_unique_id(idbuf, 128))
L.check(lib.knpemi_comm_init(dp.h, 0, 1, idbuf.raw, 128))
peer = np.zeros(1, np.int32)
off0 = np.zeros(1, np.int64)
cnt = np.full(1, n * w, np.int64)
i64 = C.POINTER(C.c_int64)


def exchange_native():
    L.check(lib.knpemi_halo_pack(dp.h, 0, send_idx.data_ptr(), n, send_buf.data_ptr()))
    L.check(lib.knpemi_comm_sendrecv(dp.h, send_buf.data_ptr(), recv_buf.data_ptr(), 1, L.iptr(peer), off0.ctypes.data_as(i64),
                                     cnt.ctypes.data_as(i64), off0.ctypes.data_as(i64), cnt.ctypes.data_as(i64)))
    L.check(lib.knpemi_halo_unpack(dp.h, 0, recv_idx.data_ptr(), n, recv_buf.data_ptr()))


for it in range(5):
    phi0.x.array[:] = 1000.0 + it + np.arange(n0) * 1e-6
    dp.push(L.F_PHI, 0, 0, phi0)
    recv_buf.zero_()
    torch.cuda.synchronize()
    exchange_native()
    dp.sync()
    got = recv_buf.cpu().numpy().reshape(n, w)[:, w - 1]
    si = send_idx.cpu().numpy()
    good = np.array_equal(got[si < n0], (1000.0 + it + si * 1e-6)[si < n0])
    ok &= bool(good)
    print("library RCCL exchange", it, "correct:", good, flush=True)
red = torch.arange(8, dtype=torch.float64, device=dev)
L.check(lib.knpemi_comm_allreduce(dp.h, red.data_ptr(), 8))
dp.sync()
ok &= bool(torch.equal(red.cpu(), torch.arange(8, dtype=torch.float64)))
print("library RCCL all-reduce (one rank) correct:", bool(torch.equal(red.cpu(), torch.arange(8, dtype=torch.float64))), flush=True)

# the distributed Krylov solves with the library's own hooks (one rank: no neighbours, every vertex owned) against the
# plain single-GPU solves of the same systems
from knpemi.pdeSolver import create_solver_emi, create_solver_knp
s.perturb()
emi = create_solver_emi(s.a_emi, s.L_emi, s.phi, s.entity_maps, s.subdomain_list, None, p=s.p_emi, direct=False)
knp = create_solver_knp(s.a_knp, s.L_knp, s.c, s.entity_maps, s.subdomain_list, None, p=s.p_knp, direct=False)
emi.assemble()
n_emi = dp._pattern(L.A_EMI)[0]
n_knp = dp._pattern(L.A_KNP)[0]
it0, _ = dp.solve(L.B_EMI, 1e-10, 1e-40)
x0 = dp.get_solution(L.B_EMI, n_emi)
knp.assemble()
dp.solve(L.B_KNP, 1e-10, 1e-40)
c0 = dp.get_solution(L.B_KNP, n_knp)
Ak, bk = dp.csr(L.A_KNP), dp.rhs(L.B_KNP)
r0 = np.linalg.norm(bk - Ak @ c0) / np.linalg.norm(bk)
red8 = torch.zeros(8, dtype=torch.float64, device=dev)
own = np.ones(nv, np.uint8)
empty_i, empty_d = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
z32, z64 = np.zeros(0, np.int32), np.zeros(0, np.int64)
for which in (L.B_EMI, L.B_KNP):
    L.check(lib.knpemi_comm_set_vector_plan(dp.h, which, empty_i.data_ptr(), 0, empty_i.data_ptr(), 0, empty_d.data_ptr(),
                                            empty_d.data_ptr(), 0, L.iptr(z32), z64.ctypes.data_as(i64), z64.ctypes.data_as(i64),
                                            z64.ctypes.data_as(i64), z64.ctypes.data_as(i64)))
L.check(lib.knpemi_set_distributed(dp.h, own.ctypes.data_as(L.c_u8_p), red8.data_ptr(),
                                   C.cast(lib.knpemi_comm_allreduce_hook, C.c_void_p),
                                   C.cast(lib.knpemi_comm_halo_hook, C.c_void_p), dp.h))
dp.set_solution(L.B_EMI, np.zeros(n_emi))
emi.assemble()
it1, _ = dp.solve(L.B_EMI, 1e-10, 1e-40)
x1 = dp.get_solution(L.B_EMI, n_emi)
dp.set_solution(L.B_EMI, x0)
knp.assemble()
dp.solve(L.B_KNP, 1e-10, 1e-40)
c1 = dp.get_solution(L.B_KNP, n_knp)
Ak, bk = dp.csr(L.A_KNP), dp.rhs(L.B_KNP)
r1 = np.linalg.norm(bk - Ak @ c1) / np.linalg.norm(bk)
e_phi = np.abs((x1 - x1.mean()) - (x0 - x0.mean())).max() / np.abs(x0 - x0.mean()).max()
e_c = max(r0, r1)          # the two KNP systems differ (phi in place vs re-uploaded): each solution against its own system
good = e_phi < 1e-6 and e_c < 1e-9
ok &= bool(good)
print(f"distributed solves through the library's hooks (one rank): EMI {it0} -> {it1} iterations, "
      f"EMI difference {e_phi:.2e}, KNP residuals {r0:.1e} / {r1:.1e}:", "correct" if good else "WRONG", flush=True)
L.check(lib.knpemi_set_distributed(dp.h, None, None, None, None, None))

# host-side cost of one stream-ordered exchange (enqueue only) against its duration on the stream
for name, fn in (("library RCCL", exchange_native),):
    for _ in range(20):
        fn()
    dp.sync()
    ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(ext):
        ea.record()
    t0 = time.perf_counter()
    for _ in range(200):
        fn()
    t_host = time.perf_counter() - t0
    with torch.cuda.stream(ext):
        eb.record()
    dp.sync()
    torch.cuda.synchronize()
    print(f"{name}: host enqueue {t_host / 200 * 1e6:.1f} us per exchange, on the stream {ea.elapsed_time(eb) / 200 * 1e3:.1f} us", flush=True)
for _ in range(20):
    exchange()
dp.sync()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
with torch.cuda.stream(ext):
    e0.record()
t0 = time.perf_counter()
for _ in range(200):
    exchange()
t_host = time.perf_counter() - t0
with torch.cuda.stream(ext):
    e1.record()
dp.sync()
torch.cuda.synchronize()
print(f"stream-ordered: host enqueue {t_host / 200 * 1e6:.1f} us per exchange, on the stream {e0.elapsed_time(e1) / 200 * 1e3:.1f} us", flush=True)
pc.finish(barrier=False)
sys.exit(0 if ok else 1)
