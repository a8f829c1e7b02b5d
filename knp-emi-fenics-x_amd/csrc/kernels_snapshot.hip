// Field snapshots on gfx950: every watched field of every watched space packed into one contiguous frame, in ONE launch
// per record.
//
// The reference's astrocyte study writes every field every save_frequency steps
// (examples/local_astrocyte_depolarization/run_stim_duration.py:52-90, 487-494); with the fields resident on the device
// that was one strided gather and one blocking copy per field.  Here one launch gathers all of them into a frame that a
// copy stream takes to pinned host memory in one piece (knpemi_record.hip: knpemi_snapshot_record).
//
// Layout: one item per lane, 256-thread workgroups; KnSnapTab groups the watches by space (the vertices of a sub-domain,
// the membrane dofs of a cell) and every workgroup belongs to one space (bstart), so the loop over the watches of the space
// and the branch on a watch's source and width are uniform over the workgroup.  Lane i of a space stores position i of
// every watch of the space: writes are contiguous, 4 or 8 bytes per lane, and a watch starts at a multiple of
// KNPEMI_SNAPSHOT_ALIGN (256 bytes), so every wavefront's store covers whole 128-byte lines.  With a selection the lane reads
// item sel[i], without one item i.  A bulk lane reads slots 3 .. 7 of its 64-byte vertex record once, with three 16-byte loads
// (the coordinates x, y are not fetched), and serves phi, every c_prev and the eliminated ion from registers; the solver's c,
// phi_M, I_ch and the rows of the models' state tables are dense arrays, read with unit stride.
//
// The frame is read next by the copy engine, never by a kernel: the stores may be streaming (non-temporal) ones or plain
// ones (kn_snapshot_stream_stores; DESIGN.md 3.4.7 has the measurement behind the default).
#include "knpemi_internal.h"

#define SNAP_THREADS 256

namespace {

// 1: streaming stores, 0: plain ones
int g_stream_stores = 1;

struct SnapArgs {
  const KnSnapTab* tab;
  const double* VR;
  char* frame;
};

// the space of workgroup b: at most KN_MAPS_MAXSPACE - 1 steps, uniform
__device__ inline int space_of(const KnSnapTab& T, int b) {
  int p = 0;
  while (p + 1 < T.n_space && b >= T.bstart[p + 1]) ++p;
  return p;
}

template <bool STREAM, class V>
__device__ __forceinline__ void put(V v, V* dst) {
  if constexpr (STREAM) __builtin_nontemporal_store(v, dst);
  else *dst = v;
}

template <bool STREAM>
__global__ __launch_bounds__(SNAP_THREADS) void snapshot_pack_kernel(SnapArgs A) {
  const KnSnapTab& T = *A.tab;
  const int p = space_of(T, (int)blockIdx.x);
  const int i = ((int)blockIdx.x - T.bstart[p]) * SNAP_THREADS + (int)threadIdx.x;
  if (i >= T.n_items[p]) return;
  const int* sel = T.sel[p];
  const int item = sel ? sel[i] : i;

  // slots 3 .. 7 of the vertex record: c3 | c0 c1 | c2 phi (KN_CSLOT); r[0] is slot 2 and unused
  double r[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (T.need_rec[p]) {
    const double2* q = reinterpret_cast<const double2*>(A.VR + ((size_t)T.first[p] + (size_t)item) * KN_REC);
    const double2 b = q[1], c = q[2], d = q[3];
    r[0] = b.x; r[1] = b.y; r[2] = c.x; r[3] = c.y; r[4] = d.x; r[5] = d.y;
  }
  for (int k = T.wstart[p]; k < T.wstart[p + 1]; ++k) {
    const KnSnapWatch& W = T.w[k];
    double v;
    if (W.dense) {
      v = W.dense[item];
    } else {
      const int s = W.slot - 2;      // 1 .. 5; selected without indexing r by a run-time value
      v = r[1];
#pragma unroll
      for (int j = 2; j < 6; ++j) v = s == j ? r[j] : v;
    }
    char* dst = A.frame + W.off;
    if (W.f32) put<STREAM>((float)v, reinterpret_cast<float*>(dst) + i);      // round to nearest even
    else put<STREAM>(v, reinterpret_cast<double*>(dst) + i);
  }
}

}  // namespace

// mode 0 / 1: plain / streaming stores from the next launch on; anything else only asks.  Returns the mode in force.
extern "C" int kn_snapshot_stream_stores(int mode) {
  if (mode == 0 || mode == 1) g_stream_stores = mode;
  return g_stream_stores;
}

int kn_launch_snapshot_pack(knpemi_handle* h, char* frame) {
  const auto& S = h->snap;
  if (S.n_blk == 0) return KNPEMI_OK;
  const SnapArgs A{S.tab, h->dev.VR, frame};
  KnProfScope prof(h->prof, KNPEMI_K_SNAPSHOT, h->stream);
  if (g_stream_stores)
    hipLaunchKernelGGL(snapshot_pack_kernel<true>, dim3(S.n_blk), dim3(SNAP_THREADS), 0, h->stream, A);
  else
    hipLaunchKernelGGL(snapshot_pack_kernel<false>, dim3(S.n_blk), dim3(SNAP_THREADS), 0, h->stream, A);
  return kn_launch_check("snapshot_pack_kernel");
}
