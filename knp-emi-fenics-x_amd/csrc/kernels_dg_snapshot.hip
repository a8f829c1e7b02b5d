// Field snapshots of a DG run on gfx950: every watched field of every watched space packed into one contiguous frame, in
// ONE launch per record (knpemi_record.hip: knpemi_dg_snapshot_record; the ring and the copy stream are the conforming
// path's).
//
// A DG field is broken: a mesh vertex carries one dof per cell that touches it.  A space is therefore (sub-domain or
// membrane tag, form), and the form says what an item is (KnDgSnapTab, dg_internal.h):
//   broken     one lane per dof (cell, local vertex) in the cell order of the sub-domain, or per membrane node (facet, a) of a
//              tag.  A bulk lane reads slots 3 .. 7 of its 64-byte record once, with three 16-byte loads (the coordinates
//              are not fetched), and serves every watch of the space from registers;
//   cell_mean  one lane per cell: its nv records are 64 nv contiguous bytes; the nodal values are summed in local-vertex
//              order 0 .. nv - 1 and divided by nv;
//   vertex     one lane per mesh vertex the space touches, in increasing vertex id: the lane walks its run of the incidence
//              list (vptr, vdof; dofs ascending), sums in list order and divides by the count.  Valence is unbounded, so
//              this is a loop.  Membrane spaces gather phi_M, I_ch and state columns the same way over the nodes of the tag
//              that share a mesh vertex.
// The three forms are one loop over the entries [lo, hi) of the item -- direct (broken: one entry, cell_mean: nv consecutive
// ones) or through vdof -- so the branch on the form, the loop over the watches and the branch on a watch's width are all
// uniform over the workgroup, as in snapshot_pack_kernel.  No LDS, no barrier, no atomics.
//
// Arithmetic: the sum starts from the first entry (so a lone -0.0 stays -0.0), then additions in list order, then one IEEE
// double division by the count; the broken form divides by nothing.  There is no multiply, so nothing can be contracted
// into an fma, and a frame is a bit-exact function of the fields (knpemi/dg_snapshots.py: frame_host restates it in numpy).
// An f32 watch stores (float)v: round to nearest even, denormals kept.
//
// Layout of the stores as in kernels_snapshot.hip: lane i of a space writes position i of every watch of the space, a
// watch starts at a multiple of KNPEMI_SNAPSHOT_ALIGN, and the stores are streaming or plain as kn_snapshot_stream_stores
// says -- the frame is read next by the copy engine, never by a kernel.
#include "dg_internal.h"

#define DG_SNAP_THREADS 256

extern "C" int kn_snapshot_stream_stores(int mode);

namespace {

struct DgSnapArgs {
  const KnDgSnapTab* tab;
  const double* rec;
  char* frame;
};

// the space of workgroup b: at most KNPEMI_DG_SNAPSHOT_MAX_SPACE - 1 steps, uniform
__device__ inline int space_of(const KnDgSnapTab& T, int b) {
  int p = 0;
  while (p + 1 < T.n_space && b >= T.bstart[p + 1]) ++p;
  return p;
}

template <bool STREAM, class V>
__device__ __forceinline__ void put(V v, V* dst) {
  if constexpr (STREAM) __builtin_nontemporal_store(v, dst);
  else *dst = v;
}

// slots 3 .. 7 of a dof record: c3 | c0 c1 | c2 phi (KN_CSLOT) into r[0 .. 4]
__device__ __forceinline__ void load_slots(const double* rec, int dof, double (&r)[5]) {
  const double2* q = reinterpret_cast<const double2*>(rec + (size_t)dof * KN_REC);
  const double2 b = q[1], c = q[2], d = q[3];
  r[0] = b.y; r[1] = c.x; r[2] = c.y; r[3] = d.x; r[4] = d.y;
}

template <bool STREAM>
__global__ __launch_bounds__(DG_SNAP_THREADS) void dg_snapshot_pack_kernel(DgSnapArgs A) {
  const KnDgSnapTab& T = *A.tab;
  const int p = space_of(T, (int)blockIdx.x);
  const int i = ((int)blockIdx.x - T.bstart[p]) * DG_SNAP_THREADS + (int)threadIdx.x;
  if (i >= T.n_items[p]) return;
  const int* sel = T.sel[p];
  const int item = sel ? sel[i] : i;
  const int form = T.form[p];

  // the entries of the item: [lo, hi), read through `list` (vertex) or taken as they are
  const int* list = nullptr;
  int lo, hi;
  if (form == KNPEMI_DG_SNAP_VERTEX) {
    list = T.vdof[p];
    lo = T.vptr[p][item];
    hi = T.vptr[p][item + 1];
  } else {
    const int* src = T.src[p];
    const int s = src ? src[item] : T.first[p] + item;
    const int n = form == KNPEMI_DG_SNAP_CELL_MEAN ? T.nv[p] : 1;
    lo = s * n;
    hi = lo + n;
  }
  const double cnt = (double)(hi - lo);
  const bool mean = form != KNPEMI_DG_SNAP_BROKEN;

  if (T.bulk[p]) {
    double r[5];
    load_slots(A.rec, list ? list[lo] : lo, r);
    for (int e = lo + 1; e < hi; ++e) {
      double q[5];
      load_slots(A.rec, list ? list[e] : e, q);
#pragma unroll
      for (int j = 0; j < 5; ++j) r[j] += q[j];
    }
    for (int k = T.wstart[p]; k < T.wstart[p + 1]; ++k) {
      const KnSnapWatch& W = T.w[k];
      const int s = W.slot - 3;      // 0 .. 4; selected without indexing r by a run-time value
      double v = r[0];
#pragma unroll
      for (int j = 1; j < 5; ++j) v = s == j ? r[j] : v;
      if (mean) v = v / cnt;
      char* dst = A.frame + W.off;
      if (W.f32) put<STREAM>((float)v, reinterpret_cast<float*>(dst) + i);      // round to nearest even
      else put<STREAM>(v, reinterpret_cast<double*>(dst) + i);
    }
  } else {
    for (int k = T.wstart[p]; k < T.wstart[p + 1]; ++k) {
      const KnSnapWatch& W = T.w[k];
      const double* d = W.dense;
      double v = d[list ? list[lo] : lo];
      for (int e = lo + 1; e < hi; ++e) v += d[list ? list[e] : e];
      if (mean) v = v / cnt;
      char* dst = A.frame + W.off;
      if (W.f32) put<STREAM>((float)v, reinterpret_cast<float*>(dst) + i);
      else put<STREAM>(v, reinterpret_cast<double*>(dst) + i);
    }
  }
}

}  // namespace

int kn_dg_launch_snapshot_pack(KnDevice* own, const KnDgSnap& S, const double* rec, char* frame) {
  if (S.n_blk == 0) return KNPEMI_OK;
  const DgSnapArgs A{S.tab, rec, frame};
  if (kn_snapshot_stream_stores(-1))
    hipLaunchKernelGGL(dg_snapshot_pack_kernel<true>, dim3(S.n_blk), dim3(DG_SNAP_THREADS), 0, own->stream, A);
  else
    hipLaunchKernelGGL(dg_snapshot_pack_kernel<false>, dim3(S.n_blk), dim3(DG_SNAP_THREADS), 0, own->stream, A);
  return kn_launch_check("dg_snapshot_pack_kernel");
}
