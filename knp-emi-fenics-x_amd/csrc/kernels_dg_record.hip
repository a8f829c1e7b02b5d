// The jump seminorm of the DG variant on gfx950: for every sub-domain s and every field u (the K concentrations, the
// eliminated ion included, and the potential)
//
//     J_s(u) = sum over the interior facets F with both cells in s of  int_F (1 / h_F) [u]^2 dS,
//
// the quantity the interior penalty of the assembly kernels controls (kernels_dg.hip, kernels_dg_hex.hip: pen = gamma / h_F),
// in ONE launch per record.  The reference has no DG code and so no such diagnostic (kernels_dg.hip says what it does
// have); the definition is that of the penalty terms of oracle/knpemi_dg_oracle.py with kappa = gamma = 1.
//
// Decomposition.  One lane per (cell, local facet): the lane of the LOWER-numbered cell of an interior facet (finfo kind
// 1) computes the facet, every other lane contributes zeros -- a facet is counted once, membrane and boundary facets never.
// The lane loads the records of its facet's vertices on both sides (the neighbour's through finfo's vertex map) and, for
// the geometry, the vertex behind the facet on either side; the five values of a record (c0 c1 c2 c3 phi) come with one
// 64-byte load, so all K + 1 fields cost what one costs.
//   simplices   [u] is linear on F and 1 / h_F constant: J_F = (1 / h_F) |F| d^T M d with M the facet's P1 mass matrix over
//               |F|, i.e. (sum_a d_a^2 + (sum_a d_a)^2) / (nf (nf + 1)); 1 / h_F = (1 / h_T + 1 / h_N) / 2 with the heights of
//               the two opposite vertices over the facet, which are the |grad lambda_opposite| of the assembly;
//   hexahedra   the 2 x 2 Gauss rule on the facet; 1 / h_F at a point is (|c_T| + |c_N|) / 2 of the assembly's facet frame,
//               |c| = |t_s x t_t| / |(t_s x t_t) . d| with the shared tangents and the cell's depth vector d; box meshes use
//               the constant edge lengths of box_h as the box kernels do.
// Reduction, in a fixed order and without floating-point atomics: per sub-domain and field a butterfly over the wave, the
// four waves of the workgroup in order, the workgroup's partial published as record_tail.h says; the workgroup that arrives
// last (kn_arrive_last) folds every column over the workgroups -- lane l of a wave takes the workgroups l, l + 64, ... in
// order, then the butterfly -- and leaves the n_sub x 5 values in a small table.  A KNPEMI_DG_JUMP observable is an
// OBS_SUM entry of observe_kernel on that table (knpemi_record.hip), so the row is appended by the observe launch that
// follows on the same stream.  Two identical runs give identical bits.
#include "dg_internal.h"
#include "record_tail.h"

namespace {

using namespace kn_dg;

constexpr int JP_THREADS = 256;
constexpr double JP_G0 = 0.21132486540518711775, JP_G1 = 0.78867513459481288225;   // 2-point Gauss on [0, 1]

struct JumpArgs {
  int n_sub, box, n_blk;
  double* part;                  // [n_blk][n_sub * KN_DG_JSLOTS]
  double* tab;                   // [KN_MAXSUB * KN_DG_JSLOTS]
  unsigned long long* ctl;       // [4]: only the ticket is used
};

// the five field values of a record in table order: ions 0..3, phi
__device__ __forceinline__ void jp_values(const DofRec& r, double (&v)[KN_DG_JSLOTS]) {
#pragma unroll
  for (int q = 0; q < KN_MAXK; ++q) v[q] = r.c[q];
  v[KN_MAXK] = r.phi;
}

// facet f of simplex T against its neighbour N: acc[q] = (1 / h_F) |F| d^T M d of field q
template <int NV>
__device__ __forceinline__ void jp_simplex(const DgDev& D, int T, int f, int N, unsigned fi, double (&acc)[KN_DG_JSLOTS]) {
  constexpr int GD = NV - 1, NF = NV - 1;
  double P[NF][GD], sum[KN_DG_JSLOTS], sq[KN_DG_JSLOTS];
#pragma unroll
  for (int q = 0; q < KN_DG_JSLOTS; ++q) sum[q] = sq[q] = 0.0;
#pragma unroll
  for (int m = 0; m < NF; ++m) {
    const int a = m < f ? m : m + 1;                 // local vertex at facet position m
    const int jn = (fi >> (4 + 2 * a)) & 3;          // the neighbour's local index of the same vertex
    const DofRec rT = load_rec(D.rec, T * NV + a), rN = load_rec(D.rec, N * NV + jn);
    double vT[KN_DG_JSLOTS], vN[KN_DG_JSLOTS];
    jp_values(rT, vT);
    jp_values(rN, vN);
#pragma unroll
    for (int d = 0; d < GD; ++d) P[m][d] = rT.x[d];
#pragma unroll
    for (int q = 0; q < KN_DG_JSLOTS; ++q) {
      const double d = vT[q] - vN[q];
      sum[q] += d;
      sq[q] = fma(d, d, sq[q]);
    }
  }
  const DofRec oT = load_rec(D.rec, T * NV + f), oN = load_rec(D.rec, N * NV + (int)((fi >> 2) & 3));
  // cr: normal to the facet with |cr| = (nf - 1)! |F|; the heights of the opposite vertices are |(x - P_0) . cr| / |cr|
  double cr[GD], eT[GD], eN[GD];
#pragma unroll
  for (int d = 0; d < GD; ++d) { eT[d] = oT.x[d] - P[0][d]; eN[d] = oN.x[d] - P[0][d]; }
  if constexpr (NV == 3) {
    cr[0] = P[1][1] - P[0][1];
    cr[1] = -(P[1][0] - P[0][0]);
  } else {
    const double ux = P[1][0] - P[0][0], uy = P[1][1] - P[0][1], uz = P[1][2] - P[0][2];
    const double vx = P[2][0] - P[0][0], vy = P[2][1] - P[0][1], vz = P[2][2] - P[0][2];
    cr[0] = uy * vz - uz * vy; cr[1] = uz * vx - ux * vz; cr[2] = ux * vy - uy * vx;
  }
  double a2 = 0.0, dT = 0.0, dN = 0.0;
#pragma unroll
  for (int d = 0; d < GD; ++d) { a2 = fma(cr[d], cr[d], a2); dT = fma(cr[d], eT[d], dT); dN = fma(cr[d], eN[d], dN); }
  // (1 / h_F) |F| = (|cr| / |dT| + |cr| / |dN|) / 2 * |cr| / (nf - 1)!
  const double w = 0.5 * a2 * (fast_rcp(fabs(dT)) + fast_rcp(fabs(dN))) * (NV == 3 ? 1.0 : 0.5) * (1.0 / (NF * (NF + 1)));
#pragma unroll
  for (int q = 0; q < KN_DG_JSLOTS; ++q) acc[q] = w * fma(sum[q], sum[q], sq[q]);
}

// facet f = 2 a + b of hexahedron T against its neighbour N, 2 x 2 Gauss rule
__device__ __forceinline__ void jp_hex(const DgDev& D, int T, int f, int N, unsigned fi, int box, double (&acc)[KN_DG_JSLOTS]) {
  const int a = f >> 1, b = f & 1, a1 = a == 0 ? 1 : 0, a2 = a == 2 ? 1 : 2;
  const int ao = ((fi >> 2) & 7) >> 1;
  double xm[4][3], dT[4][3], dN[4][3], dv[4][KN_DG_JSLOTS];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int jv = (b << a) | ((m & 1) << a1) | ((m >> 1) << a2);      // this cell's vertex at facet position m
    const int jn = (fi >> (5 + 3 * m)) & 7;                            // ... and the neighbour's
    const DofRec rT = load_rec(D.rec, T * 8 + jv), rN = load_rec(D.rec, N * 8 + jn);
    double vT[KN_DG_JSLOTS], vN[KN_DG_JSLOTS];
    jp_values(rT, vT);
    jp_values(rN, vN);
#pragma unroll
    for (int q = 0; q < KN_DG_JSLOTS; ++q) dv[m][q] = vT[q] - vN[q];
    if (!box) {                                                        // the vertices behind the facet: the depth vectors
      const double* bT = D.rec + (size_t)(T * 8 + (jv ^ (1 << a))) * KN_REC;
      const double* bN = D.rec + (size_t)(N * 8 + (jn ^ (1 << ao))) * KN_REC;
#pragma unroll
      for (int d = 0; d < 3; ++d) { xm[m][d] = rT.x[d]; dT[m][d] = bT[d] - rT.x[d]; dN[m][d] = bN[d] - rT.x[d]; }
    }
  }
  double wbox = 0.0;
  if (box) {
    const double* hT = D.box_h + (size_t)T * 3;
    wbox = 0.25 * hT[a1] * hT[a2] * 0.5 * (fast_rcp(hT[a]) + fast_rcp(D.box_h[(size_t)N * 3 + ao]));
  }
#pragma unroll
  for (int q = 0; q < KN_DG_JSLOTS; ++q) acc[q] = 0.0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    double Nm[4], ds[4], dt[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const double ws = ((m ^ p) & 1) ? JP_G0 : JP_G1, wt = (((m ^ p) >> 1) & 1) ? JP_G0 : JP_G1;
      Nm[m] = ws * wt;
      ds[m] = (m & 1) ? wt : -wt;
      dt[m] = (m >> 1) ? ws : -ws;
    }
    double w = wbox;
    if (!box) {
      double ts[3] = {0, 0, 0}, tt[3] = {0, 0, 0}, eT[3] = {0, 0, 0}, eN[3] = {0, 0, 0};
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          ts[d] = fma(ds[m], xm[m][d], ts[d]); tt[d] = fma(dt[m], xm[m][d], tt[d]);
          eT[d] = fma(Nm[m], dT[m][d], eT[d]); eN[d] = fma(Nm[m], dN[m][d], eN[d]);
        }
      const double cx = ts[1] * tt[2] - ts[2] * tt[1], cy = ts[2] * tt[0] - ts[0] * tt[2], cz = ts[0] * tt[1] - ts[1] * tt[0];
      const double A2 = cx * cx + cy * cy + cz * cz;                   // (surface element)^2
      const double detT = cx * eT[0] + cy * eT[1] + cz * eT[2], detN = cx * eN[0] + cy * eN[1] + cz * eN[2];
      // 0.25 A (|c_T| + |c_N|) / 2 with |c| = A / |det|
      w = 0.125 * A2 * (fast_rcp(fabs(detT)) + fast_rcp(fabs(detN)));
    }
#pragma unroll
    for (int q = 0; q < KN_DG_JSLOTS; ++q) {
      const double u = Nm[0] * dv[0][q] + Nm[1] * dv[1][q] + Nm[2] * dv[2][q] + Nm[3] * dv[3][q];
      acc[q] = fma(w * u, u, acc[q]);
    }
  }
}

template <int NV>
__global__ __launch_bounds__(JP_THREADS) void dg_jump_kernel(DgDev D, JumpArgs A) {
  constexpr int NFC = NV == 8 ? 6 : NV;
  __shared__ double sh[JP_THREADS / 64][KN_MAXSUB * KN_DG_JSLOTS];
  __shared__ int last;
  const int t = blockIdx.x * JP_THREADS + threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ns = A.n_sub * KN_DG_JSLOTS;
  double acc[KN_DG_JSLOTS];
#pragma unroll
  for (int q = 0; q < KN_DG_JSLOTS; ++q) acc[q] = 0.0;
  int s = -1;
  if (t < D.n_cell * NFC) {
    const int T = t / NFC, f = t - T * NFC;
    const int N = D.nbr[t];
    const unsigned fi = D.finfo[t];
    if (N > T && (fi & 3) == 1) {                    // interior, and this is its lower-numbered cell
      s = D.cell_sub[T];
      if constexpr (NV == 8) jp_hex(D, T, f, N, fi, A.box, acc);
      else jp_simplex<NV>(D, T, f, N, fi, acc);
    }
  }
  for (int ss = 0; ss < A.n_sub; ++ss)
#pragma unroll
    for (int q = 0; q < KN_DG_JSLOTS; ++q) {
      const double v = kn_wave_sum(s == ss ? acc[q] : 0.0);
      if (lane == 0) sh[wave][ss * KN_DG_JSLOTS + q] = v;
    }
  __syncthreads();
  const bool pub = (int)threadIdx.x < ns;
  if (pub) {
    double v = sh[0][threadIdx.x];
    for (int w = 1; w < JP_THREADS / 64; ++w) v += sh[w][threadIdx.x];
    kn_part_store(&A.part[(size_t)blockIdx.x * ns + threadIdx.x], v);
  }
  if (!kn_arrive_last(A.ctl, pub, &last)) return;
  // every column over the workgroups, in an order that does not depend on which workgroup came last
  for (int j = wave; j < ns; j += JP_THREADS / 64) {
    double v = 0.0;
    for (int p = lane; p < A.n_blk; p += 64) v += kn_part_load(&A.part[(size_t)p * ns + j]);
    v = kn_wave_sum(v);
    if (lane == 0) A.tab[j] = v;
  }
  if (threadIdx.x == 0) kn_reset_ticket(A.ctl);
}

}  // namespace

int kn_dg_jump_blocks(int n_cell, int NV) {
  const long long tasks = (long long)n_cell * (NV == 8 ? 6 : NV);
  return (int)((tasks + JP_THREADS - 1) / JP_THREADS);
}

int kn_dg_launch_jump(KnDevice* own, const kn_dg::DgDev& D, int NV, int n_sub, int box, const KnDgJump& J) {
  const JumpArgs a{n_sub, box, J.n_blk, J.part, J.tab, J.ctl};
  if (!kn_pick<3, 4, 8>(NV, [&](auto nv) {
        constexpr int V = decltype(nv)::value;
        hipLaunchKernelGGL(dg_jump_kernel<V>, dim3(J.n_blk), dim3(JP_THREADS), 0, own->stream, D, a);
      }))
    return kn_dg_not_built("dg_jump_kernel", NV, 0);
  return kn_launch_check("dg_jump_kernel");
}
