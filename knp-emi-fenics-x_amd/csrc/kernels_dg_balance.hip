// The per-cell ion balance of the DG variant on gfx950: what the scheme conserves cell by cell, recorded on the device.
// Testing the system of a solved ion k with v = 1 on one cell T leaves (the gradients of a cell's basis sum to zero)
//
//     (m_T,k(new) - m_T,k(old)) / dt + sum over the interior facets F of T of H_F,k(c_new, phi) = mem_T,k + src_T,k  (+ residual)
//
// with m_T,k = int_T c_k, mem the membrane term of b_knp, src the ECS source and H_F the numerical outflow of the assembly
// kernels (kernels_dg.hip, kernels_dg_hex.hip), kept in its three parts
//     consistency  - int_F {D_k grad c_k} . n_T
//     penalty        int_F (gamma / h_F) {D_k} [c_k]
//     drift          int_F beta_F c_k^up,   beta_F = -z_k psi {D_k grad phi} . n_T,  upwind side T when beta_F > 0.
// The reference has no DG code and so no such record (kernels_dg.hip says what it does have); the definitions are those of
// oracle/knpemi_dg_oracle.py tested with the indicator of a cell, the membrane transfer that of knpemi/exchange.py.
//
// Two launches per recorded step, both on the handle's stream:
//   dg_balance_membrane_kernel  between the assembly and the solve of the concentrations (c old, phi new, phi_M old, I_ch):
//       mem, m_old and src of every cell and ion into the cell table, and per membrane tag the integrals of j_k^e, j_k^i,
//       I_cap, I_ch,tot and the area;
//   dg_balance_flux_kernel      at the end of the step (c new): the three parts of the outflow, m_new and the defect into
//       the table, and the series row.
// Decomposition, both launches.  A workgroup owns BL_THREADS / (facets per cell) whole cells and stages their records --
// consecutive in memory -- in LDS with one coalesced pass.  Phase 1: one lane per (cell, local facet) computes its facet
// for all K ions from the records of the two cells -- the five field values of a record come with one 64-byte read, the
// own cell's from LDS, the neighbour's from LDS when it is one of the workgroup's cells -- and leaves the result in LDS;
// the lanes of BOTH cells of a facet compute it, so phase 2, one lane per cell, sums the cell's facets in local-facet
// order without atomics and without a second pass, adds the cell's mass integrals (records from LDS) and writes the
// cell's entries of the table, which is stored column by column so that consecutive lanes write consecutive addresses.
//   simplices   D, beta and 1 / h_F = (|grad lambda_T| + |grad lambda_N|) / 2 are constant on the facet: |F| times facet
//               means, with the gradients of `geometry` (dg_internal.h); the lane renumbers both cells so that the vertex
//               opposite the facet is local vertex 0, as the assembly's lanes do;
//   hexahedra   the 2 x 2 Gauss rule with the normal, both cells' normal derivatives, beta (and so the upwind side) and
//               1 / h_F per point from hx_frame (dg_internal.h); box meshes take the constant frame of box_h;
//   masses      closed form on simplices, the 2 x 2 x 2 Gauss rule with |det J| per point on hexahedra;
//   membrane    the assembly's degree-6 facet rule (D.qtab; hexahedra: 4 x 4 Gauss with the surface element per point).
// Reduction, in a fixed order and without floating-point atomics (record_tail.h, as dg_jump_kernel): a butterfly over the
// wave, the waves of the workgroup in order, the workgroup's partial published by its first wave; the workgroup that
// arrives last folds every column over the workgroups -- lane l takes the workgroups l, l + 64, ... in order, then the
// butterfly -- and appends the row.  Two identical runs give identical bits.
#include "dg_internal.h"
#include "record_tail.h"

namespace {

using namespace kn_dg;

constexpr int BL_THREADS = 256, BL_WAVES = BL_THREADS / 64;
enum { BL_MEM = 0, BL_CONS, BL_PEN, BL_DRIFT, BL_MOLD, BL_MNEW, BL_SRC, BL_DEFECT };
static_assert(BL_DEFECT + 1 == KN_DG_BCOLS, "columns of the cell table");

template <int NV> constexpr int bl_nfc() { return NV == 8 ? 6 : NV; }
template <int NV> constexpr int bl_cpb() { return BL_THREADS / bl_nfc<NV>(); }      // cells per workgroup

struct BalArgs {
  int K, n_sub, n_tag, box, splitting, want_cells, n_blk, capacity, n_cols;
  double* cells;
  double* part;
  double* mpart;
  double* tagtab;
  unsigned long long* ctl;
  unsigned long long* mctl;
  double* rows;
  const int* facet_tag;
};

// The cell table on the device is [K][KN_DG_BCOLS][n_cell]: the lanes of phase 2 are consecutive cells, so every column is
// written (and read back) with consecutive addresses; knpemi_dg_balance_cells transposes it on the way out.
static_assert(KN_REC == 8, "bl_stage copies a record as four 16-byte pieces");
__device__ __forceinline__ double* bl_at(double* cells, int n_cell, int k, int col, int T) {
  return cells + (size_t)(k * KN_DG_BCOLS + col) * n_cell + T;
}

// integrals of the cell's basis functions: sum_j W[j] u_j = int_T u
template <int NV>
__device__ __forceinline__ void bl_cell_weights(const double (&X)[NV][3], double (&W)[NV]) {
  if constexpr (NV != 8) {
    double Y[NV][NV - 1];
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int d = 0; d < NV - 1; ++d) Y[j][d] = X[j][d];
    Geo<NV> G;
    geometry<NV>(Y, G);
#pragma unroll
    for (int j = 0; j < NV; ++j) W[j] = G.vol * (1.0 / NV);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) W[j] = 0.0;
#pragma unroll 1
    for (int p = 0; p < 8; ++p) {
      double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, Nj[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int x = j ^ p;
        const double w0 = (x & 1) ? HX_G0 : HX_G1, w1 = (x & 2) ? HX_G0 : HX_G1, w2 = (x & 4) ? HX_G0 : HX_G1;
        const double d0 = (j & 1) ? w1 * w2 : -(w1 * w2), d1 = (j & 2) ? w0 * w2 : -(w0 * w2), d2 = (j & 4) ? w0 * w1 : -(w0 * w1);
        Nj[j] = w0 * w1 * w2;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          J[0][d] = fma(d0, X[j][d], J[0][d]); J[1][d] = fma(d1, X[j][d], J[1][d]); J[2][d] = fma(d2, X[j][d], J[2][d]);
        }
      }
      const double det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) + J[0][1] * (J[1][2] * J[2][0] - J[1][0] * J[2][2]) +
                         J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
      const double wd = 0.125 * fabs(det);
#pragma unroll
      for (int j = 0; j < 8; ++j) W[j] = fma(wd, Nj[j], W[j]);
    }
  }
}

// The records of the workgroup's own cells are consecutive: one coalesced pass stages them in LDS (16 bytes per lane and
// instruction, the 10-double pitch of the assembly kernels), and both phases read them from there; a neighbour's record
// comes from LDS when the neighbour is one of the workgroup's cells, else from memory.
struct BlOwn {
  const double* lrec;
  int row0, nrows;               // the staged records are the dofs row0 .. row0 + nrows - 1
};
template <int NV>
__device__ __forceinline__ void bl_stage(double* lrec, const double* __restrict__ rec, int cell0, int ncell, int tid) {
  const double2* src = reinterpret_cast<const double2*>(rec + (size_t)cell0 * NV * KN_REC);
  const int n = ncell * NV * (KN_REC / 2);
  for (int e = tid; e < n; e += BL_THREADS)
    *reinterpret_cast<double2*>(lrec + (e >> 2) * DG_RPITCH + (e & 3) * 2) = src[e];
}
__device__ __forceinline__ DofRec bl_rec(const DgDev& D, const BlOwn& O, int dof) {
  const int l = dof - O.row0;
  return l >= 0 && l < O.nrows ? lds_rec(O.lrec, l) : load_rec(D.rec, dof);
}

// the records of the own cell T: concentrations, and the integral weights from the coordinates
template <int NV>
__device__ __forceinline__ void bl_cell(const BlOwn& O, int T, double (&c)[NV][KN_MAXK], double (&W)[NV]) {
  double X[NV][3];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const DofRec r = lds_rec(O.lrec, T * NV + j - O.row0);
#pragma unroll
    for (int d = 0; d < 3; ++d) X[j][d] = r.x[d];
#pragma unroll
    for (int k = 0; k < KN_MAXK; ++k) c[j][k] = r.c[k];
  }
  bl_cell_weights<NV>(X, W);
}

// ---------------------------------------------------------------------------------------------------------------------
// membrane launch
// ---------------------------------------------------------------------------------------------------------------------
// One point of the membrane rule: the traces at the point -> w j_k of every ion on this side, w I_cap, w I_ch,tot, w.
// j_k^s = (I_ch,k + alpha_k^s (I_cap - S I_ch,tot)) / (F z_k),  I_cap = C_M ([phi] - phi_M) / dt  (knpemi/exchange.py)
__device__ __forceinline__ void bl_mem_point(const DgConsts& C, int K, int s, int splitting, double w, const double (&cq)[KN_MAXK],
                                             const double (&iq)[KN_MAXK], double jq, double pq, double itq,
                                             double (&acc)[KN_MAXK], double& cap, double& chan, double& area) {
  double asum = 0.0;
#pragma unroll
  for (int k = 0; k < KN_MAXK; ++k)
    if (k < K) asum += C.az2D[s][k] * cq[k];
  const double icap = C.C_M * C.inv_dt * (jq - pq);
  const double drive = splitting ? icap - itq : icap;
  const double ra = 1.0 / asum;
#pragma unroll
  for (int k = 0; k < KN_MAXK; ++k)
    if (k < K) acc[k] += w * (iq[k] + C.az2D[s][k] * cq[k] * ra * drive) / (C.F * C.z[k]);
  cap += w * icap;
  chan += w * itq;
  area += w;
}

template <int NV>
__global__ __launch_bounds__(BL_THREADS) void dg_balance_membrane_kernel(DgDev D, const DgConsts* __restrict__ Cp, BalArgs A) {
  constexpr int NFC = bl_nfc<NV>(), CPB = bl_cpb<NV>(), NF = NV == 8 ? 4 : NV - 1;
  __shared__ __attribute__((aligned(16))) double lrec[CPB * NV * DG_RPITCH];
  __shared__ double fm[KN_MAXK][BL_THREADS];      // [ion][lane]: phase 1 writes it without bank conflicts
  __shared__ double sh[BL_WAVES][KN_DG_MAXTAG * KN_DG_BTAG];
  __shared__ int last;
  const DgConsts& C = *Cp;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int cell0 = blockIdx.x * CPB, ncell = min(CPB, D.n_cell - cell0);
  const int lc = tid / NFC, f = tid - lc * NFC;
  const int K = A.K;
  const BlOwn own{lrec, cell0 * NV, ncell * NV};
  bl_stage<NV>(lrec, D.rec, cell0, ncell, tid);
  __syncthreads();
  double acc[KN_MAXK], tv[KN_DG_BTAG];
#pragma unroll
  for (int k = 0; k < KN_MAXK; ++k) acc[k] = 0.0;
#pragma unroll
  for (int j = 0; j < KN_DG_BTAG; ++j) tv[j] = 0.0;
  int tg = -1;
  if (lc < ncell) {
    const int T = cell0 + lc;
    const unsigned fi = D.finfo[T * NFC + f];
    const int kind = fi & 3;
    if (kind >= 2) {
      const int N = D.nbr[T * NFC + f], mf = D.mfid[T * NFC + f], s = D.cell_sub[T];
      tg = A.facet_tag[mf];
      double xm[NF][3], cT[NF][KN_MAXK], jm[NF], pm[NF], It[NF], Ik[NF][KN_MAXK];
#pragma unroll
      for (int m = 0; m < NF; ++m) {
        int jv, jn, nd;
        if constexpr (NV == 8) {
          const int a = f >> 1, b = f & 1, a1 = a == 0 ? 1 : 0, a2 = a == 2 ? 1 : 2;
          jv = (b << a) | ((m & 1) << a1) | ((m >> 1) << a2);
          jn = (fi >> (5 + 3 * m)) & 7;
          nd = (fi >> (17 + 2 * m)) & 3;
        } else {
          jv = m < f ? m : m + 1;
          jn = (fi >> (4 + 2 * jv)) & 3;
          nd = (fi >> (12 + 2 * jv)) & 3;
        }
        const DofRec rT = lds_rec(lrec, T * NV + jv - own.row0);
        const double phN = D.rec[(size_t)(N * NV + jn) * KN_REC + 7];
#pragma unroll
        for (int d = 0; d < 3; ++d) xm[m][d] = rT.x[d];
#pragma unroll
        for (int k = 0; k < KN_MAXK; ++k) cT[m][k] = rT.c[k];
        jm[m] = kind == 2 ? phN - rT.phi : rT.phi - phN;      // phi_i - phi_e
        const int q = mf * NF + nd;
        pm[m] = D.phiM[q];
        double it = 0.0;
#pragma unroll
        for (int k = 0; k < KN_MAXK; ++k) {
          Ik[m][k] = k < K ? D.Ich[(size_t)k * D.nq + q] : 0.0;
          it += Ik[m][k];
        }
        It[m] = it;
      }
      double area0 = 0.0;                                      // simplices: weight of the reference rule -> the facet
      if constexpr (NV == 3) {
        const double ex = xm[1][0] - xm[0][0], ey = xm[1][1] - xm[0][1];
        area0 = sqrt(ex * ex + ey * ey);
      } else if constexpr (NV == 4) {
        const Vec3 u{xm[1][0] - xm[0][0], xm[1][1] - xm[0][1], xm[1][2] - xm[0][2]};
        const Vec3 v{xm[2][0] - xm[0][0], xm[2][1] - xm[0][1], xm[2][2] - xm[0][2]};
        const Vec3 cr = cross(u, v);
        area0 = sqrt(dot3(cr, cr));                            // 2 |F|: the reference triangle's weights sum to 1 / 2
      }
      const double* qw = D.qtab;
      const double* qN = D.qtab + D.nquad;
      const double* qd = D.qtab + D.nquad * 5;                 // hexahedra: derivatives of the facet's shape functions
      double cap = 0.0, chan = 0.0, area = 0.0;
      for (int q = 0; q < D.nquad; ++q) {
        double cq[KN_MAXK], iq[KN_MAXK], jq = 0.0, pq = 0.0, itq = 0.0;
        Vec3 ts{0, 0, 0}, tt{0, 0, 0};
#pragma unroll
        for (int k = 0; k < KN_MAXK; ++k) { cq[k] = 0.0; iq[k] = 0.0; }
#pragma unroll
        for (int m = 0; m < NF; ++m) {
          const double Nq = qN[q * NF + m];
          if constexpr (NV == 8) {
            const double d0 = qd[(q * 4 + m) * 2], d1 = qd[(q * 4 + m) * 2 + 1];
            ts.x += d0 * xm[m][0]; ts.y += d0 * xm[m][1]; ts.z += d0 * xm[m][2];
            tt.x += d1 * xm[m][0]; tt.y += d1 * xm[m][1]; tt.z += d1 * xm[m][2];
          }
#pragma unroll
          for (int k = 0; k < KN_MAXK; ++k) { cq[k] += Nq * cT[m][k]; iq[k] += Nq * Ik[m][k]; }
          jq += Nq * jm[m]; pq += Nq * pm[m]; itq += Nq * It[m];
        }
        double w = qw[q] * area0;
        if constexpr (NV == 8) {
          const Vec3 cr = cross(ts, tt);
          w = qw[q] * sqrt(dot3(cr, cr));
        }
        bl_mem_point(C, K, s, A.splitting, w, cq, iq, jq, pq, itq, acc, cap, chan, area);
      }
      // positive INTO the cell that owns the value: j is counted out of the intracellular cell
#pragma unroll
      for (int k = 0; k < KN_MAXK; ++k) {
        tv[(kind == 2 ? 0 : KN_MAXK) + k] = acc[k];
        if (kind == 3) acc[k] = -acc[k];
      }
      if (kind == 2) { tv[2 * KN_MAXK] = cap; tv[2 * KN_MAXK + 1] = chan; tv[2 * KN_MAXK + 2] = area; }
    }
  }
#pragma unroll
  for (int k = 0; k < KN_MAXK; ++k) fm[k][tid] = acc[k];
  for (int t = 0; t < A.n_tag; ++t)
#pragma unroll
    for (int j = 0; j < KN_DG_BTAG; ++j) {
      const double v = kn_wave_sum(tg == t ? tv[j] : 0.0);
      if (lane == 0) sh[wave][t * KN_DG_BTAG + j] = v;
    }
  __syncthreads();
  // phase 2: one lane per cell
  if (tid < ncell) {
    const int T = cell0 + tid, s = D.cell_sub[T];
    double c[NV][KN_MAXK], W[NV];
    bl_cell<NV>(own, T, c, W);
#pragma unroll
    for (int k = 0; k < KN_MAXK; ++k) {
      if (k >= K) continue;
      double mem = 0.0, m_old = 0.0, src = 0.0;
#pragma unroll
      for (int g = 0; g < NFC; ++g) mem += fm[k][tid * NFC + g];
#pragma unroll
      for (int j = 0; j < NV; ++j) m_old = fma(W[j], c[j][k], m_old);
      if (s == 0 && D.fsrc && k < K - 1) {
#pragma unroll
        for (int j = 0; j < NV; ++j) src = fma(W[j], D.fsrc[(size_t)k * D.n_dof + T * NV + j], src);
      }
      *bl_at(A.cells, D.n_cell, k, BL_MEM, T) = mem;
      *bl_at(A.cells, D.n_cell, k, BL_MOLD, T) = m_old;
      *bl_at(A.cells, D.n_cell, k, BL_SRC, T) = src;
    }
  }
  const int ns = A.n_tag * KN_DG_BTAG;
  bool pub = false;
  if (wave == 0)
    for (int j = lane; j < ns; j += 64) {
      double v = sh[0][j];
      for (int w = 1; w < BL_WAVES; ++w) v += sh[w][j];
      kn_part_store(&A.mpart[(size_t)blockIdx.x * ns + j], v);
      pub = true;
    }
  if (!kn_arrive_last(A.mctl, pub, &last)) return;
  for (int j = wave; j < ns; j += BL_WAVES) {
    double v = 0.0;
    for (int p = lane; p < A.n_blk; p += 64) v += kn_part_load(&A.mpart[(size_t)p * ns + j]);
    v = kn_wave_sum(v);
    if (lane == 0) A.tagtab[j] = v;
  }
  if (tid == 0) kn_reset_ticket(A.mctl);
}

// ---------------------------------------------------------------------------------------------------------------------
// flux launch
// ---------------------------------------------------------------------------------------------------------------------
// the five field values of a record: ions 0..3, phi
__device__ __forceinline__ void bl_values(const DofRec& r, double (&v)[KN_MAXK + 1]) {
#pragma unroll
  for (int q = 0; q < KN_MAXK; ++q) v[q] = r.c[q];
  v[KN_MAXK] = r.phi;
}

// the three parts of the outflow of ion k through a facet (or a facet point) of weight w, from the means (traces) cT, cN of
// the two sides, the normal derivatives gT, gN of c_k and pT, pN of phi, and pen = gamma / h_F
__device__ __forceinline__ void bl_parts(const DgConsts& C, int s, int k, double w, double pen, double cT, double cN, double gT,
                                         double gN, double pT, double pN, double* out) {
  const double Dk = C.D[s][k];
  const double beta = -C.z[k] * C.psi * 0.5 * Dk * (pT + pN);
  out[0] += -w * 0.5 * Dk * (gT + gN);
  out[1] += w * pen * Dk * (cT - cN);
  out[2] += w * beta * (beta > 0.0 ? cT : cN);
}

// facet f of simplex T against its neighbour N: out[3 k + (cons, pen, drift)]
template <int NV>
__device__ __forceinline__ void bl_simplex(const DgDev& D, const BlOwn& own, const DgConsts& C, int K, int T, int f, int N,
                                           unsigned fi, int s, double (&out)[3 * KN_MAXK]) {
  constexpr int GD = NV - 1;
  // both cells renumbered: local vertex 0 is the one opposite the facet, 1 .. NV - 1 the shared ones in T's order
  double XT[NV][GD], XN[NV][GD], vT[NV][KN_MAXK + 1], vN[NV][KN_MAXK + 1];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int pj = f + j >= NV ? f + j - NV : f + j;
    const int jn = j == 0 ? (fi >> 2) & 3 : (fi >> (4 + 2 * pj)) & 3;
    const DofRec rT = lds_rec(own.lrec, T * NV + pj - own.row0), rN = bl_rec(D, own, N * NV + jn);
#pragma unroll
    for (int d = 0; d < GD; ++d) { XT[j][d] = rT.x[d]; XN[j][d] = rN.x[d]; }
    bl_values(rT, vT[j]);
    bl_values(rN, vN[j]);
  }
  Geo<NV> GT, GN;
  geometry<NV>(XT, GT);
  geometry<NV>(XN, GN);
  const double g2 = dot<GD>(GT.g[0], GT.g[0]), rgf = fast_rsqrt(g2), gf = g2 * rgf;
  const double h2 = dot<GD>(GN.g[0], GN.g[0]), ghN = h2 * fast_rsqrt(h2);
  double n[GD];
#pragma unroll
  for (int d = 0; d < GD; ++d) n[d] = -GT.g[0][d] * rgf;
  const double area = GD * GT.vol * gf, pen = C.gamma * 0.5 * (gf + ghN);
  double gnT[KN_MAXK + 1], gnN[KN_MAXK + 1], mT[KN_MAXK + 1], mN[KN_MAXK + 1];
#pragma unroll
  for (int q = 0; q <= KN_MAXK; ++q) { gnT[q] = gnN[q] = mT[q] = mN[q] = 0.0; }
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const double a = dot<GD>(GT.g[j], n), b = dot<GD>(GN.g[j], n);
#pragma unroll
    for (int q = 0; q <= KN_MAXK; ++q) {
      gnT[q] = fma(a, vT[j][q], gnT[q]);
      gnN[q] = fma(b, vN[j][q], gnN[q]);
      if (j > 0) { mT[q] += vT[j][q]; mN[q] += vN[j][q]; }
    }
  }
#pragma unroll
  for (int k = 0; k < KN_MAXK; ++k)
    if (k < K)
      bl_parts(C, s, k, area, pen, mT[k] * (1.0 / GD), mN[k] * (1.0 / GD), gnT[k], gnN[k], gnT[KN_MAXK], gnN[KN_MAXK], &out[3 * k]);
}

// facet f = 2 a + b of hexahedron T against its neighbour N, 2 x 2 Gauss rule
__device__ __forceinline__ void bl_hex(const DgDev& D, const BlOwn& own, const DgConsts& C, int K, int T, int f, int N, unsigned fi,
                                       int s, int box, double (&out)[3 * KN_MAXK]) {
  const int a = f >> 1, b = f & 1, a1 = a == 0 ? 1 : 0, a2 = a == 2 ? 1 : 2;
  const int ao = ((fi >> 2) & 7) >> 1;
  double xm[4][3], dT[4][3], dN[4][3];
  double uT0[4][KN_MAXK + 1], uT1[4][KN_MAXK + 1], uN0[4][KN_MAXK + 1], uN1[4][KN_MAXK + 1];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int jv = (b << a) | ((m & 1) << a1) | ((m >> 1) << a2);      // this cell's vertex at facet position m
    const int jn = (fi >> (5 + 3 * m)) & 7;                            // ... and the neighbour's
    const DofRec rT0 = lds_rec(own.lrec, T * 8 + jv - own.row0), rT1 = lds_rec(own.lrec, T * 8 + (jv ^ (1 << a)) - own.row0);
    const DofRec rN0 = bl_rec(D, own, N * 8 + jn), rN1 = bl_rec(D, own, N * 8 + (jn ^ (1 << ao)));
    bl_values(rT0, uT0[m]); bl_values(rT1, uT1[m]);
    bl_values(rN0, uN0[m]); bl_values(rN1, uN1[m]);
#pragma unroll
    for (int d = 0; d < 3; ++d) { xm[m][d] = rT0.x[d]; dT[m][d] = rT1.x[d] - rT0.x[d]; dN[m][d] = rN1.x[d] - rT0.x[d]; }
  }
  double bA = 0.0, bcT = 0.0, bcN = 0.0;
  if (box) {      // the depth vectors are parallel to the normal: a_s = a_t = 0, c = -/+ 1 / |e_a|
    const double* hT = D.box_h + (size_t)T * 3;
    bA = hT[a1] * hT[a2];
    bcT = -fast_rcp(hT[a]);
    bcN = fast_rcp(D.box_h[(size_t)N * 3 + ao]);
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    FacetFrame F;
    if (box) {
      hx_shapes(p, F.N, F.ds, F.dt);
      F.A = bA; F.cT = bcT; F.cN = bcN;
      F.aTs = F.aTt = F.aNs = F.aNt = 0.0;
    } else {
      hx_frame(p, xm, dT, dN, true, F);
    }
    double gnT[KN_MAXK + 1], gnN[KN_MAXK + 1], trT[KN_MAXK], trN[KN_MAXK];
#pragma unroll
    for (int q = 0; q <= KN_MAXK; ++q) gnT[q] = gnN[q] = 0.0;
#pragma unroll
    for (int k = 0; k < KN_MAXK; ++k) trT[k] = trN[k] = 0.0;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const double gT0 = F.ds[m] * F.aTs + F.dt[m] * F.aTt - F.N[m] * F.cT, gT1 = F.N[m] * F.cT;
      const double gN0 = F.ds[m] * F.aNs + F.dt[m] * F.aNt - F.N[m] * F.cN, gN1 = F.N[m] * F.cN;
#pragma unroll
      for (int q = 0; q <= KN_MAXK; ++q) {
        gnT[q] += uT0[m][q] * gT0 + uT1[m][q] * gT1;
        gnN[q] += uN0[m][q] * gN0 + uN1[m][q] * gN1;
      }
#pragma unroll
      for (int k = 0; k < KN_MAXK; ++k) { trT[k] = fma(F.N[m], uT0[m][k], trT[k]); trN[k] = fma(F.N[m], uN0[m][k], trN[k]); }
    }
    const double w = 0.25 * F.A, pen = C.gamma * 0.5 * (fabs(F.cT) + fabs(F.cN));
#pragma unroll
    for (int k = 0; k < KN_MAXK; ++k)
      if (k < K) bl_parts(C, s, k, w, pen, trT[k], trN[k], gnT[k], gnN[k], gnT[KN_MAXK], gnN[KN_MAXK], &out[3 * k]);
  }
}

template <int NV>
__global__ __launch_bounds__(BL_THREADS) void dg_balance_flux_kernel(DgDev D, const DgConsts* __restrict__ Cp, BalArgs A) {
  constexpr int NFC = bl_nfc<NV>(), CPB = bl_cpb<NV>();
  __shared__ __attribute__((aligned(16))) double lrec[CPB * NV * DG_RPITCH];
  __shared__ double fl[3 * KN_MAXK][BL_THREADS];  // [part of ion][lane]: phase 1 writes it without bank conflicts
  __shared__ double sh[BL_WAVES][KN_MAXSUB * KN_MAXK * KN_DG_BSLOTS];
  __shared__ int last;
  __shared__ unsigned long long row;
  const DgConsts& C = *Cp;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int cell0 = blockIdx.x * CPB, ncell = min(CPB, D.n_cell - cell0);
  const int lc = tid / NFC, f = tid - lc * NFC;
  const int K = A.K;
  const BlOwn own{lrec, cell0 * NV, ncell * NV};
  bl_stage<NV>(lrec, D.rec, cell0, ncell, tid);
  __syncthreads();
  double out[3 * KN_MAXK];
#pragma unroll
  for (int j = 0; j < 3 * KN_MAXK; ++j) out[j] = 0.0;
  if (lc < ncell) {
    const int T = cell0 + lc;
    const unsigned fi = D.finfo[T * NFC + f];
    if ((fi & 3) == 1) {                               // membrane and boundary facets contribute nothing
      const int N = D.nbr[T * NFC + f], s = D.cell_sub[T];
      if constexpr (NV == 8) bl_hex(D, own, C, K, T, f, N, fi, s, A.box, out);
      else bl_simplex<NV>(D, own, C, K, T, f, N, fi, s, out);
    }
  }
#pragma unroll
  for (int j = 0; j < 3 * KN_MAXK; ++j) fl[j][tid] = out[j];
  __syncthreads();
  // phase 2: one lane per cell; q[k][slot]: what the cell adds to the row of its sub-domain
  double q[KN_MAXK][KN_DG_BSLOTS];
#pragma unroll
  for (int k = 0; k < KN_MAXK; ++k)
#pragma unroll
    for (int j = 0; j < KN_DG_BSLOTS; ++j) q[k][j] = 0.0;
  int s = -1;
  if (tid < ncell) {
    const int T = cell0 + tid;
    s = D.cell_sub[T];
    double c[NV][KN_MAXK], W[NV];
    bl_cell<NV>(own, T, c, W);
#pragma unroll
    for (int k = 0; k < KN_MAXK; ++k) {
      if (k >= K) continue;
      double part[3] = {0.0, 0.0, 0.0}, m_new = 0.0;
#pragma unroll
      for (int g = 0; g < NFC; ++g)
#pragma unroll
        for (int j = 0; j < 3; ++j) part[j] += fl[3 * k + j][tid * NFC + g];
#pragma unroll
      for (int j = 0; j < NV; ++j) m_new = fma(W[j], c[j][k], m_new);
      const int nc = D.n_cell;
      const double outflow = (part[0] + part[1]) + part[2];
      double defect = 0.0;
      if (k < K - 1)
        defect = (m_new - *bl_at(A.cells, nc, k, BL_MOLD, T)) * C.inv_dt + outflow - *bl_at(A.cells, nc, k, BL_MEM, T) -
                 *bl_at(A.cells, nc, k, BL_SRC, T);
      if (A.want_cells) {
        *bl_at(A.cells, nc, k, BL_CONS, T) = part[0];
        *bl_at(A.cells, nc, k, BL_PEN, T) = part[1];
        *bl_at(A.cells, nc, k, BL_DRIFT, T) = part[2];
        *bl_at(A.cells, nc, k, BL_MNEW, T) = m_new;
        *bl_at(A.cells, nc, k, BL_DEFECT, T) = defect;
      }
      q[k][0] = m_new; q[k][1] = outflow; q[k][2] = fabs(part[1]); q[k][3] = fabs(defect);
    }
  }
  for (int ss = 0; ss < A.n_sub; ++ss)
#pragma unroll
    for (int k = 0; k < KN_MAXK; ++k) {
      if (k >= K) continue;
#pragma unroll
      for (int j = 0; j < KN_DG_BSLOTS; ++j) {
        const double x = s == ss ? q[k][j] : 0.0;
        const double v = j == 3 ? kn_wave_max(x) : kn_wave_sum(x);
        if (lane == 0) sh[wave][(ss * K + k) * KN_DG_BSLOTS + j] = v;
      }
    }
  __syncthreads();
  const int ns = A.n_sub * K * KN_DG_BSLOTS;
  bool pub = false;
  if (wave == 0)
    for (int j = lane; j < ns; j += 64) {
      const bool is_max = (j & 3) == 3;
      double v = sh[0][j];
      for (int w = 1; w < BL_WAVES; ++w) v = is_max ? fmax(v, sh[w][j]) : v + sh[w][j];
      kn_part_store(&A.part[(size_t)blockIdx.x * ns + j], v);
      pub = true;
    }
  if (!kn_arrive_last(A.ctl, pub, &last)) return;
  const bool room = kn_claim_row(A.ctl, A.capacity, &row);
  double* o = A.rows + (size_t)row * A.n_cols;         // (written only with room)
  // every column over the workgroups, in an order that does not depend on which workgroup came last
  for (int j = wave; j < ns; j += BL_WAVES) {
    const bool is_max = (j & 3) == 3;
    double v = 0.0;
    for (int p = lane; p < A.n_blk; p += 64) {
      const double x = kn_part_load(&A.part[(size_t)p * ns + j]);
      v = is_max ? fmax(v, x) : v + x;
    }
    v = is_max ? kn_wave_max(v) : kn_wave_sum(v);
    if (lane == 0 && room) o[j] = v;
  }
  // the membrane launch's sums: per tag the K ions' j^e, j^i, then capacitive, channel, area
  const int per = 2 * K + 3;
  for (int j = tid; j < A.n_tag * per; j += BL_THREADS) {
    const int t = j / per, c = j - t * per;
    const int src = c < K ? c : c < 2 * K ? KN_MAXK + (c - K) : 2 * KN_MAXK + (c - 2 * K);
    if (room) o[ns + j] = A.tagtab[t * KN_DG_BTAG + src];
  }
  if (tid == 0) {
    kn_commit_row(A.ctl, row, room);
    kn_reset_ticket(A.ctl);
  }
}

BalArgs bl_args(const knpemi_dg* h, int splitting) {
  const KnDgBalance& B = h->balance;
  return {h->K, h->n_sub, B.n_tag, h->hex_box, splitting, B.want_cells, B.n_blk, B.ser.capacity, B.ser.n_cols,
          B.cells, B.part, B.mpart, B.tagtab, B.ser.ctl, B.mctl, B.ser.rows, B.facet_tag};
}

}  // namespace

int kn_dg_balance_blocks(int n_cell, int NV) {
  const int cpb = BL_THREADS / (NV == 8 ? 6 : NV);
  return (n_cell + cpb - 1) / cpb;
}

int kn_dg_launch_balance_membrane(knpemi_dg* h, int splitting) {
  const BalArgs a = bl_args(h, splitting);
  if (!kn_pick<3, 4, 8>(h->NV, [&](auto nv) {
        constexpr int V = decltype(nv)::value;
        hipLaunchKernelGGL(dg_balance_membrane_kernel<V>, dim3(a.n_blk), dim3(BL_THREADS), 0, h->stream, h->dev, h->d_consts, a);
      }))
    return kn_dg_not_built("dg_balance_membrane_kernel", h->NV, 0);
  return kn_launch_check("dg_balance_membrane_kernel");
}

int kn_dg_launch_balance_flux(knpemi_dg* h) {
  const BalArgs a = bl_args(h, 0);
  if (!kn_pick<3, 4, 8>(h->NV, [&](auto nv) {
        constexpr int V = decltype(nv)::value;
        hipLaunchKernelGGL(dg_balance_flux_kernel<V>, dim3(a.n_blk), dim3(BL_THREADS), 0, h->stream, h->dev, h->d_consts, a);
      }))
    return kn_dg_not_built("dg_balance_flux_kernel", h->NV, 0);
  return kn_launch_check("dg_balance_flux_kernel");
}
