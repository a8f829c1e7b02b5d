// Element rows of the Q1 quadrilateral (the 2-D cell of dolfinx.mesh.create_rectangle(..., CellType.quadrilateral)) for
// the row kernels emi_rows_quad_v2 / knp_rows_quad_v2 of kernels_assemble.hip.  Device only, anonymous namespace.
//
// Local vertex j sits at the reference point (j & 1, j >> 1).  Two forms of the same integrals (emiWeakForm.py:138-241,
// knpWeakForm.py:123-216; degree 3, i.e. the 2 x 2 Gauss rule, as the 2 x 2 x 2 rule on hexahedra):
//   quadq   general bilinear cells: the rule itself, the 2 x 2 Jacobian inverted at every point, all weights constants of
//           the instruction stream (four points, four vertices: everything is unrolled, no table is read)
//   quadcf  parallelograms: closed forms in the frame of the row vertex (see hexcf in kernels_assemble.hip); the rule is
//           exact for these integrands on a constant Jacobian, so both give the same numbers up to rounding
// Nothing here is shared with the hexahedral helpers: those stay instruction for instruction what they were.
#pragma once

#include "membrane_facet.h"   // kn_rcp

namespace {

// staged records of a quadrilateral row block (emi_rows.h: write_staged<KS, false, 2>)
struct RecQ4 { double x, y, k, s; };                       // EMI: x y | kappa sigma
__device__ __forceinline__ RecQ4 lds_recq4(const double* recs, int i) {
  const double2* p = reinterpret_cast<const double2*>(recs + (size_t)i * 4);
  const double2 u = p[0], v = p[1];
  return RecQ4{u.x, u.y, v.x, v.y};
}
template <int KS>
struct RecQK { double x, y, f[KS], c; };                   // KNP: x y | f_0 .. f_{KS-1} | phi
template <int KS>
__device__ __forceinline__ RecQK<KS> lds_recqk(const double* recs, int i) {
  RecQK<KS> r;
  const double* p = recs + (size_t)i * (3 + KS);
  r.x = p[0]; r.y = p[1];
#pragma unroll
  for (int k = 0; k < KS; ++k) r.f[k] = p[2 + k];
  r.c = p[2 + KS];
  return r;
}

namespace quadq {
constexpr double G0 = 0.5 - 0.28867513459481287, G1 = 0.5 + 0.28867513459481287;
// 1-D factor of N_v along axis ax at Gauss point q
__host__ __device__ constexpr double f(int q, int v, int ax) {
  const double x = ((q >> ax) & 1) ? G1 : G0;
  return ((v >> ax) & 1) ? x : 1.0 - x;
}
__host__ __device__ constexpr double N(int q, int v) { return f(q, v, 0) * f(q, v, 1); }
// dN_v / dxi_t at point q
__host__ __device__ constexpr double dN(int q, int v, int t) { return (((v >> t) & 1) ? 1.0 : -1.0) * f(q, v, 1 - t); }

struct Geo {      // geometry of the row vertex at one Gauss point
  double w[2];    // J^-1 J^-T dN_l
  double wd;      // weight * |det J|
  double Nl;      // N_l
};

// li, the row's local vertex, is a run-time value: its two bits select between constants
template <int Q, class R>
__device__ __forceinline__ Geo geo(const R (&r)[4], int l0, int l1) {
  constexpr double x0 = (Q & 1) ? G1 : G0, x1 = (Q & 2) ? G1 : G0;
  // J[a][t] = d x_a / d xi_t
  const double J00 = (1.0 - x1) * (r[1].x - r[0].x) + x1 * (r[3].x - r[2].x);
  const double J10 = (1.0 - x1) * (r[1].y - r[0].y) + x1 * (r[3].y - r[2].y);
  const double J01 = (1.0 - x0) * (r[2].x - r[0].x) + x0 * (r[3].x - r[1].x);
  const double J11 = (1.0 - x0) * (r[2].y - r[0].y) + x0 * (r[3].y - r[1].y);
  const double det = J00 * J11 - J01 * J10, inv = kn_rcp(det);
  const double i00 = J11 * inv, i01 = -J01 * inv, i10 = -J10 * inv, i11 = J00 * inv;   // J^-1[t][a]
  const double f0 = l0 ? x0 : 1.0 - x0, f1 = l1 ? x1 : 1.0 - x1;
  const double a = l0 ? f1 : -f1, b = l1 ? f0 : -f0;                                   // dN_l
  const double g0 = a * i00 + b * i10, g1 = a * i01 + b * i11;                         // J^-T dN_l
  Geo G;
  G.w[0] = i00 * g0 + i01 * g1;
  G.w[1] = i10 * g0 + i11 * g1;
  G.wd = 0.25 * fabs(det);
  G.Nl = f0 * f1;
  return G;
}

// Row li of the EMI element matrix: ra = kappa-stiffness (kappa interpolated at the points), bvol -= the volume
// right-hand side grad sigma . grad N_l
template <int Q>
__device__ __forceinline__ void emi_point(const RecQ4 (&r)[4], int l0, int l1, double (&ra)[4], double& bvol) {
  const Geo G = geo<Q>(r, l0, l1);
  double kq = 0.0, gs0 = 0.0, gs1 = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    kq += N(Q, j) * r[j].k;
    gs0 += dN(Q, j, 0) * r[j].s;
    gs1 += dN(Q, j, 1) * r[j].s;
  }
  bvol -= G.wd * (G.w[0] * gs0 + G.w[1] * gs1);
  const double wk = G.wd * kq, v0 = G.w[0] * wk, v1 = G.w[1] * wk;
#pragma unroll
  for (int j = 0; j < 4; ++j) ra[j] += dN(Q, j, 0) * v0 + dN(Q, j, 1) * v1;
}
__device__ __forceinline__ void emi_row(const RecQ4 (&r)[4], int li, double (&ra)[4], double& bvol) {
#pragma unroll
  for (int j = 0; j < 4; ++j) ra[j] = 0.0;
  const int l0 = li & 1, l1 = (li >> 1) & 1;
  emi_point<0>(r, l0, l1, ra, bvol);
  emi_point<1>(r, l0, l1, ra, bvol);
  emi_point<2>(r, l0, l1, ra, bvol);
  emi_point<3>(r, l0, l1, ra, bvol);
}

// Row li of the KNP element matrices: M = mass, S = stiffness, Cc = drift (grad phi . grad N_l) N_j
template <int Q, class R>
__device__ __forceinline__ void knp_point(const R (&r)[4], int l0, int l1, double (&M)[4], double (&S)[4], double (&Cc)[4]) {
  const Geo G = geo<Q>(r, l0, l1);
  double gp0 = 0.0, gp1 = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    gp0 += dN(Q, j, 0) * r[j].c;
    gp1 += dN(Q, j, 1) * r[j].c;
  }
  const double drift = G.w[0] * gp0 + G.w[1] * gp1;   // grad phi . grad N_l
  const double v0 = G.w[0] * G.wd, v1 = G.w[1] * G.wd, m = G.wd * G.Nl, c = G.wd * drift;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    S[j] += dN(Q, j, 0) * v0 + dN(Q, j, 1) * v1;
    M[j] += N(Q, j) * m;
    Cc[j] += N(Q, j) * c;
  }
}
template <class R>
__device__ __forceinline__ void knp_row(const R (&r)[4], int li, double (&M)[4], double (&S)[4], double (&Cc)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) { M[j] = 0.0; S[j] = 0.0; Cc[j] = 0.0; }
  const int l0 = li & 1, l1 = (li >> 1) & 1;
  knp_point<0>(r, l0, l1, M, S, Cc);
  knp_point<1>(r, l0, l1, M, S, Cc);
  knp_point<2>(r, l0, l1, M, S, Cc);
  knp_point<3>(r, l0, l1, M, S, Cc);
}
}  // namespace quadq

// ---------------------------------------------------------------------------------------------
// Parallelograms.  The row vertex l is moved to local vertex 0 by reflecting the reference square along the axes where l
// has a bit set: the caller loads the records in the order j' = j ^ l, the edge vectors taken from the permuted records
// carry the reflection, and every result of the frame belongs to the cell's local vertex j' ^ l -- no register array is
// indexed with a run-time value.  With N_j = p_{j0}(xi) p_{j1}(eta), p_0 = 1 - x, p_1 = x, the integrals over the unit
// square factor into
//   a(m, j) = int p_m p_j = 1/3 (m = j), 1/6;      b(m, 0, j) = int p_m p_0 p_j = 1/4 (m = j = 0), 1/12;      int p_m = 1/2
// and the metric g = |det J| J^-1 J^-T is a symmetric 2 x 2 matrix whose mixed entry vanishes on rectangles.
// ---------------------------------------------------------------------------------------------
namespace quadcf {
constexpr double T4 = 0.25, T12 = 1.0 / 12.0, A3 = 1.0 / 3.0, A6 = 1.0 / 6.0;
__host__ __device__ constexpr double a0(int j) { return j ? A6 : A3; }
__host__ __device__ constexpr double a(int m, int j) { return m == j ? A3 : A6; }

struct Geo { double g00, g11, g01, det; bool skew; };
template <class R>
__device__ __forceinline__ Geo geometry(const R (&r)[4]) {
  const double ax = r[1].x - r[0].x, ay = r[1].y - r[0].y;      // E_0
  const double bx = r[2].x - r[0].x, by = r[2].y - r[0].y;      // E_1
  const double det = ax * by - ay * bx;
  Geo G;
  G.det = fabs(det);
  const double inv = kn_rcp(G.det);
  G.g00 = (bx * bx + by * by) * inv;
  G.g11 = (ax * ax + ay * ay) * inv;
  G.g01 = -(ax * bx + ay * by) * inv;
  // wave-uniform: no lane of the wavefront that is at this pair has a mixed term (every cell of a rectangle mesh)
  G.skew = __any(G.g01 != 0.0);
  return G;
}

// Row of local vertex 0 (records in the reflected order): kappa-stiffness ra, volume right-hand side
__device__ __forceinline__ void emi_row0(const RecQ4 (&r)[4], double (&ra)[4], double& bvol) {
  const Geo G = geometry(r);
  // axis 0: -s(j0) g00 / 2 sum_m1 b(m1, 0, j1) (k[0, m1] + k[1, m1]); axis 1 alike
  const double k0a = r[0].k + r[1].k, k0b = r[2].k + r[3].k;      // summed along axis 0, by m1
  const double k1a = r[0].k + r[2].k, k1b = r[1].k + r[3].k;      // summed along axis 1, by m0
  const double P0[2] = {T4 * k0a + T12 * k0b, T12 * (k0a + k0b)};
  const double P1[2] = {T4 * k1a + T12 * k1b, T12 * (k1a + k1b)};
  const double c0 = 0.5 * G.g00, c1 = 0.5 * G.g11;
#pragma unroll
  for (int j = 0; j < 4; ++j) ra[j] = ((j & 1) ? -c0 : c0) * P0[j >> 1] + ((j & 2) ? -c1 : c1) * P1[j & 1];
  double bv = G.g00 * (A3 * (r[1].s - r[0].s) + A6 * (r[3].s - r[2].s)) + G.g11 * (A3 * (r[2].s - r[0].s) + A6 * (r[3].s - r[1].s));
  if (G.skew) {
    // g01 (d_0 N_0 d_1 N_j + d_1 N_0 d_0 N_j):  -s(j1) sum_m k_m a(m0, j0) a0(m1)  and  -s(j0) sum_m k_m a0(m0) a(m1, j1)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double q01 = 0.0, q10 = 0.0;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        q01 += (a(m & 1, j & 1) * a0(m >> 1)) * r[m].k;
        q10 += (a0(m & 1) * a(m >> 1, j >> 1)) * r[m].k;
      }
      ra[j] += G.g01 * (((j & 2) ? -q01 : q01) + ((j & 1) ? -q10 : q10));
    }
    bv += 0.25 * G.g01 * ((r[2].s - r[0].s) + (r[3].s - r[1].s) + (r[1].s - r[0].s) + (r[3].s - r[2].s));
  }
  bvol += bv;
}

// Row of local vertex 0 of the KNP element matrices (records in the reflected order): mass, stiffness, drift
template <class R>
__device__ __forceinline__ void knp_row0(const R (&r)[4], double (&M)[4], double (&S)[4], double (&Cc)[4]) {
  const Geo G = geometry(r);
  const double dp0[2] = {r[1].c - r[0].c, r[3].c - r[2].c};      // d phi along axis 0, by m1
  const double dp1[2] = {r[2].c - r[0].c, r[3].c - r[1].c};      // d phi along axis 1, by m0
  const double P0[2] = {T4 * dp0[0] + T12 * dp0[1], T12 * (dp0[0] + dp0[1])};
  const double P1[2] = {T4 * dp1[0] + T12 * dp1[1], T12 * (dp1[0] + dp1[1])};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    M[j] = G.det * (a0(j & 1) * a0(j >> 1));
    S[j] = ((j & 1) ? -G.g00 : G.g00) * a0(j >> 1) + ((j & 2) ? -G.g11 : G.g11) * a0(j & 1);
    Cc[j] = -0.5 * (G.g00 * P0[j >> 1] + G.g11 * P1[j & 1]);
  }
  if (G.skew) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      S[j] += G.g01 * (((j & 2) ? -0.25 : 0.25) + ((j & 1) ? -0.25 : 0.25));
      // d_0 N_0 d_1 phi N_j = -a0(j1) sum_m0 a(m0, j0) dp1[m0];   d_1 N_0 d_0 phi N_j = -a0(j0) sum_m1 a(m1, j1) dp0[m1]
      const double q01 = a0(j >> 1) * (a(0, j & 1) * dp1[0] + a(1, j & 1) * dp1[1]);
      const double q10 = a0(j & 1) * (a(0, j >> 1) * dp0[0] + a(1, j >> 1) * dp0[1]);
      Cc[j] -= G.g01 * (q01 + q10);
    }
  }
}
}  // namespace quadcf

}  // namespace
