// One side of a membrane facet and the fields of the KNP coupling integrand at a quadrature point of it
// (knpWeakForm.py:168-214), shared by the assembly kernels (kernels_assemble.hip: the membrane part of b_knp) and the
// membrane-exchange record (kernels_exchange.hip: the molar fluxes that part of b_knp integrates).  Device code only;
// every function is inlined into its caller, so the assembly kernels keep the arithmetic they had with this text in place.
#pragma once

#include "knpemi_internal.h"

namespace {

struct Rec {
  double x, y, z, c[KN_MAXK], phi;   // c[k]: ion k (record slot KN_CSLOT(k))
};

__device__ __forceinline__ Rec load_rec(const double* __restrict__ VR, int v) {
  const double4* p = reinterpret_cast<const double4*>(VR) + 2 * (size_t)v;
  const double4 a = p[0], b = p[1];
  Rec r;
  r.x = a.x; r.y = a.y; r.z = a.z; r.c[0] = b.x; r.c[1] = b.y; r.c[2] = b.z; r.c[3] = a.w; r.phi = b.w;
  return r;
}

// the record without its last component (phi is left unset)
__device__ __forceinline__ Rec load_rec_nophi(const double* __restrict__ VR, int v) {
  const double4* p = reinterpret_cast<const double4*>(VR) + 2 * (size_t)v;
  const double4 a = p[0];
  const double2 b = *reinterpret_cast<const double2*>(p + 1);
  Rec r;
  r.x = a.x; r.y = a.y; r.z = a.z; r.c[0] = b.x; r.c[1] = b.y; r.c[2] = VR[(size_t)v * KN_REC + 6]; r.c[3] = a.w;
  return r;
}

// measure of a simplex facet: the length of an interval, the area of a triangle
template <int NF>
__device__ __forceinline__ double facet_measure(const Rec (&p)[NF]) {
  if constexpr (NF == 2) {
    const double dx = p[1].x - p[0].x, dy = p[1].y - p[0].y;
    return sqrt(dx * dx + dy * dy);
  } else {
    const double ax = p[1].x - p[0].x, ay = p[1].y - p[0].y, az = p[1].z - p[0].z;
    const double bx = p[2].x - p[0].x, by = p[2].y - p[0].y, bz = p[2].z - p[0].z;
    const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    return 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
  }
}

// 1 / a from the hardware estimate and two Newton steps (relative error of a few 1e-16): five instructions instead of the
// eleven of the IEEE division sequence, once per (row, cell) pair and per quadrature point of the Q1 kernels.
__device__ __forceinline__ double kn_rcp(double a) {
  double r = __builtin_amdgcn_rcp(a);
  r = fma(fma(-a, r, 1.0), r, r);
  return fma(fma(-a, r, 1.0), r, r);
}

// KN_MEM_LQ adjacent lanes share one (facet, side): each takes every KN_MEM_LQ-th quadrature point and the partial
// integrals meet in a shuffle reduction.  The membrane is a 2-D set: with one thread per (facet, side) a config-2 launch
// has 46 workgroups whose threads walk 12 points of ~150 instructions one after the other; spreading the points
// turns that latency chain into four times as many, four times shorter waves.
#ifndef KN_MEM_LQ
#define KN_MEM_LQ 4
#endif

// everything one side of a membrane facet contributes to the integrand: loaded once per (facet, side)
template <int NF>
struct FacetData {
  Rec pe[NF], pi[NF];
  double pm[NF], Ik[NF][KN_MAXK], It[NF];
  double meas, sgn;
  const KnSubConst* so;    // own-side constants
  bool cell_side;
};

// The indices of a facet -- the vertices of its two sides and its Q dofs.  They depend on the facet alone, so a caller
// that knows its facet early (knp_membrane_block) fetches them beside its other first loads and the facet's data are one
// memory round trip behind them, not two.
template <int NF>
struct FacetIdx { int vi[NF], ve[NF], q[NF]; };

template <int NF>
__device__ __forceinline__ FacetIdx<NF> load_facet_idx(const KnDev& D, int fg) {
  FacetIdx<NF> ix;
#pragma unroll
  for (int bb = 0; bb < NF; ++bb) {
    ix.vi[bb] = D.fi[(size_t)fg * NF + bb];
    ix.ve[bb] = D.fe[(size_t)fg * NF + bb];
    ix.q[bb] = D.fq[(size_t)fg * NF + bb];
  }
  return ix;
}

// phi_x != NULL: the potential is taken from that vector (one value per vertex, e.g. the solver's solution before it is
// written into the records -- a constant shift of it cancels in the jump) instead of the records' component 7.
// ms: a model slot in range (a caller that loads for a facet without a model passes slot 0 and drops the result).
template <int NF>
__device__ __forceinline__ void load_facet(const KnDev& D, const KnConsts& C, const FacetIdx<NF>& ix, bool cell_side, int ms,
                                           FacetData<NF>& f, const double* __restrict__ phi_x = nullptr) {
  const int K = C.K;
#pragma unroll
  for (int bb = 0; bb < NF; ++bb) {
    const int vi = ix.vi[bb], ve = ix.ve[bb];
    // the potential through a chosen address, not loaded with the record and overwritten: the dead half of that 16-byte
    // load would be a register the compiler reuses at once, and waits for the load to do so
    f.pe[bb] = load_rec_nophi(D.VR, ve);
    f.pi[bb] = load_rec_nophi(D.VR, vi);
    f.pe[bb].phi = *(phi_x ? phi_x + ve : D.VR + (size_t)ve * KN_REC + 7);
    f.pi[bb].phi = *(phi_x ? phi_x + vi : D.VR + (size_t)vi * KN_REC + 7);
    const int q = ix.q[bb];
    f.pm[bb] = D.phiM[q];
    const double* ich = D.Ich + (size_t)ms * KN_MAXK * D.NQtot + q;
    double it = 0.0;
#pragma unroll
    for (int k = 0; k < KN_MAXK; ++k) {
      f.Ik[bb][k] = k < K ? ich[(size_t)k * D.NQtot] : 0.0;
      it += f.Ik[bb][k];
    }
    f.It[bb] = it;
  }
  int si = 0;  // sub-domain of the cell side of this facet
  for (int tt = 1; tt < C.n_sub; ++tt) si += ix.vi[0] >= C.voff[tt];
  f.so = &C.sc[cell_side ? si : 0];
  f.meas = 0.0;
  if constexpr (NF != 4) f.meas = facet_measure<NF>(f.pe);
  f.sgn = cell_side ? 1.0 : -1.0;
  f.cell_side = cell_side;
}

// the same by the facet's number, for the callers that learn it late: indices, then data
template <int NF>
__device__ __forceinline__ void load_facet(const KnDev& D, const KnConsts& C, int fg, bool cell_side, int ms,
                                           FacetData<NF>& f, const double* __restrict__ phi_x = nullptr) {
  load_facet<NF>(D, C, load_facet_idx<NF>(D, fg), cell_side, ms, f, phi_x);
}

// The fields of the integrand at quadrature point q of one (facet, side): the own side's concentrations cq, the channel
// currents iq per ion and their sum it, the potential on both sides, phi_M of the previous step, the quadrature weight
// times the surface Jacobian wq, and asum = sum_j D_j z_j^2 c_j over ALL K ions (knpWeakForm.py:97; az2D = 0 beyond K).
struct FacetPoint {
  double cq[KN_MAXK], iq[KN_MAXK], ph_e, ph_i, pmq, it, wq, asum;
};

template <int NF>
__device__ __forceinline__ void facet_point_fields(const FacetData<NF>& f, int q, const double* qw, const double* qN,
                                                   const double* qdN, FacetPoint& P) {
  double cq[KN_MAXK], iq[KN_MAXK], ph_e = 0, ph_i = 0, pmq = 0, it = 0;
#pragma unroll
  for (int k = 0; k < KN_MAXK; ++k) { cq[k] = 0.0; iq[k] = 0.0; }
#pragma unroll
  for (int bb = 0; bb < NF; ++bb) {
    const double N = qN[q * NF + bb];
    const Rec& o = f.cell_side ? f.pi[bb] : f.pe[bb];
#pragma unroll
    for (int k = 0; k < KN_MAXK; ++k) { cq[k] += N * o.c[k]; iq[k] += N * f.Ik[bb][k]; }
    ph_e += N * f.pe[bb].phi; ph_i += N * f.pi[bb].phi;
    pmq += N * f.pm[bb]; it += N * f.It[bb];
  }
  double wq;
  if constexpr (NF == 4) {
    // surface Jacobian of the bilinear facet at this point
    double ux = 0, uy = 0, uz = 0, vx = 0, vy = 0, vz = 0;
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) {
      const double da = qdN[(q * 4 + bb) * 2], db = qdN[(q * 4 + bb) * 2 + 1];
      ux += da * f.pe[bb].x; uy += da * f.pe[bb].y; uz += da * f.pe[bb].z;
      vx += db * f.pe[bb].x; vy += db * f.pe[bb].y; vz += db * f.pe[bb].z;
    }
    const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    wq = qw[q] * sqrt(nx * nx + ny * ny + nz * nz);
  } else {
    wq = qw[q] * f.meas * (NF == 2 ? 1.0 : 2.0);  // reference measure 1 (interval), 1/2 (triangle)
  }
  double asum = 0.0;      // sum over ALL K ions (knpWeakForm.py:97); az2D = 0 beyond K
#pragma unroll
  for (int k = 0; k < KN_MAXK; ++k) asum += f.so->az2D[k] * cq[k];
#pragma unroll
  for (int k = 0; k < KN_MAXK; ++k) { P.cq[k] = cq[k]; P.iq[k] = iq[k]; }
  P.ph_e = ph_e; P.ph_i = ph_i; P.pmq = pmq; P.it = it; P.wq = wq; P.asum = asum;
}

}  // namespace
