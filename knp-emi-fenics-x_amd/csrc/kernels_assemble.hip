// gfx950 assembly kernels of the knpemi hot path.
//
// Design: "owner-computes rows".  A block of 256 / LPR consecutive matrix rows
// (= sub-mesh vertices) owns a contiguous CSR range.  It stages the 48-byte records of the distinct
// vertices its rows touch in LDS once, then LPR lanes per row walk the cells incident to the row's
// vertex (sliced-ELL list, coalesced index reads), recompute the closed-form P1 element row (or the
// Gauss-quadrature Q1 row) and accumulate into the block's slice of the CSR value array held in LDS.
// The final write to HBM is a plain coalesced stream: no global atomics, bit-reproducible results,
// and the matrix, the preconditioner and the RHS come out of one pass over the mesh.
//
// Forms restated (paths relative to the reference repository):
//   EMI  a, p, L : src/knpemi/emiWeakForm.py:138-241
//   KNP  a, L    : src/knpemi/knpWeakForm.py:123-216
//   update       : src/knpemi/utils.py:238-295
#include "knpemi_internal.h"
#include "kn_pick.h"
#include "membrane_facet.h"
// what the simplex EMI row block is made of (logical_block, the membrane part of an EMI row, the block descriptors and the
// staging of the records, which the other row kernels here use too) and the block itself: shared with the fused launch
#include "emi_rows.h"
// element rows of the Q1 quadrilateral
#include "quad_rows.h"

namespace {

// surface Jacobian of a bilinear quadrilateral facet (lexicographic vertices) at (xi, eta)
__device__ __forceinline__ double quad_jac(const Rec (&p)[4], double xi, double eta) {
  const double ux = (1 - eta) * (p[1].x - p[0].x) + eta * (p[3].x - p[2].x);
  const double uy = (1 - eta) * (p[1].y - p[0].y) + eta * (p[3].y - p[2].y);
  const double uz = (1 - eta) * (p[1].z - p[0].z) + eta * (p[3].z - p[2].z);
  const double vx = (1 - xi) * (p[2].x - p[0].x) + xi * (p[3].x - p[1].x);
  const double vy = (1 - xi) * (p[2].y - p[0].y) + xi * (p[3].y - p[1].y);
  const double vz = (1 - xi) * (p[2].z - p[0].z) + xi * (p[3].z - p[1].z);
  const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  return sqrt(nx * nx + ny * ny + nz * nz);
}

// Facet mass matrix row M[a][b], b = 0..NF-1 (degree-2 integrand: closed form on simplices,
// 2x2 Gauss on quadrilaterals as FFCx would choose).
template <int NF>
__device__ __forceinline__ void facet_mass_row(const Rec (&p)[NF], int a, double (&M)[NF]) {
  if constexpr (NF == 4) {
    const double g0 = 0.5 - 0.28867513459481287, g1 = 0.5 + 0.28867513459481287;
#pragma unroll
    for (int b = 0; b < 4; ++b) M[b] = 0.0;
#pragma unroll
    for (int qj = 0; qj < 2; ++qj)
#pragma unroll
      for (int qi = 0; qi < 2; ++qi) {
        const double xi = qi ? g1 : g0, eta = qj ? g1 : g0;
        const double N[4] = {(1 - xi) * (1 - eta), xi * (1 - eta), (1 - xi) * eta, xi * eta};
        const double Na = a == 0 ? N[0] : (a == 1 ? N[1] : (a == 2 ? N[2] : N[3]));
        const double w = 0.25 * quad_jac(p, xi, eta) * Na;
#pragma unroll
        for (int b = 0; b < 4; ++b) M[b] += w * N[b];
      }
  } else {
    const double m = facet_measure<NF>(p) * (1.0 / (NF * (NF + 1)));
#pragma unroll
    for (int b = 0; b < NF; ++b) M[b] = (b == a) ? 2.0 * m : m;
  }
}

// one-time fill of the facet-mass rows of the membrane entries (set-up; geometry is static)
template <int NF>
__global__ void membrane_mass_kernel(KnDev D, int n_entries, int v_cells, const int* __restrict__ entry_row,
                                     double* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_entries) return;
  const int ent = D.mentry[e];
  const int fg = ent >> 3, a = ent & 7;
  const int* fown = entry_row[e] >= v_cells ? D.fi : D.fe;
  Rec p[NF];
#pragma unroll
  for (int bb = 0; bb < NF; ++bb) p[bb] = load_rec(D.VR, fown[(size_t)fg * NF + bb]);
  double Mr[NF];
  facet_mass_row<NF>(p, a, Mr);
#pragma unroll
  for (int bb = 0; bb < NF; ++bb) out[(size_t)e * NF + bb] = Mr[bb];
}

// =============================================================================================
// Simplex row kernels, version 2: neighbour records staged in LDS.
//
// The Laplacian row of vertex g lists exactly the vertices of its incident cells, so a (row, cell)
// pair needs nothing but NV row-relative slot bytes.  Phase A gathers, once per row block, the 48-byte
// record of every entry of the block's Laplacian segment into LDS (~15 gathers per row instead of
// 3 per incident cell, i.e. 72 for a Kuhn tetrahedral mesh) and zeroes the accumulators; phase B
// walks the pairs (4 bytes each, coalesced), reads the NV records from LDS and accumulates with
// LDS fp64 adds (ds_add_f64).  All lanes that add into a given row belong to one wavefront, so the
// order of the adds is fixed by program order and lane order: results are bit-reproducible.
// =============================================================================================
// (defined with the membrane-facet code further down)
template <int NF, int KS>
__device__ __forceinline__ void membrane_entries_to_lds(const KnDev& D, const KnConsts& C, int e0, int ne, bool cell_side,
                                                        int splitting, int tid, double* gam);

// Early membrane integrals (knp_membrane_pre_kernel): b_knp contribution of membrane entry e from the potential that
// now sits in the vertex records.
template <int NF, int KS>
__device__ __forceinline__ void membrane_entry_early(const KnDev& D, int e, double (&bk)[KS]) {
  constexpr int GS = (1 + NF) * KS;
  const double* g = D.gpre + (size_t)GS * e;
  const int fg = D.mentry[e] >> 3;
  double jump[NF];
#pragma unroll
  for (int b = 0; b < NF; ++b)
    jump[b] = D.VR[(size_t)D.fi[(size_t)fg * NF + b] * KN_REC + 7] - D.VR[(size_t)D.fe[(size_t)fg * NF + b] * KN_REC + 7];
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    double v = g[k];
#pragma unroll
    for (int b = 0; b < NF; ++b) v -= g[(1 + b) * KS + k] * jump[b];
    bk[k] += v;
  }
}

// staged record of a KNP row block: coordinates, f_k = c_prev_k / dt (+ f_source_k) of the KS solved ions, phi
template <int KS>
struct RecK {
  double x, y, z, f[KS], c;   // c = phi
};

template <int KS>
__device__ __forceinline__ RecK<KS> lds_rec(const double* recs, int i) {
  RecK<KS> r;
  if constexpr (KS == 2) {   // 48-byte records: three 16-byte LDS reads
    const double2* p = reinterpret_cast<const double2*>(recs + (size_t)i * 6);
    const double2 u = p[0], v = p[1], w = p[2];
    r.x = u.x; r.y = u.y; r.z = v.x; r.f[0] = v.y; r.f[1] = w.x; r.c = w.y;
  } else {
    const double* p = recs + (size_t)i * (4 + KS);
    r.x = p[0]; r.y = p[1]; r.z = p[2];
#pragma unroll
    for (int k = 0; k < KS; ++k) r.f[k] = p[3 + k];
    r.c = p[3 + KS];
  }
  return r;
}

// Staged records of a UNIFORM hexahedral mesh (every cell the same parallelepiped: the geometry is a constant of the
// mesh, knpemi_handle::hex_geo, and no coordinates are staged): EMI 16 bytes (kappa, sigma), KNP 8 (KS + 1) bytes
// (f_0 .. f_{KS-1}, phi) -- 40 % / 50 % of the 40- / 48-byte records, in LDS bytes staged, LDS bytes read per (row, cell)
// pair and registers held per pair (8 records at once).
template <int KS>
struct RecU { double f[KS], c; };   // c = phi
template <int KS>
__device__ __forceinline__ RecU<KS> lds_recu(const double* recs, int i) {
  RecU<KS> r;
  const double* p = recs + (size_t)i * (KS + 1);
#pragma unroll
  for (int k = 0; k < KS; ++k) r.f[k] = p[k];
  r.c = p[KS];
  return r;
}

// ---- which row kernels are built ----------------------------------------------------------------------------------------
// The launchers (kn_launch_emi_rows, kn_launch_knp_rows) instantiate exactly what these predicates admit and refuse the
// rest by name.  L: lanes per row -- 2 (triangles) or 4 by default, KNPEMI_LPR for experiments; KS = K - 1 = 1..3 solved
// ions; MEM: the membrane path of knp_rows (below).  A new value of an axis: list it in the launcher's kn_pick and admit it here.
constexpr bool emi_rows_built(int L) { return L == 1 || L == 2 || L == 4 || L == 8; }
// simplices, geometry variant `geo` of KnRowShape: general everywhere, the lattice form for tetrahedra
constexpr bool simplex_geo_built(int gdim, int geo) { return geo == 0 || (geo == 2 && gdim == 3); }
// every ion count and membrane path for the default lanes per row only; the others with two solved ions, default path
constexpr bool knp_rows_built(int L, int KS, int MEM) {
  return (L == 2 || L == 4) ? KS >= 1 && KS <= 3 && MEM >= 0 && MEM <= 2 : (L == 1 || L == 8) && KS == 2 && MEM == 0;
}
constexpr bool knp_rows_hex_built(int L, int KS, int MEM) {
  return L == 4 ? KS >= 1 && KS <= 3 && MEM >= 0 && MEM <= 2 : (L == 1 || L == 2 || L == 8) && KS == 2 && MEM == 0;
}
// quadrilaterals: 2 lanes per row (the default) and 4, every ion count and membrane path with both; general cells and
// parallelograms, no uniform-cell variant.  KS = 0: the EMI kernel
constexpr bool rows_quad_built(int L, int KS, int MEM, int GEO) {
  return (L == 2 || L == 4) && KS >= 0 && KS <= 3 && MEM >= 0 && MEM <= 2 && (GEO == 0 || GEO == 1);
}
// vertices per cell of a cell kind, and the kinds by their row kernels
constexpr int kind_nv(int kind) { return kind == KNPEMI_TRIANGLE ? 3 : (kind == KNPEMI_HEXAHEDRON ? 8 : 4); }
constexpr bool kind_simplex(int kind) { return kind == KNPEMI_TRIANGLE || kind == KNPEMI_TETRAHEDRON; }

// one simplex EMI row block per workgroup (emi_rows.h).  UT: lattice tetrahedra of a uniform grid
template <int GDIM, int LPR, bool UT = false>
__global__ __launch_bounds__(KN_BLOCK) void emi_rows_v2(KnDev D, const KnConsts* __restrict__ Cp, int acc_n,
                                                        int rec_n, int want_p, int splitting) {
  emi_rows_block<GDIM, LPR, UT>(D, *Cp, acc_n, rec_n, want_p, splitting, blockIdx.x);
}

// MEM: where the membrane integrals of b_knp come from -- 0: the partial integrals knp_membrane_kernel left in gam_e
// (default), 1: evaluated here into LDS (KNPEMI_OPT_FUSE_MEMBRANE), 2: the early form (KNPEMI_MEMBRANE_EARLY).  A
// template parameter, not a run-time switch: the two optional paths cost the default one 46 registers per lane
// (140 instead of 94: three instead of five waves per SIMD).
template <int GDIM, int LPR, int KS, int MEM, bool UT = false>
__global__ __launch_bounds__(KN_BLOCK) void knp_rows_v2(KnDev D, const KnConsts* __restrict__ Cp, int acc_n, int rec_n,
                                                        int gam_n, int splitting) {
  constexpr int NV = GDIM + 1;
  const KnConsts& C = *Cp;
  extern __shared__ __align__(16) double lds[];
  constexpr int RD = UT ? KS + 1 : 4 + KS;             // doubles per staged record
  constexpr int SM = UT ? 31 : 255;                    // slot mask of a pair-entry byte (= the "no slot" value)
  using RecT = std::conditional_t<UT, RecU<KS>, RecK<KS>>;
  double* acc = lds;                                   // KS accumulator arrays of acc_n doubles, one per solved ion
  double* tab = lds + (size_t)KS * acc_n;              // UT: the shape table of the lattice tetrahedra
  double* recs = tab + (UT ? KN_TET_TAB : 0);
  double* gam = recs + (size_t)RD * rec_n + ((RD * rec_n) & 1);   // gam_n > 0: fused membrane integrals
  uint16_t* eloc = reinterpret_cast<uint16_t*>(gam + (size_t)KS * gam_n);
  const int tid = threadIdx.x;
  const int b = logical_block(blockIdx.x, D.nblocks);
  const BlkInfo B = load_blk(D, b, tid >> 6);
  const int s = B.sub, nnzLb = B.nnzLb;
  const int v0 = C.voff[s], nvs = C.voff[s + 1] - v0;
  const double* fs0 = (D.fsrc && s == 0) ? D.fsrc : nullptr;
  const int rloc = tid / LPR, sub = tid % LPR;
  const BlkRows<LPR, KN_CHUNK_SIMPLEX> rows(D, b);
  bool valid;
  const int g = rows.row(rloc, valid);
  const int64_t base = (int64_t)B.slbase * KN_SLICE + (tid & 63);
  const int np = B.np;
  uint32_t slr[KN_PREFETCH];
#pragma unroll
  for (int p = 0; p < KN_PREFETCH; ++p)
    slr[p] = (valid && p < np) ? D.pair_sl[base + (int64_t)p * KN_SLICE] : 0xFFFFFFFFu;
  const int4 ri = D.row_info[g];
  for (int i = tid; i < nnzLb; i += KN_BLOCK) {
#pragma unroll
    for (int k = 0; k < KS; ++k) acc[(size_t)k * acc_n + i] = 0.0;
  }
  if constexpr (UT) { if (tid < KN_TET_TAB) tab[tid] = D.tet_tab[tid]; }
  stage_records<KS, UT>(D, B, recs, eloc, tid, C.inv_dt, fs0, nvs);
  if constexpr (MEM == 1) membrane_entries_to_lds<GDIM, KS>(D, C, B.me0, B.mne, s > 0, splitting, tid, gam);
  __syncthreads();

  const KnSubConst& sc = C.sc[s];
  double bk[KS];
#pragma unroll
  for (int k = 0; k < KS; ++k) bk[k] = 0.0;
  if (valid) {
    const int rL = ri.z;
    int diag = -1;
    double dk[KS];   // diagonal entries of the ion blocks, added once after the loop
#pragma unroll
    for (int k = 0; k < KS; ++k) dk[k] = 0.0;
    RecT r[NV];
    auto rec = [&](int i) { if constexpr (UT) return lds_recu<KS>(recs, i); else return lds_rec<KS>(recs, i); };
    // The host orders a lane's pairs in strips: consecutive cells share all but one vertex, at the same byte positions
    // of the pair entry.  The records of the shared vertices stay in registers; only a slot that changed is read from
    // LDS again (one 48-byte record per pair instead of three: knp_rows 53.6 -> 46.9 us at 995 k tets, with four
    // instead of five blocks per CU -- 112 registers; capping them at 96 spills and gives the gain back).
    uint32_t have = 0xFFFFFFFFu;     // slots of the records r[1..] (and of the pending sums) currently held; 255: none
    double pend[NV][KS];
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int k = 0; k < KS; ++k) pend[j][k] = 0.0;
    auto do_pair = [&](uint32_t sl) {
      int slot[NV];
#pragma unroll
      for (int j = 0; j < NV; ++j) slot[j] = (sl >> (8 * j)) & SM;
      if (diag < 0) { diag = slot[0]; r[0] = rec(eloc[rL + diag]); }
#pragma unroll
      for (int j = 1; j < NV; ++j)
        if (slot[j] != (int)((have >> (8 * j)) & SM)) r[j] = rec(eloc[rL + slot[j]]);
      double d[NV];
      double vol;
      if constexpr (UT) vol = tet_table_row0<NV>(tab, sl, d);
      else vol = simplex_row0<GDIM>(r, d);
      double gp = 0;
#pragma unroll
      for (int j = 0; j < NV; ++j) gp += r[j].c * d[j];
      const double m = vol * (1.0 / ((GDIM + 1) * (GDIM + 2)));
      const double drift = gp * vol * (1.0 / (GDIM + 1));
#pragma unroll
      for (int k = 0; k < KS; ++k) {
        dk[k] += 2.0 * m * C.inv_dt + sc.D[k] * vol * d[0] + sc.zpsiD[k] * drift;
        bk[k] += 2.0 * m * r[0].f[k];
      }
      // off-diagonal entries: summed in registers while a vertex keeps its position, to LDS when it leaves (emi_rows_v2)
#pragma unroll
      for (int j = 1; j < NV; ++j) {
        const int hs = (int)((have >> (8 * j)) & SM);
        const bool moved = slot[j] != hs;
#pragma unroll
        for (int k = 0; k < KS; ++k) {
          if (moved) {
            if (hs != SM) unsafeAtomicAdd(&acc[(size_t)k * acc_n + rL + hs], pend[j][k]);
            pend[j][k] = 0.0;
          }
          pend[j][k] += m * C.inv_dt + sc.D[k] * vol * d[j] + sc.zpsiD[k] * drift;
          bk[k] += m * r[j].f[k];
        }
      }
      have = sl;
    };
#pragma unroll
    for (int p = 0; p < KN_PREFETCH; ++p)
      if (slr[p] != 0xFFFFFFFFu) do_pair(slr[p]);
    for (int p = KN_PREFETCH; p < np; ++p) {
      const uint32_t sl = D.pair_sl[base + (int64_t)p * KN_SLICE];
      if (sl != 0xFFFFFFFFu) do_pair(sl);
    }
#pragma unroll
    for (int j = 1; j < NV; ++j) {
      const int hs = (int)((have >> (8 * j)) & SM);
#pragma unroll
      for (int k = 0; k < KS; ++k)
        if (hs != SM) unsafeAtomicAdd(&acc[(size_t)k * acc_n + rL + hs], pend[j][k]);
    }
    if (diag >= 0) {
#pragma unroll
      for (int k = 0; k < KS; ++k) unsafeAtomicAdd(&acc[(size_t)k * acc_n + rL + diag], dk[k]);
    }
    // membrane Robin/coupling contributions, written per (row, facet) entry by knp_membrane_kernel
    {   // the row's LPR lanes share its membrane entries (the sums meet in the reduction below)
      const int ne = (unsigned)ri.y >> 16;
      for (int e = ri.w + sub; e < ri.w + ne; e += LPR) {
        if constexpr (MEM == 2) membrane_entry_early<GDIM, KS>(D, e, bk);
        else {
#pragma unroll
          for (int k = 0; k < KS; ++k) bk[k] += MEM == 1 ? gam[(size_t)(e - B.me0) * KS + k] : D.gam_e[(size_t)KS * e + k];
        }
      }
    }
  }
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) {
#pragma unroll
    for (int k = 0; k < KS; ++k) bk[k] += __shfl_xor(bk[k], m);
  }
  if (valid && sub == 0) {
    const size_t bb = (size_t)KS * v0 + (size_t)(g - v0);
#pragma unroll
    for (int k = 0; k < KS; ++k) D.b_knp[bb + (size_t)k * nvs] = bk[k];
  }
  __syncthreads();
  const int64_t subnnz0 = D.rowptrL[v0], subnnz = D.rowptrL[v0 + nvs] - subnnz0;
  double* out0 = D.A_knp + (size_t)KS * subnnz0 - subnnz0;
  rows.for_each_entry(tid, 1, [&](int i, int64_t gp) {
#pragma unroll
    for (int k = 0; k < KS; ++k) KN_ROW_STORE(acc[(size_t)k * acc_n + i], &out0[(size_t)k * subnnz + gp]);
  });
}

// =============================================================================================
// Q1 hexahedra, version 2: the same row-block scheme as the simplex kernels (distinct vertex records
// staged in LDS, LDS fp64 adds, one launch descriptor per block) with the 2x2x2 Gauss tables folded
// into the instruction stream: every loop over quadrature points and vertices is unrolled with constexpr
// weights, so no table is read at run time.  Per quadrature point the row of vertex l needs
//   d_j = grad N_l . grad N_j = dN_j . w,   w = J^-1 (J^-T dN_l)
// i.e. the Jacobian (from the 12 edge vectors), its inverse and one 3-vector; the physical gradients
// of the other seven basis functions are never formed.  Nodal fields enter through their reference
// gradients (edge differences), the mass row M_j = sum_q w_q N_l N_j is shared by the time-derivative,
// drift and right-hand-side terms.
// =============================================================================================
namespace hexq {
constexpr double G0 = 0.5 - 0.28867513459481287, G1 = 0.5 + 0.28867513459481287;
__host__ __device__ constexpr double f(int q, int v, int ax) {
  const double x = ((q >> ax) & 1) ? G1 : G0;
  return ((v >> ax) & 1) ? x : 1.0 - x;
}
__host__ __device__ constexpr double N(int q, int v) { return f(q, v, 0) * f(q, v, 1) * f(q, v, 2); }
// |dN_v/dxi_t| at point q (independent of bit t of v); the sign is + when bit t of v is set
__host__ __device__ constexpr double E(int q, int v, int t) { return f(q, v, (t + 1) % 3) * f(q, v, (t + 2) % 3); }
// k-th vertex (k = 0..3) whose bit t is clear, and the inverse map
__host__ __device__ constexpr int lo(int t, int k) { return ((k >> t) << (t + 1)) | (k & ((1 << t) - 1)); }
__host__ __device__ constexpr int kof(int t, int v) { return ((v >> (t + 1)) << t) | (v & ((1 << t) - 1)); }
struct Point { double E[3][4]; double N[8]; double x[3]; };   // weights of one Gauss point
struct Table { Point p[8]; };
constexpr Table make_table() {
  Table T{};
  for (int q = 0; q < 8; ++q) {
    for (int t = 0; t < 3; ++t) {
      for (int k = 0; k < 4; ++k) T.p[q].E[t][k] = E(q, lo(t, k), t);
      T.p[q].x[t] = ((q >> t) & 1) ? G1 : G0;
    }
    for (int v = 0; v < 8; ++v) T.p[q].N[v] = N(q, v);
  }
  return T;
}
}  // namespace hexq

// read with a wave-uniform index: the weights arrive in scalar registers
__constant__ hexq::Table c_hex = hexq::make_table();

struct HexGeo {   // geometry of the row vertex l at one Gauss point
  double w[3];    // J^-1 J^-T dN_l
  double wd;      // weight * |det J|
  double Nl;      // N_l
};

// edge vectors of the cell: e[t][k] = x[v | 1 << t] - x[v], v = lo(t, k)
struct HexEdges { double x[3][4], y[3][4], z[3][4]; };

template <class R>
__device__ __forceinline__ HexEdges hex_edges(const R (&r)[8]) {
  HexEdges e;
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = hexq::lo(t, k), u = v | (1 << t);
      e.x[t][k] = r[u].x - r[v].x; e.y[t][k] = r[u].y - r[v].y; e.z[t][k] = r[u].z - r[v].z;
    }
  return e;
}

struct HexInv { double i[3][3]; double wd; };   // J^-1[t][g] and weight * |det J|

// Jacobian (from the edge vectors) and its inverse at the Gauss point with weights P
__device__ __forceinline__ HexInv hex_inverse(const HexEdges& e, const hexq::Point& P) {
  double J[3][3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    double jx = 0, jy = 0, jz = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { jx += P.E[t][k] * e.x[t][k]; jy += P.E[t][k] * e.y[t][k]; jz += P.E[t][k] * e.z[t][k]; }
    J[0][t] = jx; J[1][t] = jy; J[2][t] = jz;
  }
  const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
  const double c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
  const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
  const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02, inv = kn_rcp(det);
  HexInv I;
  I.i[0][0] = c00 * inv; I.i[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * inv;
  I.i[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * inv;
  I.i[1][0] = c01 * inv; I.i[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * inv;
  I.i[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * inv;
  I.i[2][0] = c02 * inv; I.i[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * inv;
  I.i[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * inv;
  I.wd = 0.125 * fabs(det);
  return I;
}

// Parallelepipeds (every box mesh of the reference, make_mesh_3D.py:101) have a constant Jacobian: the four
// edge vectors of each axis coincide.  The row kernels then invert it once per cell instead of per point.
__device__ __forceinline__ bool hex_is_affine(const HexEdges& e) {
  double dev = 0.0, len = 0.0;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    len += fabs(e.x[t][0]) + fabs(e.y[t][0]) + fabs(e.z[t][0]);
#pragma unroll
    for (int k = 1; k < 4; ++k)
      dev += fabs(e.x[t][k] - e.x[t][0]) + fabs(e.y[t][k] - e.y[t][0]) + fabs(e.z[t][k] - e.z[t][0]);
  }
  return dev <= 1e-13 * len;
}

__device__ __forceinline__ HexGeo hex_geo(const HexInv& I, const hexq::Point& P, int l0, int l1, int l2) {
  const double f0 = l0 ? P.x[0] : 1.0 - P.x[0], f1 = l1 ? P.x[1] : 1.0 - P.x[1], f2 = l2 ? P.x[2] : 1.0 - P.x[2];
  const double a = (l0 ? f1 : -f1) * f2, b = (l1 ? f0 : -f0) * f2, c = (l2 ? f0 : -f0) * f1;   // dN_l
  const double g0 = a * I.i[0][0] + b * I.i[1][0] + c * I.i[2][0];
  const double g1 = a * I.i[0][1] + b * I.i[1][1] + c * I.i[2][1];
  const double g2 = a * I.i[0][2] + b * I.i[1][2] + c * I.i[2][2];
  HexGeo G;
  G.w[0] = I.i[0][0] * g0 + I.i[0][1] * g1 + I.i[0][2] * g2;
  G.w[1] = I.i[1][0] * g0 + I.i[1][1] * g1 + I.i[1][2] * g2;
  G.w[2] = I.i[2][0] * g0 + I.i[2][1] * g1 + I.i[2][2] * g2;
  G.wd = I.wd;
  G.Nl = f0 * f1 * f2;
  return G;
}

// reference gradient of a nodal field given by its edge differences d[t][k]
__device__ __forceinline__ void hex_ref_grad(const hexq::Point& P, const double (&d)[3][4], double (&g)[3]) {
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    double s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += P.E[t][k] * d[t][k];
    g[t] = s;
  }
}

__device__ __forceinline__ void hex_edge_diffs(const double (&u)[8], double (&d)[3][4]) {
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int k = 0; k < 4; ++k) d[t][k] = u[hexq::lo(t, k) | (1 << t)] - u[hexq::lo(t, k)];
}

// acc[j] += dN_j . v   (dN_j[t] = +-E[t][k(j)], the sign is that of bit t of j)
__device__ __forceinline__ void hex_add_grad_dot(const hexq::Point& P, double (&acc)[8], const double (&v)[3]) {
  double pv[3][4];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int k = 0; k < 4; ++k) pv[t][k] = P.E[t][k] * v[t];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const double a0 = pv[0][hexq::kof(0, j)], a1 = pv[1][hexq::kof(1, j)], a2 = pv[2][hexq::kof(2, j)];
    acc[j] += ((j & 1) ? a0 : -a0) + ((j & 2) ? a1 : -a1) + ((j & 4) ? a2 : -a2);
  }
}

__device__ __forceinline__ void hex_add_shape(const hexq::Point& P, double (&acc)[8], double a) {
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] += P.N[j] * a;
}

__device__ __forceinline__ double hex_interp(const hexq::Point& P, const double (&u)[8]) {
  double s = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += P.N[j] * u[j];
  return s;
}

// Row l of the EMI element matrix of one hexahedron: ra = kappa-stiffness, and the volume right-hand side
// (emiWeakForm.py:138-241).  The ICS mass of P_emi is static and added at write-out (D.P_mass).
template <bool AFFINE>
__device__ __forceinline__ void hex_emi_row(const Rec5 (&r)[8], int li, double (&ra)[8], double& bvol) {
  double kv[8], sv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { kv[j] = r[j].k; sv[j] = r[j].s; ra[j] = 0.0; }
  double ds[3][4];
  hex_edge_diffs(sv, ds);
  const HexEdges e = hex_edges(r);
  const bool aff = AFFINE || hex_is_affine(e);
  HexInv I = hex_inverse(e, c_hex.p[0]);
  const int l0 = li & 1, l1 = (li >> 1) & 1, l2 = (li >> 2) & 1;
#pragma unroll 1
  for (int q = 0; q < 8; ++q) {
    const hexq::Point& P = c_hex.p[q];
    if (!AFFINE && !aff && q > 0) I = hex_inverse(e, P);
    const HexGeo G = hex_geo(I, P, l0, l1, l2);
    const double kq = hex_interp(P, kv);
    double gs[3];
    hex_ref_grad(P, ds, gs);
    bvol -= G.wd * (G.w[0] * gs[0] + G.w[1] * gs[1] + G.w[2] * gs[2]);
    const double wk = G.wd * kq;
    const double v[3] = {G.w[0] * wk, G.w[1] * wk, G.w[2] * wk};
    hex_add_grad_dot(P, ra, v);
  }
}

// Row l of the KNP element matrices: M = mass, S = stiffness, Cc = drift (grad phi . grad N_l) N_j
template <bool AFFINE, class R8>
__device__ __forceinline__ void hex_knp_row(const R8 (&r)[8], int li, double (&M)[8], double (&S)[8], double (&Cc)[8]) {
  double phi[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { phi[j] = r[j].c; M[j] = 0.0; S[j] = 0.0; Cc[j] = 0.0; }
  double dphi[3][4];
  hex_edge_diffs(phi, dphi);
  const HexEdges e = hex_edges(r);
  const bool aff = AFFINE || hex_is_affine(e);
  HexInv I = hex_inverse(e, c_hex.p[0]);
  const int l0 = li & 1, l1 = (li >> 1) & 1, l2 = (li >> 2) & 1;
#pragma unroll 1
  for (int q = 0; q < 8; ++q) {
    const hexq::Point& P = c_hex.p[q];
    if (!AFFINE && !aff && q > 0) I = hex_inverse(e, P);
    const HexGeo G = hex_geo(I, P, l0, l1, l2);
    double gp[3];
    hex_ref_grad(P, dphi, gp);
    const double drift = G.w[0] * gp[0] + G.w[1] * gp[1] + G.w[2] * gp[2];   // grad phi . grad N_l
    const double v[3] = {G.w[0] * G.wd, G.w[1] * G.wd, G.w[2] * G.wd};
    hex_add_grad_dot(P, S, v);
    hex_add_shape(P, M, G.wd * G.Nl);
    hex_add_shape(P, Cc, G.wd * drift);
  }
}

// ---------------------------------------------------------------------------------------------
// Parallelepipeds: closed forms instead of the 2 x 2 x 2 rule (which is exact for these integrands when the Jacobian
// is constant, so both give the same numbers up to rounding).  The row vertex l is moved to local vertex 0 by
// reflecting the reference cell along the axes where l has a bit set: the caller loads the records in the order
// j' = j ^ l, the edge vectors taken from the permuted records carry the reflection, and every result of the frame
// belongs to the cell's local vertex j' ^ l.  With l = 0 the integrals over the unit cube factor into 1D integrals of
// two or three linear functions (1/3, 1/6; 1/4, 1/12), contracted axis by axis (sum factorisation): ~1/5 of the
// operations of the quadrature loop on a box mesh, whose metric tensor is diagonal.
// ---------------------------------------------------------------------------------------------
namespace hexcf {
constexpr double T4 = 0.25, T12 = 1.0 / 12.0, A3 = 1.0 / 3.0, A6 = 1.0 / 6.0;
__host__ __device__ constexpr int ix(int s, int ms, int a, int ma, int b, int mb) { return (ms << s) | (ma << a) | (mb << b); }
__host__ __device__ constexpr double a0(int j) { return j ? A6 : A3; }
// P[ja][jb] = sum_{ma, mb} b(ma, 0, ja) b(mb, 0, jb) k[ma][mb],  b(m, 0, j) = 1/4 if m = j = 0 else 1/12
__device__ __forceinline__ void contract_bb(const double (&k)[2][2], double (&P)[2][2]) {
  const double r00 = T4 * k[0][0] + T12 * k[1][0], r01 = T4 * k[0][1] + T12 * k[1][1];
  const double r10 = T12 * (k[0][0] + k[1][0]), r11 = T12 * (k[0][1] + k[1][1]);
  P[0][0] = T4 * r00 + T12 * r01; P[0][1] = T12 * (r00 + r01);
  P[1][0] = T4 * r10 + T12 * r11; P[1][1] = T12 * (r10 + r11);
}
// Q[js][ju] = sum_{ms, mu} a(ms, js) b(mu, 0, ju) k[ms][mu],  a(m, j) = 1/3 if m = j else 1/6
__device__ __forceinline__ void contract_ab(const double (&k)[2][2], double (&Q)[2][2]) {
  const double v00 = T4 * k[0][0] + T12 * k[0][1], v01 = T12 * (k[0][0] + k[0][1]);
  const double v10 = T4 * k[1][0] + T12 * k[1][1], v11 = T12 * (k[1][0] + k[1][1]);
  Q[0][0] = A3 * v00 + A6 * v10; Q[0][1] = A3 * v01 + A6 * v11;
  Q[1][0] = A6 * v00 + A3 * v10; Q[1][1] = A6 * v01 + A3 * v11;
}
struct Geo { double g[3][3]; double det; bool skew; };   // g = |det J| J^-1 J^-T
template <class R>
__device__ __forceinline__ Geo geometry(const R (&r)[8]) {
  double J[3][3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    J[0][t] = r[1 << t].x - r[0].x; J[1][t] = r[1 << t].y - r[0].y; J[2][t] = r[1 << t].z - r[0].z;
  }
  const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
  const double c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
  const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
  const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02, inv = kn_rcp(det);
  double I[3][3];
  I[0][0] = c00 * inv; I[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * inv; I[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * inv;
  I[1][0] = c01 * inv; I[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * inv; I[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * inv;
  I[2][0] = c02 * inv; I[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * inv; I[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * inv;
  Geo G;
  G.det = fabs(det);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = a; b < 3; ++b) {
      const double v = G.det * (I[a][0] * I[b][0] + I[a][1] * I[b][1] + I[a][2] * I[b][2]);
      G.g[a][b] = v; G.g[b][a] = v;
    }
  G.skew = G.g[0][1] != 0.0 || G.g[0][2] != 0.0 || G.g[1][2] != 0.0;   // false on every cell of a box mesh
  return G;
}
}  // namespace hexcf

namespace hexcf {
// The geometry of a cell of a uniform mesh in the frame of the row vertex: local vertex j ^ li takes position j, i.e. the
// edge vectors of the axes whose bit is set in li change sign: g[s][t] -> d_s d_t g[s][t], |det| unchanged.
__device__ __forceinline__ Geo reflected(const KnHexGeo& U, int li) {
  Geo G;
  G.det = U.det;
  G.skew = U.skew != 0;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) G.g[a][b] = (a != b && (((li >> a) ^ (li >> b)) & 1)) ? -U.g[a][b] : U.g[a][b];
  return G;
}
}  // namespace hexcf

// Row of local vertex 0 (records in the reflected order, see above): kappa-stiffness ra, volume right-hand side.
// BOX: the metric tensor is known to be diagonal (uniform box meshes): the mixed terms are not even compiled
template <bool BOX = false, class R>
__device__ __forceinline__ void hex_emi_row0_g(const R (&r)[8], const hexcf::Geo& G, double (&ra)[8], double& bvol);
__device__ __forceinline__ void hex_emi_row0(const Rec5 (&r)[8], double (&ra)[8], double& bvol) {
  hex_emi_row0_g(r, hexcf::geometry(r), ra, bvol);
}
template <bool BOX, class R>
__device__ __forceinline__ void hex_emi_row0_g(const R (&r)[8], const hexcf::Geo& G, double (&ra)[8], double& bvol) {
  using namespace hexcf;
#pragma unroll
  for (int j = 0; j < 8; ++j) ra[j] = 0.0;
  double bv = 0.0;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int a = (s + 1) % 3, b = (s + 2) % 3;
    double kb[2][2], P[2][2], ds = 0.0;
#pragma unroll
    for (int ma = 0; ma < 2; ++ma)
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) {
        kb[ma][mb] = r[ix(s, 0, a, ma, b, mb)].k + r[ix(s, 1, a, ma, b, mb)].k;
        ds += a0(ma) * a0(mb) * (r[ix(s, 1, a, ma, b, mb)].s - r[ix(s, 0, a, ma, b, mb)].s);
      }
    contract_bb(kb, P);
    const double c = 0.5 * G.g[s][s];
#pragma unroll
    for (int j = 0; j < 8; ++j) ra[j] += (((j >> s) & 1) ? -c : c) * P[(j >> a) & 1][(j >> b) & 1];
    bv += G.g[s][s] * ds;
  }
  if (!BOX && G.skew) {
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        if (s == t) continue;
        const int u = 3 - s - t;
        double kt[2][2], Q[2][2], ds = 0.0;
#pragma unroll
        for (int ms = 0; ms < 2; ++ms)
#pragma unroll
          for (int mu = 0; mu < 2; ++mu) {
            kt[ms][mu] = A3 * r[ix(s, ms, u, mu, t, 0)].k + A6 * r[ix(s, ms, u, mu, t, 1)].k;
            ds += a0(mu) * (r[ix(s, ms, u, mu, t, 1)].s - r[ix(s, ms, u, mu, t, 0)].s);
          }
        contract_ab(kt, Q);
        const double g = G.g[s][t];
#pragma unroll
        for (int j = 0; j < 8; ++j) ra[j] += (((j >> t) & 1) ? -g : g) * Q[(j >> s) & 1][(j >> u) & 1];
        bv += 0.25 * g * ds;
      }
  }
  bvol += bv;
}

// Row of local vertex 0 of the KNP element matrices (records in the reflected order): mass, stiffness, drift.
template <bool BOX = false, class R8>
__device__ __forceinline__ void hex_knp_row0_g(const R8 (&r)[8], const hexcf::Geo& G, double (&M)[8], double (&S)[8], double (&Cc)[8]);
template <class R8>
__device__ __forceinline__ void hex_knp_row0(const R8 (&r)[8], double (&M)[8], double (&S)[8], double (&Cc)[8]) {
  hex_knp_row0_g(r, hexcf::geometry(r), M, S, Cc);
}
template <bool BOX, class R8>
__device__ __forceinline__ void hex_knp_row0_g(const R8 (&r)[8], const hexcf::Geo& G, double (&M)[8], double (&S)[8], double (&Cc)[8]) {
  using namespace hexcf;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    M[j] = G.det * (a0(j & 1) * a0((j >> 1) & 1) * a0((j >> 2) & 1));
    S[j] = 0.0; Cc[j] = 0.0;
  }
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int a = (s + 1) % 3, b = (s + 2) % 3;
    double dp[2][2], P[2][2];
#pragma unroll
    for (int ma = 0; ma < 2; ++ma)
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) dp[ma][mb] = r[ix(s, 1, a, ma, b, mb)].c - r[ix(s, 0, a, ma, b, mb)].c;
    contract_bb(dp, P);
    const double g = G.g[s][s];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const double w = a0((j >> a) & 1) * a0((j >> b) & 1);
      S[j] += (((j >> s) & 1) ? -g : g) * w;
      Cc[j] -= 0.5 * g * P[(j >> a) & 1][(j >> b) & 1];
    }
  }
  if (!BOX && G.skew) {
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        if (s == t) continue;
        const int u = 3 - s - t;
        double dp[2][2], Q[2][2];
#pragma unroll
        for (int ms = 0; ms < 2; ++ms)
#pragma unroll
          for (int mu = 0; mu < 2; ++mu) dp[ms][mu] = r[ix(s, ms, u, mu, t, 1)].c - r[ix(s, ms, u, mu, t, 0)].c;
        contract_ab(dp, Q);
        const double g = G.g[s][t];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          S[j] += (((j >> t) & 1) ? -0.25 * g : 0.25 * g) * a0((j >> u) & 1);
          Cc[j] -= g * a0((j >> t) & 1) * Q[(j >> s) & 1][(j >> u) & 1];
        }
      }
  }
}

// GEO: 0 general trilinear cells (2 x 2 x 2 quadrature), 1 every cell a parallelepiped (closed forms, geometry from the
// staged coordinates), 2 every cell the SAME box (closed forms, the diagonal metric U a constant of the mesh, records without
// coordinates: 16 instead of 40 bytes).  Measured at 165 888 hexahedra (config 2h, round 4): GEO 1 -> 2 takes emi_rows from
// 134 to 99 registers (3 -> 4 waves per SIMD) and 59.9 -> 45.0 us alone (0.29 -> 0.39 of 8 TB/s), 99 -> 64.5 us beside the
// ODE sweep; knp_rows 168 registers + spills -> 123, 59.1 -> 46.1 us (0.285 -> 0.365).  Capping emi_rows at 96 registers
// for a fifth wave per SIMD is slower (53.8 us): fewer registers serialise the eight record reads of a pair.
template <int LPR, int GEO>
__global__ __launch_bounds__(KN_BLOCK, GEO == 2 ? 4 : (GEO == 1 ? 3 : 2)) void emi_rows_hex_v2(
    KnDev D, const KnConsts* __restrict__ Cp, int acc_n, int rec_n, int want_p, int splitting, KnHexGeo U) {
  constexpr int NF = 4;
  constexpr bool AFFINE = GEO >= 1, UNI = GEO == 2;
  constexpr int RW = UNI ? 2 : 5;
  const KnConsts& C = *Cp;
  extern __shared__ __align__(16) double lds[];
  double* accA = lds;
  double* recs = lds + (size_t)acc_n;
  uint16_t* eloc = reinterpret_cast<uint16_t*>(recs + RW * (size_t)rec_n + ((RW * rec_n) & 1));
  const int tid = threadIdx.x;
  const int b = logical_block(blockIdx.x, D.nblocks);
  const BlkInfo B = load_blk(D, b, tid >> 6);
  const int s = B.sub, seglen = B.seglen;
  const int rloc = tid / LPR, sub = tid % LPR;
  const BlkRows<LPR, KN_CHUNK_HEX> rows(D, b);
  bool valid;
  const int g = rows.row(rloc, valid);
  const int64_t base = (int64_t)B.slbase * KN_SLICE + (tid & 63);
  const int np = B.np;
  // first pair entry of this lane: issued before phase A so that its latency overlaps the staging
  int pc0 = -1;
  uint2 sl0 = {0u, 0u};
  if (valid && np > 0) {
    pc0 = D.pair_cell[base];
    sl0 = *reinterpret_cast<const uint2*>(D.pair_slots + 2 * base);
  }
  const int4 ri = D.row_info[g];
  for (int i = tid; i < seglen; i += KN_BLOCK) accA[i] = 0.0;
  const KnSubConst& sc = C.sc[s];
  stage_records<0, UNI>(D, B, recs, eloc, tid, 0.0, nullptr, 0, &sc);
  __syncthreads();

  const bool cell_side = s > 0;
  double bacc = 0.0, gam = 0.0;
  if (valid) {
    const int rowbase = ri.x, lap = ri.y & 0xFFFF, ne = (unsigned)ri.y >> 16, rL = ri.z;
    auto do_pair = [&](int pc, uint2 sl) {
      if constexpr (UNI) {
        const int li = pc & 7;
        const uint64_t s64 = ((uint64_t)sl.y << 32) | sl.x;
        int slot[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) slot[j] = (int)((s64 >> (8 * (j ^ li))) & 255);
        Rec2 r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = lds_rec2(recs, eloc[rL + slot[j]]);
        double ra[8];
        hexcf::Geo G;          // box: diagonal metric, invariant under the reflections of the row-vertex frame
        G.det = U.det; G.skew = false;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int b2 = 0; b2 < 3; ++b2) G.g[a][b2] = a == b2 ? U.g[a][a] : 0.0;
        hex_emi_row0_g<true>(r, G, ra, bacc);
#pragma unroll
        for (int j = 0; j < 8; ++j) unsafeAtomicAdd(&accA[lap + slot[j]], ra[j]);
        return;
      }
      const int li = pc & 7;
      int slot[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) { slot[j] = (sl.x >> (8 * j)) & 255; slot[4 + j] = (sl.y >> (8 * j)) & 255; }
      if constexpr (AFFINE) {   // frame of the row vertex: local vertex j ^ li takes position j
        const uint64_t s64 = ((uint64_t)sl.y << 32) | sl.x;
#pragma unroll
        for (int j = 0; j < 8; ++j) slot[j] = (int)((s64 >> (8 * (j ^ li))) & 255);
      }
      Rec5 r[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = lds_rec5(recs, eloc[rL + slot[j]]);
      double ra[8];
      if constexpr (AFFINE) hex_emi_row0(r, ra, bacc);
      else hex_emi_row<false>(r, li, ra, bacc);
#pragma unroll
      for (int j = 0; j < 8; ++j) unsafeAtomicAdd(&accA[lap + slot[j]], ra[j]);
    };
    if (pc0 >= 0) do_pair(pc0, sl0);
    for (int p = 1; p < np; ++p) {
      const int64_t ent = base + (int64_t)p * KN_SLICE;
      const int pc = D.pair_cell[ent];
      if (pc >= 0) do_pair(pc, *reinterpret_cast<const uint2*>(D.pair_slots + 2 * ent));
    }
    if (ne > 0) emi_membrane_row<NF>(D, C, ri.w, ne, sub, LPR, cell_side, rowbase, accA, splitting, gam);
  }
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) { bacc += __shfl_xor(bacc, m); gam += __shfl_xor(gam, m); }
  if (valid && sub == 0) D.b_emi[g] = bacc + gam;
  __syncthreads();
  rows.for_each_entry(tid, 0, [&](int i, int64_t gp) {
    const double a = accA[i];
    KN_ROW_STORE(a, &D.A_emi[gp]);
    if (want_p) KN_ROW_STORE(cell_side ? a + D.P_mass[gp - D.pmass0] : a, &D.P_emi[gp]);
  });
}

template <int LPR, int GEO, int KS, int MEM>
__global__ __launch_bounds__(KN_BLOCK, GEO == 2 ? 4 : (GEO == 1 ? 3 : 2)) void knp_rows_hex_v2(
    KnDev D, const KnConsts* __restrict__ Cp, int acc_n, int rec_n, int gam_n, int splitting, KnHexGeo U) {
  constexpr bool AFFINE = GEO >= 1, UNI = GEO == 2;
  constexpr int RW = UNI ? KS + 1 : 4 + KS;
  const KnConsts& C = *Cp;
  extern __shared__ __align__(16) double lds[];
  double* acc = lds;
  double* recs = lds + (size_t)KS * acc_n;
  double* gam = recs + (size_t)RW * rec_n + ((RW * rec_n) & 1);
  uint16_t* eloc = reinterpret_cast<uint16_t*>(gam + (size_t)KS * gam_n);
  const int tid = threadIdx.x;
  const int b = logical_block(blockIdx.x, D.nblocks);
  const BlkInfo B = load_blk(D, b, tid >> 6);
  const int s = B.sub, nnzLb = B.nnzLb;
  const int v0 = C.voff[s], nvs = C.voff[s + 1] - v0;
  const double* fs0 = (D.fsrc && s == 0) ? D.fsrc : nullptr;
  const int rloc = tid / LPR, sub = tid % LPR;
  const BlkRows<LPR, KN_CHUNK_HEX> rows(D, b);
  bool valid;
  const int g = rows.row(rloc, valid);
  const int64_t base = (int64_t)B.slbase * KN_SLICE + (tid & 63);
  const int np = B.np;
  int pc0 = -1;
  uint2 sl0 = {0u, 0u};
  if (valid && np > 0) {
    pc0 = D.pair_cell[base];
    sl0 = *reinterpret_cast<const uint2*>(D.pair_slots + 2 * base);
  }
  const int4 ri = D.row_info[g];
  for (int i = tid; i < nnzLb; i += KN_BLOCK) {
#pragma unroll
    for (int k = 0; k < KS; ++k) acc[(size_t)k * acc_n + i] = 0.0;
  }
  stage_records<KS, UNI>(D, B, recs, eloc, tid, C.inv_dt, fs0, nvs);
  if constexpr (MEM == 1) membrane_entries_to_lds<4, KS>(D, C, B.me0, B.mne, s > 0, splitting, tid, gam);
  __syncthreads();

  const KnSubConst& sc = C.sc[s];
  double bk[KS];
#pragma unroll
  for (int k = 0; k < KS; ++k) bk[k] = 0.0;
  if (valid) {
    const int rL = ri.z;
    auto do_pair = [&](int pc, uint2 sl) {
      const int li = pc & 7;
      if constexpr (UNI) {
        const uint64_t s64 = ((uint64_t)sl.y << 32) | sl.x;
        int slot[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) slot[j] = (int)((s64 >> (8 * (j ^ li))) & 255);
        RecU<KS> r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = lds_recu<KS>(recs, eloc[rL + slot[j]]);
        double M[8], S[8], Cc[8];
        hexcf::Geo G;
        G.det = U.det; G.skew = false;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int b2 = 0; b2 < 3; ++b2) G.g[a][b2] = a == b2 ? U.g[a][a] : 0.0;
        hex_knp_row0_g<true>(r, G, M, S, Cc);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
#pragma unroll
          for (int k = 0; k < KS; ++k) {
            unsafeAtomicAdd(&acc[(size_t)k * acc_n + rL + slot[j]], M[j] * C.inv_dt + sc.D[k] * S[j] + sc.zpsiD[k] * Cc[j]);
            bk[k] += M[j] * r[j].f[k];
          }
        }
        return;
      }
      int slot[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) { slot[j] = (sl.x >> (8 * j)) & 255; slot[4 + j] = (sl.y >> (8 * j)) & 255; }
      if constexpr (AFFINE) {   // frame of the row vertex: local vertex j ^ li takes position j
        const uint64_t s64 = ((uint64_t)sl.y << 32) | sl.x;
#pragma unroll
        for (int j = 0; j < 8; ++j) slot[j] = (int)((s64 >> (8 * (j ^ li))) & 255);
      }
      RecK<KS> r[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = lds_rec<KS>(recs, eloc[rL + slot[j]]);
      double M[8], S[8], Cc[8];
      if constexpr (AFFINE) hex_knp_row0(r, M, S, Cc);
      else hex_knp_row<false>(r, li, M, S, Cc);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int k = 0; k < KS; ++k) {
          unsafeAtomicAdd(&acc[(size_t)k * acc_n + rL + slot[j]], M[j] * C.inv_dt + sc.D[k] * S[j] + sc.zpsiD[k] * Cc[j]);
          bk[k] += M[j] * r[j].f[k];
        }
      }
    };
    if (pc0 >= 0) do_pair(pc0, sl0);
    for (int p = 1; p < np; ++p) {
      const int64_t ent = base + (int64_t)p * KN_SLICE;
      const int pc = D.pair_cell[ent];
      if (pc >= 0) do_pair(pc, *reinterpret_cast<const uint2*>(D.pair_slots + 2 * ent));
    }
    {   // the row's LPR lanes share its membrane entries (the sums meet in the reduction below)
      const int ne = (unsigned)ri.y >> 16;
      for (int e = ri.w + sub; e < ri.w + ne; e += LPR) {
        if constexpr (MEM == 2) membrane_entry_early<4, KS>(D, e, bk);
        else {
#pragma unroll
          for (int k = 0; k < KS; ++k) bk[k] += MEM == 1 ? gam[(size_t)(e - B.me0) * KS + k] : D.gam_e[(size_t)KS * e + k];
        }
      }
    }
  }
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) {
#pragma unroll
    for (int k = 0; k < KS; ++k) bk[k] += __shfl_xor(bk[k], m);
  }
  if (valid && sub == 0) {
    const size_t bb = (size_t)KS * v0 + (size_t)(g - v0);
#pragma unroll
    for (int k = 0; k < KS; ++k) D.b_knp[bb + (size_t)k * nvs] = bk[k];
  }
  __syncthreads();
  const int64_t subnnz0 = D.rowptrL[v0], subnnz = D.rowptrL[v0 + nvs] - subnnz0;
  double* out0 = D.A_knp + (size_t)KS * subnnz0 - subnnz0;
  rows.for_each_entry(tid, 1, [&](int i, int64_t gp) {
#pragma unroll
    for (int k = 0; k < KS; ++k) KN_ROW_STORE(acc[(size_t)k * acc_n + i], &out0[(size_t)k * subnnz + gp]);
  });
}

// =============================================================================================
// Q1 quadrilaterals: the row-block scheme once more, with 2-D records (EMI x y kappa sigma, KNP x y f_0 .. phi) and the
// element rows of quad_rows.h.  A (row, cell) pair is pair_cell (cell * 8 + the row vertex's local index) and ONE word of
// four row-relative slot bytes; the membrane facets are intervals, the NF = 2 code of the triangles.
// GEO: 0 general bilinear cells (2 x 2 quadrature), 1 every cell a parallelogram (closed forms in the frame of the row
// vertex).  There is no uniform-cell variant.
// =============================================================================================
template <int LPR, int GEO>
__global__ __launch_bounds__(KN_BLOCK) void emi_rows_quad_v2(KnDev D, const KnConsts* __restrict__ Cp, int acc_n, int rec_n,
                                                             int want_p, int splitting) {
  constexpr int NF = 2, RW = 4;
  const KnConsts& C = *Cp;
  extern __shared__ __align__(16) double lds[];
  double* accA = lds;
  double* recs = lds + (size_t)acc_n;
  uint16_t* eloc = reinterpret_cast<uint16_t*>(recs + RW * (size_t)rec_n);
  const int tid = threadIdx.x;
  const int b = logical_block(blockIdx.x, D.nblocks);
  const BlkInfo B = load_blk(D, b, tid >> 6);
  const int s = B.sub, seglen = B.seglen;
  const int rloc = tid / LPR, sub = tid % LPR;
  const BlkRows<LPR, KN_CHUNK_SIMPLEX> rows(D, b);
  bool valid;
  const int g = rows.row(rloc, valid);
  const int64_t base = (int64_t)B.slbase * KN_SLICE + (tid & 63);
  const int np = B.np;
  // first pair entry of this lane: issued before phase A so that its latency overlaps the staging
  int pc0 = -1;
  uint32_t sl0 = 0u;
  if (valid && np > 0) {
    pc0 = D.pair_cell[base];
    sl0 = D.pair_slots[base];
  }
  const int4 ri = D.row_info[g];
  for (int i = tid; i < seglen; i += KN_BLOCK) accA[i] = 0.0;
  const KnSubConst& sc = C.sc[s];
  stage_records<0, false, 2>(D, B, recs, eloc, tid, 0.0, nullptr, 0, &sc);
  __syncthreads();

  const bool cell_side = s > 0;
  double bacc = 0.0, gam = 0.0;
  if (valid) {
    const int rowbase = ri.x, lap = ri.y & 0xFFFF, ne = (unsigned)ri.y >> 16, rL = ri.z;
    auto do_pair = [&](int pc, uint32_t sl) {
      const int li = pc & 3;
      int slot[4];
      // GEO 1: the frame of the row vertex, local vertex j ^ li takes position j
#pragma unroll
      for (int j = 0; j < 4; ++j) slot[j] = (int)((sl >> (8 * (GEO == 1 ? j ^ li : j))) & 255);
      RecQ4 r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = lds_recq4(recs, eloc[rL + slot[j]]);
      double ra[4];
      if constexpr (GEO == 1) quadcf::emi_row0(r, ra, bacc);
      else quadq::emi_row(r, li, ra, bacc);
#pragma unroll
      for (int j = 0; j < 4; ++j) unsafeAtomicAdd(&accA[lap + slot[j]], ra[j]);
    };
    if (pc0 >= 0) do_pair(pc0, sl0);
    for (int p = 1; p < np; ++p) {
      const int64_t ent = base + (int64_t)p * KN_SLICE;
      const int pc = D.pair_cell[ent];
      if (pc >= 0) do_pair(pc, D.pair_slots[ent]);
    }
    if (ne > 0) emi_membrane_row<NF>(D, C, ri.w, ne, sub, LPR, cell_side, rowbase, accA, splitting, gam);
  }
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) { bacc += __shfl_xor(bacc, m); gam += __shfl_xor(gam, m); }
  if (valid && sub == 0) D.b_emi[g] = bacc + gam;
  __syncthreads();
  rows.for_each_entry(tid, 0, [&](int i, int64_t gp) {
    const double a = accA[i];
    KN_ROW_STORE(a, &D.A_emi[gp]);
    if (want_p) KN_ROW_STORE(cell_side ? a + D.P_mass[gp - D.pmass0] : a, &D.P_emi[gp]);
  });
}

template <int LPR, int GEO, int KS, int MEM>
__global__ __launch_bounds__(KN_BLOCK) void knp_rows_quad_v2(KnDev D, const KnConsts* __restrict__ Cp, int acc_n, int rec_n,
                                                             int gam_n, int splitting) {
  constexpr int RW = 3 + KS;
  const KnConsts& C = *Cp;
  extern __shared__ __align__(16) double lds[];
  double* acc = lds;
  double* recs = lds + (size_t)KS * acc_n;
  double* gam = recs + (size_t)RW * rec_n + ((RW * rec_n) & 1);
  uint16_t* eloc = reinterpret_cast<uint16_t*>(gam + (size_t)KS * gam_n);
  const int tid = threadIdx.x;
  const int b = logical_block(blockIdx.x, D.nblocks);
  const BlkInfo B = load_blk(D, b, tid >> 6);
  const int s = B.sub, nnzLb = B.nnzLb;
  const int v0 = C.voff[s], nvs = C.voff[s + 1] - v0;
  const double* fs0 = (D.fsrc && s == 0) ? D.fsrc : nullptr;
  const int rloc = tid / LPR, sub = tid % LPR;
  const BlkRows<LPR, KN_CHUNK_SIMPLEX> rows(D, b);
  bool valid;
  const int g = rows.row(rloc, valid);
  const int64_t base = (int64_t)B.slbase * KN_SLICE + (tid & 63);
  const int np = B.np;
  int pc0 = -1;
  uint32_t sl0 = 0u;
  if (valid && np > 0) {
    pc0 = D.pair_cell[base];
    sl0 = D.pair_slots[base];
  }
  const int4 ri = D.row_info[g];
  for (int i = tid; i < nnzLb; i += KN_BLOCK) {
#pragma unroll
    for (int k = 0; k < KS; ++k) acc[(size_t)k * acc_n + i] = 0.0;
  }
  stage_records<KS, false, 2>(D, B, recs, eloc, tid, C.inv_dt, fs0, nvs);
  if constexpr (MEM == 1) membrane_entries_to_lds<2, KS>(D, C, B.me0, B.mne, s > 0, splitting, tid, gam);
  __syncthreads();

  const KnSubConst& sc = C.sc[s];
  double bk[KS];
#pragma unroll
  for (int k = 0; k < KS; ++k) bk[k] = 0.0;
  if (valid) {
    const int rL = ri.z;
    auto do_pair = [&](int pc, uint32_t sl) {
      const int li = pc & 3;
      int slot[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) slot[j] = (int)((sl >> (8 * (GEO == 1 ? j ^ li : j))) & 255);
      RecQK<KS> r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = lds_recqk<KS>(recs, eloc[rL + slot[j]]);
      double M[4], S[4], Cc[4];
      if constexpr (GEO == 1) quadcf::knp_row0(r, M, S, Cc);
      else quadq::knp_row(r, li, M, S, Cc);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int k = 0; k < KS; ++k) {
          unsafeAtomicAdd(&acc[(size_t)k * acc_n + rL + slot[j]], M[j] * C.inv_dt + sc.D[k] * S[j] + sc.zpsiD[k] * Cc[j]);
          bk[k] += M[j] * r[j].f[k];
        }
      }
    };
    if (pc0 >= 0) do_pair(pc0, sl0);
    for (int p = 1; p < np; ++p) {
      const int64_t ent = base + (int64_t)p * KN_SLICE;
      const int pc = D.pair_cell[ent];
      if (pc >= 0) do_pair(pc, D.pair_slots[ent]);
    }
    {   // the row's LPR lanes share its membrane entries (the sums meet in the reduction below)
      const int ne = (unsigned)ri.y >> 16;
      for (int e = ri.w + sub; e < ri.w + ne; e += LPR) {
        if constexpr (MEM == 2) membrane_entry_early<2, KS>(D, e, bk);
        else {
#pragma unroll
          for (int k = 0; k < KS; ++k) bk[k] += MEM == 1 ? gam[(size_t)(e - B.me0) * KS + k] : D.gam_e[(size_t)KS * e + k];
        }
      }
    }
  }
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) {
#pragma unroll
    for (int k = 0; k < KS; ++k) bk[k] += __shfl_xor(bk[k], m);
  }
  if (valid && sub == 0) {
    const size_t bb = (size_t)KS * v0 + (size_t)(g - v0);
#pragma unroll
    for (int k = 0; k < KS; ++k) D.b_knp[bb + (size_t)k * nvs] = bk[k];
  }
  __syncthreads();
  const int64_t subnnz0 = D.rowptrL[v0], subnnz = D.rowptrL[v0 + nvs] - subnnz0;
  double* out0 = D.A_knp + (size_t)KS * subnnz0 - subnnz0;
  rows.for_each_entry(tid, 1, [&](int i, int64_t gp) {
#pragma unroll
    for (int k = 0; k < KS; ++k) KN_ROW_STORE(acc[(size_t)k * acc_n + i], &out0[(size_t)k * subnnz + gp]);
  });
}

// ---------------------------------------------------------------------------------------------
// KNP membrane-facet kernel: the rational Robin/coupling integrand of knpWeakForm.py:168-214 with
// degree-6 quadrature (tables staged in LDS).  One thread per (membrane facet, side): it evaluates the
// integrand once per quadrature point and tests it against all NF facet basis functions, writing
// NF x 2 (ions) partial integrals to `gam_contrib`; the row kernel adds them into b_knp in a fixed
// order, so nothing is accumulated atomically.
// ---------------------------------------------------------------------------------------------
// (FacetData, load_facet and the fields at a quadrature point, facet_point_fields: membrane_facet.h)

// weight x integrand of the K - 1 solved ions at quadrature point q (knpWeakForm.py:178-214):
//   fk[k] = w_q * sgn * (C_k g_k - C_k [phi]),  C_k = alpha_k C_M / (F z_k dt),  alpha_k = D_k z_k^2 c_k / sum_j D_j z_j^2 c_j
template <int NF>
__device__ __forceinline__ void facet_point(const FacetData<NF>& f, const KnConsts& C, int q, const double* qw,
                                            const double* qN, const double* qdN, int splitting, double (&fk)[KN_MAXK - 1]) {
  const int KS = C.K - 1;
  FacetPoint P;
  facet_point_fields<NF>(f, q, qw, qN, qdN, P);
  const double (&cq)[KN_MAXK] = P.cq, (&iq)[KN_MAXK] = P.iq;
  const double pmq = P.pmq, it = P.it, wq = P.wq;
  const double jump = P.ph_i - P.ph_e;
  const double rasum = kn_rcp(P.asum);
#pragma unroll
  for (int k = 0; k < KN_MAXK - 1; ++k) {
    fk[k] = 0.0;
    if (k < KS) {
      const double al = f.so->az2D[k] * cq[k] * rasum;
      const double Cc = al * C.C_M * kn_rcp(C.F * C.z[k] * C.dt);
      double gr = pmq - C.dt * kn_rcp(C.C_M * al) * iq[k];
      if (splitting) gr += (C.dt / C.C_M) * it;
      fk[k] = wq * f.sgn * (Cc * gr - Cc * jump);
    }
  }
}

// The same point for the early form: cw[k] = w sgn C_k (the factor of -[phi]) and pg[k] = w sgn C_k g_k.
template <int NF>
__device__ __forceinline__ void facet_point_split(const FacetData<NF>& f, const KnConsts& C, int q, const double* qw,
                                                  const double* qN, const double* qdN, int splitting,
                                                  double (&cw)[KN_MAXK - 1], double (&pg)[KN_MAXK - 1]) {
  const int KS = C.K - 1;
  double cq[KN_MAXK], iq[KN_MAXK], pmq = 0, it = 0;
#pragma unroll
  for (int k = 0; k < KN_MAXK; ++k) { cq[k] = 0.0; iq[k] = 0.0; }
#pragma unroll
  for (int bb = 0; bb < NF; ++bb) {
    const double N = qN[q * NF + bb];
    const Rec& o = f.cell_side ? f.pi[bb] : f.pe[bb];
#pragma unroll
    for (int k = 0; k < KN_MAXK; ++k) { cq[k] += N * o.c[k]; iq[k] += N * f.Ik[bb][k]; }
    pmq += N * f.pm[bb]; it += N * f.It[bb];
  }
  double wq;
  if constexpr (NF == 4) {
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
    wq = qw[q] * f.meas * (NF == 2 ? 1.0 : 2.0);
  }
  double asum = 0.0;
#pragma unroll
  for (int k = 0; k < KN_MAXK; ++k) asum += f.so->az2D[k] * cq[k];
#pragma unroll
  for (int k = 0; k < KN_MAXK - 1; ++k) {
    cw[k] = 0.0; pg[k] = 0.0;
    if (k < KS) {
      const double al = f.so->az2D[k] * cq[k] / asum;
      const double Cc = al * C.C_M / (C.F * C.z[k] * C.dt);
      double gr = pmq - C.dt / (C.C_M * al) * iq[k];
      if (splitting) gr += (C.dt / C.C_M) * it;
      cw[k] = wq * f.sgn * Cc;
      pg[k] = cw[k] * gr;
    }
  }
}

// Stand-alone form (diagnostics, KNPEMI_OPT_FUSE_MEMBRANE = 0): one thread per (facet, side) tests the integrand
// against all NF facet functions and writes NF x (K - 1) partial integrals to gam_e.
// (KN_MEM_LQ adjacent lanes share one (facet, side): membrane_facet.h)
// One workgroup's share of the facet integrals; `bid` = its index among the `nb` workgroups that do this work (after the
// XCD-aware remap: consecutive facets share vertex records, so each XCD takes one contiguous run of facets and fetches a
// record once instead of once per XCD that meets it: 2.5 MB instead of ... of HBM-side traffic at config 2).
template <int NF>
__device__ __forceinline__ void knp_membrane_block(const KnDev& D, const KnConsts& C, int splitting, int bid,
                                                   const double* __restrict__ phi_x, double* qt) {
  const int nq = D.nq_gamma;
  const int ntab = nq * (1 + NF + (NF == 4 ? 2 * NF : 0));
  const int gt = bid * blockDim.x + threadIdx.x;
  const int t = gt / KN_MEM_LQ, lq = gt % KN_MEM_LQ;
  // lanes past the last (facet, side) repeat the last one and drop their results: the shuffles below see whole groups
  const bool live = t < 2 * D.nftot;
  const int tt = live ? t : 2 * D.nftot - 1;
  const int KS = C.K - 1;
  const int fg = tt >> 1;
  const bool cell_side = tt & 1;
  // Two memory round trips before the quadrature.  The first: everything whose address the thread index gives -- the table,
  // the facet's model and indices, the entries its integrals go to.  The second: the facet's data, for every facet -- one
  // without a model loads with slot 0 (always allocated) and drops what it loaded -- issued before the barrier that
  // publishes the table, so that the barrier is not a third.
  const int ms = D.fmodel[fg];
  const FacetIdx<NF> ix = load_facet_idx<NF>(D, fg);
  int pos[NF];   // entry of (facet, side, local vertex) in the membrane row lists
#pragma unroll
  for (int a = 0; a < NF; ++a) pos[a] = D.gam_pos[(size_t)tt * NF + a];
  for (int i = threadIdx.x; i < ntab; i += blockDim.x) qt[i] = D.qtab[i];
  FacetData<NF> f;
  load_facet<NF>(D, C, ix, cell_side, ms < 0 ? 0 : ms, f, phi_x);
  __syncthreads();
  const double* qw = qt;
  const double* qN = qt + nq;
  const double* qdN = qt + nq * (1 + NF);
  double acc[NF][KN_MAXK - 1];
#pragma unroll
  for (int a = 0; a < NF; ++a)
#pragma unroll
    for (int k = 0; k < KN_MAXK - 1; ++k) acc[a][k] = 0.0;
  if (ms >= 0) {
    for (int q = lq; q < nq; q += KN_MEM_LQ) {
      double fk[KN_MAXK - 1];
      facet_point<NF>(f, C, q, qw, qN, qdN, splitting, fk);
#pragma unroll
      for (int a = 0; a < NF; ++a)
#pragma unroll
        for (int k = 0; k < KN_MAXK - 1; ++k) acc[a][k] += qN[q * NF + a] * fk[k];
    }
  }
#pragma unroll
  for (int m = 1; m < KN_MEM_LQ; m <<= 1)
#pragma unroll
    for (int a = 0; a < NF; ++a)
#pragma unroll
      for (int k = 0; k < KN_MAXK - 1; ++k) acc[a][k] += __shfl_xor(acc[a][k], m);
  if (live && lq == 0) {
#pragma unroll
    for (int a = 0; a < NF; ++a)
#pragma unroll
      for (int k = 0; k < KN_MAXK - 1; ++k)
        if (k < KS) D.gam_e[(size_t)KS * pos[a] + k] = acc[a][k];
  }
}

template <int NF>
__global__ __launch_bounds__(256) void knp_membrane_kernel(KnDev D, const KnConsts* __restrict__ Cp, int splitting) {
  extern __shared__ double qt[];
  knp_membrane_block<NF>(D, *Cp, splitting, logical_block(blockIdx.x, gridDim.x), nullptr, qt);
}

// The write-back of the potential and the facet integrals of b_knp in ONE launch: the first `nbm` workgroups integrate the
// membrane facets with the potential taken from the solution vector x itself (the mean that the write-back removes cancels
// in the jump phi_i - phi_e), the others write phi = x - mean into the vertex records (mean = inv_n x the sum of the np
// partial sums in `part`; np = 0: no shift, e.g. a pasted solution).  This takes the facet kernel out of the chain
// EMI solve -> KNP assembly: knpemi_assemble_knp finds the integrals in gam_e (knpemi_handle::gam_gen).
template <int NF>
__global__ __launch_bounds__(256) void emi_writeback_membrane_kernel(KnDev D, const KnConsts* __restrict__ Cp, int splitting,
                                                                     int nbm, const double* __restrict__ x, int n,
                                                                     const double* __restrict__ part, int np, double inv_n,
                                                                     double* __restrict__ mean_out) {
  extern __shared__ double qt[];
  if ((int)blockIdx.x < nbm) {
    knp_membrane_block<NF>(D, *Cp, splitting, logical_block(blockIdx.x, nbm), x, qt);
    return;
  }
  const int vb = blockIdx.x - nbm, nvb = gridDim.x - nbm;
  int i = vb * 256 + threadIdx.x;
  double xi = i < n ? x[i] : 0.0;
  double mean = 0.0;
  if (np > 0) {          // the <= 1 024 partial sums, all of a thread's loads in flight; fixed order: the same bits in every block
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
    const int t = threadIdx.x;
    if (t < np) v0 = part[t];
    if (t + 256 < np) v1 = part[t + 256];
    if (t + 512 < np) v2 = part[t + 512];
    if (t + 768 < np) v3 = part[t + 768];
    double sum = ((v0 + v1) + v2) + v3;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
    __shared__ double sh[4];
    if ((t & 63) == 0) sh[t >> 6] = sum;
    __syncthreads();
    mean = ((sh[0] + sh[1]) + (sh[2] + sh[3])) * inv_n;
    if (vb == 0 && t == 0 && mean_out) *mean_out = mean;
  }
  while (i < n) {
    D.VR[(size_t)i * KN_REC + 7] = xi - mean;
    i += nvb * 256;
    if (i < n) xi = x[i];
  }
}

// Early form (KNPEMI_MEMBRANE_EARLY): everything of the integrand that does not depend on the potential is integrated
// BEFORE the EMI solve, beside it on the auxiliary stream.  With  [phi](q) = sum_b N_b(q) [phi]_b  the integrand
//   w sgn (C_k g_k - C_k [phi])  tested with N_a  splits into
//   P[a][k] = sum_q N_a w sgn C_k g_k      and      W[a][b][k] = sum_q N_a N_b w sgn C_k,
// so that the KNP row kernel only has to form  P[a][k] - sum_b W[a][b][k] [phi]_b  from the potential just solved for:
// the degree-6 quadrature leaves the chain  EMI solve -> KNP assembly.  (1 + NF) (K - 1) doubles per entry in gpre.
template <int NF>
__global__ __launch_bounds__(256) void knp_membrane_pre_kernel(KnDev D, const KnConsts* __restrict__ Cp, int splitting) {
  const KnConsts& C = *Cp;
  extern __shared__ double qt[];
  const int nq = D.nq_gamma;
  const int ntab = nq * (1 + NF + (NF == 4 ? 2 * NF : 0));
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  // as in knp_membrane_block: what the thread index addresses beside the table, the facet's data before the barrier
  const bool live = t < 2 * D.nftot;
  const int tt = live ? t : 2 * D.nftot - 1;
  const int KS = C.K - 1, GS = (1 + NF) * KS;
  const int fg = tt >> 1;
  const bool cell_side = tt & 1;
  const int ms = D.fmodel[fg];
  const FacetIdx<NF> ix = load_facet_idx<NF>(D, fg);
  int pos[NF];
#pragma unroll
  for (int a = 0; a < NF; ++a) pos[a] = D.gam_pos[(size_t)tt * NF + a];
  for (int i = threadIdx.x; i < ntab; i += blockDim.x) qt[i] = D.qtab[i];
  FacetData<NF> f;
  load_facet<NF>(D, C, ix, cell_side, ms < 0 ? 0 : ms, f);
  __syncthreads();
  const double* qw = qt;
  const double* qN = qt + nq;
  const double* qdN = qt + nq * (1 + NF);
  if (!live) return;
  if (ms < 0) {
#pragma unroll
    for (int a = 0; a < NF; ++a)
      for (int j = 0; j < GS; ++j) D.gpre[(size_t)GS * pos[a] + j] = 0.0;
    return;
  }
  double P[NF][KN_MAXK - 1], W[NF][NF][KN_MAXK - 1];
#pragma unroll
  for (int a = 0; a < NF; ++a)
#pragma unroll
    for (int k = 0; k < KN_MAXK - 1; ++k) {
      P[a][k] = 0.0;
#pragma unroll
      for (int b = 0; b < NF; ++b) W[a][b][k] = 0.0;
    }
  for (int q = 0; q < nq; ++q) {
    double cw[KN_MAXK - 1], pg[KN_MAXK - 1];
    facet_point_split<NF>(f, C, q, qw, qN, qdN, splitting, cw, pg);
#pragma unroll
    for (int a = 0; a < NF; ++a) {
      const double Na = qN[q * NF + a];
#pragma unroll
      for (int k = 0; k < KN_MAXK - 1; ++k) {
        P[a][k] += Na * pg[k];
#pragma unroll
        for (int b = 0; b < NF; ++b) W[a][b][k] += Na * qN[q * NF + b] * cw[k];
      }
    }
  }
#pragma unroll
  for (int a = 0; a < NF; ++a) {
    double* g = D.gpre + (size_t)GS * pos[a];
#pragma unroll
    for (int k = 0; k < KN_MAXK - 1; ++k)
      if (k < KS) {
        g[k] = P[a][k];
#pragma unroll
        for (int b = 0; b < NF; ++b) g[(1 + b) * KS + k] = W[a][b][k];
      }
  }
}

// Fused form: the KNP row kernels call this before their barrier.  The membrane entries (row, facet, local vertex a)
// of a row block are contiguous [e0, e0 + ne); each thread integrates the entries i = tid, tid + 256, ... against the
// ONE facet function of its entry -- the same sums, in the same order, as the stand-alone kernel forms for that
// function -- and leaves the K - 1 integrals in LDS for the row's lane.  No separate launch, nothing through HBM.
template <int NF, int KS>
__device__ __forceinline__ void membrane_entries_to_lds(const KnDev& D, const KnConsts& C, int e0, int ne, bool cell_side,
                                                        int splitting, int tid, double* gam) {
  const int nq = D.nq_gamma;
  const double* qw = D.qtab;
  const double* qN = D.qtab + nq;
  const double* qdN = D.qtab + nq * (1 + NF);
  for (int i = tid; i < ne; i += KN_BLOCK) {
    const int e = e0 + i;
    const int ms = D.me_model[e];
    double acc[KN_MAXK - 1];
#pragma unroll
    for (int k = 0; k < KN_MAXK - 1; ++k) acc[k] = 0.0;
    if (ms >= 0) {
      const int ent = D.mentry[e];
      const int fg = ent >> 3, a = ent & 7;
      FacetData<NF> f;
      load_facet<NF>(D, C, fg, cell_side, ms, f);
      for (int q = 0; q < nq; ++q) {
        double fk[KN_MAXK - 1];
        facet_point<NF>(f, C, q, qw, qN, qdN, splitting, fk);
        const double Na = qN[q * NF + a];
#pragma unroll
        for (int k = 0; k < KN_MAXK - 1; ++k) acc[k] += Na * fk[k];
      }
    }
#pragma unroll
    for (int k = 0; k < KS; ++k) gam[(size_t)i * KS + k] = acc[k];
  }
}

// ---------------------------------------------------------------------------------------------
// small data-movement kernels
// ---------------------------------------------------------------------------------------------
__global__ void scatter_kernel(const double* __restrict__ src, double* __restrict__ dst, int n, int stride) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[(size_t)i * stride] = src[i];
}

__global__ void gather_kernel(const double* __restrict__ src, int stride, double* __restrict__ dst, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[(size_t)i * stride];
}

// buf[i] = vec[idx[i]] (gather) or vec[idx[i]] = buf[i] (scatter): pack / unpack of the halo of a solver vector
__global__ void vec_index_kernel(double* __restrict__ vec, const int* __restrict__ idx, int n, double* __restrict__ buf,
                                 int gather) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (gather) buf[i] = vec[idx[i]];
  else vec[idx[i]] = buf[i];
}

// interpolate_to_membrane (utils.py:150-207): for CG-1 on matching meshes the trace is a gather.
// ue / ui are sub-mesh-local arrays, q2e / q2i hold global vertex ids (offsets v0e = 0, v0i).
__global__ void trace_kernel(const double* __restrict__ ue, const double* __restrict__ ui,
                             const int* __restrict__ q2e, const int* __restrict__ q2i, int q0, int nq,
                             int v0i, double* __restrict__ qe, double* __restrict__ qi) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nq) {
    qe[i] = ue[q2e[q0 + i]];
    qi[i] = ui[q2i[q0 + i] - v0i];
  }
}

// update_pde_variables (utils.py:238-295): c_prev <- c, eliminated ion from electroneutrality,
// phi_M_prev <- tr(phi_i) - tr(phi_e).
__global__ void update_pde_kernel(KnDev D, const KnConsts* __restrict__ Cp) {
  const KnConsts& C = *Cp;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < D.Ntot) {
    int s = 0;
    for (int t = 1; t < C.n_sub; ++t) s += i >= C.voff[t];
    const int KS = C.K - 1;
    double* rec = D.VR + (size_t)i * KN_REC;  // the phi component is left untouched
    double el = C.sc[s].rho_term;
    for (int k = 0; k < KS; ++k) {
      const double ck = D.csol[(size_t)k * D.Ntot + i];
      el += C.elim_coef[k] * ck;
      rec[KN_CSLOT(k)] = ck;
    }
    rec[KN_CSLOT(KS)] = el;
  }
  if (i < D.NQtot) D.phiM[i] = D.VR[(size_t)D.q2i[i] * KN_REC + 7] - D.VR[(size_t)D.q2e[i] * KN_REC + 7];
}

// Write-back of the KNP solve fused with update_pde_variables (KNPEMI_OPT_FUSE_UPDATE): x holds the solution in the
// reference's block order [sub-domain][ion][vertex] (pdeSolver.py:117); same arithmetic as update_pde_kernel.
__global__ void knp_writeback_update_kernel(KnDev D, const KnConsts* __restrict__ Cp, const double* __restrict__ x) {
  const KnConsts& C = *Cp;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < D.Ntot) {
    int s = 0;
    for (int t = 1; t < C.n_sub; ++t) s += i >= C.voff[t];
    const int v0 = C.voff[s], nv = C.voff[s + 1] - v0;
    const int KS = C.K - 1;
    const size_t xb = (size_t)KS * v0 + (size_t)(i - v0);
    double* rec = D.VR + (size_t)i * KN_REC;
    double el = C.sc[s].rho_term;
    for (int k = 0; k < KS; ++k) {
      const double ck = x[xb + (size_t)k * nv];
      D.csol[(size_t)k * D.Ntot + i] = ck;
      el += C.elim_coef[k] * ck;
      rec[KN_CSLOT(k)] = ck;
    }
    rec[KN_CSLOT(KS)] = el;
  }
  if (i < D.NQtot) D.phiM[i] = D.VR[(size_t)D.q2i[i] * KN_REC + 7] - D.VR[(size_t)D.q2e[i] * KN_REC + 7];
}

// Forward-halo pack / unpack (owner -> ghost copies of dof fields between GPUs).
__global__ void halo_kernel(KnDev D, int kind, int pack, const int* __restrict__ idx, int n, int n_slots,
                            double* __restrict__ buf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int g = idx[i];
  if (kind == 0) {   // record slots 3..7: every concentration (K <= 4) and phi
    double* rec = D.VR + (size_t)g * KN_REC + 3;
    double* b = buf + (size_t)i * 5;
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      if (pack) b[c] = rec[c];
      else rec[c] = b[c];
    }
  } else {
    const int w = 1 + KN_MAXK * n_slots;
    double* b = buf + (size_t)i * w;
    if (pack) b[0] = D.phiM[g];
    else D.phiM[g] = b[0];
    for (int c = 0; c < KN_MAXK * n_slots; ++c) {
      double* f = D.Ich + (size_t)c * D.NQtot + g;
      if (pack) b[1 + c] = *f;
      else *f = b[1 + c];
    }
  }
}

// Membrane Robin term of b_emi alone (emiWeakForm.py:228-239), for the runs that assemble the EMI
// matrix beside the ODE sweep: one thread per membrane row, same arithmetic and entry order as the
// row kernels, so b_emi is bit-identical to the fused path.
template <int NF, int LPR>
__global__ __launch_bounds__(256) void emi_membrane_rhs_kernel(KnDev D, const KnConsts* __restrict__ Cp, int splitting) {
  const KnConsts& C = *Cp;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int mm = t / LPR, sub = t % LPR;
  const bool live = mm < D.M;                  // lanes past the last row repeat it: the shuffles see whole groups
  const int m = live ? mm : D.M - 1;
  const int g = D.mrow[m];
  const bool cell_side = g >= C.voff[1];
  double gam = 0.0;
  for (int e = D.mptr[m] + sub; e < D.mptr[m + 1]; e += LPR) {
    const int ms = D.me_model[e];
    if (ms < 0) continue;
    gam += (cell_side ? 1.0 : -1.0) * C.C_phi * emi_membrane_entry_rhs<NF>(D, C, e, ms, splitting);
  }
#pragma unroll
  for (int k = 1; k < LPR; k <<= 1) gam += __shfl_xor(gam, k);
  if (live && sub == 0) D.b_emi[g] = D.b_emi[g] + gam;
}

// dynamic LDS of the membrane-facet kernels: per point of the degree-6 rule the weight and the NF shape values, on
// quadrilateral facets the two tangent derivatives of the shape functions as well
size_t membrane_quad_lds(const knpemi_handle* h) {
  const int NF = h->NF;
  return (size_t)h->dev.nq_gamma * (1 + NF + (NF == 4 ? 2 * NF : 0)) * sizeof(double);
}

// A launch of a membrane kernel, which are built for NF = 2..4 vertices per facet: f(integral_constant<NF>) launches, the
// check follows.  (Any other NF is unreachable with a handle knpemi_create made, and an error, not some default.)
template <class F>
int launch_nf(const knpemi_handle* h, const char* name, F&& f) {
  if (!kn_pick<2, 3, 4>(h->NF, f))
    return kn_fail(KNPEMI_EINVAL, std::string(name) + ": not built for " + std::to_string(h->NF) + " vertices per facet");
  return kn_launch_check(name);
}

// One row launch of `system`, whatever the kernel: the 160 KiB refusal, the record of the LDS bytes, then `pick`, which
// finds the instantiation for the handle (nested kn_pick under the kernel's ..._built predicate) and hands its name, the
// kernel (as a RowKernel<...>) and the arguments behind (D, consts) to `go` -- the raised dynamic-LDS limit, the profile bracket, the launch on
// h->cur; no call of `go`: nothing is built for the handle, refused by name.  Last the launch check.  mem: knp_rows' MEM.
inline const char* kn_cell_kind_name(int kind) {
  switch (kind) {
    case KNPEMI_TRIANGLE: return "triangles";
    case KNPEMI_TETRAHEDRON: return "tetrahedra";
    case KNPEMI_HEXAHEDRON: return "hexahedra";
    case KNPEMI_QUADRILATERAL: return "quadrilaterals";
  }
  return "unknown cells";
}
template <auto KERNEL> struct RowKernel { static constexpr auto value = KERNEL; };
template <class Pick>
int launch_rows(knpemi_handle* h, int system, const KnRowShape& s, int mem, Pick&& pick) {
  const bool knp = system == KN_ROWS_KNP;
  if (s.lds > 160 * 1024)
    return kn_fail(KNPEMI_EINVAL, std::string(knp ? "KNP" : "EMI") + " row block does not fit in 160 KiB of LDS");
  (knp ? h->lds_bytes_knp : h->lds_bytes_emi) = s.lds;
  int rc = KNPEMI_OK;
  const char* name = nullptr;
  pick([&](const char* kernel_name, auto k, auto... args) {
    constexpr auto kernel = decltype(k)::value;   // a constant, not a pointer handed down: the launch calls its stub directly
    name = kernel_name;
    if ((rc = kn_set_lds_limit(reinterpret_cast<const void*>(kernel), s.lds))) return;
    KnProfScope prof(h->prof, knp ? KNPEMI_K_KNP_ROWS : KNPEMI_K_EMI_ROWS, h->cur);
    hipLaunchKernelGGL(kernel, dim3(h->dev.nblocks), dim3(KN_BLOCK), s.lds, h->cur, h->dev, h->d_consts, args...);
  });
  if (!name) {
    static const char* const path[] = {"default", "fused (KNPEMI_OPT_FUSE_MEMBRANE)", "early (KNPEMI_MEMBRANE_EARLY)"};
    return kn_fail(KNPEMI_EINVAL,
                   std::string(knp ? "knp_rows: unsupported lanes-per-row / ion-count / membrane-option combination: "
                                   : "emi_rows: bad lanes-per-row: ") +
                       std::to_string(h->lpr) + " lanes per row, " + std::to_string(h->K - 1) + " solved ion(s), " +
                       path[mem] + " membrane path, " + kn_cell_kind_name(h->cell_kind));
  }
  return rc ? rc : kn_launch_check(name);
}

}  // namespace

KnRowShape kn_rows_shape(const knpemi_handle* h, int system) {
  const bool knp = system == KN_ROWS_KNP;
  const size_t S = knp ? h->K - 1 : 1;   // fields a row block solves for: accumulators, and values per staged record
  const bool hexa = h->cell_kind == KNPEMI_HEXAHEDRON, quad = h->cell_kind == KNPEMI_QUADRILATERAL;
  const bool lattice_tets = h->cell_kind == KNPEMI_TETRAHEDRON && h->tet_uniform && h->dev.tet_tab;
  KnRowShape s;
  s.acc_n = ((knp ? h->lds_doubles_knp : h->lds_doubles_emi) + 1) & ~1;
  s.rec_n = h->lds_uniq_max;
  s.gam_n = knp && h->fuse_membrane ? std::max(1, h->lds_gam_max) : 0;
  s.geo = hexa ? (h->hex_uniform ? 2 : (h->hex_affine ? 1 : 0)) : (quad ? (h->hex_affine ? 1 : 0) : (lattice_tets ? 2 : 0));
  // accumulators | staged records (without coordinates where the cells are a lattice's, with two on quadrilaterals) and a
  // double of padding | the shape table of the lattice tetrahedra | fused membrane integrals | the entries' 16-bit locations
  const size_t rec_w = s.geo == 2 ? S + 1 : (quad ? 3 + S : 4 + S);
  s.lds = (S * s.acc_n + rec_w * (size_t)s.rec_n + 1 + (lattice_tets ? KN_TET_TAB : 0) +
           S * s.gam_n) * sizeof(double) + 2 * (size_t)h->lds_doubles_knp + 16;
  return s;
}

int kn_launch_emi_rows(knpemi_handle* h, int flags) {
  if (h->dev.nblocks == 0) return KNPEMI_OK;
  const int want_p = (flags & KNPEMI_WANT_P) ? 1 : 0;
  const int split = ((flags & KNPEMI_NO_SPLITTING) ? 0 : 1) | ((flags & KNPEMI_SKIP_MEMBRANE_RHS) ? 2 : 0);
  const KnRowShape s = kn_rows_shape(h, KN_ROWS_EMI);
  // cell kind (simplices of dimension NV - 1, hexahedra, quadrilaterals) x lanes per row x geometry variant
  const int rc = launch_rows(h, KN_ROWS_EMI, s, 0, [&](auto go) {
    kn_pick<KNPEMI_TRIANGLE, KNPEMI_TETRAHEDRON, KNPEMI_HEXAHEDRON, KNPEMI_QUADRILATERAL>(h->cell_kind, [&](auto kind) {
      kn_pick<1, 2, 4, 8>(h->lpr, [&](auto l) { kn_pick<0, 1, 2>(s.geo, [&](auto geo) {
      constexpr int KIND = decltype(kind)::value, NV = kind_nv(KIND), L = decltype(l)::value, GEO = decltype(geo)::value;
      if constexpr (KIND == KNPEMI_HEXAHEDRON && emi_rows_built(L))
        go("emi_rows_hex_v2", RowKernel<emi_rows_hex_v2<L, GEO>>{}, s.acc_n, s.rec_n, want_p, split, h->hex_geo);
      else if constexpr (kind_simplex(KIND) && emi_rows_built(L) && simplex_geo_built(NV - 1, GEO))
        go("emi_rows_v2", RowKernel<emi_rows_v2<NV - 1, L, GEO == 2>>{}, s.acc_n, s.rec_n, want_p, split);
      else if constexpr (KIND == KNPEMI_QUADRILATERAL && rows_quad_built(L, 0, 0, GEO))
        go("emi_rows_quad_v2", RowKernel<emi_rows_quad_v2<L, GEO>>{}, s.acc_n, s.rec_n, want_p, split);
    }); }); });
  });
#ifdef KN_ROW_STAMPS
  static int launches = 0;
  if (h->cell_kind == KNPEMI_TRIANGLE || h->cell_kind == KNPEMI_TETRAHEDRON)
    kn_stamps_report(&row_stamp_acc, 8, 5, 16, ++launches, h->dev.nblocks, "[row stamps]", "emi_rows_v2", "cycles", "workgroup");
#endif
  return rc;
}

int kn_launch_knp_rows(knpemi_handle* h, int flags) {
  if (h->dev.nblocks == 0) return KNPEMI_OK;
  const int split = (flags & KNPEMI_NO_SPLITTING) ? 0 : 1;
  const KnRowShape s = kn_rows_shape(h, KN_ROWS_KNP);
  // the membrane integrals of b_knp: from knp_membrane_pre_kernel (2), evaluated in the row block (1), from gam_e (0)
  const int mem = (flags & KNPEMI_MEMBRANE_EARLY) ? 2 : (s.gam_n > 0 ? 1 : 0);
  return launch_rows(h, KN_ROWS_KNP, s, mem, [&](auto go) {
    kn_pick<KNPEMI_TRIANGLE, KNPEMI_TETRAHEDRON, KNPEMI_HEXAHEDRON, KNPEMI_QUADRILATERAL>(h->cell_kind, [&](auto kind) {
      kn_pick<1, 2, 4, 8>(h->lpr, [&](auto l) { kn_pick<0, 1, 2>(s.geo, [&](auto geo) {
      kn_pick<1, 2, 3>(h->K - 1, [&](auto ks) { kn_pick<0, 1, 2>(mem, [&](auto m) {
        constexpr int KIND = decltype(kind)::value, NV = kind_nv(KIND), L = decltype(l)::value, GEO = decltype(geo)::value;
        constexpr int KS = decltype(ks)::value, MEM = decltype(m)::value;
        if constexpr (KIND == KNPEMI_HEXAHEDRON && knp_rows_hex_built(L, KS, MEM))
          go("knp_rows_hex_v2", RowKernel<knp_rows_hex_v2<L, GEO, KS, MEM>>{}, s.acc_n, s.rec_n, s.gam_n, split, h->hex_geo);
        else if constexpr (kind_simplex(KIND) && knp_rows_built(L, KS, MEM) && simplex_geo_built(NV - 1, GEO))
          go("knp_rows_v2", RowKernel<knp_rows_v2<NV - 1, L, KS, MEM, GEO == 2>>{}, s.acc_n, s.rec_n, s.gam_n, split);
        else if constexpr (KIND == KNPEMI_QUADRILATERAL && rows_quad_built(L, KS, MEM, GEO))
          go("knp_rows_quad_v2", RowKernel<knp_rows_quad_v2<L, GEO, KS, MEM>>{}, s.acc_n, s.rec_n, s.gam_n, split);
      }); });
    }); }); });
  });
}

int kn_launch_membrane_mass(knpemi_handle* h, int n_entries, const int* d_entry_row, double* d_out) {
  if (n_entries == 0) return KNPEMI_OK;
  const KnDev& D = h->dev;
  dim3 grid((n_entries + 255) / 256), block(256);
  const int v_cells = h->voff[1];
  return launch_nf(h, "membrane_mass_kernel", [&](auto nf) {
    hipLaunchKernelGGL(membrane_mass_kernel<decltype(nf)::value>, grid, block, 0, h->stream, D, n_entries, v_cells, d_entry_row, d_out);
  });
}

int kn_launch_knp_membrane(knpemi_handle* h, int flags) {
  const KnDev& D = h->dev;
  if (D.nftot == 0) return KNPEMI_OK;
  const int split = (flags & KNPEMI_NO_SPLITTING) ? 0 : 1;
  const size_t lds = membrane_quad_lds(h);
  dim3 grid((2 * (size_t)D.nftot * KN_MEM_LQ + 255) / 256), block(256);
  KnProfScope prof(h->prof, KNPEMI_K_KNP_MEMBRANE, h->cur);
  return launch_nf(h, "knp_membrane_kernel", [&](auto nf) {
    hipLaunchKernelGGL(knp_membrane_kernel<decltype(nf)::value>, grid, block, lds, h->cur, D, h->d_consts, split);
  });
}

// phi <- x - mean and the membrane-facet integrals of b_knp for that potential, one launch (see the kernel).  np = 0: x is
// written as it is.  The caller records the integrals in gam_e as current (kn_gam_formed).
int kn_launch_emi_writeback_membrane(knpemi_handle* h, const double* x, const double* part, int np, double inv_n, double* mean_out) {
  const KnDev& D = h->dev;
  const int n = D.Ntot;
  if (n == 0) return KNPEMI_OK;
  const int split = (h->emi_flags & KNPEMI_NO_SPLITTING) ? 0 : 1;
  const size_t lds = membrane_quad_lds(h);
  const int nbm = (int)((2 * (size_t)D.nftot * KN_MEM_LQ + 255) / 256);
  const int nbv = std::max(1, std::min(1024, (n + 255) / 256));
  dim3 grid(nbm + nbv), block(256);
  KnProfScope prof(h->prof, KNPEMI_K_KNP_MEMBRANE, h->cur);
  return launch_nf(h, "emi_writeback_membrane_kernel", [&](auto nf) {
    hipLaunchKernelGGL(emi_writeback_membrane_kernel<decltype(nf)::value>, grid, block, lds, h->cur, D, h->d_consts, split, nbm,
                       x, n, part, np, inv_n, mean_out);
  });
}

int kn_launch_knp_membrane_pre(knpemi_handle* h, int flags) {
  const KnDev& D = h->dev;
  if (D.nftot == 0) return KNPEMI_OK;
  const int split = (flags & KNPEMI_NO_SPLITTING) ? 0 : 1;
  const size_t lds = membrane_quad_lds(h);
  dim3 grid((2 * D.nftot + 255) / 256), block(256);
  KnProfScope prof(h->prof, KNPEMI_K_KNP_MEMBRANE, h->cur);
  return launch_nf(h, "knp_membrane_pre_kernel", [&](auto nf) {
    hipLaunchKernelGGL(knp_membrane_pre_kernel<decltype(nf)::value>, grid, block, lds, h->cur, D, h->d_consts, split);
  });
}

int kn_launch_emi_membrane_rhs(knpemi_handle* h, int flags) {
  const KnDev& D = h->dev;
  if (D.M == 0) return KNPEMI_OK;
  const int split = (flags & KNPEMI_NO_SPLITTING) ? 0 : 1;
  const int lpr = h->lpr;      // the same lane groups as the row kernels, so that both forms produce the same bits
  dim3 grid(((size_t)D.M * lpr + 255) / 256), block(256);
  KnProfScope prof(h->prof, KNPEMI_K_EMI_MEMBRANE, h->cur);
  bool built = false;
  const int rc = launch_nf(h, "emi_membrane_rhs_kernel", [&](auto nf) {
    built = kn_pick<1, 2, 4, 8>(lpr, [&](auto l) {
      hipLaunchKernelGGL((emi_membrane_rhs_kernel<decltype(nf)::value, decltype(l)::value>), grid, block, 0, h->stream, D,
                         h->d_consts, split);
    });
  });
  if (rc == KNPEMI_OK && !built)
    return kn_fail(KNPEMI_EINVAL, "emi_membrane_rhs_kernel: not built for " + std::to_string(lpr) + " lanes per row");
  return rc;
}

int kn_launch_update_pde(knpemi_handle* h) {
  const KnDev& D = h->dev;
  const int n = std::max(D.Ntot, D.NQtot);
  if (n == 0) return KNPEMI_OK;
  KnProfScope prof(h->prof, KNPEMI_K_UPDATE, h->cur);
  hipLaunchKernelGGL(update_pde_kernel, dim3((n + 255) / 256), dim3(256), 0, h->cur, D, h->d_consts);
  return kn_launch_check("update_pde_kernel");
}

int kn_launch_knp_writeback_update(knpemi_handle* h, const double* x) {
  const KnDev& D = h->dev;
  const int n = std::max(D.Ntot, D.NQtot);
  if (n == 0) return KNPEMI_OK;
  KnProfScope prof(h->prof, KNPEMI_K_UPDATE, h->cur);
  hipLaunchKernelGGL(knp_writeback_update_kernel, dim3((n + 255) / 256), dim3(256), 0, h->cur, D, h->d_consts, x);
  return kn_launch_check("knp_writeback_update_kernel");
}

int kn_launch_halo(knpemi_handle* h, int kind, int pack, const int32_t* idx, int n, double* buf) {
  if (n == 0) return KNPEMI_OK;
  hipLaunchKernelGGL(halo_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->dev, kind, pack, idx, n,
                     h->moff[h->n_sub], buf);
  return kn_launch_check("halo_kernel");
}

int kn_launch_field_scatter(hipStream_t st, const double* src, double* dst, int n, int dst_stride) {
  if (n == 0) return KNPEMI_OK;
  hipLaunchKernelGGL(scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, st, src, dst, n, dst_stride);
  return kn_launch_check("scatter_kernel");
}

int kn_launch_field_gather(hipStream_t st, const double* src, int src_stride, double* dst, int n) {
  if (n == 0) return KNPEMI_OK;
  hipLaunchKernelGGL(gather_kernel, dim3((n + 255) / 256), dim3(256), 0, st, src, src_stride, dst, n);
  return kn_launch_check("gather_kernel");
}

int kn_launch_vec_index(hipStream_t st, double* vec, const int32_t* idx, int n, double* buf, int gather) {
  if (n == 0) return KNPEMI_OK;
  hipLaunchKernelGGL(vec_index_kernel, dim3((n + 255) / 256), dim3(256), 0, st, vec, idx, n, buf, gather);
  return kn_launch_check("vec_index_kernel");
}

int kn_launch_trace(knpemi_handle* h, const double* ue, const double* ui, int sub, double* qe, double* qi) {
  const int nq = h->n_q[sub];
  if (nq == 0) return KNPEMI_OK;
  hipLaunchKernelGGL(trace_kernel, dim3((nq + 255) / 256), dim3(256), 0, h->stream, ue, ui,
                     h->dev.q2e, h->dev.q2i, h->qoff[sub], nq, h->voff[sub], qe, qi);
  return kn_launch_check("trace_kernel");
}
