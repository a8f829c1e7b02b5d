// The row block of the simplex EMI kernel ("owner-computes rows") as a __device__ function, with
// the helpers it needs.  Two kernels call it: emi_rows_v2 (kernels_assemble.hip), one row block per workgroup, and the
// fused launch of kernels_sweep_emi.hip, whose workgroups behind the membrane sweep's are row blocks.  Device only;
// everything sits in an anonymous namespace, as it did in kernels_assemble.hip: every translation unit has its own copy.
#pragma once

#include "knpemi_internal.h"
#include "membrane_facet.h"   // kn_rcp

// The operators leave the row kernels as streaming stores: they are read next by another kernel and would only push the vertex
// records, which neighbouring row blocks re-read, out of the L2 (round 4, A/B on one box: 2-4 % per row kernel at 995 k tets and
// on the 166 k-hexahedron mesh).
#define KN_ROW_STORE(v, p) __builtin_nontemporal_store((v), (p))
// (the pair entries are also read once per kernel, but loading them non-temporally costs 3-10 %: measured, not kept)

#define KN_PREFETCH 8   // pair entries per lane fetched ahead into registers

namespace {

__device__ __forceinline__ int logical_block(int bid, int nb) {
  // Workgroups are dealt round-robin over the 8 XCDs; give each XCD one contiguous chunk of row
  // blocks so neighbouring rows (which share vertices and cells) meet in the same L2.
  const int q = nb >> 3, r = nb & 7, xcd = bid & 7, idx = bid >> 3;
  return xcd * q + (xcd < r ? xcd : r) + idx;
}

// ---------------------------------------------------------------------------------------------
// Membrane part of an EMI row: coupling C_phi (u_i - u_e)(v_i - v_e) and Robin RHS
// (emiWeakForm.py:160-165,228-239).  Everything static about the (row, facet) entries e0 .. e0 + ne - 1 was
// flattened at set-up -- model slot, the facet-mass row (computed once on the device by
// `membrane_mass_kernel`, same `facet_mass_row` as before), the Q dofs and the byte-packed CSR slots -- so the
// row needs one level of loads for the matrix and one more (phi_M) for the right-hand side, instead of the
// former chain row -> list pointer -> entry -> facet -> vertex ids -> vertex records.
// ---------------------------------------------------------------------------------------------
template <int NF>
__device__ __forceinline__ double emi_membrane_entry_rhs(const KnDev& D, const KnConsts& C, int e, int ms, int splitting) {
  double gs = 0.0;
#pragma unroll
  for (int bb = 0; bb < NF; ++bb) {
    const int q = D.me_q[(size_t)e * NF + bb];
    double gq = D.phiM[q];
    if (!(splitting & 1)) {
      double it = 0.0;
      for (int k = 0; k < C.K; ++k) it += D.Ich[((size_t)ms * KN_MAXK + k) * D.NQtot + q];
      gq -= it / C.C_phi;
    }
    gs += D.me_mass[(size_t)e * NF + bb] * gq;
  }
  return gs;
}

template <int NF>
__device__ __forceinline__ void emi_membrane_row(const KnDev& D, const KnConsts& C, int e0, int ne, int first, int stride,
                                                 bool cell_side, int rowbase, double* accA, int splitting, double& gam) {
  // the lanes of a row share its membrane entries: lane `first` of `stride` takes every stride-th one; the partial
  // Robin sums meet in the caller's shuffle reduction (emi_membrane_rhs_kernel forms the same partial sums)
  for (int e = e0 + first; e < e0 + ne; e += stride) {
    const int ms = D.me_model[e];
    if (ms < 0) continue;
    const uint64_t sl = D.mslots[e];
#pragma unroll
    for (int bb = 0; bb < NF; ++bb) {
      const double val = C.C_phi * D.me_mass[(size_t)e * NF + bb];
      const int io = rowbase + (int)((sl >> (8 * bb)) & 255);
      const int it2 = rowbase + (int)((sl >> (8 * (4 + bb))) & 255);
      unsafeAtomicAdd(&accA[io], val);
      unsafeAtomicAdd(&accA[it2], -val);
    }
    if (!(splitting & 2))
      gam += (cell_side ? 1.0 : -1.0) * C.C_phi * emi_membrane_entry_rhs<NF>(D, C, e, ms, splitting);
  }
}

// the 16-byte staged EMI record (kappa, sigma) of the meshes whose geometry is a constant: lattice tetrahedra here, uniform
// hexahedra in kernels_assemble.hip (see RecU there)
struct Rec2 { double k, s; };
__device__ __forceinline__ Rec2 lds_rec2(const double* recs, int i) {
  const double2 u = *reinterpret_cast<const double2*>(recs + (size_t)i * 2);
  return Rec2{u.x, u.y};
}

template <int GDIM, class R>
__device__ __forceinline__ double simplex_row0(const R (&r)[GDIM + 1], double (&d)[GDIM + 1]) {
  // gradient dot products of lambda_0 with all lambda_j, and the cell measure
  if constexpr (GDIM == 2) {
    const double e1x = r[1].x - r[0].x, e1y = r[1].y - r[0].y;
    const double e2x = r[2].x - r[0].x, e2y = r[2].y - r[0].y;
    const double det = e1x * e2y - e1y * e2x, inv = kn_rcp(det);
    const double g1x = e2y * inv, g1y = -e2x * inv;
    const double g2x = -e1y * inv, g2y = e1x * inv;
    const double g0x = -(g1x + g2x), g0y = -(g1y + g2y);
    d[0] = g0x * g0x + g0y * g0y;
    d[1] = g0x * g1x + g0y * g1y;
    d[2] = g0x * g2x + g0y * g2y;
    return 0.5 * fabs(det);
  } else {
    const double ax = r[1].x - r[0].x, ay = r[1].y - r[0].y, az = r[1].z - r[0].z;
    const double bx = r[2].x - r[0].x, by = r[2].y - r[0].y, bz = r[2].z - r[0].z;
    const double cx = r[3].x - r[0].x, cy = r[3].y - r[0].y, cz = r[3].z - r[0].z;
    double g1x = by * cz - bz * cy, g1y = bz * cx - bx * cz, g1z = bx * cy - by * cx;
    double g2x = cy * az - cz * ay, g2y = cz * ax - cx * az, g2z = cx * ay - cy * ax;
    double g3x = ay * bz - az * by, g3y = az * bx - ax * bz, g3z = ax * by - ay * bx;
    const double det = ax * g1x + ay * g1y + az * g1z, inv = kn_rcp(det);
    g1x *= inv; g1y *= inv; g1z *= inv;
    g2x *= inv; g2y *= inv; g2z *= inv;
    g3x *= inv; g3y *= inv; g3z *= inv;
    const double g0x = -(g1x + g2x + g3x), g0y = -(g1y + g2y + g3y), g0z = -(g1z + g2z + g3z);
    d[0] = g0x * g0x + g0y * g0y + g0z * g0z;
    d[1] = g0x * g1x + g0y * g1y + g0z * g1z;
    d[2] = g0x * g2x + g0y * g2y + g0z * g2z;
    d[3] = g0x * g3x + g0y * g3y + g0z * g3z;
    return fabs(det) * (1.0 / 6.0);
  }
}


// Block descriptor (uniform) and the staging of the block's Laplacian-entry records: all index loads
// are issued together, then all record loads, so a wave waits for memory twice instead of 2 x trips.
struct BlkInfo {
  int row0, nrows, sub, seg0, seglen, segL0, nnzLb, uoff, nuniq, slbase, np, me0, mne;
};

__device__ __forceinline__ BlkInfo load_blk(const KnDev& D, int b, int wave) {
  const int4* p = D.blk_info + 4 * (size_t)b;
  const int4 i0 = p[0], i1 = p[1], i2 = p[2], i3 = p[3];
  BlkInfo B;
  B.row0 = i0.x; B.nrows = i0.y; B.sub = i0.z; B.seg0 = i0.w;
  B.seglen = i1.x; B.segL0 = i1.y; B.nnzLb = i1.z; B.uoff = i1.w;
  B.slbase = wave == 0 ? i2.x : (wave == 1 ? i2.y : (wave == 2 ? i2.z : i2.w));
  B.np = ((unsigned)i3.x >> (8 * wave)) & 255;
  B.nuniq = i3.y;
  B.me0 = i3.z; B.mne = i3.w;      // membrane entries of the block's rows: [me0, me0 + mne)
  return B;
}

// Rows of a block: KN_BLOCK / LPR / KN_CHUNK chunks of (up to) KN_CHUNK consecutive rows each (KN_CHUNK_SIMPLEX or
// KN_CHUNK_HEX; D.blk_rng, six ints per
// chunk: first row, rows, end of the chunk's entries in the block's concatenated EMI segment, global EMI position minus
// concatenated position, the same two for the Laplacian pattern).  A block of consecutive rows is the special case of
// consecutive chunks; clustered chunks (knpemi_create) touch fewer distinct vertices.
template <int LPR, int KN_CHUNK>
struct BlkRows {
  static constexpr int NR = KN_BLOCK / LPR / KN_CHUNK;
  const int* rng;
  __device__ __forceinline__ BlkRows(const KnDev& D, int b) : rng(D.blk_rng + (size_t)b * (6 * NR)) {}
  // global row of block-local row rloc (valid = false: a lane without a row; it takes the block's first row)
  __device__ __forceinline__ int row(int rloc, bool& valid) const {
    const int2 c = *reinterpret_cast<const int2*>(rng + 6 * (rloc / KN_CHUNK));
    valid = (rloc % KN_CHUNK) < c.y;
    return valid ? c.x + (rloc % KN_CHUNK) : rng[0];
  }
  // f(i, global CSR position) for every position i of the block's concatenated segment (which = 0: EMI pattern,
  // 1: Laplacian pattern), two chunks per pass: bounds and offsets are wave-uniform, the stores of a pass cover two
  // contiguous pieces of the global array
  template <class F>
  __device__ __forceinline__ void for_each_entry(int tid, int which, F&& f) const {
    static_assert(NR % 2 == 0, "chunks are walked in pairs");
    int lo = 0;
#pragma unroll
    for (int r = 0; r < NR; r += 2) {
      const int mid = rng[6 * r + 2 + 2 * which], hi = rng[6 * (r + 1) + 2 + 2 * which];
      const int d0 = rng[6 * r + 3 + 2 * which], d1 = rng[6 * (r + 1) + 3 + 2 * which];
      for (int i = lo + tid; i < hi; i += KN_BLOCK) f(i, (int64_t)i + (i >= mid ? d1 : d0));
      lo = hi;
    }
  }
};

#define KN_STAGE 3   // distinct vertices per thread staged with batched loads (256 threads x 3 = 768)

// Phase A of the v2 kernels: the 48-byte records of the block's distinct vertices go to `recs`, the
// 2-byte local index of every Laplacian entry to `eloc`.
// EMI records are 5 doubles: x y z | kappa = sum_k kap_k c_k | sigma = sum_k sig_k c_k (the two combinations of
// the concentrations the forms need; every staged vertex belongs to the block's sub-domain, so its constants
// apply).  KNP records are 6: x y z | f0 f1 | phi.
struct Rec5 { double x, y, z, k, s; };

__device__ __forceinline__ Rec5 lds_rec5(const double* recs, int i) {
  const double* p = recs + (size_t)i * 5;
  return Rec5{p[0], p[1], p[2], p[3], p[4]};
}

// one staged record from the 64-byte vertex record u (x y | z c3 | c0 c1 | c2 phi).  KS = 0: EMI (5 doubles),
// KS >= 1: KNP with KS solved ions (4 + KS doubles).  fs / nvs: ECS source term (NULL when unused), v the vertex.
// GD = 2 (quadrilaterals): the records without z -- EMI x y | kappa sigma (4 doubles), KNP x y f_0 .. f_{KS-1} phi (3 + KS).
template <int KS, bool UNI = false, int GD = 3>
__device__ __forceinline__ void write_staged(double* recs, int i, const double2 (&u)[4], double inv_dt, const double* fs0,
                                             int nvs, int v, const KnSubConst* scp) {
  if constexpr (GD == 2) {
    static_assert(!UNI, "2-D records carry their coordinates");
    if constexpr (KS == 0) {
      const double c0 = u[2].x, c1 = u[2].y, c2 = u[3].x, c3 = u[1].y;
      const double kap = scp->kap[0] * c0 + scp->kap[1] * c1 + scp->kap[2] * c2 + scp->kap[3] * c3;
      const double sig = scp->sig[0] * c0 + scp->sig[1] * c1 + scp->sig[2] * c2 + scp->sig[3] * c3;
      double2* dst = reinterpret_cast<double2*>(recs + (size_t)i * 4);
      dst[0] = double2{u[0].x, u[0].y}; dst[1] = double2{kap, sig};
    } else {
      const double cp[3] = {u[2].x, u[2].y, u[3].x};
      double* d = recs + (size_t)i * (3 + KS);
      d[0] = u[0].x; d[1] = u[0].y;
#pragma unroll
      for (int k = 0; k < KS; ++k) {
        double f = cp[k] * inv_dt;
        if (fs0) f += fs0[(size_t)k * nvs + v];
        d[2 + k] = f;
      }
      d[2 + KS] = u[3].y;
    }
  } else if constexpr (KS == 0) {
    const double c0 = u[2].x, c1 = u[2].y, c2 = u[3].x, c3 = u[1].y;   // ions beyond K have kap = sig = 0 (and c = 0)
    const double kap = scp->kap[0] * c0 + scp->kap[1] * c1 + scp->kap[2] * c2 + scp->kap[3] * c3;
    const double sig = scp->sig[0] * c0 + scp->sig[1] * c1 + scp->sig[2] * c2 + scp->sig[3] * c3;
    if constexpr (UNI) {
      *reinterpret_cast<double2*>(recs + (size_t)i * 2) = double2{kap, sig};
    } else {
      double* d5 = recs + (size_t)i * 5;
      d5[0] = u[0].x; d5[1] = u[0].y; d5[2] = u[1].x;
      d5[3] = kap;
      d5[4] = sig;
    }
  } else if constexpr (UNI) {
    const double cp[3] = {u[2].x, u[2].y, u[3].x};
    double* d = recs + (size_t)i * (KS + 1);
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      double f = cp[k] * inv_dt;
      if (fs0) f += fs0[(size_t)k * nvs + v];
      d[k] = f;
    }
    d[KS] = u[3].y;
  } else {
    const double cp[3] = {u[2].x, u[2].y, u[3].x};     // the solved ions live in slots 4..6
    double f[KS];
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      f[k] = cp[k] * inv_dt;                            // (1/dt) c_prev (+ f_source on the ECS)
      if (fs0) f[k] += fs0[(size_t)k * nvs + v];
    }
    if constexpr (KS == 2) {
      double2* dst = reinterpret_cast<double2*>(recs + (size_t)i * 6);
      dst[0] = u[0]; dst[1] = double2{u[1].x, f[0]}; dst[2] = double2{f[1], u[3].y};
    } else {
      double* d = recs + (size_t)i * (4 + KS);
      d[0] = u[0].x; d[1] = u[0].y; d[2] = u[1].x;
#pragma unroll
      for (int k = 0; k < KS; ++k) d[3 + k] = f[k];
      d[3 + KS] = u[3].y;
    }
  }
}

template <int KS, bool UNI = false, int GD = 3>
__device__ __forceinline__ void stage_records(const KnDev& D, const BlkInfo& B, double* recs, uint16_t* eloc, int tid,
                                              double inv_dt, const double* fs0, int nvs,
                                              const KnSubConst* scp = nullptr) {
  int vv[KN_STAGE];
#pragma unroll
  for (int k = 0; k < KN_STAGE; ++k) {
    const int i = tid + k * KN_BLOCK;
    vv[k] = i < B.nuniq ? D.blk_uverts[B.uoff + i] : -1;
  }
  for (int i = tid; i < B.nnzLb; i += KN_BLOCK) eloc[i] = D.ent_loc[B.segL0 + i];
  double2 u[KN_STAGE][4];
#pragma unroll
  for (int k = 0; k < KN_STAGE; ++k)
    if (vv[k] >= 0) {
      const double2* src = reinterpret_cast<const double2*>(D.VR + (size_t)vv[k] * KN_REC);
      u[k][0] = src[0]; u[k][1] = src[1]; u[k][2] = src[2]; u[k][3] = src[3];   // x y | z c3 | c0 c1 | c2 phi
    }
#pragma unroll
  for (int k = 0; k < KN_STAGE; ++k)
    if (vv[k] >= 0) write_staged<KS, UNI, GD>(recs, tid + k * KN_BLOCK, u[k], inv_dt, fs0, nvs, vv[k], scp);
  for (int i = tid + KN_STAGE * KN_BLOCK; i < B.nuniq; i += KN_BLOCK) {   // oversized blocks only
    const int v = D.blk_uverts[B.uoff + i];
    const double2* src = reinterpret_cast<const double2*>(D.VR + (size_t)v * KN_REC);
    const double2 uu[4] = {src[0], src[1], src[2], src[3]};
    write_staged<KS, UNI, GD>(recs, i, uu, inv_dt, fs0, nvs, v, scp);
  }
}

// Lattice tetrahedra of a uniform grid (knpemi_create, KnDev::tet_tab): a cell is one of at most eight shapes whose gradient
// dot products and volume are constants of the mesh, so the row kernels stage no coordinates and do no geometry: the pair
// entry names the shape and the canonical number of each of its vertices, the 4 + 1 numbers come from a 136-double table in
// LDS.  KN_TET_TAB doubles: [shape][a][b] g_a . g_b, then [shape] |T|.
constexpr int KN_TET_TAB = 8 * 16 + 8;
template <int NV>
__device__ __forceinline__ double tet_table_row0(const double* tab, uint32_t sl, double (&d)[NV]) {
  static_assert(NV == 4, "lattice tetrahedra");
  const int shape = (sl >> 5) & 7;
  const int c1 = (sl >> 13) & 3, c2 = (sl >> 21) & 3, c3 = (sl >> 29) & 3, c0 = 6 - c1 - c2 - c3;
  const double* row = tab + (shape * 4 + c0) * 4;
  d[0] = row[c0]; d[1] = row[c1]; d[2] = row[c2]; d[3] = row[c3];
  return tab[128 + shape];
}

// Diagnostic build (make CXXFLAGS+=-DKN_ROW_STAMPS): emi_rows_v2 adds up s_memtime differences between its phases (first wave
// of every workgroup); the launcher prints the averages every 16 launches.
#ifdef KN_ROW_STAMPS
__device__ unsigned long long row_stamp_acc[1024 * 8];
#define ROW_STAMP_BEGIN unsigned long long row_t_ = __builtin_amdgcn_s_memtime();
#define ROW_STAMP(i) do { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); \
                          if (threadIdx.x == 0) atomicAdd(&row_stamp_acc[(blockIdx.x & 1023) * 8 + (i)], n_ - row_t_); row_t_ = n_; } while (0)
#else
#define ROW_STAMP_BEGIN
#define ROW_STAMP(i) do {} while (0)
#endif

// Row block `bid` of `D.nblocks` (the workgroup's index among the row blocks: blockIdx.x in emi_rows_v2, blockIdx.x minus
// the sweep's workgroups in the fused launch, so logical_block deals the blocks over the XCDs alike in both).
// UT: lattice tetrahedra of a uniform grid (tet_table_row0)
template <int GDIM, int LPR, bool UT>
__device__ __forceinline__ void emi_rows_block(const KnDev& D, const KnConsts& C, int acc_n, int rec_n, int want_p,
                                               int splitting, int bid) {
  constexpr int NV = GDIM + 1, NF = GDIM;
  extern __shared__ __align__(16) double lds[];
  constexpr int RD = UT ? 2 : 5;                       // doubles per staged record
  constexpr int SM = UT ? 31 : 255;                    // slot mask of a pair-entry byte (= the "no slot" value)
  using RecT = std::conditional_t<UT, Rec2, Rec5>;
  double* accA = lds;
  double* tab = lds + (size_t)acc_n;                   // UT: the shape table
  double* recs = tab + (UT ? KN_TET_TAB : 0);
  uint16_t* eloc = reinterpret_cast<uint16_t*>(recs + RD * (size_t)rec_n + ((RD * rec_n) & 1));
  const int tid = threadIdx.x;
  ROW_STAMP_BEGIN
  const int b = logical_block(bid, D.nblocks);
  const BlkInfo B = load_blk(D, b, tid >> 6);
  const int s = B.sub, seglen = B.seglen;
  // this lane's pair entries and row descriptor: issued first, their latency overlaps phase A
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
  // phase A: zero accumulators, stage the records of the block's Laplacian entries
  for (int i = tid; i < seglen; i += KN_BLOCK) accA[i] = 0.0;
  const KnSubConst& sc = C.sc[s];
  if constexpr (UT) { if (tid < KN_TET_TAB) tab[tid] = D.tet_tab[tid]; }
  stage_records<0, UT>(D, B, recs, eloc, tid, 0.0, nullptr, 0, &sc);
  ROW_STAMP(0);     // descriptors -> vertex ids -> records -> LDS
  __syncthreads();
  ROW_STAMP(1);     // barrier

  const bool cell_side = s > 0;
  double bacc = 0.0, gam = 0.0;   // volume part / membrane Robin part of b_emi
  if (valid) {
    const int rowbase = ri.x, lap = ri.y & 0xFFFF, ne = (unsigned)ri.y >> 16, rL = ri.z;
    // The diagonal entry receives a term from every pair: keep it in registers and add it once.
    int diag = -1;
    double dA = 0.0;
    RecT r[NV];
    auto rec = [&](int i) { if constexpr (UT) return lds_rec2(recs, i); else return lds_rec5(recs, i); };
    uint32_t have = 0xFFFFFFFFu;     // slots whose contributions pend[1..] currently hold (SM: none)
    double pend[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) pend[j] = 0.0;
    auto do_pair = [&](uint32_t sl) {
      int slot[NV];
#pragma unroll
      for (int j = 0; j < NV; ++j) slot[j] = (sl >> (8 * j)) & SM;
      if (diag < 0) { diag = slot[0]; r[0] = rec(eloc[rL + diag]); }   // the row's own vertex, once
      // (The host orders a lane's pairs in strips that share all but one vertex; knp_rows_v2 keeps the shared records
      // in registers.  Here that costs the fifth block per CU -- 104 instead of 84 registers -- and the LDS pipe is
      // less loaded, 36 % against 51 %: measured 49.4 against 47.7 us at 995 k tets, so every record is read again.)
#pragma unroll
      for (int j = 1; j < NV; ++j) r[j] = rec(eloc[rL + slot[j]]);
      double d[NV];
      double vol;
      if constexpr (UT) vol = tet_table_row0<NV>(tab, sl, d);
      else vol = simplex_row0<GDIM>(r, d);
      double ksum = 0, sd = 0;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        ksum += r[j].k;
        sd += r[j].s * d[j];
      }
      const double kbar = ksum * (1.0 / NV);
      bacc -= vol * sd;
      dA += vol * kbar * d[0];
      // Off-diagonal entries: in the strip order a vertex keeps its position over consecutive pairs, so its
      // contributions are summed in a register and go to LDS when another vertex takes the position.
#pragma unroll
      for (int j = 1; j < NV; ++j) {
        const int hs = (int)((have >> (8 * j)) & SM);
        if (slot[j] != hs) {
          if (hs != SM) unsafeAtomicAdd(&accA[lap + hs], pend[j]);
          pend[j] = 0.0;
        }
        pend[j] += vol * kbar * d[j];
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
      if (hs != SM) unsafeAtomicAdd(&accA[lap + hs], pend[j]);
    }
    if (diag >= 0) unsafeAtomicAdd(&accA[lap + diag], dA);
    if (ne > 0) emi_membrane_row<NF>(D, C, ri.w, ne, sub, LPR, cell_side, rowbase, accA, splitting, gam);
  }
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) { bacc += __shfl_xor(bacc, m); gam += __shfl_xor(gam, m); }
  if (valid && sub == 0) D.b_emi[g] = bacc + gam;
  ROW_STAMP(2);     // pair loop
  __syncthreads();
  ROW_STAMP(3);     // barrier
  rows.for_each_entry(tid, 0, [&](int i, int64_t gp) {
    const double a = accA[i];
    KN_ROW_STORE(a, &D.A_emi[gp]);
    if (want_p) KN_ROW_STORE(cell_side ? a + D.P_mass[gp - D.pmass0] : a, &D.P_emi[gp]);
  });
  ROW_STAMP(4);     // write-out issued
}

}  // namespace
