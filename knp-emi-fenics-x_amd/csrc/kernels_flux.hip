// Ion fluxes and current density per cell on gfx950: fields and their series row in ONE launch per record.
//
// The reference writes these quantities in its manufactured-solution scripts only (tests/run_mms.py:270-301:
// J_k = -D_k grad c_k - z_k D_k psi c_k grad phi, total flux F sum_k z_k J_k); a user of its drivers who wants a flux
// downloads every field at every step and differentiates on the host.  Here one lane takes one cell of a watched
// sub-domain, gathers the cell's 64-byte vertex records (the data the row kernels read, in the layout they read it in)
// with 16-byte loads, and evaluates, for every ion k = 0 .. K-1 (the eliminated one included),
//   c_k, g(u)   value and gradient, at the cell's centroid, of the P1 / Q1 interpolant of the nodal field
//               (simplices: mean of the vertex values, constant gradient; hexahedra, tensor vertex order: mean of the
//               eight values, reference derivative along t = 1/4 sum_v +-u_v with the sign from bit t of v, mapped by
//               the Jacobian at the centre; quadrilaterals, the same in 2-D: mean of the four values, reference
//               derivative 1/2 sum_v +-u_v)
//   J_diff  = -D_k^s g(c_k)
//   J_drift = -z_k psi D_k^s c_k g(phi)          J = J_diff + J_drift
//   i       = F sum_k z_k J_k, split the same way into i_diff and i_drift
//   vol_T   = |det| / d! on simplices, |det J(centre)| on hexahedra and quadrilaterals (midpoint rule): the sign of det
//             cancels, so left-handed cells give the same answer
// from phi (slot 7) and c_prev / the eliminated ion's c (KN_CSLOT) as the records hold them: behind the end-of-step
// update that is the new state.  The coordinates come from the same records, so lattice tetrahedra and uniform
// hexahedra take no path of their own.
//
// Geometry, the same for the four cell kinds: with edge vectors E_t (simplices: x_t+1 - x_0; hexahedra and
// quadrilaterals: the columns of the Jacobian at the centre) and the differences d_t of a field along them (u_t+1 - u_0; the reference
// derivatives), g = (sum_t d_t cof_t) / det, cof_0 = E_1 x E_2 and cyclic, det = E_0 . cof_0.  A hexahedron
// accumulates the sum and the three signed face sums of all eight slots of the record as the records stream by (32
// doubles); it never holds eight records.
//
// With write_fields the vectors go to structure-of-arrays buffers [component][cell] through non-temporal stores:
// consecutive lanes write consecutive doubles, and nothing of it is read again by the device.
//
// Series row (KnWatchTab): per watched (sub-domain, ion) sum_T vol_T J_diff, sum_T vol_T J_drift (gdim values each) and
// max_T |J|; per watched sub-domain with the current sum_T vol_T i and max_T |i|.  The reduction is a fixed tree inside
// the workgroup (xor butterfly over the 64 lanes of a wave, then the four waves in order), one partial of KN_FLUX_SLOTS
// doubles per workgroup, and the tail of record_tail.h: the last workgroup to arrive folds the partials of every
// column in workgroup order and appends the row, or counts it as dropped when the buffer is full.
//
// Partitioned runs (knpemi_flux_set_partitioned; PART): a rank's cells include its ghost layer, whose records are valid
// after the bulk halo.  One byte per cell says whether this rank records it: a cell that is not recorded gets its fields
// written like any other and enters no sum (vol = 0, as a lane past the last cell) and no maximum.  The byte of lane t
// sits next to that of lane t + 1, a coalesced load beside the cell's vertex ids.  The last workgroup writes the folded
// columns into this rank's slots of the exchange buffer and leaves the row counters alone: the caller sums the buffer
// over the ranks and record_combine_kernel (kernels_observe.hip) appends the row.  PART is a template flag: the
// single-rank instantiations are the code they were without it.
#include <cmath>

#include "knpemi_internal.h"
#include "record_tail.h"

#define FLUX_THREADS KN_FLUX_CHUNK      // one lane per cell
#define FLUX_WAVES (FLUX_THREADS / 64)
// loads the fold of the partials has in flight (kn_fold_column): the largest depth that leaves the allocation of every
// instantiation where its body puts it -- 13 raises the triangles' from 68 to 70 VGPRs, 14 takes one of their 7 waves
// per SIMD, 16 two
#define FLUX_FOLD_DEPTH 12

namespace {

struct FluxArgs {
  int K, capacity;
  const KnWatchTab* tab;
  const KnConsts* consts;
  const int* cells;
  const double* VR;
  double* part;
  unsigned long long* ctl;
  double* rows;
  double* fld;
  const uint8_t* recorded;   // PART: [cells of every watch] 1 = this rank records the cell
  double* slot;              // PART: this rank's n_cols slots of the exchange buffer
};

template <int KIND> struct FluxCell {
  static constexpr int GD = KIND == KNPEMI_TRIANGLE || KIND == KNPEMI_QUADRILATERAL ? 2 : 3;
  static constexpr int NV = KIND == KNPEMI_TRIANGLE ? 3 : KIND == KNPEMI_HEXAHEDRON ? 8 : 4;
  static constexpr bool TENSOR = KIND == KNPEMI_HEXAHEDRON || KIND == KNPEMI_QUADRILATERAL;
  // |det| -> cell measure: 1 on the tensor cells (midpoint rule), 1 / d! on simplices
  static constexpr double VOL = TENSOR ? 1.0 : (KIND == KNPEMI_TETRAHEDRON ? 1.0 / 6.0 : 0.5);
};

// the five fields of a record in the order phi, c_0 .. c_3 (KN_CSLOT)
struct FluxRec { double x[3]; double u[5]; };
__device__ inline FluxRec load_record(const double* __restrict__ VR, int v) {
  const double2* p = reinterpret_cast<const double2*>(VR + (size_t)v * KN_REC);
  const double2 a = p[0], b = p[1], c = p[2], d = p[3];
  return FluxRec{{a.x, a.y, b.x}, {d.y, c.x, c.y, d.x, b.y}};
}

// edge vectors E[t][a], field differences d[f][t] along them and centroid values m[f] of one cell
template <int KIND>
__device__ inline void gather_cell(const int* __restrict__ cells, const double* __restrict__ VR, size_t cell,
                                   double (&E)[FluxCell<KIND>::GD][FluxCell<KIND>::GD],
                                   double (&d)[5][FluxCell<KIND>::GD], double (&m)[5]) {
  constexpr int GD = FluxCell<KIND>::GD, NV = FluxCell<KIND>::NV;
  int v[NV];
  if constexpr (NV == 3) {
    for (int i = 0; i < 3; ++i) v[i] = cells[cell * 3 + i];
  } else {
    const int4* p = reinterpret_cast<const int4*>(cells + cell * NV);
#pragma unroll
    for (int i = 0; i < NV / 4; ++i) {
      const int4 q = p[i];
      v[4 * i] = q.x; v[4 * i + 1] = q.y; v[4 * i + 2] = q.z; v[4 * i + 3] = q.w;
    }
  }
  if constexpr (KIND == KNPEMI_QUADRILATERAL) {
    double S[5] = {}, Dx[2][2] = {}, Du[5][2] = {};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const FluxRec r = load_record(VR, v[i]);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const bool up = (i >> t) & 1;
#pragma unroll
        for (int a = 0; a < 2; ++a) Dx[t][a] += up ? r.x[a] : -r.x[a];
#pragma unroll
        for (int f = 0; f < 5; ++f) Du[f][t] += up ? r.u[f] : -r.u[f];
      }
#pragma unroll
      for (int f = 0; f < 5; ++f) S[f] += r.u[f];
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int a = 0; a < 2; ++a) E[t][a] = 0.5 * Dx[t][a];
#pragma unroll
      for (int f = 0; f < 5; ++f) d[f][t] = 0.5 * Du[f][t];
    }
#pragma unroll
    for (int f = 0; f < 5; ++f) m[f] = 0.25 * S[f];
  } else if constexpr (NV != 8) {
    const FluxRec r0 = load_record(VR, v[0]);
#pragma unroll
    for (int f = 0; f < 5; ++f) m[f] = r0.u[f];
#pragma unroll
    for (int t = 0; t < NV - 1; ++t) {
      const FluxRec r = load_record(VR, v[t + 1]);
#pragma unroll
      for (int a = 0; a < GD; ++a) E[t][a] = r.x[a] - r0.x[a];
#pragma unroll
      for (int f = 0; f < 5; ++f) { d[f][t] = r.u[f] - r0.u[f]; m[f] += r.u[f]; }
    }
#pragma unroll
    for (int f = 0; f < 5; ++f) m[f] *= 1.0 / NV;
  } else {
    double S[5] = {}, Dx[3][3] = {}, Du[5][3] = {};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const FluxRec r = load_record(VR, v[i]);
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const bool up = (i >> t) & 1;
#pragma unroll
        for (int a = 0; a < 3; ++a) Dx[t][a] += up ? r.x[a] : -r.x[a];
#pragma unroll
        for (int f = 0; f < 5; ++f) Du[f][t] += up ? r.u[f] : -r.u[f];
      }
#pragma unroll
      for (int f = 0; f < 5; ++f) S[f] += r.u[f];
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
#pragma unroll
      for (int a = 0; a < 3; ++a) E[t][a] = 0.25 * Dx[t][a];
#pragma unroll
      for (int f = 0; f < 5; ++f) d[f][t] = 0.25 * Du[f][t];
    }
#pragma unroll
    for (int f = 0; f < 5; ++f) m[f] = 0.125 * S[f];
  }
}

template <int KIND, bool FIELDS, bool PART>
__global__ __launch_bounds__(FLUX_THREADS) void flux_kernel(FluxArgs A) {
  constexpr int GD = FluxCell<KIND>::GD;
  constexpr int PER_ION = 2 * GD + 1;
  __shared__ double sh[FLUX_WAVES][KN_FLUX_SLOTS];
  __shared__ int last;
  __shared__ unsigned long long row;
  const KnWatchTab& T = *A.tab;
  const int K = A.K;
  int w = 0;
  while (w + 1 < T.n_watch && (int)blockIdx.x >= T.bstart[w + 1]) ++w;      // at most KN_MAXSUB - 1 steps, uniform
  const int s = T.sub[w], mask = T.mask[w], nc = T.count[w];
  const bool cur = (mask & KN_WATCH_CURRENT) != 0;
  const int lc = ((int)blockIdx.x - T.bstart[w]) * FLUX_THREADS + (int)threadIdx.x;
  const bool valid = lc < nc;
  // rec: the cell enters the sums and the maxima
  bool rec = valid;
  if constexpr (PART) rec = valid && A.recorded[(size_t)T.ibase[w] + lc] != 0;
  // a lane past the sub-domain's last cell repeats that cell (it takes part in the wave reductions) and contributes
  // nothing
  const size_t cell = (size_t)T.first[w] + (size_t)(valid ? lc : nc - 1);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (threadIdx.x < FLUX_WAVES * KN_FLUX_SLOTS) (&sh[0][0])[threadIdx.x] = 0.0;
  __syncthreads();

  double E[GD][GD], d[5][GD], m[5];
  gather_cell<KIND>(A.cells, A.VR, cell, E, d, m);
  double cof[GD][GD], det;
  if constexpr (GD == 2) {
    cof[0][0] = E[1][1]; cof[0][1] = -E[1][0];
    cof[1][0] = -E[0][1]; cof[1][1] = E[0][0];
    det = E[0][0] * E[1][1] - E[0][1] * E[1][0];
  } else {
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int p = (t + 1) % 3, q = (t + 2) % 3;
      cof[t][0] = E[p][1] * E[q][2] - E[p][2] * E[q][1];
      cof[t][1] = E[p][2] * E[q][0] - E[p][0] * E[q][2];
      cof[t][2] = E[p][0] * E[q][1] - E[p][1] * E[q][0];
    }
    det = E[0][0] * cof[0][0] + E[0][1] * cof[0][1] + E[0][2] * cof[0][2];
  }
  const double inv_det = 1.0 / det;
  const double vol = rec ? fabs(det) * FluxCell<KIND>::VOL : 0.0;
  auto grad = [&](int f, double (&g)[GD]) {
#pragma unroll
    for (int a = 0; a < GD; ++a) {
      double t = d[f][0] * cof[0][a];
#pragma unroll
      for (int e = 1; e < GD; ++e) t += d[f][e] * cof[e][a];
      g[a] = t * inv_det;
    }
  };
  double gphi[GD];
  grad(0, gphi);

  const KnSubConst& sc = A.consts->sc[s];
  double* __restrict__ fld = FIELDS ? A.fld + T.fbase[w] + lc : nullptr;      // this cell's place in component 0
  auto put = [&](int comp, double v) {
    if (FIELDS && valid) __builtin_nontemporal_store(v, fld + (size_t)comp * nc);
  };
  double i_diff[GD] = {}, i_drift[GD] = {};
  int comp = 0;
#pragma unroll
  for (int k = 0; k < KN_MAXK; ++k) {
    const bool sel = (mask >> k) & 1;
    if (!(sel || (cur && k < K))) continue;                 // uniform over the workgroup
    double g[GD], Jd[GD], Jr[GD];
    grad(1 + k, g);
    const double Dk = sc.D[k], zpD = sc.zpsiD[k] * m[1 + k], Fz = A.consts->F * A.consts->z[k];
    double n2 = 0.0;
#pragma unroll
    for (int a = 0; a < GD; ++a) {
      Jd[a] = -Dk * g[a];
      Jr[a] = -zpD * gphi[a];
      i_diff[a] += Fz * Jd[a];
      i_drift[a] += Fz * Jr[a];
      const double J = Jd[a] + Jr[a];
      n2 += J * J;
    }
    if (!sel) continue;
#pragma unroll
    for (int a = 0; a < GD; ++a) {
      put(comp + a, Jd[a]);
      put(comp + GD + a, Jr[a]);
      const double sd = kn_wave_sum(vol * Jd[a]), sr = kn_wave_sum(vol * Jr[a]);
      if (lane == 0) { sh[wave][k * PER_ION + a] = sd; sh[wave][k * PER_ION + GD + a] = sr; }
    }
    comp += 2 * GD;
    const double mx = kn_wave_max(rec ? sqrt(n2) : 0.0);
    if (lane == 0) sh[wave][k * PER_ION + 2 * GD] = mx;
  }
  if (cur) {
    double n2 = 0.0;
#pragma unroll
    for (int a = 0; a < GD; ++a) {
      put(comp + a, i_diff[a]);
      put(comp + GD + a, i_drift[a]);
      const double i = i_diff[a] + i_drift[a];
      n2 += i * i;
      const double si = kn_wave_sum(vol * i);
      if (lane == 0) sh[wave][KN_MAXK * PER_ION + a] = si;
    }
    const double mx = kn_wave_max(rec ? sqrt(n2) : 0.0);
    if (lane == 0) sh[wave][KN_MAXK * PER_ION + GD] = mx;
  }
  __syncthreads();

  // the workgroup's partial: the four waves in order; slots nobody wrote stay 0 and no column reads them
  if (threadIdx.x < KN_FLUX_SLOTS) {
    const int j = threadIdx.x;
    const bool is_max = j < KN_MAXK * PER_ION ? j % PER_ION == 2 * GD : j == KN_MAXK * PER_ION + GD;
    double v = sh[0][j];
#pragma unroll
    for (int q = 1; q < FLUX_WAVES; ++q) v = is_max ? fmax(v, sh[q][j]) : v + sh[q][j];
    kn_part_store(&A.part[(size_t)blockIdx.x * KN_FLUX_SLOTS + j], v);
  }
  if (!kn_arrive_last(A.ctl, threadIdx.x < KN_FLUX_SLOTS, &last)) return;
  auto fold = [&](int q) {
    const int cw = T.col_watch[q];
    return kn_fold_column<KN_FLUX_SLOTS, FLUX_FOLD_DEPTH>(A.part, T.col_slot[q], T.bstart[cw], T.bstart[cw + 1], T.col_max[q] != 0);
  };
  if constexpr (PART) {      // this rank's slots; a watch without local cells folds nothing: 0
    for (int q = threadIdx.x; q < T.n_cols; q += FLUX_THREADS) A.slot[q] = fold(q);
    if (threadIdx.x == 0) kn_reset_ticket(A.ctl);
    return;
  }
  const bool room = kn_claim_row(A.ctl, A.capacity, &row);
  if (room) {
    for (int q = threadIdx.x; q < T.n_cols; q += FLUX_THREADS) A.rows[(size_t)row * T.n_cols + q] = fold(q);
  }
  if (threadIdx.x == 0) {
    kn_commit_row(A.ctl, row, room);
    kn_reset_ticket(A.ctl);
  }
}

template <int KIND, bool PART>
void launch_as(knpemi_handle* h, const FluxArgs& a, int n_blk, bool fields) {
  if (fields) hipLaunchKernelGGL((flux_kernel<KIND, true, PART>), dim3(n_blk), dim3(FLUX_THREADS), 0, h->stream, a);
  else hipLaunchKernelGGL((flux_kernel<KIND, false, PART>), dim3(n_blk), dim3(FLUX_THREADS), 0, h->stream, a);
}
template <int KIND>
void launch(knpemi_handle* h, const FluxArgs& a, int n_blk, bool fields) {
  if (a.slot) launch_as<KIND, true>(h, a, n_blk, fields);
  else launch_as<KIND, false>(h, a, n_blk, fields);
}

}  // namespace

int kn_launch_flux(knpemi_handle* h, int write_fields) {
  const auto& X = h->flux;
  if (X.n_blk == 0) return KNPEMI_OK;      // partitioned, no local cell: this rank's slots stay the zeros of the set-up
  const FluxArgs a{h->K, X.ser.capacity, X.tab, h->d_consts, h->dev.cells, h->dev.VR, X.part, X.ser.ctl, X.ser.rows,
                   write_fields ? X.fields.fld : nullptr, X.recorded,
                   X.slots.xbuf ? X.slots.xbuf + (size_t)X.slots.rank * X.ser.n_cols : nullptr};
  const bool fields = write_fields != 0;
  if (h->cell_kind == KNPEMI_TRIANGLE) launch<KNPEMI_TRIANGLE>(h, a, X.n_blk, fields);
  else if (h->cell_kind == KNPEMI_TETRAHEDRON) launch<KNPEMI_TETRAHEDRON>(h, a, X.n_blk, fields);
  else if (h->cell_kind == KNPEMI_HEXAHEDRON) launch<KNPEMI_HEXAHEDRON>(h, a, X.n_blk, fields);
  else if (h->cell_kind == KNPEMI_QUADRILATERAL) launch<KNPEMI_QUADRILATERAL>(h, a, X.n_blk, fields);
  else return kn_fail(KNPEMI_EINVAL, "flux_kernel: not built for this cell kind");
  return kn_launch_check("flux_kernel");
}

extern "C" int kn_flux_chunk() { return KN_FLUX_CHUNK; }
extern "C" int kn_flux_fold_depth() { return FLUX_FOLD_DEPTH; }
