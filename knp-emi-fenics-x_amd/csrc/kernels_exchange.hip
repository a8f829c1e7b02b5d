// Membrane ion exchange per cell on gfx950: what crosses the membranes, per-facet means and the series row in ONE launch
// per record.
//
// The membrane term of b_knp (knpWeakForm.py:168-214; facet_point in kernels_assemble.hip) is minus the transmembrane
// molar flux of each ion, tested against the facet functions.  With wq the quadrature weight times the surface Jacobian
// and sgn = +1 on the cell side, -1 on the ECS side, fk = wq sgn (C_k g_k - C_k [phi]) expands, on side s in {e, i}, to
//   fk     = -wq sgn j_k^s
//   j_k^s  = (I_ch,k + alpha_k^s (I_cap - S I_ch,tot)) / (F z_k)        [mol / (m^2 s), positive out of the cell]
//   I_cap  = C_M (phi_M - phi_M_prev) / dt,   phi_M = phi_i - phi_e (the potential just solved for)
//   alpha_k^s = D_k^s z_k^2 c_k^s / sum_j D_j^s z_j^2 c_j^s             (c = c_prev on side s, the sum over all K ions)
//   I_ch,tot = sum_j I_ch,j,   S = 1 with the splitting scheme, 0 without.
// The assembly integrates these numbers and keeps only their sum with everything else in b_knp; this kernel integrates
// them again, for every ion (the eliminated one included: its alpha comes from az2D like the others'), and keeps them.
//
// It reads what knp_membrane_kernel reads -- the vertex records of the two sides, phi_M_prev, I_ch per model, fmodel and
// the degree-6 facet table qtab -- through the SAME device code (membrane_facet.h: FacetData, load_facet,
// facet_point_fields), in the same lane layout: KN_MEM_LQ adjacent lanes share one (facet, side), each takes every
// KN_MEM_LQ-th quadrature point and the lanes meet in a shuffle reduction.  The grid covers the facets of the watched
// cells only (KnWatchTab: workgroup b belongs to one watch), both sides of each; a facet without a membrane model
// (fmodel < 0) contributes nothing.
//
// Per (facet, side): int j_k^s dS and int I_ch,k dS for the watched ions only (the mask is uniform over a workgroup);
// int I_cap dS, int I_ch,tot dS and the facet's area sum_q wq always -- the means need the area.  The cell side carries on
// what is the same on both sides.  With write_fields the per-facet means
// (integral / area; 0 on a facet without a model, whose area is written as 0) go to structure-of-arrays buffers
// [component][facet] through non-temporal stores: nothing of it is read again by the device.
//
// Series row: per watched (cell, ion) int j^e, int j^i [mol/s] and int I_ch,k [A]; with the current columns int I_cap,
// int I_ch,tot [A] and the membrane area.  The reduction follows flux_kernel: a fixed tree inside the workgroup (xor
// butterfly over the 64 lanes of a wave, then the four waves in order), one partial of KN_EX_SLOTS doubles per workgroup,
// and the tail of record_tail.h: the last workgroup to arrive folds the partials of every column in workgroup order and
// appends the row, or counts it as dropped when the buffer is full.  The row does not depend on write_fields.
//
// Partitioned runs (knpemi_exchange_set_partitioned; PART): a rank's facets include those of its ghost layer, whose inputs
// are valid after the bulk halo and whose membrane dofs are integrated redundantly.  One byte per facet says whether
// this rank records it: a facet that is not recorded gets its means written like any other and enters no sum.  The
// KN_MEM_LQ lanes of a (facet, side) read the same byte, neighbouring groups neighbouring bytes.  The last workgroup
// writes the folded columns into this rank's slots of the exchange buffer and leaves the row counters alone: the caller
// sums the buffer over the ranks and record_combine_kernel (kernels_observe.hip) appends the row.  PART is a template
// flag: the single-rank instantiations are the code they were without it.
//
// The membrane is a 2-D set: a launch is a few dozen workgroups that wait for their gathers, like knp_membrane_kernel.
#include "knpemi_internal.h"
#include "membrane_facet.h"
#include "record_tail.h"

#define EX_THREADS 256
#define EX_WAVES (EX_THREADS / 64)
#define EX_CHUNK (EX_THREADS / (2 * KN_MEM_LQ))      // facets per workgroup
#define EX_QTAB (16 * (1 + 4 + 8))                   // the largest facet table (quadrilaterals: 16 points)
#define EX_FOLD_DEPTH 16                             // loads the fold of the partials has in flight (kn_fold_column)

namespace {

struct ExArgs {
  int K, capacity, splitting;
  const KnWatchTab* tab;
  double* part;
  unsigned long long* ctl;
  double* rows;
  double* fld;
  const uint8_t* recorded;   // PART: [facets of every watch] 1 = this rank records the facet
  double* slot;              // PART: this rank's n_cols slots of the exchange buffer
};

template <int NF, bool FIELDS, bool PART>
__global__ __launch_bounds__(EX_THREADS) void exchange_kernel(KnDev D, const KnConsts* __restrict__ Cp, ExArgs A) {
  __shared__ double qt[EX_QTAB];
  __shared__ double sh[EX_WAVES][KN_EX_SLOTS];
  __shared__ int last;
  __shared__ unsigned long long row;
  const KnConsts& C = *Cp;
  const KnWatchTab& T = *A.tab;
  const int K = A.K;
  const int nq = D.nq_gamma;
  const int ntab = nq * (1 + NF + (NF == 4 ? 2 * NF : 0));
  for (int i = threadIdx.x; i < ntab; i += EX_THREADS) qt[i] = D.qtab[i];
  if (threadIdx.x < EX_WAVES * KN_EX_SLOTS) (&sh[0][0])[threadIdx.x] = 0.0;
  __syncthreads();
  const double* qw = qt;
  const double* qN = qt + nq;
  const double* qdN = qt + nq * (1 + NF);

  int w = 0;
  while (w + 1 < T.n_watch && (int)blockIdx.x >= T.bstart[w + 1]) ++w;      // at most KN_MAXSUB - 1 steps, uniform
  const int mask = T.mask[w], nf = T.count[w];
  const bool cur = (mask & KN_WATCH_CURRENT) != 0;
  const int gt = ((int)blockIdx.x - T.bstart[w]) * EX_THREADS + (int)threadIdx.x;
  const int t = gt / KN_MEM_LQ, lq = gt % KN_MEM_LQ;
  // lanes past the watch's last (facet, side) repeat the last one and contribute nothing: the shuffles see whole groups
  const bool live = t < 2 * nf;
  const int tt = live ? t : 2 * nf - 1;
  const int fl = tt >> 1, fg = T.first[w] + fl;
  const bool cell_side = tt & 1;
  const int ms = D.fmodel[fg];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;

  double aj[KN_MAXK], ai[KN_MAXK], acap = 0.0, atot = 0.0, area = 0.0;
#pragma unroll
  for (int k = 0; k < KN_MAXK; ++k) { aj[k] = 0.0; ai[k] = 0.0; }
  if (ms >= 0) {
    FacetData<NF> f;
    load_facet<NF>(D, C, fg, cell_side, ms, f);
    double rFz[KN_MAXK];
#pragma unroll
    for (int k = 0; k < KN_MAXK; ++k) rFz[k] = k < K ? 1.0 / (C.F * C.z[k]) : 0.0;
    const double cm_dt = C.C_M * C.inv_dt;
    for (int q = lq; q < nq; q += KN_MEM_LQ) {
      FacetPoint P;
      facet_point_fields<NF>(f, q, qw, qN, qdN, P);
      const double rasum = kn_rcp(P.asum);
      const double icap = cm_dt * ((P.ph_i - P.ph_e) - P.pmq);
      const double shared_part = A.splitting ? icap - P.it : icap;      // what the ions share by their alpha
#pragma unroll
      for (int k = 0; k < KN_MAXK; ++k) {
        if ((mask >> k) & 1) {                                           // a watched ion (k < K): uniform over the workgroup
          const double al = f.so->az2D[k] * P.cq[k] * rasum;
          aj[k] += P.wq * ((P.iq[k] + al * shared_part) * rFz[k]);
          ai[k] += P.wq * P.iq[k];
        }
      }
      acap += P.wq * icap;
      atot += P.wq * P.it;
      area += P.wq;
    }
  }
#pragma unroll
  for (int m = 1; m < KN_MEM_LQ; m <<= 1) {
#pragma unroll
    for (int k = 0; k < KN_MAXK; ++k) { aj[k] += __shfl_xor(aj[k], m); ai[k] += __shfl_xor(ai[k], m); }
    acap += __shfl_xor(acap, m); atot += __shfl_xor(atot, m); area += __shfl_xor(area, m);
  }
  // one lane per (facet, side) carries the integrals on; the cell side also carries what both sides share
  const bool lead = live && lq == 0;
  const bool lead_i = lead && cell_side, lead_e = lead && !cell_side;
  // sum_i / sum_e: the lanes whose integrals enter the sums
  bool rec = true;
  if constexpr (PART) rec = A.recorded[(size_t)T.ibase[w] + fl] != 0;
  const bool sum_i = lead_i && rec, sum_e = lead_e && rec;
  const double inv_area = area > 0.0 ? 1.0 / area : 0.0;
  double* __restrict__ fld = FIELDS ? A.fld + T.fbase[w] + fl : nullptr;      // this facet's place in component 0
  auto put = [&](bool who, int comp, double v) {
    if (FIELDS && who) __builtin_nontemporal_store(v, fld + (size_t)comp * nf);
  };
  int comp = 0;
#pragma unroll
  for (int k = 0; k < KN_MAXK; ++k) {
    if (!((mask >> k) & 1)) continue;                 // uniform over the workgroup
    put(lead_e, comp, aj[k] * inv_area);
    put(lead_i, comp + 1, aj[k] * inv_area);
    put(lead_i, comp + 2, ai[k] * inv_area);
    comp += 3;
    const double se = kn_wave_sum(sum_e ? aj[k] : 0.0), si = kn_wave_sum(sum_i ? aj[k] : 0.0);
    const double sc = kn_wave_sum(sum_i ? ai[k] : 0.0);
    if (lane == 0) { sh[wave][3 * k] = se; sh[wave][3 * k + 1] = si; sh[wave][3 * k + 2] = sc; }
  }
  if (cur) {
    put(lead_i, comp, acap * inv_area);
    put(lead_i, comp + 1, area);
    const double sc = kn_wave_sum(sum_i ? acap : 0.0), st = kn_wave_sum(sum_i ? atot : 0.0);
    const double sa = kn_wave_sum(sum_i ? area : 0.0);
    if (lane == 0) { sh[wave][3 * KN_MAXK] = sc; sh[wave][3 * KN_MAXK + 1] = st; sh[wave][3 * KN_MAXK + 2] = sa; }
  }
  __syncthreads();

  // the workgroup's partial: the four waves in order; slots nobody wrote stay 0 and no column reads them
  if (threadIdx.x < KN_EX_SLOTS) {
    const int j = threadIdx.x;
    double v = sh[0][j];
#pragma unroll
    for (int q = 1; q < EX_WAVES; ++q) v += sh[q][j];
    kn_part_store(&A.part[(size_t)blockIdx.x * KN_EX_SLOTS + j], v);
  }
  if (!kn_arrive_last(A.ctl, threadIdx.x < KN_EX_SLOTS, &last)) return;
  auto fold = [&](int q) {
    const int cw = T.col_watch[q];      // every column is a sum: col_max is all zero here
    return kn_fold_column<KN_EX_SLOTS, EX_FOLD_DEPTH>(A.part, T.col_slot[q], T.bstart[cw], T.bstart[cw + 1], false);
  };
  if constexpr (PART) {      // this rank's slots; a watch without local facets folds nothing: 0
    for (int q = threadIdx.x; q < T.n_cols; q += EX_THREADS) A.slot[q] = fold(q);
    if (threadIdx.x == 0) kn_reset_ticket(A.ctl);
    return;
  }
  const bool room = kn_claim_row(A.ctl, A.capacity, &row);
  if (room) {
    for (int q = threadIdx.x; q < T.n_cols; q += EX_THREADS) A.rows[(size_t)row * T.n_cols + q] = fold(q);
  }
  if (threadIdx.x == 0) {
    kn_commit_row(A.ctl, row, room);
    kn_reset_ticket(A.ctl);
  }
}

template <int NF, bool PART>
void launch_as(knpemi_handle* h, const ExArgs& a, int n_blk, bool fields) {
  if (fields) hipLaunchKernelGGL((exchange_kernel<NF, true, PART>), dim3(n_blk), dim3(EX_THREADS), 0, h->stream, h->dev, h->d_consts, a);
  else hipLaunchKernelGGL((exchange_kernel<NF, false, PART>), dim3(n_blk), dim3(EX_THREADS), 0, h->stream, h->dev, h->d_consts, a);
}
template <int NF>
void launch(knpemi_handle* h, const ExArgs& a, int n_blk, bool fields) {
  if (a.slot) launch_as<NF, true>(h, a, n_blk, fields);
  else launch_as<NF, false>(h, a, n_blk, fields);
}

}  // namespace

int kn_launch_exchange(knpemi_handle* h, int write_fields) {
  const auto& X = h->exchange;
  if (X.n_blk == 0) return KNPEMI_OK;      // partitioned, no local facet: this rank's slots stay the zeros of the set-up
  if (h->dev.nq_gamma * (1 + h->NF + (h->NF == 4 ? 2 * h->NF : 0)) > EX_QTAB)
    return kn_fail(KNPEMI_EINVAL, "exchange_kernel: the facet quadrature table does not fit its LDS copy (EX_QTAB)");
  const int split = (h->knp_flags & KNPEMI_NO_SPLITTING) ? 0 : 1;
  const ExArgs a{h->K, X.ser.capacity, split, X.tab, X.part, X.ser.ctl, X.ser.rows, write_fields ? X.fields.fld : nullptr,
                 X.recorded, X.slots.xbuf ? X.slots.xbuf + (size_t)X.slots.rank * X.ser.n_cols : nullptr};
  const bool fields = write_fields != 0;
  if (h->NF == 2) launch<2>(h, a, X.n_blk, fields);
  else if (h->NF == 3) launch<3>(h, a, X.n_blk, fields);
  else launch<4>(h, a, X.n_blk, fields);
  return kn_launch_check("exchange_kernel");
}

extern "C" int kn_exchange_chunk() { return EX_CHUNK; }
extern "C" int kn_exchange_fold_depth() { return EX_FOLD_DEPTH; }
