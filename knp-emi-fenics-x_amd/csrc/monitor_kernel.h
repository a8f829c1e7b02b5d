// The record kernel of the membrane monitors (see kernels_monitor.hip for what it does and why it is laid out this way).
// Like ode_kernel.h this header is compiled twice: by hipcc into libknpemi_hip.so with the monitors of the shipped models
// (membrane_monitors.h), and at run time by hipRTC with the `monitor` function a plug-in brings as HIP source
// (knpemi_monitor_bind_source) -- the same body under both.  It includes nothing but ode_kernel.h (OdeDev, the layout of a
// vertex record), monitor_table.h and record_tail.h, and uses plain types only.
//
// EVAL::eval(D, W, q, t, out) fills out[0 .. count) with the quantities of dof q of watch W at time t; mon_load is the
// state rule of include/knpemi_hip.h for its use.
#pragma once

#include "ode_kernel.h"
#include "monitor_table.h"
#include "record_tail.h"

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
// no multiply-add of the kernel is contracted (host restatements form the same sums with a multiply and an add)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define MON_THREADS 256
#define MON_WAVES (MON_THREADS / 64)
// loads the fold of the partials has in flight (record_tail.h).  The body -- a parameter row of up to 23 doubles beside the
// quantities -- takes 121 VGPRs; the fold's x[DEPTH] live beside nothing else of the kernel: depths 8, 16 and 32 all
// leave the allocation at those 121, 64 take it to 248: 32
#ifndef MON_FOLD_DEPTH
#define MON_FOLD_DEPTH 32
#endif

// NaN-propagating minimum and maximum
__device__ __forceinline__ double mon_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double mon_max(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double mon_wave_min(double v) {
  for (int o = 32; o > 0; o >>= 1) v = mon_min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ double mon_wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = mon_max(v, __shfl_xor(v, o));
  return v;
}
// op 0: sum from 0, 1: minimum from +inf, 2: maximum from -inf
__device__ __forceinline__ double mon_combine(int op, double v, double x) {
  return op == 0 ? v + x : (op == 1 ? mon_min(v, x) : mon_max(v, x));
}
// kn_fold_column with the three operations of this kernel: slot `slot` of the partials [p0, p1) in workgroup order
template <int DEPTH>
__device__ inline double mon_fold(const double* __restrict__ part, int slot, int p0, int p1, int op) {
  const double* __restrict__ pp = part + slot;
  int p = p0;
  double v = op == 0 ? 0.0 : (op == 1 ? __builtin_inf() : -__builtin_inf());
  for (; p + DEPTH <= p1; p += DEPTH) {
    double x[DEPTH];
#pragma unroll
    for (int i = 0; i < DEPTH; ++i) x[i] = kn_part_load(pp + (size_t)(p + i) * KN_MON_SLOTS);
#pragma unroll
    for (int i = 0; i < DEPTH; ++i) v = mon_combine(op, v, x[i]);
  }
  for (; p < p1; ++p) v = mon_combine(op, v, kn_part_load(pp + (size_t)p * KN_MON_SLOTS));
  return v;
}

// kn_arrive_last for a record of several launches and for partials that any lane of the workgroup may have stored: every
// lane fences its stores, the barrier orders them before the ticket lane 0 takes; the workgroup that draws the last of
// the record's `total` tickets goes on alone and sees every partial.
__device__ inline bool mon_arrive_last(unsigned long long* ctl, int total, int* last) {
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) *last = atomicAdd(&ctl[2], 1ull) == (unsigned long long)(total - 1);
  __syncthreads();
  if (!*last) return false;
  __threadfence();
  return true;
}

// The state a monitor sees: state and parameter row of dof q (0 <= q < W.nq) of watch W, in registers (every index of
// the unrolled loops is a constant).
template <int NS, int NP>
__device__ __forceinline__ void mon_load(const OdeDev& D, const KnMonWatch& W, int q, double (&y)[NS], double (&row)[NP]) {
  const size_t nq = (size_t)W.nq;
#pragma unroll
  for (int j = 0; j < NS; ++j) y[j] = W.states[(size_t)j * nq + q];
#pragma unroll
  for (int j = 0; j < NP; ++j) row[j] = W.params[(size_t)j * nq + q];
  if (W.pde) {
    const int qg = W.q0 + q;
    const double* re = D.VR + (size_t)D.q2e[qg] * KN_ODE_REC;
    const double* ri = D.VR + (size_t)D.q2i[qg] * KN_ODE_REC;
    const double v = D.phiM[qg];
#pragma unroll
    for (int k = 0; k < KN_ODE_MAXK; ++k) {
      if (k < W.n_ions) {
        const double ce = re[KN_ODE_CSLOT(k)], ci = ri[KN_ODE_CSLOT(k)];
        const int je = W.ion_e[k], ji = W.ion_i[k];
#pragma unroll
        for (int j = 0; j < NP; ++j) row[j] = j == je ? ce : (j == ji ? ci : row[j]);   // (no computed index: registers)
      }
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) y[j] = j == W.v_index ? v : y[j];
  }
}

template <class EVAL, bool FIELDS>
__device__ __forceinline__ void monitor_body(const OdeDev& D, const KnMonArgs& A) {
  __shared__ double sh[MON_WAVES][KN_MON_SLOTS];
  __shared__ int last;
  __shared__ unsigned long long row;
  const KnMonTab& T = *A.tab;
  const int gb = A.blk0 + (int)blockIdx.x;                                   // this workgroup within the record
  int w = 0;
  while (w + 1 < T.n_watch && gb >= T.bstart[w + 1]) ++w;                    // at most KN_MON_MAXW - 1 steps, uniform
  const KnMonWatch& W = T.w[w];
  const int ql = (gb - T.bstart[w]) * MON_THREADS + (int)threadIdx.x;
  // lanes past the watch's last dof repeat the last one and contribute nothing: the shuffles see whole waves
  const bool live = ql < W.nq;
  const int q = live ? ql : W.nq - 1;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < MON_WAVES * KN_MON_SLOTS; i += MON_THREADS) (&sh[0][0])[i] = 0.0;

  double out[KN_MON_MAX];
#pragma unroll
  for (int i = 0; i < KN_MON_MAX; ++i) out[i] = 0.0;
  EVAL::eval(D, W, q, A.t, out);

  if (FIELDS && live) {
    double* __restrict__ f = A.fld + W.fbase + q;
    int c = 0;
#pragma unroll
    for (int i = 0; i < KN_MON_MAX; ++i) {
      if (!((W.mask >> i) & 1u)) continue;              // uniform over the workgroup
      __builtin_nontemporal_store(out[i], f + (size_t)c * W.nq);
      ++c;
    }
  }
  if (!A.ctl) return;

  __syncthreads();                                      // sh is zero
  if (W.rmask) {
    const double wq = live ? W.weight[q] : 0.0;
    const bool valid = live && wq > 0.0;
#pragma unroll
    for (int i = 0; i < KN_MON_MAX; ++i) {
      if (!((W.rmask >> i) & 1u)) continue;             // uniform over the workgroup
      const double s = kn_wave_sum(valid ? wq * out[i] : 0.0);
      const double mn = mon_wave_min(valid ? out[i] : __builtin_inf());
      const double mx = mon_wave_max(valid ? out[i] : -__builtin_inf());
      if (lane == 0) { sh[wave][3 * i] = s; sh[wave][3 * i + 1] = mn; sh[wave][3 * i + 2] = mx; }
    }
  }
  __syncthreads();
  // the workgroup's partial: the four waves in order, one quantity per lane of the first wave
  if (threadIdx.x < KN_MON_MAX) {
    const int j = 3 * threadIdx.x;
    double s = sh[0][j], mn = sh[0][j + 1], mx = sh[0][j + 2];
#pragma unroll
    for (int k = 1; k < MON_WAVES; ++k) {
      s += sh[k][j];
      mn = mon_min(mn, sh[k][j + 1]);
      mx = mon_max(mx, sh[k][j + 2]);
    }
    double* p = A.part + (size_t)gb * KN_MON_SLOTS + j;
    kn_part_store(p, s);
    kn_part_store(p + 1, mn);
    kn_part_store(p + 2, mx);
  }
  // the points of this watch: its first workgroup evaluates the model at their dofs itself -- lane e takes dof e % 4 of
  // point e / 4, all quantities -- so a point column depends on no workgroup's per-dof field stores and exists without
  // fields; the values travel to the row's writer as the partials do
  if (gb == T.bstart[w]) {
    for (int e = threadIdx.x; e < 4 * T.n_pts; e += MON_THREADS) {
      const int pq = A.pt_q[e];
      if (pq < 0 || A.pt_watch[e >> 2] != w) continue;
      double o[KN_MON_MAX];
#pragma unroll
      for (int i = 0; i < KN_MON_MAX; ++i) o[i] = 0.0;
      EVAL::eval(D, W, pq, A.t, o);
#pragma unroll
      for (int i = 0; i < KN_MON_MAX; ++i) kn_part_store(A.pt_val + (size_t)e * KN_MON_MAX + i, o[i]);
    }
  }
  if (!mon_arrive_last(A.ctl, A.n_blk_total, &last)) return;
  // partitioned (A.slot, uniform over the launch): the columns go to this rank's slots, the average undivided, and no row
  // is claimed -- record_combine_kernel folds the ranks' slots, divides and appends the row
  double* const slot = A.slot;
  const bool room = slot ? true : kn_claim_row(A.ctl, A.capacity, &row);
  if (room) {                                           // uniform over the workgroup
    double* const dst = slot ? slot : A.rows + (size_t)row * T.n_cols;
    for (int c = threadIdx.x; c < T.n_cols; c += MON_THREADS) {
      const int kind = A.cols[4 * c], cw = A.cols[4 * c + 1], cq = A.cols[4 * c + 2], cp = A.cols[4 * c + 3];
      double v = 0.0;
      if (kind == 0) {                                  // KNPEMI_MON_POINT: w_j v(q_j) in the order of the facet's dofs
        for (int j = 0; j < 4; ++j) {
          const int e = 4 * cp + j;
          if (A.pt_q[e] >= 0) v += A.pt_w[e] * kn_part_load(A.pt_val + (size_t)e * KN_MON_MAX + cq);
        }
      } else {                                          // _INTEGRAL 1, _AVERAGE 2, _MIN 3, _MAX_OP 4
        const int op = kind == 3 ? 1 : (kind == 4 ? 2 : 0);
        v = mon_fold<MON_FOLD_DEPTH>(A.part, 3 * cq + op, T.bstart[cw], T.bstart[cw + 1], op);
        if (kind == 2 && !slot) v = v / T.w[cw].wsum;
      }
      dst[c] = v;
    }
  }
  if (threadIdx.x == 0) {
    if (!slot) kn_commit_row(A.ctl, row, room);
    kn_reset_ticket(A.ctl);
  }
}
#endif
