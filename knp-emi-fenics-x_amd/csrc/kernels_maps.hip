// Field maps on gfx950: per vertex of a bulk field, or per membrane dof, the running peak, trough, time integral, arrival
// time, exposure and excess over a level, advanced in ONE launch per record.
//
// The reference's astrocyte study normalises the glial membrane potential in space by its maximum and its minimum over
// the run (examples/local_astrocyte_depolarization/results/compare_1D_3D.py:89-105, compare_tort.py:114-130,
// make_figures.py:336-352) and plots ECS concentrations in space at chosen times (make_figures.py:135); its users get
// such maps by checkpointing every field at every step.  Here every item of a watch keeps its statistics on the device.
//
// The rules (knpemi_hip.h and knpemi/maps.py state the same).  A watch is a field (phi, c of an ion, phi_M) of a
// sub-domain, an optional threshold thr, a direction s = +1 ("beyond" = at or above) or -1 (at or below) and a selection
// of the statistics peak, trough, integral, threshold.  State per item after set-up or reset: v_prev, v_max, t_max,
// v_min, t_min, t_arrival NaN; integral, exposure, excess and count (int32) 0.  One record at time t (previous record's
// time t_prev, D = t - t_prev) with sample v, in this order:
//   v not finite: v_prev <- v.  Nothing else changes.
//   v_prev not finite (the first record, or the record after a non-finite sample): no interval is accounted for; peak and
//     trough as in step 3; with the threshold statistic and s (v - thr) >= 0: count += 1, t_arrival <- t when count == 1;
//     v_prev <- v.
//   otherwise, with a = s (v_prev - thr), b = s (v - thr):
//     1. integral += 0.5 D (v_prev + v);
//     2. with theta = a / (a - b) where used:
//          onset (a < 0 <= b): t_c = t_prev + D theta; count += 1; t_arrival <- t_c when count == 1;
//            exposure += (1 - theta) D; excess += 0.5 (1 - theta) D b;
//          stays beyond (a >= 0 && b >= 0): exposure += D; excess += 0.5 D (a + b);
//          offset (a >= 0 > b): exposure += theta D; excess += 0.5 theta D a;
//     3. !(v <= v_max) -> v_max <- v, t_max <- t.  !(v >= v_min) -> v_min <- v, t_min <- t;
//     4. v_prev <- v.
// A statistic that is not selected keeps its initial value and costs no memory traffic.  A series watch contributes two
// columns per record: the sum of the item weights over the items with s (v - thr) >= 0, and their number.
//
// Layout: one item per lane, 256-thread workgroups; KnMapTab groups the watches by space (the vertices of a sub-domain,
// the membrane dofs of a cell) and every workgroup belongs to one space (bstart), so the loop over the watches of the
// space and every branch on a watch's selection is uniform over the workgroup.  A bulk lane reads slots 3 .. 7 of its
// 64-byte vertex record once, with three 16-byte loads (the coordinates x, y are not fetched), and serves every record
// field of the space -- phi, the eliminated ion -- from registers; the solver's c and phi_M are dense arrays.  State is
// structure-of-arrays per watch: consecutive lanes read and write consecutive doubles, only the arrays of the selected
// statistics exist, and t_max, t_min, t_arrival and count are written only when they change.  v_prev exists with the
// integral or the threshold only: peak and trough do not depend on it.
//
// Series tail (record_tail.h): a workgroup's partial holds (measure, n) of the series watches of its space, the four waves
// summed in order; the last workgroup folds every column over the workgroups of the column's space in their order and
// appends the row.  Without a series watch the kernel is instantiated without the tail: no ticket, no buffer.
// Partitioned runs (knpemi_maps_set_partitioned): the item weights of a series watch are lumped from the cells (facets)
// this rank records, n counts the items the rank owns (one byte per item), and the last workgroup writes the folded columns
// into this rank's slots of the exchange buffer instead of appending a row; the caller sums the buffer over the ranks and
// record_combine_kernel (kernels_observe.hip) sums the ranks' slots in rank order and appends the row.  That is a third
// instantiation (PART): the two single-rank ones do not know of it.
// This file is built with -ffp-contract=off: the increments are the expressions as written.
#include <cmath>

#include "knpemi_internal.h"
#include "record_tail.h"

#define MAPS_THREADS 256
#define MAPS_WAVES (MAPS_THREADS / 64)
// loads in flight in the last workgroup's fold (record_tail.h).  Measured, 8 against 32, alternating: 12.3 against 14.5 us
// per record at config 2 (86 workgroups), 41.8 against 37.1 us on the 995 k-tet mesh (624); 8 keeps the series
// instantiation at the 48 VGPRs of its body (32: 92).  DESIGN.md 3.4.5
#define MAPS_FOLD_DEPTH 8

namespace {

struct MapsArgs {
  double t, t_prev;
  const KnMapTab* tab;
  const double* VR;
  int capacity;
  double* part;
  unsigned long long* ctl;
  double* rows;
  double* slot;              // partitioned: this rank's n_cols slots of the exchange buffer; nullptr: append the row here
};

// the space of workgroup b: at most KN_MAPS_MAXSPACE - 1 steps, uniform
__device__ inline int space_of(const KnMapTab& T, int b) {
  int p = 0;
  while (p + 1 < T.n_space && b >= T.bstart[p + 1]) ++p;
  return p;
}

// PART: the series of a partitioned run (a template flag: the single-rank instantiations are the code they were)
template <bool SERIES, bool PART = false>
__global__ __launch_bounds__(MAPS_THREADS) void maps_record_kernel(MapsArgs A) {
  __shared__ double sh[MAPS_WAVES][KN_MAPS_SLOTS];
  __shared__ int last;
  __shared__ unsigned long long row;
  const KnMapTab& T = *A.tab;
  const int p = space_of(T, (int)blockIdx.x);
  const int n = T.n_items[p];
  const int i = ((int)blockIdx.x - T.bstart[p]) * MAPS_THREADS + (int)threadIdx.x;
  const bool valid = i < n;
  const double nan = __builtin_nan("");
  const double t = A.t, t_prev = A.t_prev, dt = A.t - A.t_prev;

  // slots 3 .. 7 of the vertex record: c3 | c0 c1 | c2 phi (KN_CSLOT); r[0] is slot 2 and unused
  double r[6] = {nan, nan, nan, nan, nan, nan};
  if (T.need_rec[p] && valid) {
    const double2* q = reinterpret_cast<const double2*>(A.VR + ((size_t)T.first[p] + (size_t)i) * KN_REC);
    const double2 b = q[1], c = q[2], d = q[3];
    r[0] = b.x; r[1] = b.y; r[2] = c.x; r[3] = c.y; r[4] = d.x; r[5] = d.y;
  }
  if constexpr (SERIES) {
    if (threadIdx.x < MAPS_WAVES * KN_MAPS_SLOTS) (&sh[0][0])[threadIdx.x] = 0.0;
    __syncthreads();
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;

  for (int k = T.wstart[p]; k < T.wstart[p + 1]; ++k) {
    const KnMapWatch& W = T.w[k];
    const int flags = W.flags;
    double v = nan;
    if (valid) {
      if (W.dense) {
        v = W.dense[i];
      } else {
        const int s = W.slot - 2;      // 1 .. 5; selected without indexing r by a run-time value
        v = r[1];
#pragma unroll
        for (int j = 2; j < 6; ++j) v = s == j ? r[j] : v;
      }
    }
    const bool fin = std::isfinite(v);
    const double thr = W.thr, sg = W.sgn;
    const double b = sg * (v - thr);
    if (valid) {
      const bool keep_prev = W.v_prev != nullptr;
      const double vp = keep_prev ? W.v_prev[i] : nan;
      if (keep_prev) W.v_prev[i] = v;
      if (fin) {
        const bool first = !std::isfinite(vp);
        if ((flags & KNPEMI_MAPS_INTEGRAL) && !first) W.integral[i] += 0.5 * dt * (vp + v);
        if (flags & KNPEMI_MAPS_THRESHOLD) {
          if (first) {
            if (b >= 0.0) {
              const int c = W.count[i] + 1;
              W.count[i] = c;
              if (c == 1) W.t_arrival[i] = t;
            }
          } else {
            const double a = sg * (vp - thr);
            if (a < 0.0) {
              if (b >= 0.0) {
                const double th = a / (a - b);
                const int c = W.count[i] + 1;
                W.count[i] = c;
                if (c == 1) W.t_arrival[i] = t_prev + dt * th;
                W.exposure[i] += (1.0 - th) * dt;
                W.excess[i] += 0.5 * (1.0 - th) * dt * b;
              }
            } else if (b >= 0.0) {
              W.exposure[i] += dt;
              W.excess[i] += 0.5 * dt * (a + b);
            } else {
              const double th = a / (a - b);
              W.exposure[i] += th * dt;
              W.excess[i] += 0.5 * th * dt * a;
            }
          }
        }
        if (flags & KNPEMI_MAPS_PEAK) {
          if (!(v <= W.v_max[i])) { W.v_max[i] = v; W.t_max[i] = t; }
        }
        if (flags & KNPEMI_MAPS_TROUGH) {
          if (!(v >= W.v_min[i])) { W.v_min[i] = v; W.t_min[i] = t; }
        }
      }
    }
    if constexpr (SERIES) {
      if (W.ser >= 0) {                // uniform over the workgroup
        const bool beyond = valid && fin && b >= 0.0;
        // partitioned: the weights carry the recorded cells (facets), n counts the items this rank owns
        bool counted = beyond;
        if constexpr (PART) counted = beyond && W.owned[i];
        const double sw = kn_wave_sum(beyond ? W.weight[i] : 0.0), sn = kn_wave_sum(counted ? 1.0 : 0.0);
        if (lane == 0) { sh[wave][2 * W.ser] = sw; sh[wave][2 * W.ser + 1] = sn; }
      }
    }
  }

  if constexpr (SERIES) {
    __syncthreads();
    // the workgroup's partial: the four waves in order; slots nobody wrote stay 0 and no column reads them
    if (threadIdx.x < KN_MAPS_SLOTS) {
      const int j = threadIdx.x;
      double v = sh[0][j];
#pragma unroll
      for (int q = 1; q < MAPS_WAVES; ++q) v += sh[q][j];
      kn_part_store(&A.part[(size_t)blockIdx.x * KN_MAPS_SLOTS + j], v);
    }
    if (!kn_arrive_last(A.ctl, threadIdx.x < KN_MAPS_SLOTS, &last)) return;
    if constexpr (PART) {
      // the columns go to this rank's slots and no row is claimed: record_combine_kernel sums the ranks' slots and appends it
      for (int q = threadIdx.x; q < T.n_cols; q += MAPS_THREADS) {
        const int cp = T.col_space[q];
        A.slot[q] = kn_fold_column<KN_MAPS_SLOTS, MAPS_FOLD_DEPTH>(A.part, T.col_slot[q], T.bstart[cp], T.bstart[cp + 1], false);
      }
      if (threadIdx.x == 0) kn_reset_ticket(A.ctl);
      return;
    }
    const bool room = kn_claim_row(A.ctl, A.capacity, &row);
    if (room) {
      for (int q = threadIdx.x; q < T.n_cols; q += MAPS_THREADS) {
        const int cp = T.col_space[q];
        A.rows[(size_t)row * T.n_cols + q] =
            kn_fold_column<KN_MAPS_SLOTS, MAPS_FOLD_DEPTH>(A.part, T.col_slot[q], T.bstart[cp], T.bstart[cp + 1], false);
      }
    }
    if (threadIdx.x == 0) {
      kn_commit_row(A.ctl, row, room);
      kn_reset_ticket(A.ctl);
    }
  }
}

// the state "before the first record" of every item of every watch (knpemi_maps_set, knpemi_maps_reset)
__global__ __launch_bounds__(MAPS_THREADS) void maps_reset_kernel(MapsArgs A) {
  const KnMapTab& T = *A.tab;
  const int p = space_of(T, (int)blockIdx.x);
  const int i = ((int)blockIdx.x - T.bstart[p]) * MAPS_THREADS + (int)threadIdx.x;
  if (i >= T.n_items[p]) return;
  const double nan = __builtin_nan("");
  for (int k = T.wstart[p]; k < T.wstart[p + 1]; ++k) {
    const KnMapWatch& W = T.w[k];
    if (W.v_prev) W.v_prev[i] = nan;
    if (W.v_max) { W.v_max[i] = nan; W.t_max[i] = nan; }
    if (W.v_min) { W.v_min[i] = nan; W.t_min[i] = nan; }
    if (W.integral) W.integral[i] = 0.0;
    if (W.count) { W.count[i] = 0; W.t_arrival[i] = nan; W.exposure[i] = 0.0; W.excess[i] = 0.0; }
  }
}

MapsArgs maps_args(knpemi_handle* h, double t, double t_prev) {
  const auto& M = h->maps;
  return MapsArgs{t, t_prev, M.tab, h->dev.VR, M.ser.capacity, M.part, M.ser.ctl, M.ser.rows,
                  M.slots.xbuf ? M.slots.xbuf + (size_t)M.slots.rank * M.host.n_cols : nullptr};
}

}  // namespace

int kn_launch_maps_record(knpemi_handle* h, double t, double t_prev) {
  const auto& M = h->maps;
  if (M.n_blk == 0) return KNPEMI_OK;
  if (M.slots.xbuf)
    hipLaunchKernelGGL((maps_record_kernel<true, true>), dim3(M.n_blk), dim3(MAPS_THREADS), 0, h->stream, maps_args(h, t, t_prev));
  else if (M.host.n_cols > 0)
    hipLaunchKernelGGL(maps_record_kernel<true>, dim3(M.n_blk), dim3(MAPS_THREADS), 0, h->stream, maps_args(h, t, t_prev));
  else
    hipLaunchKernelGGL(maps_record_kernel<false>, dim3(M.n_blk), dim3(MAPS_THREADS), 0, h->stream, maps_args(h, t, t_prev));
  return kn_launch_check("maps_record_kernel");
}

int kn_launch_maps_reset(knpemi_handle* h) {
  const auto& M = h->maps;
  if (M.n_blk == 0) return KNPEMI_OK;
  hipLaunchKernelGGL(maps_reset_kernel, dim3(M.n_blk), dim3(MAPS_THREADS), 0, h->stream, maps_args(h, 0.0, 0.0));
  return kn_launch_check("maps_reset_kernel");
}
