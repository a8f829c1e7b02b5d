// Observables on gfx950: every linear functional / min / max of the nodal fields in ONE launch per recorded row.
//
// The reference evaluates its time series on the host from checkpoints (scifem.evaluate_function at fixed points,
// examples/idealized_geometries/make_figures.py:24-117; means and maxima of the downloaded arrays,
// local_astrocyte_depolarization/run_stim_duration.py:239-246).  Here a point is a sparse dot product over the <= 8
// vertices of its cell and a reduction a dense one over a sub-domain; the host cuts every observable's entries into
// chunks of OBS_CHUNK and gives each chunk one workgroup.  A workgroup reduces its chunk in a fixed order (strided
// per-lane sums, then a fixed LDS tree) and publishes the partial; the tail is that of record_tail.h: the last
// workgroup to arrive combines the partials of every observable in block order, with the observable's own op and
// identity, and appends the row, or counts it as dropped when the buffer is full.
//
// Partitioned runs (knpemi_observe_set_partitioned): the last workgroup writes each observable's fold of its block
// partials, without the denominator, into this rank's slot xbuf[rank * n_obs + q] instead of appending a row (an
// observable without local entries, or a rank without any, writes the op's identity).  The caller sums xbuf over the
// ranks -- every slot has one non-zero contributor, so the sum is an exact all-gather -- and record_combine_kernel
// folds the slots in rank order, divides by the denominators and appends the row.
#include <algorithm>
#include <cmath>

#include "knpemi_internal.h"
#include "record_tail.h"

#define OBS_THREADS 256
#define OBS_CHUNK (OBS_THREADS * 8)     // entries per workgroup: 8 loads per lane in flight on the dense reductions

namespace {

struct ObsArgs {
  int n_obs, capacity, n_blk;
  const int4* blk;
  const int* blk_ptr;
  const int* op;
  const int* stride;
  const double* const* base;
  const double* denom;
  const int* idx;
  const double* w;
  double* part;
  unsigned long long* ctl;
  double* rows;
  double* slot;              // partitioned: this rank's n_obs slots of xbuf; nullptr: append the row here
};

// the combine launch of a partitioned record, shared with the fluxes and the membrane exchange (kernels_flux.hip,
// kernels_exchange.hip): their columns have no op table but the watch table's col_max, and no denominators; with the maps'
// series (kernels_maps.hip: every column a sum) and with the membrane monitors (kernels_monitor.hip: an op and a divisor
// per column, and minima and maxima that keep a NaN)
struct CombineArgs {
  int n_cols, capacity, world, rank;
  const int* op;             // the columns' ops; nullptr: col_max decides, sums and maxima start from 0
  const double* denom;       // divisor of a sum; nullptr: none
  const uint8_t* col_max;    // nullptr (and no op): every column is a sum
  bool keep_nan;             // minimum and maximum keep a NaN (the monitors' mon_min / mon_max), not fmin / fmax
  double* xbuf;              // [world][n_cols], summed over the ranks
  unsigned long long* ctl;
  double* rows;
};

__device__ inline double obs_combine(int op, double a, double b) {
  return op == KNPEMI_OBS_SUM ? a + b : op == KNPEMI_OBS_MIN ? fmin(a, b) : fmax(a, b);
}

// the monitors' fold: a NaN on either side stays (monitor_kernel.h, mon_min / mon_max)
__device__ inline double obs_combine_keep_nan(int op, double a, double b) {
  return op == KNPEMI_OBS_SUM ? a + b : op == KNPEMI_OBS_MIN ? ((a < b || a != a) ? a : b) : ((a > b || a != a) ? a : b);
}

__device__ inline double obs_identity(int op) {
  return op == KNPEMI_OBS_SUM ? 0.0 : op == KNPEMI_OBS_MIN ? INFINITY : -INFINITY;
}

__global__ __launch_bounds__(OBS_THREADS) void observe_kernel(ObsArgs A) {
  __shared__ double sh[OBS_THREADS];
  __shared__ int last;
  __shared__ unsigned long long row;
  // a partitioned rank without entries runs one workgroup that has no block: it only publishes the identities
  const bool has_blk = (int)blockIdx.x < A.n_blk;
  if (has_blk) {
    const int4 b = A.blk[blockIdx.x];
    const int o = b.x, op = A.op[o], stride = A.stride[o];
    const double* __restrict__ u = A.base[o];
    double acc = obs_identity(op);
    // lane t takes entries b.y + t, b.y + t + 256, ...: consecutive lanes read consecutive entries (and, on the dense
    // reductions, consecutive vertices)
    if (op == KNPEMI_OBS_SUM) {
      for (int e = b.y + threadIdx.x; e < b.z; e += OBS_THREADS) acc += A.w[e] * u[(size_t)A.idx[e] * stride];
    } else {
      for (int e = b.y + threadIdx.x; e < b.z; e += OBS_THREADS) acc = obs_combine(op, acc, u[(size_t)A.idx[e] * stride]);
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = OBS_THREADS / 2; s > 0; s >>= 1) {
      if (threadIdx.x < s) sh[threadIdx.x] = obs_combine(op, sh[threadIdx.x], sh[threadIdx.x + s]);
      __syncthreads();
    }
  }
  if (threadIdx.x == 0 && has_blk) kn_part_store(&A.part[blockIdx.x], sh[0]);
  if (!kn_arrive_last(A.ctl, threadIdx.x == 0, &last)) return;
  // this observable's block partials in block order: independent of which block came last
  auto fold = [&](int q, int qop) {
    double v = obs_identity(qop);
    for (int p = A.blk_ptr[q]; p < A.blk_ptr[q + 1]; ++p) v = obs_combine(qop, v, kn_part_load(&A.part[p]));
    return v;
  };
  if (A.slot) {                             // partitioned: this rank's slots; the row is appended by the combine kernel
    for (int q = threadIdx.x; q < A.n_obs; q += OBS_THREADS) A.slot[q] = fold(q, A.op[q]);
    if (threadIdx.x == 0) kn_reset_ticket(A.ctl);
    return;
  }
  const bool room = kn_claim_row(A.ctl, A.capacity, &row);
  if (room) {
    for (int q = threadIdx.x; q < A.n_obs; q += OBS_THREADS) {
      const int qop = A.op[q];
      double v = fold(q, qop);
      if (qop == KNPEMI_OBS_SUM) v /= A.denom[q];
      A.rows[(size_t)row * A.n_obs + q] = v;
    }
  }
  if (threadIdx.x == 0) {
    kn_commit_row(A.ctl, row, room);
    kn_reset_ticket(A.ctl);
  }
}

// One workgroup: fold the ranks' slots of every column in rank order (the same order on every rank, so every rank
// appends the same row) -- with the observable's op from its identity, or by col_max as a sum or a maximum from 0 --
// divide the observables' sums by the global denominator, append the row, then zero the other ranks' slots so that the
// next sum over the ranks again has one non-zero contributor per slot.
__global__ __launch_bounds__(OBS_THREADS) void record_combine_kernel(CombineArgs A) {
  __shared__ unsigned long long row;
  const bool room = kn_claim_row(A.ctl, A.capacity, &row);
  for (int q = threadIdx.x; q < A.n_cols; q += OBS_THREADS) {
    const int qop = A.op ? A.op[q] : (A.col_max && A.col_max[q]) ? KNPEMI_OBS_MAX : KNPEMI_OBS_SUM;
    double v = A.op ? obs_identity(qop) : 0.0;
    for (int k = 0; k < A.world; ++k) {
      const double x = A.xbuf[(size_t)k * A.n_cols + q];
      v = A.keep_nan ? obs_combine_keep_nan(qop, v, x) : obs_combine(qop, v, x);
    }
    if (A.denom && qop == KNPEMI_OBS_SUM) v /= A.denom[q];
    if (room) A.rows[(size_t)row * A.n_cols + q] = v;
  }
  __syncthreads();                          // every slot read before any is zeroed
  const int n = A.world * A.n_cols;
  for (int i = threadIdx.x; i < n; i += OBS_THREADS)
    if (i / A.n_cols != A.rank) A.xbuf[i] = 0.0;
  if (threadIdx.x == 0) kn_commit_row(A.ctl, row, room);      // one workgroup: no ticket
}

}  // namespace

int kn_launch_observe(KnDevice* own, const knpemi_handle::KnObserve& O) {
  if (O.n_blk == 0 && !O.slots.xbuf) return KNPEMI_OK;
  ObsArgs a{O.n_obs, O.ser.capacity, O.n_blk, O.blk, O.blk_ptr, O.op, O.stride, O.base, O.denom, O.idx, O.w, O.part, O.ser.ctl,
            O.ser.rows, O.slots.xbuf ? O.slots.xbuf + (size_t)O.slots.rank * O.n_obs : nullptr};
  hipLaunchKernelGGL(observe_kernel, dim3(std::max(O.n_blk, 1)), dim3(OBS_THREADS), 0, own->stream, a);
  return kn_launch_check("observe_kernel");
}

int kn_launch_record_combine(knpemi_handle* h, const char* who, int n_cols, int capacity, int world, int rank, const int* op,
                             const double* denom, const uint8_t* col_max, double* xbuf, unsigned long long* ctl, double* rows,
                             bool keep_nan) {
  CombineArgs a{n_cols, capacity, world, rank, op, denom, col_max, keep_nan, xbuf, ctl, rows};
  hipLaunchKernelGGL(record_combine_kernel, dim3(1), dim3(OBS_THREADS), 0, h->stream, a);
  return kn_launch_check(who);
}

int kn_launch_observe_combine(knpemi_handle* h) {
  const auto& O = h->obs;
  return kn_launch_record_combine(h, "record_combine_kernel (observables)", O.n_obs, O.ser.capacity, O.slots.world, O.slots.rank, O.op,
                                  O.denom, nullptr, O.slots.xbuf, O.ser.ctl, O.ser.rows);
}

int kn_observe_chunk() { return OBS_CHUNK; }
