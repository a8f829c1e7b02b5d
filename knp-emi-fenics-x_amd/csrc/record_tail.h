// The tail the recording kernels share (kernels_observe.hip, kernels_flux.hip, kernels_exchange.hip): how the workgroups
// of one launch turn their partials into one row of a series buffer, without floating-point atomics and without a
// second launch.
//
//   1. every workgroup publishes its partial with relaxed agent-scope stores (kn_part_store);
//   2. kn_arrive_last: the lanes that published fence, one lane takes a ticket on ctl[2], and the workgroup that drew
//      the last ticket fences again and goes on alone: it sees every partial;
//   3. kn_claim_row: it reads the row index ctl[0], last written by the previous launch -- the launch carries no row
//      number, so a replayed launch records into consecutive rows -- and whether the buffer has room for it;
//   4. it folds the partials of every column in workgroup order (kn_fold_column, or a fold of the kernel's own), so the
//      row does not depend on which workgroup came last: two identical runs give identical bits;
//   5. one lane appends the row or counts it as dropped (kn_commit_row) and zeroes the ticket for the next launch
//      (kn_reset_ticket), with plain stores.
// ctl is the series buffer's [4] counters: rows written, rows dropped (buffer full), ticket.
#pragma once
#if !defined(__HIPCC_RTC__)   // (hipRTC provides the runtime's device declarations itself: monitor programs of plug-ins)
#include <hip/hip_runtime.h>
#endif

__device__ inline double kn_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ inline double kn_wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

__device__ inline void kn_part_store(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline double kn_part_load(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Every thread of the workgroup calls it; `published`: this lane has stored a part of the workgroup's partial (lanes of
// the first wave, lane 0 among them, so the ticket follows their stores and fences in program order).  True in the
// workgroup that arrived last, for all of its threads.  *last is a __shared__ int of the caller.
__device__ inline bool kn_arrive_last(unsigned long long* ctl, bool published, int* last) {
  if (published) __threadfence();
  if (threadIdx.x == 0) *last = atomicAdd(&ctl[2], 1ull) == (unsigned long long)(gridDim.x - 1);
  __syncthreads();
  if (!*last) return false;
  __threadfence();
  return true;
}

// Every thread of the one workgroup that writes the row calls it: the row index goes to *row, a __shared__ unsigned long
// long of the caller; returns whether the buffer has room for the row.
__device__ inline bool kn_claim_row(const unsigned long long* ctl, int capacity, unsigned long long* row) {
  if (threadIdx.x == 0) *row = ctl[0];     // last written by the previous launch
  __syncthreads();
  return *row < (unsigned long long)capacity;
}
// One lane, after the row is written.
__device__ inline void kn_commit_row(unsigned long long* ctl, unsigned long long row, bool room) {
  if (room) ctl[0] = row + 1;
  else ctl[1] = ctl[1] + 1;
}
__device__ inline void kn_reset_ticket(unsigned long long* ctl) { ctl[2] = 0; }

// Slot `slot` of the partials [p0, p1) of SLOTS doubles each, summed (or, is_max, maximised from 0) in workgroup order:
// v = 0; v = v o x[p0]; v = v o x[p0 + 1]; ...  DEPTH loads are in flight before the first is combined: one load per
// combination is a chain of L2 round trips, 60 us per record at config 2 (184 partials).  The x[DEPTH] live in registers
// beside nothing else of the kernel, but the allocation of a kernel is that of its widest point: a kernel takes the
// largest DEPTH that leaves its allocation where its body puts it.
template <int SLOTS, int DEPTH>
__device__ inline double kn_fold_column(const double* __restrict__ part, int slot, int p0, int p1, bool is_max) {
  const double* __restrict__ pp = part + slot;
  int p = p0;
  double v = 0.0;
  for (; p + DEPTH <= p1; p += DEPTH) {
    double x[DEPTH];
#pragma unroll
    for (int i = 0; i < DEPTH; ++i) x[i] = kn_part_load(pp + (size_t)(p + i) * SLOTS);
#pragma unroll
    for (int i = 0; i < DEPTH; ++i) v = is_max ? fmax(v, x[i]) : v + x[i];
  }
  for (; p < p1; ++p) {
    const double x = kn_part_load(pp + (size_t)p * SLOTS);
    v = is_max ? fmax(v, x) : v + x;
  }
  return v;
}
