// Membrane events on gfx950: per-dof threshold crossings, activation times and peaks of phi_M in ONE launch per record.
//
// The reference has no such quantity: its users checkpoint phi_M at every step (run_3D.py:57-60, 376) and read the
// checkpoints back on the host (make_figures.py:67-89 for one point); when a membrane dof fired, how often and where
// the action potential went follow from post-processing every one of those arrays.  Here each membrane dof of a
// watched cell keeps a few words of state on the device -- the previous sample, an armed flag, the crossing count,
// the first and the latest crossing time, a ring of the latest `keep` crossing times, the running peak and its time
// -- and one launch behind the end-of-step update advances all of them.  The work is local per dof: no LDS, no
// atomics, no reductions, no communication (a partitioned run integrates its ghost membrane dofs redundantly with
// identical bits, so their events are identical too).
//
// Layout: one dof per lane, 256-thread workgroups.  The state is structure-of-arrays over the handle's concatenated
// membrane dofs (qoff), the ring [keep][NQtot], so the lanes of a wave read and write consecutive doubles in every
// array.  The grid covers the dofs of the watched sub-domains only (KnEvTab::gstart maps a lane to its segment); the
// threshold and the reset level come from the table, indexed by the dof's sub-domain.  The time of the record and of
// the previous one are kernel arguments: the handle remembers the latter on the host.
//
// One record with sample v at time t (knpemi_hip.h: knpemi_events_record states the same rules):
//   first record:  v_prev <- v, armed <- (v < threshold), v_peak <- v, t_peak <- t
//   later records: a non-finite v only replaces v_prev; otherwise
//     1. !armed && v < reset      ->  armed
//     2. armed && v >= threshold  ->  crossing at t_prev + (t - t_prev) (threshold - v_prev) / (v - v_prev); disarmed
//     3. v > v_peak               ->  v_peak <- v, t_peak <- t
//     4. v_prev <- v
// An armed dof's previous finite sample lies below the threshold (it would have crossed otherwise), so v - v_prev > 0
// at a crossing; a crossing right after a non-finite sample is counted with a NaN time.
#include <cmath>

#include "knpemi_internal.h"

#define EV_THREADS 256

namespace {

struct EvArgs {
  int n, keep, first;
  size_t nq_tot;               // stride of the ring's rows
  double t, t_prev;
  const KnEvTab* tab;
  const double* phiM;
  double* v_prev;
  uint8_t* armed;
  int* count;
  double* t_first;
  double* t_last;
  double* v_peak;
  double* t_peak;
  double* ring;
};

__global__ __launch_bounds__(EV_THREADS) void events_record_kernel(EvArgs A) {
  const int i = blockIdx.x * EV_THREADS + threadIdx.x;
  if (i >= A.n) return;
  const KnEvTab& T = *A.tab;
  int w = 0;
  while (w + 1 < T.n_watch && i >= T.gstart[w + 1]) ++w;      // at most KN_MAXSUB - 2 steps, uniform but at a boundary
  const int q = T.q0[w] + (i - T.gstart[w]);
  const double thr = T.threshold[T.sub[w]], rst = T.reset[T.sub[w]];
  const double v = A.phiM[q];
  if (A.first) {
    A.v_prev[q] = v;
    A.armed[q] = v < thr ? 1 : 0;
    A.v_peak[q] = v;
    A.t_peak[q] = A.t;
    return;
  }
  const double vp = A.v_prev[q];
  A.v_prev[q] = v;
  if (!std::isfinite(v)) return;
  bool armed = A.armed[q] != 0;
  const bool was = armed;
  if (!armed && v < rst) armed = true;
  if (armed && v >= thr) {
    const double tc = A.t_prev + (A.t - A.t_prev) * ((thr - vp) / (v - vp));
    const int n = A.count[q] + 1;
    A.count[q] = n;
    A.t_last[q] = tc;
    if (n == 1) A.t_first[q] = tc;
    if (A.keep > 0) A.ring[(size_t)((n - 1) % A.keep) * A.nq_tot + q] = tc;
    armed = false;
  }
  if (armed != was) A.armed[q] = armed ? 1 : 0;
  if (v > A.v_peak[q]) {
    A.v_peak[q] = v;
    A.t_peak[q] = A.t;
  }
}

// the state "before the first record" of every membrane dof (knpemi_events_set, knpemi_events_reset)
__global__ __launch_bounds__(EV_THREADS) void events_reset_kernel(EvArgs A) {
  const size_t q = (size_t)blockIdx.x * EV_THREADS + threadIdx.x;
  if (q >= A.nq_tot) return;
  const double nan = __builtin_nan("");
  A.v_prev[q] = nan;
  A.armed[q] = 0;
  A.count[q] = 0;
  A.t_first[q] = nan;
  A.t_last[q] = nan;
  A.v_peak[q] = nan;
  A.t_peak[q] = nan;
  for (int k = 0; k < A.keep; ++k) A.ring[(size_t)k * A.nq_tot + q] = nan;
}

EvArgs ev_args(const knpemi_handle::KnEvents& E, const KnEvSamples& V, int first, double t, double t_prev) {
  return EvArgs{E.n_grid, E.keep, first, (size_t)V.nq_tot, t, t_prev, E.tab, V.phiM, E.v_prev, E.armed,
                E.count, E.t_first, E.t_last, E.v_peak, E.t_peak, E.ring};
}

}  // namespace

int kn_launch_events_record(KnDevice* own, const knpemi_handle::KnEvents& E, const KnEvSamples& V, int first, double t,
                            double t_prev) {
  if (E.n_grid == 0) return KNPEMI_OK;
  hipLaunchKernelGGL(events_record_kernel, dim3((E.n_grid + EV_THREADS - 1) / EV_THREADS), dim3(EV_THREADS), 0,
                     own->stream, ev_args(E, V, first, t, t_prev));
  return kn_launch_check("events_record_kernel");
}

int kn_launch_events_reset(KnDevice* own, const knpemi_handle::KnEvents& E, const KnEvSamples& V) {
  const int n = V.nq_tot;
  if (n == 0) return KNPEMI_OK;
  hipLaunchKernelGGL(events_reset_kernel, dim3((n + EV_THREADS - 1) / EV_THREADS), dim3(EV_THREADS), 0, own->stream,
                     ev_args(E, V, 0, 0.0, 0.0));
  return kn_launch_check("events_reset_kernel");
}
