// Membrane monitors on gfx950: the named intermediates of the membrane models per dof, their per-dof fields and the
// series row in ONE launch per record.
//
// The models' device code computes the Nernst potentials, the conductances and the currents by mechanism inside prepare /
// rhs / rates and throws them away; membrane_monitors.h hands them out (KnMonitor<Model>::eval), and this kernel evaluates
// them from the state the next sweep would start from (include/knpemi_hip.h, "The state a monitor sees"): a private copy
// of the dof's parameter row with the traces of the vertex records in the <ion>_e / <ion>_i columns, V = phi_M, the gates
// of the state table.  It writes nothing but its own buffers.
//
// Layout.  One membrane dof per lane, 256-thread workgroups.  The grid covers the dofs of the watched (sub-domain, model)
// slots only (KnMonTab: workgroup b belongs to one watch; the model is uniform over a workgroup).  The tables are read
// [column][dof]: consecutive lanes read consecutive doubles.  With fields the selected quantities go to [quantity][n_q]
// through non-temporal stores: nothing of it is read again by the device.
//
// Reductions over a watch (integral = sum w_q v_q, average = integral / sum w_q, min, max, all over the dofs with
// w_q > 0): a fixed tree inside the workgroup -- xor butterfly over the 64 lanes of a wave, then the four waves in order
// -- one partial of KN_MON_SLOTS doubles per workgroup (only the quantities some column reduces are formed), and the tail
// of record_tail.h: the last workgroup to arrive folds the partials of every such column in workgroup order and appends
// the row, or counts it as dropped when the buffer is full.  Minimum and maximum propagate a NaN (fmin / fmax would drop
// it): a non-finite value makes the columns it enters non-finite.
//
// Point columns: the first workgroup of a watch evaluates the model at each of its points' up to 4 dofs itself (one lane per
// (point, dof), all quantities; the model is that workgroup's own, so nothing diverges), so a point column depends on no
// workgroup's per-dof field stores and exists without fields; the values travel through pt_val to the workgroup that
// writes the row as the partials do, and a column sums w_j v(q_j) in the order of the facet's dofs.
//
// Plug-in models: the body is monitor_kernel.h, compiled here with the monitors of the shipped models and by hipRTC with
// the `monitor` function a plug-in brings (kernels_rtc.hip: a program of its own per monitor source).  A record is one
// launch per run of consecutive watches of one program -- one launch for a table of shipped models; the workgroups of all
// launches of a record share the partials, the ticket and the tail.
//
// Partitioned runs (knpemi_monitor_set_partitioned): the dof weights are integrated over the facets this rank records, so
// the sums and extrema over "the dofs with w_q > 0" need no ownership test.  With rank slots (KnMonArgs::slot, a run-time
// branch: the hipRTC instantiation compiles from the same header) the last workgroup writes the folded columns, the
// averages undivided, into this rank's slots of the exchange buffer instead of appending a row; the caller sums the
// buffer over the ranks and record_combine_kernel (kernels_observe.hip) folds the ranks' slots with the column's
// operation, keeping a NaN as mon_min / mon_max do, divides the averages by the global sum of weights and appends the
// row.  A watch without a local dof has no workgroup; a run of launches without workgroups is skipped.
//
// This kernel is launch-latency bound: config 2 has 2 952 membrane dofs, 12 workgroups.
//
// Built with -ffp-contract=off (Makefile) so that the device and the host build of membrane_monitors.h share the order of
// the arithmetic; the model's kn_exp / kn_div carry their explicit fma's.
#include "knpemi_internal.h"
#include "ode_host.h"
#include "membrane_monitors.h"
#include "monitor_kernel.h"

static_assert(KN_MON_MAX == KNPEMI_MON_MAX && KN_MON_MAXW == KNPEMI_MON_MAX_WATCH && KN_MAXK == 4, "monitor limits");
static_assert(KnMonitor<ModelHHSI>::N <= KN_MON_MAX && KnMonitor<ModelGlial>::N <= KN_MON_MAX, "a selection is a 32-bit mask");

namespace {

// the quantities of dof q of a watch of a shipped model; entries at and beyond the model's count stay untouched
template <class M>
__device__ __forceinline__ void mon_eval(const OdeDev& D, const KnMonWatch& W, int q, double t, double (&out)[KN_MON_MAX]) {
  double y[M::NS], row[M::NP];
  mon_load<M::NS, M::NP>(D, W, q, y, row);
  M f;
  f.prepare(row);
  KnMonitor<M>::eval(f, t, y, out);
}

struct MonShipped {
  __device__ __forceinline__ static void eval(const OdeDev& D, const KnMonWatch& W, int q, double t, double (&out)[KN_MON_MAX]) {
    if (W.model_id == KNPEMI_MODEL_HH_SI) mon_eval<ModelHHSI>(D, W, q, t, out);
    else if (W.model_id == KNPEMI_MODEL_HH_MV) mon_eval<ModelHHMV>(D, W, q, t, out);
    else mon_eval<ModelGlial>(D, W, q, t, out);
  }
};

template <bool FIELDS>
__global__ __launch_bounds__(MON_THREADS) void monitor_kernel(OdeDev D, KnMonArgs A) {
  monitor_body<MonShipped, FIELDS>(D, A);
}

// one launch of `n_blk` workgroups from workgroup a.blk0 of the record on: the library's kernel, or (fn) a plug-in's
int launch(knpemi_handle* h, const KnMonArgs& a, int n_blk, bool fields, hipFunction_t fn) {
  const OdeDev dv = kn_ode_dev(h->sweeps);
  if (fn) return kn_rtc_launch_monitor(h->stream, fn, (unsigned)n_blk, MON_THREADS, dv, a);
  if (fields) hipLaunchKernelGGL((monitor_kernel<true>), dim3(n_blk), dim3(MON_THREADS), 0, h->stream, dv, a);
  else hipLaunchKernelGGL((monitor_kernel<false>), dim3(n_blk), dim3(MON_THREADS), 0, h->stream, dv, a);
  return kn_launch_check("monitor_kernel");
}

}  // namespace

int kn_launch_monitor(knpemi_handle* h, double t, int write_fields) {
  const auto& X = h->mon;
  const int f = write_fields ? 1 : 0;
  const KnMonTab& T = X.host;
  KnMonArgs a{X.tab, reinterpret_cast<const int*>(X.cols), X.pt_watch, X.pt_q, X.pt_w, X.pt_val, X.part, X.ser.ctl, X.ser.rows,
              write_fields ? X.fields.fld : nullptr, X.slots.xbuf ? X.slots.xbuf + (size_t)X.slots.rank * T.n_cols : nullptr,
              X.ser.capacity, 0, X.n_blk, t};
  for (int w0 = 0; w0 < T.n_watch;) {      // runs of consecutive watches of one program
    int w1 = w0 + 1;
    while (w1 < T.n_watch && X.fn[w1][f] == X.fn[w0][f]) ++w1;
    a.blk0 = T.bstart[w0];
    const int n_blk = T.bstart[w1] - T.bstart[w0];
    if (n_blk == 0) { w0 = w1; continue; }      // partitioned: watches without a local dof
    if (int rc = launch(h, a, n_blk, f != 0, X.fn[w0][f])) {
      // the launches of this record that did not happen took no ticket: start the next record's count from zero
      (void)hipMemsetAsync(X.ser.ctl + 2, 0, sizeof(unsigned long long), h->stream);
      return rc;
    }
    w0 = w1;
  }
  return KNPEMI_OK;
}

int kn_launch_monitor_eval(knpemi_handle* h, const KnMonTab* d_tab, int nq, double t, double* fld, hipFunction_t fn) {
  const int n_blk = (nq + MON_THREADS - 1) / MON_THREADS;
  const KnMonArgs a{d_tab, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, fld, nullptr, 0, 0, n_blk, t};
  return launch(h, a, n_blk, true, fn);
}

extern "C" int kn_monitor_fold_depth() { return MON_FOLD_DEPTH; }
extern "C" int kn_monitor_chunk() { return MON_THREADS; }
extern "C" int knpemi_monitor_count(int model_id) { return kn_monitor_count(model_id); }
extern "C" const char* knpemi_monitor_name(int model_id, int i) { return kn_monitor_name(model_id, i); }
