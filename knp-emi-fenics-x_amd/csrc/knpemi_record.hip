// The on-device recorders behind the C ABI (include/knpemi_hip.h): observables (kernels_observe.hip), membrane events
// (kernels_events.hip), ion fluxes per cell (kernels_flux.hip), the membrane exchange per cell (kernels_exchange.hip) and
// the field maps (kernels_maps.hip: per-item maps as the events, and a series with a series watch), and the membrane
// monitors (kernels_monitor.hip: a series and per-dof fields of the models' named intermediates).
//
// All but the events append rows to a series buffer (KnSeries; the device side is record_tail.h; the maps only with a
// series watch).  The fluxes and the exchange are one recorder over different items -- the cells of a watched sub-domain,
// the membrane facets of a watched cell: they share KnWatched, KnWatchTab and every routine but the launch, and a
// WatchKind names what differs.  The membrane events keep per-dof maps and no series.
//
// What several recorders need is written once, as a small struct of the handle and its routines below: the install rule of
// every knpemi_*_set (New, recorder_install), the rank slots of a partitioned record (KnRankSlots: observables, fluxes,
// exchange, monitors, the maps' series -- the record launch writes the rank's partial row into its slots of an exchange
// buffer, slots_sum sums the buffer over the ranks, and record_combine_kernel (kernels_observe.hip) folds the slots in
// rank order and appends the row), the clock of the recorders that integrate between two records (KnRecordClock: events, maps) and the per-item
// fields (KnItemFields: fluxes, exchange, monitors).
//
// The observables and the membrane events also record on a DG handle (knpemi_dg_observe_*, knpemi_dg_events_*, at the end
// of this file): the routines they need take the owner (KnDevice*: device, main stream) and are generic over the handle
// type that holds the recorder's state; what differs per handle is where a field lives (observe_build's `locate`) and
// which array the events sample (KnEvSamples).  The field snapshots of both handles (knpemi_snapshot_*, knpemi_dg_snapshot_*)
// share the ring -- copy stream, pinned frames, take -- as KnFrameRing and the ring_* routines; the tables and the pack
// kernels are each handle's own.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <string>
#include <vector>

#include "knpemi_internal.h"
#include "dg_internal.h"

int kn_observe_chunk();
extern "C" int kn_flux_chunk();
extern "C" int kn_exchange_chunk();
extern "C" int kn_monitor_chunk();

namespace {
using KnSeries = knpemi_handle::KnSeries;
using KnWatched = knpemi_handle::KnWatched;

int series_alloc(std::vector<void*>& owner, hipStream_t st, int capacity, int n_cols, KnSeries* S) {
  if (int rc = kn_zeros(owner, st, 4, &S->ctl)) return rc;
  if (int rc = kn_zeros(owner, st, (size_t)capacity * n_cols, &S->rows)) return rc;
  S->capacity = capacity; S->n_cols = n_cols;
  return KNPEMI_OK;
}

// a new series: rows written and rows dropped back to 0, stream-ordered (no synchronisation)
int series_rewind(KnDevice* h, KnSeries& S) {
  KN_HIP(hipMemsetAsync(S.ctl, 0, 2 * sizeof(unsigned long long), h->stream));
  return KNPEMI_OK;
}

// knpemi_*_read: the first min(n_rows, rows written) rows and the two counters; reset: rewind, synchronised
int series_read(KnDevice* h, KnSeries& S, bool set, const char* fn, const char* none, int n_rows, double* out,
                int64_t* rows, int64_t* overflow, int reset) {
  if (!set) return kn_fail(KNPEMI_EINVAL, std::string(fn) + ": " + none);
  if (n_rows < 0 || (n_rows > 0 && !out)) return kn_fail(KNPEMI_EINVAL, std::string(fn) + ": bad output buffer");
  KN_HIP(hipSetDevice(h->device));
  unsigned long long ctl[4];
  int rc;
  if ((rc = kn_to_host(h->stream, ctl, S.ctl, 4))) return rc;
  const size_t n = std::min<size_t>((size_t)n_rows, (size_t)ctl[0]);
  if (n && (rc = kn_to_host(h->stream, out, S.rows, n * S.n_cols))) return rc;
  if (rows) *rows = (int64_t)ctl[0];
  if (overflow) *overflow = (int64_t)ctl[1];
  if (reset) {
    if ((rc = series_rewind(h, S))) return rc;
    KN_HIP(hipStreamSynchronize(h->stream));
  }
  return KNPEMI_OK;
}

// free what a recorder's `allocs` holds and forget it; knpemi_*_clear waits for the enqueued records first
template <class R>
void recorder_free(R& rec) {
  kn_free_all(rec.allocs);
  rec = R{};
}
// the snapshots of either handle own more than device memory: the copy stream (waited for first: a copy may be in
// flight), the events and the pinned frames of their ring
void ring_free(KnFrameRing& R) {
  if (R.copy) (void)hipStreamSynchronize(R.copy);
  for (hipEvent_t e : R.copied) (void)hipEventDestroy(e);
  if (R.ev_packed) (void)hipEventDestroy(R.ev_packed);
  for (char* p : R.pinned) (void)hipHostFree(p);
  if (R.copy) (void)hipStreamDestroy(R.copy);
}
void recorder_free(knpemi_handle::KnSnap& S) {
  ring_free(S);
  kn_free_all(S.allocs);
  S = knpemi_handle::KnSnap{};
}
void recorder_free(KnDgSnap& S) {
  ring_free(S);
  kn_free_all(S.allocs);
  S = KnDgSnap{};
}
template <class H, class R>
int recorder_clear(H* h, R H::*which) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  KN_HIP(hipSetDevice(h->device));
  KN_HIP(hipStreamSynchronize(h->stream));
  recorder_free(h->*which);
  return KNPEMI_OK;
}
// The install rule of every knpemi_*_set: the new recorder is built in a local New<R>, whose allocations go to its own
// `allocs`.  A return before recorder_install frees what it owns, and the previous recorder is untouched and still records;
// recorder_install frees the previous one, which an enqueued record may still read, behind a synchronisation and moves
// the new one in.
template <class R>
struct New : R {
  ~New() { recorder_free(static_cast<R&>(*this)); }
};
template <class H, class R>
int recorder_install(H* h, R H::*which, New<R>& next) {
  KN_HIP(hipStreamSynchronize(h->stream));
  recorder_free(h->*which);
  h->*which = next;
  static_cast<R&>(next) = R{};      // the handle owns it now
  return KNPEMI_OK;
}

// -- a partitioned record's rank slots (KnRankSlots); max_cols: the caller's bound on the columns of one rank
using KnRankSlots = knpemi_handle::KnRankSlots;
int slots_check(const knpemi_handle* h, const std::string& fn, const KnRankSlots& s, size_t max_cols) {
  if (s.world < 1 || s.rank < 0 || s.rank >= s.world) return kn_fail(KNPEMI_EINVAL, fn + ": bad rank / world");
  if (!s.xbuf) return kn_fail(KNPEMI_EINVAL, fn + ": exchange buffer is required");
  if (!s.allreduce && !h->comm)
    return kn_fail(KNPEMI_EINVAL, fn + ": no all-reduce hook and no library communicator (knpemi_comm_init)");
  if ((size_t)s.world * max_cols > (size_t)INT32_MAX) return kn_fail(KNPEMI_EINVAL, fn + ": exchange buffer too large");
  return KNPEMI_OK;
}
// all zero: this rank's slots are written by the records (never, without local items), the others' by the sum
int slots_attach(knpemi_handle* h, KnRankSlots* to, const KnRankSlots& s, int n_cols) {
  *to = s;
  KN_HIP(hipMemsetAsync(s.xbuf, 0, (size_t)s.world * n_cols * sizeof(double), h->stream));
  KN_HIP(hipStreamSynchronize(h->stream));
  return KNPEMI_OK;
}
// between the record launch, which has written this rank's slots, and the combine launch: the sum over the ranks
int slots_sum(knpemi_handle* h, const std::string& fn, const KnRankSlots& s, int n_cols) {
  const int n = s.world * n_cols;
  if (!s.allreduce) return knpemi_comm_allreduce(h, s.xbuf, n);
  return s.allreduce(s.ctx, n) ? kn_fail(KNPEMI_EHIP, fn + ": allreduce hook failed") : KNPEMI_OK;
}

// -- the record clock (KnRecordClock)
using KnRecordClock = knpemi_handle::KnRecordClock;
int clock_accept(const KnRecordClock& c, const char* fn, double t) {
  if (!std::isfinite(t) || (c.have_prev && !(t > c.t_prev)))
    return kn_fail(KNPEMI_EINVAL, std::string(fn) + ": t must be finite and greater than the previous record's");
  return KNPEMI_OK;
}
void clock_advance(KnRecordClock& c, double t) { c = {true, t}; }
void clock_restart(KnRecordClock& c) { c = {}; }

// -- per-item fields (KnItemFields)
using KnItemFields = knpemi_handle::KnItemFields;
// a record launch: the first one that writes the fields allocates them, in the recorder's `owner`
template <class Launch>
int fields_record(KnItemFields& F, std::vector<void*>& owner, int write_fields, Launch launch) {
  if (write_fields && !F.fld)
    if (int rc = kn_alloc(owner, std::max<size_t>(F.fld_len, 1), &F.fld)) return rc;
  if (int rc = launch()) return rc;
  if (write_fields) F.fld_valid = true;
  return KNPEMI_OK;
}
// a new series: the fields of the old one are forgotten
void fields_forget(KnItemFields& F) { F.fld_valid = false; }
// knpemi_*_fields; record_call: the call that writes them
int fields_recorded(const KnItemFields& F, const std::string& fn, const std::string& record_call) {
  return F.fld_valid ? KNPEMI_OK : kn_fail(KNPEMI_EINVAL, fn + ": no record with fields yet (" + record_call + ")");
}
}  // namespace

void kn_record_free(knpemi_handle* h) {
  for (auto* a : {&h->obs.allocs, &h->events.allocs, &h->flux.allocs, &h->exchange.allocs, &h->maps.allocs, &h->mon.allocs})
    kn_free_all(*a);
  recorder_free(h->snap);
}

// ---------------------------------------------------------------------------------------------------
// observables (kernels_observe.hip)
// ---------------------------------------------------------------------------------------------------
namespace {
// The table of knpemi_observe_set, knpemi_observe_set_partitioned (`partitioned`: an observable may have no entries) and
// knpemi_dg_observe_set, validated on the host and built in O for recorder_install.  locate(o, field, sub, ix, &loc): where
// observable o's field lives on the owner's device, or the owner's refusal; finite: weights and denominators must be finite.
template <class Locate>
int observe_build(KnDevice* own, const std::string& fn, int n_obs, const int32_t* spec, const int64_t* ptr, const int32_t* idx,
                  const double* w, const double* denom, int capacity, bool partitioned, bool finite, Locate locate,
                  knpemi_handle::KnObserve& O) {
  if (n_obs < 1 || capacity < 1) return kn_fail(KNPEMI_EINVAL, fn + ": n_obs and capacity must be positive");
  if (ptr[0] != 0) return kn_fail(KNPEMI_EINVAL, fn + ": ptr[0] must be 0");
  if (ptr[n_obs] > 0 && (!idx || !w)) return kn_fail(KNPEMI_EINVAL, fn + ": null argument");
  const int chunk = kn_observe_chunk();
  std::vector<int4> blk;
  std::vector<int> blk_ptr(1, 0), op(n_obs), stride(n_obs);
  std::vector<const double*> base(n_obs);
  for (int o = 0; o < n_obs; ++o) {
    const int32_t field = spec[4 * o], sub = spec[4 * o + 1], ix = spec[4 * o + 2], oo = spec[4 * o + 3];
    if (oo != KNPEMI_OBS_SUM && oo != KNPEMI_OBS_MIN && oo != KNPEMI_OBS_MAX)
      return kn_fail(KNPEMI_EINVAL, fn + ": unknown op of observable " + std::to_string(o));
    if ((partitioned ? ptr[o + 1] < ptr[o] : ptr[o + 1] <= ptr[o]) || ptr[o + 1] > (int64_t)INT32_MAX)
      return kn_fail(KNPEMI_EINVAL, fn + ": observable " + std::to_string(o) + (partitioned ? " has a bad entry range" : " has no entries"));
    KnFieldLoc L;
    int rc = locate(o, field, sub, ix, &L);
    if (rc) return rc;
    if (finite && !std::isfinite(denom[o]))
      return kn_fail(KNPEMI_EINVAL, fn + ": denominator of observable " + std::to_string(o) + " is not finite");
    for (int64_t e = ptr[o]; e < ptr[o + 1]; ++e) {      // every read of the kernel stays inside the field
      if (idx[e] < 0 || (size_t)idx[e] >= L.n)
        return kn_fail(KNPEMI_EINVAL, fn + ": index out of range in observable " + std::to_string(o));
      if (finite && !std::isfinite(w[e]))
        return kn_fail(KNPEMI_EINVAL, fn + ": weight of observable " + std::to_string(o) + " is not finite");
    }
    op[o] = oo; stride[o] = L.stride; base[o] = L.base;
    for (int64_t e = ptr[o]; e < ptr[o + 1]; e += chunk)
      blk.push_back(make_int4(o, (int)e, (int)std::min<int64_t>(e + chunk, ptr[o + 1]), 0));
    blk_ptr.push_back((int)blk.size());
  }
  KN_HIP(hipSetDevice(own->device));
  const size_t ne = (size_t)ptr[n_obs];
  int rc;
  auto& A = O.allocs;
  if ((rc = kn_upload(A, blk, &O.blk)) || (rc = kn_upload(A, blk_ptr, &O.blk_ptr)) || (rc = kn_upload(A, op, &O.op))
      || (rc = kn_upload(A, stride, &O.stride)) || (rc = kn_upload(A, base, &O.base))
      || (rc = kn_upload(A, denom, (size_t)n_obs, &O.denom))
      || (rc = kn_upload(A, reinterpret_cast<const int*>(idx), ne, &O.idx)) || (rc = kn_upload(A, w, ne, &O.w)))
    return rc;
  if (kn_alloc(A, blk.size(), &O.part)) return kn_fail(KNPEMI_ENOMEM, fn + ": partials");
  if (series_alloc(A, own->stream, capacity, n_obs, &O.ser)) return kn_fail(KNPEMI_ENOMEM, fn + ": buffer");
  O.n_obs = n_obs; O.n_blk = (int)blk.size();
  return KNPEMI_OK;
}

// knpemi_observe_set and, with `part`, knpemi_observe_set_partitioned, whose table may hold observables without entries
int observe_set(knpemi_handle* h, const char* who, int n_obs, const int32_t* spec, const int64_t* ptr, const int32_t* idx,
                const double* w, const double* denom, int capacity, const KnRankSlots* part = nullptr) {
  const std::string fn(who);
  const bool partitioned = part != nullptr;
  if (!h || !spec || !ptr || !denom || (!partitioned && (!idx || !w))) return kn_fail(KNPEMI_EINVAL, fn + ": null argument");
  if (h->ode_only) return kn_fail(KNPEMI_EINVAL, fn + ": a handle of knpemi_ode_create has no fields");
  New<knpemi_handle::KnObserve> O;
  auto locate = [&](int, int field, int sub, int ix, KnFieldLoc* L) { return kn_locate(h, field, sub, ix, L); };
  int rc = observe_build(h, fn, n_obs, spec, ptr, idx, w, denom, capacity, partitioned, false, locate, O);
  if (rc) return rc;
  if (part && (rc = slots_attach(h, &O.slots, *part, n_obs))) return rc;
  return recorder_install(h, &knpemi_handle::obs, O);
}
}  // namespace

extern "C" int knpemi_observe_set(knpemi_handle* h, int n_obs, const int32_t* spec, const int64_t* ptr,
                                  const int32_t* idx, const double* w, const double* denom, int capacity) {
  return observe_set(h, "knpemi_observe_set", n_obs, spec, ptr, idx, w, denom, capacity);
}

extern "C" int knpemi_observe_set_partitioned(knpemi_handle* h, int n_obs, const int32_t* spec, const int64_t* ptr,
                                              const int32_t* idx, const double* w, const double* denom, int capacity,
                                              int rank, int world, void* xbuf_dev, knpemi_allreduce_fn allreduce,
                                              void* ctx) {
  const char* fn = "knpemi_observe_set_partitioned";
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  const KnRankSlots part{static_cast<double*>(xbuf_dev), rank, world, allreduce, ctx};
  if (int rc = slots_check(h, fn, part, (size_t)std::max(n_obs, 0))) return rc;
  return observe_set(h, fn, n_obs, spec, ptr, idx, w, denom, capacity, &part);
}

extern "C" int knpemi_observe_record(knpemi_handle* h) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  auto& O = h->obs;
  if (O.n_obs == 0) return kn_fail(KNPEMI_EINVAL, "knpemi_observe_record: no observables set");
  KN_HIP(hipSetDevice(h->device));
  int rc = kn_launch_observe(h, O);
  if (rc || !O.slots.xbuf) return rc;
  // partitioned: this rank's slots are written; sum the exchange buffer over the ranks, then fold and append
  if ((rc = slots_sum(h, "knpemi_observe_record", O.slots, O.n_obs))) return rc;
  return kn_launch_observe_combine(h);
}

extern "C" int knpemi_observe_read(knpemi_handle* h, int n_rows, double* out, int64_t* rows, int64_t* overflow,
                                   int reset) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  return series_read(h, h->obs.ser, h->obs.n_obs != 0, "knpemi_observe_read", "no observables set", n_rows, out, rows, overflow, reset);
}

extern "C" int knpemi_observe_clear(knpemi_handle* h) { return recorder_clear(h, &knpemi_handle::obs); }

// ---------------------------------------------------------------------------------------------------
// membrane events (kernels_events.hip)
// ---------------------------------------------------------------------------------------------------
namespace {
// the table and the state arrays over the owner's nq concatenated membrane dofs, in E for recorder_install
int events_build(const KnEvTab& T, size_t nq, int keep, const bool* watched, knpemi_handle::KnEvents& E) {
  auto& A = E.allocs;
  int rc;
  if ((rc = kn_upload(A, &T, 1, &E.tab)) || (rc = kn_alloc(A, nq, &E.v_prev)) || (rc = kn_alloc(A, nq, &E.armed))
      || (rc = kn_alloc(A, nq, &E.count)) || (rc = kn_alloc(A, nq, &E.t_first)) || (rc = kn_alloc(A, nq, &E.t_last))
      || (rc = kn_alloc(A, nq, &E.v_peak)) || (rc = kn_alloc(A, nq, &E.t_peak))
      || (rc = kn_alloc(A, nq * (size_t)keep, &E.ring)))
    return rc;
  E.n_watch = T.n_watch; E.keep = keep; E.n_grid = T.gstart[T.n_watch];
  std::copy(watched, watched + KN_MAXSUB, E.watched);
  return KNPEMI_OK;
}
// the maps of the nq dofs from q0 on, of nq_tot, synchronised; every pointer may be NULL
int events_copy_out(KnDevice* own, const knpemi_handle::KnEvents& E, size_t q0, size_t nq, size_t nq_tot, int32_t* count,
                    double* t_first, double* t_last, double* v_peak, double* t_peak, double* ring) {
  KN_HIP(hipSetDevice(own->device));
  if (nq) {
    auto copy = [&](auto* host, const auto* dev, size_t n) -> int {
      if (host) KN_HIP(hipMemcpyAsync(host, dev, n * sizeof(*host), hipMemcpyDeviceToHost, own->stream));
      return KNPEMI_OK;
    };
    int rc;
    if ((rc = copy(count, E.count + q0, nq)) || (rc = copy(t_first, E.t_first + q0, nq))
        || (rc = copy(t_last, E.t_last + q0, nq)) || (rc = copy(v_peak, E.v_peak + q0, nq))
        || (rc = copy(t_peak, E.t_peak + q0, nq)))
      return rc;
    for (int k = 0; ring && k < E.keep; ++k)          // row k of the ring: this piece of [keep][nq_tot]
      if ((rc = copy(ring + (size_t)k * nq, E.ring + (size_t)k * nq_tot + q0, nq))) return rc;
  }
  KN_HIP(hipStreamSynchronize(own->stream));
  return KNPEMI_OK;
}
}  // namespace

extern "C" int knpemi_events_set(knpemi_handle* h, int n_watch, const int32_t* sub, const double* threshold,
                                 const double* reset, int keep) {
  const std::string fn = "knpemi_events_set";
  if (!h || !sub || !threshold) return kn_fail(KNPEMI_EINVAL, fn + ": null argument");
  if (n_watch < 1 || n_watch > KN_MAXSUB - 1) return kn_fail(KNPEMI_EINVAL, fn + ": 1 to KNPEMI_MAX_SUB - 1 sub-domains");
  if (keep < 0 || keep > KNPEMI_EVENTS_MAX_KEEP) return kn_fail(KNPEMI_EINVAL, fn + ": keep must be in 0..KNPEMI_EVENTS_MAX_KEEP");
  KnEvTab T{};
  bool watched[KN_MAXSUB] = {};
  for (int w = 0; w < n_watch; ++w) {
    const int s = sub[w];
    if (s < 1 || s >= h->n_sub) return kn_fail(KNPEMI_EINVAL, fn + ": bad sub-domain index (the ECS has no membrane space)");
    if (watched[s]) return kn_fail(KNPEMI_EINVAL, fn + ": sub-domain " + std::to_string(s) + " is listed twice");
    const double thr = threshold[w], rst = reset ? reset[w] : thr;
    if (!(rst <= thr)) return kn_fail(KNPEMI_EINVAL, fn + ": reset must not exceed the threshold");
    watched[s] = true;
    T.gstart[w + 1] = T.gstart[w] + h->n_q[s];
    T.q0[w] = h->qoff[s];
    T.sub[w] = s;
    T.threshold[s] = thr;
    T.reset[s] = rst;
  }
  T.n_watch = n_watch;
  KN_HIP(hipSetDevice(h->device));
  New<knpemi_handle::KnEvents> E;
  int rc;
  if ((rc = events_build(T, (size_t)h->dev.NQtot, keep, watched, E))) return rc;
  if ((rc = recorder_install(h, &knpemi_handle::events, E))) return rc;
  if ((rc = kn_launch_events_reset(h, h->events, {h->dev.phiM, h->dev.NQtot}))) recorder_free(h->events);
  return rc;
}

extern "C" int knpemi_events_record(knpemi_handle* h, double t) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  auto& E = h->events;
  if (E.n_watch == 0) return kn_fail(KNPEMI_EINVAL, "knpemi_events_record: no events set (knpemi_events_set)");
  if (int rc = clock_accept(E.clock, "knpemi_events_record", t)) return rc;
  KN_HIP(hipSetDevice(h->device));
  if (int rc = kn_launch_events_record(h, E, {h->dev.phiM, h->dev.NQtot}, E.clock.have_prev ? 0 : 1, t, E.clock.t_prev)) return rc;
  clock_advance(E.clock, t);
  return KNPEMI_OK;
}

extern "C" int knpemi_events_read(knpemi_handle* h, int sub, int32_t* count, double* t_first, double* t_last,
                                  double* v_peak, double* t_peak, double* ring) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  auto& E = h->events;
  if (E.n_watch == 0) return kn_fail(KNPEMI_EINVAL, "knpemi_events_read: no events set (knpemi_events_set)");
  if (sub < 1 || sub >= h->n_sub || !E.watched[sub])
    return kn_fail(KNPEMI_EINVAL, "knpemi_events_read: sub-domain is not watched");
  return events_copy_out(h, E, (size_t)h->qoff[sub], (size_t)h->n_q[sub], (size_t)h->dev.NQtot, count, t_first, t_last, v_peak,
                         t_peak, ring);
}

extern "C" int knpemi_events_reset(knpemi_handle* h) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  auto& E = h->events;
  if (E.n_watch == 0) return kn_fail(KNPEMI_EINVAL, "knpemi_events_reset: no events set (knpemi_events_set)");
  KN_HIP(hipSetDevice(h->device));
  clock_restart(E.clock);
  return kn_launch_events_reset(h, E, {h->dev.phiM, h->dev.NQtot});
}

extern "C" int knpemi_events_clear(knpemi_handle* h) { return recorder_clear(h, &knpemi_handle::events); }

// ---------------------------------------------------------------------------------------------------
// ion fluxes and current density per cell (kernels_flux.hip), membrane ion exchange per cell (kernels_exchange.hip)
// ---------------------------------------------------------------------------------------------------
namespace {
// what differs between the two: the names in the messages, the items, and the sizes
struct WatchKind {
  const char* name;        // the entry points are knpemi_<name>_*
  const char* none;        // the message of a call before knpemi_<name>_set
  const char* watch;       // what one watch is ...
  const char* items;       // ... and what its items are
  const char* bad_sub;     // the message of a sub-domain index out of range
  const char* current;     // what bit 8 of an ion mask selects
  bool ecs;                // sub-domain 0 may be watched
  int slots;               // doubles per workgroup partial
  KnWatched knpemi_handle::*state;
  int (*launch)(knpemi_handle*, int);
  bool after_ode;          // the record reads phi_M and I_ch, which the ODE sweeps may write on the auxiliary streams
  const char* combine;     // the combine launch of a partitioned record in error messages
};
const WatchKind FLUX{"flux", "no fluxes set (knpemi_flux_set)", "sub-domain", "cells", "bad sub-domain index", "the current",
                     true, KN_FLUX_SLOTS, &knpemi_handle::flux, kn_launch_flux, false, "record_combine_kernel (fluxes)"};
const WatchKind EXCHANGE{"exchange", "no exchange set (knpemi_exchange_set)", "cell", "membrane facets",
                         "unknown cell (bad sub-domain index)", "the current columns", false, KN_EX_SLOTS,
                         &knpemi_handle::exchange, kn_launch_exchange, true, "record_combine_kernel (exchange)"};

inline std::string entry(const WatchKind& k, const char* what) { return std::string("knpemi_") + k.name + "_" + what; }
inline int popcount(int m) { int n = 0; for (; m; m &= m - 1) ++n; return n; }
inline int ions_below(int m, int ion) { return popcount(m & (ion == -1 ? 0xFF : (1 << ion) - 1)); }

// what knpemi_<name>_set_partitioned adds to knpemi_<name>_set
struct WatchPart {
  const uint8_t* recorded;
  KnRankSlots slots;
};

// knpemi_<name>_set and, with `part`, knpemi_<name>_set_partitioned: a watch may then have no local item (no workgroup,
// zeros in this rank's slots).  off / count: first item and number of items of every sub-domain; chunk: items per workgroup;
// ion_fld / cur_fld: field doubles per item of a watched ion / of the current; cols(mask, emit): the columns of one
// watch, in row order, as emit(slot, is_max).  A refused call leaves the previous table alone.
template <class Cols>
int watched_set(knpemi_handle* h, const WatchKind& k, const std::vector<int>& off, const std::vector<int>& count, int chunk,
                int ion_fld, int cur_fld, Cols cols, int n_watch, const int32_t* sub, const int32_t* ion_mask, int capacity,
                const WatchPart* part = nullptr) {
  const std::string fn = entry(k, part ? "set_partitioned" : "set");
  if (!h || !sub || !ion_mask) return kn_fail(KNPEMI_EINVAL, fn + ": null argument");
  if (part) {
    if (int rc = slots_check(h, fn, part->slots, KN_WATCH_MAXCOLS)) return rc;
    if (!part->recorded) return kn_fail(KNPEMI_EINVAL, fn + ": the recorded mask is required");
  }
  if (h->ode_only) return kn_fail(KNPEMI_EINVAL, fn + ": a handle of knpemi_ode_create has no fields");
  if (n_watch < 1 || n_watch > KN_MAXSUB) return kn_fail(KNPEMI_EINVAL, fn + ": 1 to KNPEMI_MAX_SUB " + k.watch + "s");
  if (capacity < 1) return kn_fail(KNPEMI_EINVAL, fn + ": capacity must be positive");
  KnWatchTab T{};
  int watch_of[KN_MAXSUB];
  std::fill(watch_of, watch_of + KN_MAXSUB, -1);
  long long fbase = 0, n_items = 0;
  int col = 0;
  for (int w = 0; w < n_watch; ++w) {
    const int s = sub[w], m = ion_mask[w];
    if (s == 0 && !k.ecs) return kn_fail(KNPEMI_EINVAL, fn + ": the ECS (sub-domain 0) has no membrane of its own: watch the cells");
    if (s < 0 || s >= h->n_sub) return kn_fail(KNPEMI_EINVAL, fn + ": " + k.bad_sub);
    if (watch_of[s] >= 0) return kn_fail(KNPEMI_EINVAL, fn + ": " + k.watch + " " + std::to_string(s) + " is listed twice");
    if (count[s] < (part ? 0 : 1)) return kn_fail(KNPEMI_EINVAL, fn + ": " + k.watch + " " + std::to_string(s) + " has no " + k.items);
    if (m == 0) return kn_fail(KNPEMI_EINVAL, fn + ": empty ion mask");
    if (m & ~(KN_WATCH_CURRENT | ((1 << h->K) - 1)))
      return kn_fail(KNPEMI_EINVAL, fn + ": ion mask has bits at or above the number of ions (bit 8: " + k.current + ")");
    watch_of[s] = w;
    T.sub[w] = s; T.mask[w] = m; T.first[w] = off[s]; T.count[w] = count[s];
    T.bstart[w + 1] = T.bstart[w] + (count[s] + chunk - 1) / chunk;
    T.fbase[w] = fbase;
    T.ibase[w] = (int)n_items;
    n_items += count[s];
    fbase += (long long)(ion_fld * popcount(m & 0xFF) + ((m & KN_WATCH_CURRENT) ? cur_fld : 0)) * count[s];
    cols(m, [&](int slot, bool is_max) {
      T.col_watch[col] = (uint8_t)w; T.col_slot[col] = (uint8_t)slot; T.col_max[col] = is_max;
      ++col;
    });
  }
  T.n_watch = n_watch; T.n_cols = col;
  if (n_items > (long long)INT32_MAX) return kn_fail(KNPEMI_EINVAL, fn + ": too many " + k.items);
  KN_HIP(hipSetDevice(h->device));
  New<KnWatched> X;
  const int n_blk = T.bstart[n_watch];
  int rc;
  if ((rc = kn_upload(X.allocs, &T, 1, &X.tab)) || (rc = kn_alloc(X.allocs, (size_t)n_blk * k.slots, &X.part))
      || (rc = series_alloc(X.allocs, h->stream, capacity, col, &X.ser)))
    return rc;
  if (part) {
    if (n_items && (rc = kn_upload(X.allocs, part->recorded, (size_t)n_items, &X.recorded))) return rc;
    if ((rc = slots_attach(h, &X.slots, part->slots, col))) return rc;
  }
  X.host = T; X.n_watch = n_watch; X.n_blk = n_blk; X.fields.fld_len = (size_t)fbase;
  std::copy(watch_of, watch_of + KN_MAXSUB, X.watch_of);
  return recorder_install(h, k.state, X);
}

// knpemi_<name>_record
int watched_record(knpemi_handle* h, const WatchKind& k, int write_fields) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  KnWatched& X = h->*k.state;
  if (X.n_watch == 0) return kn_fail(KNPEMI_EINVAL, entry(k, "record") + ": " + k.none);
  if (!h->have_params) return kn_fail(KNPEMI_EINVAL, entry(k, "record") + ": knpemi_set_params not called");
  KN_HIP(hipSetDevice(h->device));
  if (k.after_ode)
    if (int rc = kn_wait_ode_joins(h)) return rc;
  if (int rc = fields_record(X.fields, X.allocs, write_fields, [&] { return k.launch(h, write_fields); })) return rc;
  if (!X.slots.xbuf) return KNPEMI_OK;
  // partitioned: this rank's slots are written; sum the exchange buffer over the ranks, then fold and append
  if (int rc = slots_sum(h, entry(k, "record"), X.slots, X.ser.n_cols)) return rc;
  return kn_launch_record_combine(h, k.combine, X.ser.n_cols, X.ser.capacity, X.slots.world, X.slots.rank, nullptr, nullptr,
                                  reinterpret_cast<const uint8_t*>(X.tab) + offsetof(KnWatchTab, col_max), X.slots.xbuf,
                                  X.ser.ctl, X.ser.rows);
}

// knpemi_<name>_reset: a new series, stream-ordered; the fields of the old one are forgotten
int watched_reset(knpemi_handle* h, const WatchKind& k) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  KnWatched& X = h->*k.state;
  if (X.n_watch == 0) return kn_fail(KNPEMI_EINVAL, entry(k, "reset") + ": " + k.none);
  KN_HIP(hipSetDevice(h->device));
  fields_forget(X.fields);
  return series_rewind(h, X.ser);
}

// knpemi_<name>_fields, first half: the watch of `sub` in *w
int fields_watch(knpemi_handle* h, const WatchKind& k, int sub, const double* host, int* w) {
  const std::string fn = entry(k, "fields");
  if (!h || !host) return kn_fail(KNPEMI_EINVAL, fn + ": null argument");
  const KnWatched& X = h->*k.state;
  if (X.n_watch == 0) return kn_fail(KNPEMI_EINVAL, fn + ": " + k.none);
  if (sub < 0 || sub >= h->n_sub || X.watch_of[sub] < 0) return kn_fail(KNPEMI_EINVAL, fn + ": " + k.watch + " is not watched");
  *w = X.watch_of[sub];
  return KNPEMI_OK;
}
// ... the ion (-1: the current) is one of watch w
int fields_ion(knpemi_handle* h, const WatchKind& k, int w, int ion) {
  const int m = (h->*k.state).host.mask[w];
  if (ion == -1 ? !(m & KN_WATCH_CURRENT) : (ion < 0 || ion >= h->K || !((m >> ion) & 1)))
    return kn_fail(KNPEMI_EINVAL, entry(k, "fields") + ": " + (ion == -1 ? k.current : "this ion") + " of the " + k.watch
                                      + " is not watched");
  return KNPEMI_OK;
}
// ... and second half: n doubles from `offset` of watch w's fields; `want`: the length they have, `length`: in words
int fields_copy(knpemi_handle* h, const WatchKind& k, int w, size_t offset, double* host, size_t n, size_t want,
                const char* length) {
  const std::string fn = entry(k, "fields");
  const KnWatched& X = h->*k.state;
  if (int rc = fields_recorded(X.fields, fn, entry(k, "record") + "(h, 1)")) return rc;
  if (n != want) return kn_fail(KNPEMI_EINVAL, fn + ": length is not " + length);
  if (n == 0) return KNPEMI_OK;      // partitioned: no local item
  KN_HIP(hipSetDevice(h->device));
  return kn_to_host(h->stream, host, X.fields.fld + X.host.fbase[w] + offset, n);
}
}  // namespace

namespace {
int flux_set(knpemi_handle* h, int n_watch, const int32_t* sub, const int32_t* ion_mask, int capacity, const WatchPart* part) {
  if (!h) return kn_fail(KNPEMI_EINVAL, entry(FLUX, part ? "set_partitioned" : "set") + ": null argument");
  const int K = h->K, gd = h->gdim, per_ion = 2 * gd + 1;
  // per watched ion {sum vol J_diff}, {sum vol J_drift}, max |J|; with the current {sum vol i}, max |i|
  auto cols = [&](int m, auto emit) {
    for (int k = 0; k < K; ++k)
      if ((m >> k) & 1)
        for (int j = 0; j < per_ion; ++j) emit(k * per_ion + j, j == 2 * gd);
    if (m & KN_WATCH_CURRENT)
      for (int j = 0; j <= gd; ++j) emit(KN_MAXK * per_ion + j, j == gd);
  };
  return watched_set(h, FLUX, h->coff, h->n_cell, kn_flux_chunk(), 2 * gd, 2 * gd, cols, n_watch, sub, ion_mask, capacity, part);
}

int exchange_set(knpemi_handle* h, int n_watch, const int32_t* sub, const int32_t* ion_mask, int capacity, const WatchPart* part) {
  if (!h) return kn_fail(KNPEMI_EINVAL, entry(EXCHANGE, part ? "set_partitioned" : "set") + ": null argument");
  const int K = h->K;
  // per watched ion int j^e, int j^i, int I_ch,k; with the current columns int I_cap, int I_ch,tot and the area: all sums
  auto cols = [&](int m, auto emit) {
    for (int k = 0; k < K; ++k)
      if ((m >> k) & 1)
        for (int j = 0; j < 3; ++j) emit(3 * k + j, false);
    if (m & KN_WATCH_CURRENT)
      for (int j = 0; j < 3; ++j) emit(3 * KN_MAXK + j, false);
  };
  return watched_set(h, EXCHANGE, h->foff, h->n_facet, kn_exchange_chunk(), 3, 2, cols, n_watch, sub, ion_mask, capacity, part);
}
}  // namespace

extern "C" int knpemi_flux_set(knpemi_handle* h, int n_watch, const int32_t* sub, const int32_t* ion_mask, int capacity) {
  return flux_set(h, n_watch, sub, ion_mask, capacity, nullptr);
}
extern "C" int knpemi_exchange_set(knpemi_handle* h, int n_watch, const int32_t* sub, const int32_t* ion_mask, int capacity) {
  return exchange_set(h, n_watch, sub, ion_mask, capacity, nullptr);
}
extern "C" int knpemi_flux_set_partitioned(knpemi_handle* h, int n_watch, const int32_t* sub, const int32_t* ion_mask,
                                           int capacity, const uint8_t* recorded, int rank, int world, void* xbuf_dev,
                                           knpemi_allreduce_fn allreduce, void* ctx) {
  const WatchPart part{recorded, {static_cast<double*>(xbuf_dev), rank, world, allreduce, ctx}};
  return flux_set(h, n_watch, sub, ion_mask, capacity, &part);
}
extern "C" int knpemi_exchange_set_partitioned(knpemi_handle* h, int n_watch, const int32_t* sub, const int32_t* ion_mask,
                                               int capacity, const uint8_t* recorded, int rank, int world, void* xbuf_dev,
                                               knpemi_allreduce_fn allreduce, void* ctx) {
  const WatchPart part{recorded, {static_cast<double*>(xbuf_dev), rank, world, allreduce, ctx}};
  return exchange_set(h, n_watch, sub, ion_mask, capacity, &part);
}

extern "C" int knpemi_flux_record(knpemi_handle* h, int write_fields) { return watched_record(h, FLUX, write_fields); }
extern "C" int knpemi_exchange_record(knpemi_handle* h, int write_fields) { return watched_record(h, EXCHANGE, write_fields); }

extern "C" int knpemi_flux_read(knpemi_handle* h, int n_rows, double* out, int64_t* rows, int64_t* overflow, int reset) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  return series_read(h, h->flux.ser, h->flux.n_watch != 0, "knpemi_flux_read", FLUX.none, n_rows, out, rows, overflow, reset);
}
extern "C" int knpemi_exchange_read(knpemi_handle* h, int n_rows, double* out, int64_t* rows, int64_t* overflow, int reset) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  return series_read(h, h->exchange.ser, h->exchange.n_watch != 0, "knpemi_exchange_read", EXCHANGE.none, n_rows, out, rows,
                     overflow, reset);
}

extern "C" int knpemi_flux_fields(knpemi_handle* h, int sub, int ion, int part, double* host, size_t n) {
  int w;
  if (int rc = fields_watch(h, FLUX, sub, host, &w)) return rc;
  if (part != 0 && part != 1) return kn_fail(KNPEMI_EINVAL, "knpemi_flux_fields: part is 0 (diffusive) or 1 (drift)");
  if (int rc = fields_ion(h, FLUX, w, ion)) return rc;
  const size_t nc = (size_t)h->flux.host.count[w], gd = (size_t)h->gdim;
  const size_t comp = 2 * (size_t)ions_below(h->flux.host.mask[w], ion) + part;      // {diffusive}, {drift} per ion
  return fields_copy(h, FLUX, w, comp * gd * nc, host, n, nc * gd, "gdim * number of cells");
}

extern "C" int knpemi_exchange_fields(knpemi_handle* h, int sub, int ion, int part, double* host, size_t n) {
  int w;
  if (int rc = fields_watch(h, EXCHANGE, sub, host, &w)) return rc;
  if (int rc = fields_ion(h, EXCHANGE, w, ion)) return rc;
  if (part < 0 || part > (ion == -1 ? 1 : 2))
    return kn_fail(KNPEMI_EINVAL, "knpemi_exchange_fields: part is 0 (ECS side), 1 (cell side) or 2 (channel current) of an "
                                  "ion, 0 (capacitive current) or 1 (area) with ion == -1");
  const size_t nf = (size_t)h->exchange.host.count[w];
  const size_t comp = 3 * (size_t)ions_below(h->exchange.host.mask[w], ion) + part;  // three components per ion
  return fields_copy(h, EXCHANGE, w, comp * nf, host, n, nf, "the number of membrane facets of the cell");
}

extern "C" int knpemi_flux_reset(knpemi_handle* h) { return watched_reset(h, FLUX); }
extern "C" int knpemi_exchange_reset(knpemi_handle* h) { return watched_reset(h, EXCHANGE); }
extern "C" int knpemi_flux_clear(knpemi_handle* h) { return recorder_clear(h, &knpemi_handle::flux); }
extern "C" int knpemi_exchange_clear(knpemi_handle* h) { return recorder_clear(h, &knpemi_handle::exchange); }

// ---------------------------------------------------------------------------------------------------
// field maps (kernels_maps.hip)
// ---------------------------------------------------------------------------------------------------
namespace {
// what knpemi_maps_set_partitioned adds to knpemi_maps_set
struct MapsPart {
  const uint8_t* owned;      // one byte per item of every series watch, concatenated as `weight`
  KnRankSlots slots;
};

// knpemi_maps_set and, with `part`, knpemi_maps_set_partitioned
int maps_set(knpemi_handle* h, const char* who, int n_watch, const int32_t* spec, const double* threshold, const double* weight,
             int capacity, const MapsPart* part = nullptr) {
  const std::string fn(who);
  if (!h || !spec) return kn_fail(KNPEMI_EINVAL, fn + ": null argument");
  if (h->ode_only) return kn_fail(KNPEMI_EINVAL, fn + ": a handle of knpemi_ode_create has no fields");
  if (n_watch < 1 || n_watch > KNPEMI_MAPS_MAX_WATCH) return kn_fail(KNPEMI_EINVAL, fn + ": 1 to KNPEMI_MAPS_MAX_WATCH watches");
  const int all = KNPEMI_MAPS_PEAK | KNPEMI_MAPS_TROUGH | KNPEMI_MAPS_INTEGRAL | KNPEMI_MAPS_THRESHOLD;
  // the space of a watch: the vertices of sub-domain s (s), or the membrane dofs of cell s (KN_MAXSUB + s)
  int space[KNPEMI_MAPS_MAX_WATCH], per_space[KN_MAPS_MAXSPACE] = {};
  KnFieldLoc loc[KNPEMI_MAPS_MAX_WATCH];
  bool any_series = false;
  for (int w = 0; w < n_watch; ++w) {
    const int32_t field = spec[4 * w], sub = spec[4 * w + 1], ix = spec[4 * w + 2], fl = spec[4 * w + 3];
    const std::string who = fn + ": watch " + std::to_string(w);
    if (field != KNPEMI_F_PHI && field != KNPEMI_F_C && field != KNPEMI_F_C_ELIM && field != KNPEMI_F_PHI_M)
      return kn_fail(KNPEMI_EINVAL, who + ": unknown field (phi, c, the eliminated ion's c or phi_M)");
    if (int rc = kn_locate(h, field, sub, ix, &loc[w])) return rc;      // sub / idx out of range, phi_M on the ECS
    if (loc[w].n > (size_t)INT32_MAX) return kn_fail(KNPEMI_EINVAL, who + ": too many items");
    if (fl & ~(all | KNPEMI_MAPS_SERIES | KNPEMI_MAPS_BELOW)) return kn_fail(KNPEMI_EINVAL, who + ": unknown flag bits");
    if (!(fl & all)) return kn_fail(KNPEMI_EINVAL, who + ": no statistic selected");
    if (!(fl & KNPEMI_MAPS_THRESHOLD) && (fl & (KNPEMI_MAPS_SERIES | KNPEMI_MAPS_BELOW)))
      return kn_fail(KNPEMI_EINVAL, who + ": a series and the direction need the threshold statistic");
    if (fl & KNPEMI_MAPS_THRESHOLD) {
      if (!threshold) return kn_fail(KNPEMI_EINVAL, fn + ": null argument");
      if (!std::isfinite(threshold[w])) return kn_fail(KNPEMI_EINVAL, who + ": the threshold is not finite");
    }
    if (fl & KNPEMI_MAPS_SERIES) {
      any_series = true;
      if (!weight) return kn_fail(KNPEMI_EINVAL, fn + ": null argument (a series watch needs the item weights)");
      if (capacity < 1) return kn_fail(KNPEMI_EINVAL, fn + ": capacity must be positive with a series watch");
    }
    for (int u = 0; u < w; ++u)
      if (std::equal(spec + 4 * u, spec + 4 * u + 4, spec + 4 * w)
          && (!(fl & KNPEMI_MAPS_THRESHOLD) || threshold[u] == threshold[w]))
        return kn_fail(KNPEMI_EINVAL, who + " is listed twice");
    space[w] = field == KNPEMI_F_PHI_M ? KN_MAXSUB + sub : sub;
    if (++per_space[space[w]] > KNPEMI_MAPS_MAX_PER_SPACE)
      return kn_fail(KNPEMI_EINVAL, fn + ": more than KNPEMI_MAPS_MAX_PER_SPACE watches on one space");
  }
  if (part) {
    if (!any_series) return kn_fail(KNPEMI_EINVAL, fn + ": no watch has a series (knpemi_maps_set records the maps of a partitioned run)");
    if (!part->owned) return kn_fail(KNPEMI_EINVAL, fn + ": the owned mask is required");
    if (int rc = slots_check(h, fn, part->slots, KN_MAPS_MAXCOLS)) return rc;
  }
  // the table, grouped by space
  New<knpemi_handle::KnMaps> N;
  KnMapTab& T = N.host;
  std::vector<size_t> w_off(n_watch, 0);      // a series watch's place in `weight`
  {
    size_t o = 0;
    for (int w = 0; w < n_watch; ++w)
      if (spec[4 * w + 3] & KNPEMI_MAPS_SERIES) { w_off[w] = o; o += loc[w].n; }
  }
  KN_HIP(hipSetDevice(h->device));
  int k = 0, col_of[KNPEMI_MAPS_MAX_WATCH];
  std::fill(col_of, col_of + KNPEMI_MAPS_MAX_WATCH, -1);
  for (int sp = 0; sp < KN_MAPS_MAXSPACE; ++sp) {
    if (!per_space[sp]) continue;
    const int p = T.n_space++;
    const bool mem = sp >= KN_MAXSUB;
    const int sub = mem ? sp - KN_MAXSUB : sp;
    T.n_items[p] = mem ? h->n_q[sub] : h->n_vert[sub];
    T.first[p] = mem ? 0 : h->voff[sub];
    T.bstart[p + 1] = T.bstart[p] + (T.n_items[p] + 255) / 256;
    T.wstart[p] = k;
    int n_ser = 0;
    for (int w = 0; w < n_watch; ++w) {
      if (space[w] != sp) continue;
      const int fl = spec[4 * w + 3];
      const size_t n = loc[w].n;
      KnMapWatch& W = T.w[k];
      W = KnMapWatch{};
      if (loc[w].stride == 1) {
        W.dense = loc[w].base;
      } else {      // a slot of the vertex records: every read of the kernel stays inside the record of a vertex of `sub`
        W.slot = (int)((loc[w].base - h->dev.VR) % KN_REC);
        if (loc[w].stride != KN_REC || W.slot < 3 || n != (size_t)T.n_items[p])
          return kn_fail(KNPEMI_EINVAL, fn + ": field layout not understood");
        T.need_rec[p] = 1;
      }
      if (n != (size_t)T.n_items[p]) return kn_fail(KNPEMI_EINVAL, fn + ": field length is not the space's");
      W.flags = fl;
      W.ser = -1;
      W.thr = (fl & KNPEMI_MAPS_THRESHOLD) ? threshold[w] : 0.0;
      W.sgn = (fl & KNPEMI_MAPS_BELOW) ? -1.0 : 1.0;
      int rc = KNPEMI_OK;
      auto want = [&](bool on, auto** out) { if (on && !rc) rc = kn_alloc(N.allocs, n, out); };
      want(fl & (KNPEMI_MAPS_INTEGRAL | KNPEMI_MAPS_THRESHOLD), &W.v_prev);
      want(fl & KNPEMI_MAPS_PEAK, &W.v_max); want(fl & KNPEMI_MAPS_PEAK, &W.t_max);
      want(fl & KNPEMI_MAPS_TROUGH, &W.v_min); want(fl & KNPEMI_MAPS_TROUGH, &W.t_min);
      want(fl & KNPEMI_MAPS_INTEGRAL, &W.integral);
      want(fl & KNPEMI_MAPS_THRESHOLD, &W.t_arrival); want(fl & KNPEMI_MAPS_THRESHOLD, &W.exposure);
      want(fl & KNPEMI_MAPS_THRESHOLD, &W.excess); want(fl & KNPEMI_MAPS_THRESHOLD, &W.count);
      if (!rc && (fl & KNPEMI_MAPS_SERIES)) {
        W.ser = n_ser++;
        double* dw = nullptr;
        rc = kn_upload(N.allocs, weight + w_off[w], n, &dw);
        W.weight = dw;
        if (!rc && part) {
          uint8_t* own = nullptr;
          rc = kn_upload(N.allocs, part->owned + w_off[w], n, &own);
          W.owned = own;
        }
      }
      if (rc) return rc;
      N.slot_of[w] = k;
      N.items_of[w] = (int)n;
      col_of[w] = W.ser;
      ++k;
    }
    T.wstart[p + 1] = k;
  }
  T.n_watch = n_watch;
  for (int w = 0; w < n_watch; ++w) {      // the columns, in the order of the watches as given
    if (col_of[w] < 0) continue;
    int p = 0;
    while (N.slot_of[w] >= T.wstart[p + 1]) ++p;
    for (int j = 0; j < 2; ++j) {
      T.col_space[T.n_cols] = (uint8_t)p;
      T.col_slot[T.n_cols++] = (uint8_t)(2 * col_of[w] + j);
    }
  }
  N.n_watch = n_watch;
  N.n_blk = T.bstart[T.n_space];
  int rc = kn_upload(N.allocs, &T, 1, &N.tab);
  if (!rc && any_series) {
    rc = kn_alloc(N.allocs, (size_t)N.n_blk * KN_MAPS_SLOTS, &N.part);
    if (!rc) rc = series_alloc(N.allocs, h->stream, capacity, T.n_cols, &N.ser);
    if (!rc && part) rc = slots_attach(h, &N.slots, part->slots, T.n_cols);
  }
  if (rc || (rc = recorder_install(h, &knpemi_handle::maps, N))) return rc;
  if ((rc = kn_launch_maps_reset(h))) recorder_free(h->maps);
  return rc;
}
}  // namespace

extern "C" int knpemi_maps_set(knpemi_handle* h, int n_watch, const int32_t* spec, const double* threshold,
                               const double* weight, int capacity) {
  return maps_set(h, "knpemi_maps_set", n_watch, spec, threshold, weight, capacity);
}

extern "C" int knpemi_maps_set_partitioned(knpemi_handle* h, int n_watch, const int32_t* spec, const double* threshold,
                                           const double* weight, int capacity, const uint8_t* owned, int rank, int world,
                                           void* xbuf_dev, knpemi_allreduce_fn allreduce, void* ctx) {
  const MapsPart part{owned, {static_cast<double*>(xbuf_dev), rank, world, allreduce, ctx}};
  return maps_set(h, "knpemi_maps_set_partitioned", n_watch, spec, threshold, weight, capacity, &part);
}

extern "C" int knpemi_maps_record(knpemi_handle* h, double t) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  auto& M = h->maps;
  if (M.n_watch == 0) return kn_fail(KNPEMI_EINVAL, "knpemi_maps_record: no maps set (knpemi_maps_set)");
  if (int rc = clock_accept(M.clock, "knpemi_maps_record", t)) return rc;
  KN_HIP(hipSetDevice(h->device));
  // the first record's interval is never used: every v_prev is NaN then
  if (int rc = kn_launch_maps_record(h, t, M.clock.have_prev ? M.clock.t_prev : t)) return rc;
  clock_advance(M.clock, t);
  if (!M.slots.xbuf) return KNPEMI_OK;
  // partitioned: this rank's slots are written (never, without a local item: zeros); sum the exchange buffer over the ranks,
  // then sum the slots and append
  if (int rc = slots_sum(h, "knpemi_maps_record", M.slots, M.ser.n_cols)) return rc;
  return kn_launch_record_combine(h, "record_combine_kernel (maps)", M.ser.n_cols, M.ser.capacity, M.slots.world, M.slots.rank,
                                  nullptr, nullptr, nullptr, M.slots.xbuf, M.ser.ctl, M.ser.rows);
}

extern "C" int knpemi_maps_read(knpemi_handle* h, int watch, int which, void* host, size_t n) {
  const std::string fn = "knpemi_maps_read";
  if (!h || !host) return kn_fail(KNPEMI_EINVAL, fn + ": null argument");
  auto& M = h->maps;
  if (M.n_watch == 0) return kn_fail(KNPEMI_EINVAL, fn + ": no maps set (knpemi_maps_set)");
  if (watch < 0 || watch >= M.n_watch) return kn_fail(KNPEMI_EINVAL, fn + ": bad watch index");
  const KnMapWatch& W = M.host.w[M.slot_of[watch]];
  const double* d = nullptr;
  switch (which) {
    case KNPEMI_MAP_V_MAX: d = W.v_max; break;
    case KNPEMI_MAP_T_MAX: d = W.t_max; break;
    case KNPEMI_MAP_V_MIN: d = W.v_min; break;
    case KNPEMI_MAP_T_MIN: d = W.t_min; break;
    case KNPEMI_MAP_INTEGRAL: d = W.integral; break;
    case KNPEMI_MAP_T_ARRIVAL: d = W.t_arrival; break;
    case KNPEMI_MAP_EXPOSURE: d = W.exposure; break;
    case KNPEMI_MAP_EXCESS: d = W.excess; break;
    case KNPEMI_MAP_COUNT: break;
    default: return kn_fail(KNPEMI_EINVAL, fn + ": which is KNPEMI_MAP_V_MAX ... KNPEMI_MAP_COUNT");
  }
  if (which == KNPEMI_MAP_COUNT ? !W.count : !d) return kn_fail(KNPEMI_EINVAL, fn + ": this statistic of the watch was not selected");
  if (n != (size_t)M.items_of[watch]) return kn_fail(KNPEMI_EINVAL, fn + ": length is not the number of items of the watch");
  KN_HIP(hipSetDevice(h->device));
  if (n == 0) return KNPEMI_OK;
  if (which == KNPEMI_MAP_COUNT) return kn_to_host(h->stream, static_cast<int*>(host), (const int*)W.count, n);
  return kn_to_host(h->stream, static_cast<double*>(host), d, n);
}

extern "C" int knpemi_maps_series_read(knpemi_handle* h, int n_rows, double* out, int64_t* rows, int64_t* overflow,
                                       int reset) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  auto& M = h->maps;
  if (M.n_watch != 0 && M.host.n_cols == 0) return kn_fail(KNPEMI_EINVAL, "knpemi_maps_series_read: no watch has a series");
  return series_read(h, M.ser, M.n_watch != 0, "knpemi_maps_series_read", "no maps set (knpemi_maps_set)", n_rows, out, rows,
                     overflow, reset);
}

extern "C" int knpemi_maps_reset(knpemi_handle* h) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  auto& M = h->maps;
  if (M.n_watch == 0) return kn_fail(KNPEMI_EINVAL, "knpemi_maps_reset: no maps set (knpemi_maps_set)");
  KN_HIP(hipSetDevice(h->device));
  clock_restart(M.clock);
  if (M.host.n_cols > 0)
    if (int rc = series_rewind(h, M.ser)) return rc;
  return kn_launch_maps_reset(h);
}

extern "C" int knpemi_maps_clear(knpemi_handle* h) { return recorder_clear(h, &knpemi_handle::maps); }

// ---------------------------------------------------------------------------------------------------
// membrane monitors (kernels_monitor.hip)
// ---------------------------------------------------------------------------------------------------
namespace {
const char* const MON_NONE = "no monitors set (knpemi_monitor_set)";

// the watch of slot (sub, model) with the quantities `mask`: checks the slot, the mask, v_index and (pde) the parameter
// columns of the ions; *slot: the model slot.  weight, wsum, rmask and fbase are the caller's.  partitioned: the slot may
// have no membrane dof on this rank.
int mon_watch(knpemi_handle* h, const std::string& fn, int sub, int model, uint32_t mask, int v_index, const int32_t* ion_param,
              KnMonWatch* W, int* slot, bool partitioned = false) {
  if (sub == 0 && !h->ode_only) return kn_fail(KNPEMI_EINVAL, fn + ": the ECS (sub-domain 0) has no membrane: watch a model of a cell");
  if (sub < 1 || sub >= h->n_sub || model < 0 || model >= h->n_models[sub])
    return kn_fail(KNPEMI_EINVAL, fn + ": membrane model index out of range");
  const KnOdeModel& m = h->sweeps.ode[h->moff[sub] + model];
  if (!m.bound) return kn_fail(KNPEMI_EINVAL, fn + ": membrane model not bound (knpemi_ode_bind)");
  if (m.rtc_module && !m.mon_kernel[0])
    return kn_fail(KNPEMI_EINVAL, fn + ": a model bound from source has no monitor (knpemi_monitor_bind_source)");
  const int count = m.rtc_module ? m.n_monitored : knpemi_monitor_count(m.model_id);
  if (mask == 0) return kn_fail(KNPEMI_EINVAL, fn + ": empty quantity mask");
  if (count < 32 && (mask >> count)) return kn_fail(KNPEMI_EINVAL, fn + ": quantity mask has bits at or beyond the model's count");
  if (m.nq < (partitioned ? 0 : 1)) return kn_fail(KNPEMI_EINVAL, fn + ": the sub-domain has no membrane dofs");
  if (v_index < -1 || v_index >= m.n_states) return kn_fail(KNPEMI_EINVAL, fn + ": v_index out of range");
  *W = KnMonWatch{};
  W->model_id = m.model_id; W->nq = m.nq; W->q0 = h->qoff[sub]; W->v_index = v_index; W->mask = mask;
  W->states = m.d_states; W->params = m.d_params;
  W->pde = (!h->ode_only && ion_param) ? 1 : 0;
  if (W->pde) {
    W->n_ions = h->K;
    for (int k = 0; k < h->K; ++k) {
      const int je = ion_param[2 * k], ji = ion_param[2 * k + 1];
      if (je < 0 || je >= m.n_params || ji < 0 || ji >= m.n_params || je == ji)
        return kn_fail(KNPEMI_EINVAL, fn + ": parameter column of an ion out of range");
      W->ion_e[k] = je; W->ion_i[k] = ji;
    }
  }
  *slot = h->moff[sub] + model;
  return KNPEMI_OK;
}
}  // namespace

extern "C" int knpemi_monitor_bind_source(knpemi_handle* h, int sub, int model, int n_monitored, const char* monitor_source) {
  const std::string fn = "knpemi_monitor_bind_source";
  if (!h || !monitor_source) return kn_fail(KNPEMI_EINVAL, fn + ": null argument");
  if (sub < 1 || sub >= h->n_sub || model < 0 || model >= h->n_models[sub])
    return kn_fail(KNPEMI_EINVAL, fn + ": membrane model index out of range");
  KnOdeModel& m = h->sweeps.ode[h->moff[sub] + model];
  if (!m.bound || !m.rtc_module)
    return kn_fail(KNPEMI_EINVAL, fn + ": the slot is not bound from source (knpemi_ode_bind_source); the shipped models "
                                       "bring their monitors");
  if (m.mon_kernel[0]) return kn_fail(KNPEMI_EINVAL, fn + ": the slot has a monitor already");
  KN_HIP(hipSetDevice(h->device));
  return kn_rtc_monitor_bind(h->sweeps, m, n_monitored, monitor_source);
}

namespace {
// what knpemi_monitor_set_partitioned adds to knpemi_monitor_set
struct MonPart {
  const double* wsum_global;      // [n_watch] the weight sums over the ranks
  KnRankSlots slots;
};

// knpemi_monitor_set and, with `part`, knpemi_monitor_set_partitioned: a watch may then have no local dof (no workgroup)
// or local weights that sum to nothing, and a point no local dof (another rank takes it)
int monitor_set(knpemi_handle* h, const char* who, int n_watch, const int32_t* spec, const int32_t* ion_param,
                const double* weights, int n_cols, const int32_t* col_spec, int n_pts, const int32_t* pt_watch,
                const int32_t* pt_q, const double* pt_w, int capacity, const MonPart* part = nullptr) {
  const std::string fn(who);
  if (!h || !spec || !weights || (n_cols > 0 && !col_spec) || (n_pts > 0 && (!pt_watch || !pt_q || !pt_w)))
    return kn_fail(KNPEMI_EINVAL, fn + ": null argument");
  if (!h->ode_only && !ion_param) return kn_fail(KNPEMI_EINVAL, fn + ": null argument (the ions' parameter columns)");
  if (n_watch < 1 || n_watch > KN_MON_MAXW) return kn_fail(KNPEMI_EINVAL, fn + ": 1 to KNPEMI_MON_MAX_WATCH watches");
  if (capacity < 1) return kn_fail(KNPEMI_EINVAL, fn + ": capacity must be positive");
  if (n_cols < 0 || n_pts < 0 || n_pts > (1 << 20)) return kn_fail(KNPEMI_EINVAL, fn + ": bad number of columns or points");
  if (part) {
    if (h->ode_only) return kn_fail(KNPEMI_EINVAL, fn + ": a handle of knpemi_ode_create has no partition");
    if (!part->wsum_global) return kn_fail(KNPEMI_EINVAL, fn + ": null argument (the global weight sums)");
    if (n_cols < 1) return kn_fail(KNPEMI_EINVAL, fn + ": a partitioned record needs a column");
    if (int rc = slots_check(h, fn, part->slots, (size_t)n_cols)) return rc;
  }
  New<knpemi_handle::KnMon> N;
  KnMonTab& T = N.host;
  std::vector<size_t> woff(n_watch);
  size_t wo = 0;
  long long fbase = 0;
  for (int w = 0; w < n_watch; ++w) {
    int slot = -1;
    if (int rc = mon_watch(h, fn, spec[4 * w], spec[4 * w + 1], (uint32_t)spec[4 * w + 2], spec[4 * w + 3],
                           h->ode_only ? nullptr : ion_param + (size_t)w * 2 * h->K, &T.w[w], &slot, part != nullptr))
      return rc;
    for (int u = 0; u < w; ++u)
      if (N.slot_of[u] == slot) return kn_fail(KNPEMI_EINVAL, fn + ": watch " + std::to_string(w) + " is listed twice");
    N.slot_of[w] = slot;
    if (T.w[w].nq > 0) {
      N.fn[w][0] = h->sweeps.ode[slot].mon_kernel[0];
      N.fn[w][1] = h->sweeps.ode[slot].mon_kernel[1];
    }
    KnMonWatch& W = T.w[w];
    woff[w] = wo;
    double wsum = 0.0;
    for (int q = 0; q < W.nq; ++q) {
      const double x = weights[wo + q];
      if (!(x >= 0.0) || !std::isfinite(x)) return kn_fail(KNPEMI_EINVAL, fn + ": a dof weight is negative or not finite");
      wsum += x;
    }
    wo += (size_t)W.nq;
    // (no comparison with the local sum: the caller adds the ranks' sums in another order than this loop, and the two
    // differ in their last bits in either direction where one rank records a whole cell)
    if (part && (!(part->wsum_global[w] >= 0.0) || !std::isfinite(part->wsum_global[w])))
      return kn_fail(KNPEMI_EINVAL, fn + ": the global weight sum of watch " + std::to_string(w) + " is negative or not finite");
    W.wsum = part ? part->wsum_global[w] : wsum;
    W.fbase = fbase;
    fbase += (long long)popcount((int)(W.mask & 0x7FFFFFFFu)) * W.nq + ((W.mask >> 31) ? W.nq : 0);
    T.bstart[w + 1] = T.bstart[w] + (W.nq + kn_monitor_chunk() - 1) / kn_monitor_chunk();
  }
  for (int p = 0; p < n_pts; ++p) {
    if (pt_watch[p] < 0 || pt_watch[p] >= n_watch) return kn_fail(KNPEMI_EINVAL, fn + ": a point's watch is out of range");
    bool any = false;
    for (int j = 0; j < 4; ++j) {
      const int q = pt_q[4 * p + j];
      if (q < -1 || q >= T.w[pt_watch[p]].nq) return kn_fail(KNPEMI_EINVAL, fn + ": a point's dof is out of range");
      if (q >= 0 && !std::isfinite(pt_w[4 * p + j])) return kn_fail(KNPEMI_EINVAL, fn + ": a point's weight is not finite");
      any = any || q >= 0;
    }
    if (!any && !part) return kn_fail(KNPEMI_EINVAL, fn + ": a point without dofs");
  }
  std::vector<int4> cols((size_t)n_cols);
  std::vector<int> col_op((size_t)n_cols, KNPEMI_OBS_SUM);
  std::vector<double> col_denom((size_t)n_cols, 1.0);
  for (int c = 0; c < n_cols; ++c) {
    const int kind = col_spec[4 * c], w = col_spec[4 * c + 1], qty = col_spec[4 * c + 2], pt = col_spec[4 * c + 3];
    const std::string who = fn + ": column " + std::to_string(c);
    if (kind < KNPEMI_MON_POINT || kind > KNPEMI_MON_MAX_OP) return kn_fail(KNPEMI_EINVAL, who + ": unknown kind");
    if (w < 0 || w >= n_watch) return kn_fail(KNPEMI_EINVAL, who + ": watch out of range");
    if (qty < 0 || qty >= KN_MON_MAX || !((T.w[w].mask >> qty) & 1u))
      return kn_fail(KNPEMI_EINVAL, who + ": the quantity is not selected by its watch");
    if (kind == KNPEMI_MON_POINT) {
      if (pt < 0 || pt >= n_pts || pt_watch[pt] != w) return kn_fail(KNPEMI_EINVAL, who + ": not a point of its watch");
    } else {
      if (!(T.w[w].wsum > 0.0)) return kn_fail(KNPEMI_EINVAL, who + ": the weights of its watch sum to nothing");
      T.w[w].rmask |= 1u << qty;
    }
    cols[c] = make_int4(kind, w, qty, kind == KNPEMI_MON_POINT ? pt : 0);
    col_op[c] = kind == KNPEMI_MON_MIN ? KNPEMI_OBS_MIN : (kind == KNPEMI_MON_MAX_OP ? KNPEMI_OBS_MAX : KNPEMI_OBS_SUM);
    if (kind == KNPEMI_MON_AVERAGE) col_denom[c] = T.w[w].wsum;
  }
  T.n_watch = n_watch; T.n_cols = n_cols; T.n_pts = n_pts;
  N.n_watch = n_watch; N.n_blk = T.bstart[n_watch]; N.fields.fld_len = (size_t)fbase;
  KN_HIP(hipSetDevice(h->device));
  auto& A = N.allocs;
  int rc = KNPEMI_OK;
  for (int w = 0; w < n_watch && !rc; ++w) rc = kn_upload(A, weights + woff[w], (size_t)T.w[w].nq, &T.w[w].weight);
  if (!rc) rc = kn_upload(A, &T, 1, &N.tab);
  if (!rc) rc = kn_upload(A, cols, &N.cols);
  if (!rc) rc = kn_upload(A, pt_watch, (size_t)n_pts, &N.pt_watch);
  if (!rc) rc = kn_upload(A, pt_q, 4 * (size_t)n_pts, &N.pt_q);
  if (!rc) rc = kn_upload(A, pt_w, 4 * (size_t)n_pts, &N.pt_w);
  if (!rc) rc = kn_alloc(A, 4 * (size_t)n_pts * KN_MON_MAX, &N.pt_val);
  if (!rc) rc = kn_alloc(A, (size_t)N.n_blk * KN_MON_SLOTS, &N.part);
  if (!rc) rc = series_alloc(A, h->stream, capacity, n_cols, &N.ser);
  if (!rc && part) {
    if ((rc = kn_upload(A, col_op, &N.col_op)) || (rc = kn_upload(A, col_denom, &N.col_denom))
        || (rc = slots_attach(h, &N.slots, part->slots, n_cols)))
      return rc;
    if (N.n_blk == 0) {      // no record launch ever writes this rank's slots: they hold the operations' identities
      std::vector<double> id((size_t)n_cols);
      for (int c = 0; c < n_cols; ++c)
        id[c] = col_op[c] == KNPEMI_OBS_MIN ? INFINITY : (col_op[c] == KNPEMI_OBS_MAX ? -INFINITY : 0.0);
      KN_HIP(hipMemcpyAsync(N.slots.xbuf + (size_t)N.slots.rank * n_cols, id.data(), id.size() * sizeof(double),
                            hipMemcpyHostToDevice, h->stream));
      KN_HIP(hipStreamSynchronize(h->stream));
    }
  }
  return rc ? rc : recorder_install(h, &knpemi_handle::mon, N);
}
}  // namespace

extern "C" int knpemi_monitor_set(knpemi_handle* h, int n_watch, const int32_t* spec, const int32_t* ion_param,
                                  const double* weights, int n_cols, const int32_t* col_spec, int n_pts,
                                  const int32_t* pt_watch, const int32_t* pt_q, const double* pt_w, int capacity) {
  return monitor_set(h, "knpemi_monitor_set", n_watch, spec, ion_param, weights, n_cols, col_spec, n_pts, pt_watch, pt_q, pt_w,
                     capacity);
}

extern "C" int knpemi_monitor_set_partitioned(knpemi_handle* h, int n_watch, const int32_t* spec, const int32_t* ion_param,
                                              const double* weights, int n_cols, const int32_t* col_spec, int n_pts,
                                              const int32_t* pt_watch, const int32_t* pt_q, const double* pt_w, int capacity,
                                              const double* wsum_global, int rank, int world, void* xbuf_dev,
                                              knpemi_allreduce_fn allreduce, void* ctx) {
  const MonPart part{wsum_global, {static_cast<double*>(xbuf_dev), rank, world, allreduce, ctx}};
  return monitor_set(h, "knpemi_monitor_set_partitioned", n_watch, spec, ion_param, weights, n_cols, col_spec, n_pts, pt_watch,
                     pt_q, pt_w, capacity, &part);
}

extern "C" int knpemi_monitor_record(knpemi_handle* h, double t, int fields) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  auto& X = h->mon;
  if (X.n_watch == 0) return kn_fail(KNPEMI_EINVAL, std::string("knpemi_monitor_record: ") + MON_NONE);
  if (!std::isfinite(t)) return kn_fail(KNPEMI_EINVAL, "knpemi_monitor_record: t must be finite");
  KN_HIP(hipSetDevice(h->device));
  // the record reads phi_M and the tables, which the ODE sweeps may write on the auxiliary streams
  if (int rc = kn_wait_ode_joins(h)) return rc;
  if (int rc = fields_record(X.fields, X.allocs, fields, [&] { return kn_launch_monitor(h, t, fields); })) return rc;
  if (!X.slots.xbuf) return KNPEMI_OK;
  // partitioned: this rank's slots are written (without a local dof they hold the identities); sum the exchange buffer over
  // the ranks, then fold, divide the averages and append
  if (int rc = slots_sum(h, "knpemi_monitor_record", X.slots, X.ser.n_cols)) return rc;
  return kn_launch_record_combine(h, "record_combine_kernel (monitors)", X.ser.n_cols, X.ser.capacity, X.slots.world,
                                  X.slots.rank, X.col_op, X.col_denom, nullptr, X.slots.xbuf, X.ser.ctl, X.ser.rows, true);
}

extern "C" int knpemi_monitor_read(knpemi_handle* h, int n_rows, double* out, int64_t* rows, int64_t* overflow, int reset) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  return series_read(h, h->mon.ser, h->mon.n_watch != 0, "knpemi_monitor_read", MON_NONE, n_rows, out, rows, overflow, reset);
}

extern "C" int knpemi_monitor_fields(knpemi_handle* h, int watch, int quantity, double* out, size_t n) {
  const std::string fn = "knpemi_monitor_fields";
  if (!h || !out) return kn_fail(KNPEMI_EINVAL, fn + ": null argument");
  const auto& X = h->mon;
  if (X.n_watch == 0) return kn_fail(KNPEMI_EINVAL, fn + ": " + MON_NONE);
  if (watch < 0 || watch >= X.n_watch) return kn_fail(KNPEMI_EINVAL, fn + ": bad watch index");
  const KnMonWatch& W = X.host.w[watch];
  if (quantity < 0 || quantity >= KN_MON_MAX || !((W.mask >> quantity) & 1u))
    return kn_fail(KNPEMI_EINVAL, fn + ": the quantity is not selected by the watch");
  if (int rc = fields_recorded(X.fields, fn, "knpemi_monitor_record(h, t, 1)")) return rc;
  if (n != (size_t)W.nq) return kn_fail(KNPEMI_EINVAL, fn + ": length is not the number of membrane dofs of the sub-domain");
  KN_HIP(hipSetDevice(h->device));
  const size_t comp = (size_t)popcount((int)(W.mask & ((1u << quantity) - 1u)));
  return kn_to_host(h->stream, out, X.fields.fld + W.fbase + comp * (size_t)W.nq, n);
}

extern "C" int knpemi_monitor_reset(knpemi_handle* h) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  auto& X = h->mon;
  if (X.n_watch == 0) return kn_fail(KNPEMI_EINVAL, std::string("knpemi_monitor_reset: ") + MON_NONE);
  KN_HIP(hipSetDevice(h->device));
  fields_forget(X.fields);
  return series_rewind(h, X.ser);
}

extern "C" int knpemi_monitor_clear(knpemi_handle* h) { return recorder_clear(h, &knpemi_handle::mon); }

extern "C" int knpemi_monitor_eval(knpemi_handle* h, int sub, int model, double t, uint32_t mask, const double* states,
                                   const double* params, const int32_t* ion_param, int v_index, double* out, size_t n) {
  const std::string fn = "knpemi_monitor_eval";
  if (!h || !out) return kn_fail(KNPEMI_EINVAL, fn + ": null argument");
  if ((states == nullptr) != (params == nullptr)) return kn_fail(KNPEMI_EINVAL, fn + ": give both host tables or neither");
  if (!std::isfinite(t)) return kn_fail(KNPEMI_EINVAL, fn + ": t must be finite");
  KnMonTab T{};
  KnMonWatch& W = T.w[0];
  int slot = -1;
  if (int rc = mon_watch(h, fn, sub, model, mask, v_index, ion_param, &W, &slot)) return rc;
  const KnOdeModel& m = h->sweeps.ode[slot];
  const size_t nq = (size_t)W.nq, nb = (size_t)popcount((int)(mask & 0x7FFFFFFFu)) + (mask >> 31);
  if (n != nb * nq) return kn_fail(KNPEMI_EINVAL, fn + ": length is not (bits set) * (membrane dofs)");
  KN_HIP(hipSetDevice(h->device));
  struct Tmp { std::vector<void*> a; ~Tmp() { kn_free_all(a); } } tmp;
  int rc;
  if (states) {
    double *ds = nullptr, *dp = nullptr;
    if ((rc = kn_alloc(tmp.a, nq * m.n_states, &ds)) || (rc = kn_alloc(tmp.a, nq * m.n_params, &dp))
        || (rc = kn_table_upload(h->stream, states, ds, W.nq, m.n_states))
        || (rc = kn_table_upload(h->stream, params, dp, W.nq, m.n_params)))
      return rc;
    W.states = ds; W.params = dp;
  }
  T.n_watch = 1;
  T.bstart[1] = (W.nq + kn_monitor_chunk() - 1) / kn_monitor_chunk();
  KnMonTab* d_tab = nullptr;
  double* fld = nullptr;
  if ((rc = kn_upload(tmp.a, &T, 1, &d_tab)) || (rc = kn_alloc(tmp.a, n, &fld)) || (rc = kn_wait_ode_joins(h))
      || (rc = kn_launch_monitor_eval(h, d_tab, W.nq, t, fld, m.mon_kernel[1])))
    return rc;
  return kn_to_host(h->stream, out, fld, n);   // synchronises: the scratch memory is no longer read
}

// ---------------------------------------------------------------------------------------------------
// field snapshots (kernels_snapshot.hip)
// ---------------------------------------------------------------------------------------------------
namespace {
const char* const SNAP_NONE = "no snapshots set (knpemi_snapshot_set)";
size_t snap_align(size_t n) { return (n + KNPEMI_SNAPSHOT_ALIGN - 1) / KNPEMI_SNAPSHOT_ALIGN * KNPEMI_SNAPSHOT_ALIGN; }

// -- the ring of a snapshot recorder (KnFrameRing), on either handle: `own` gives the device and the main stream, `fn` the
// entry point's name for the error texts
// the copy stream, the "packed" event and `depth` slots of R.frame_bytes; the device frames go to `allocs`.  A return
// before the end leaves what exists to the owner's recorder_free
int ring_alloc(KnFrameRing& R, std::vector<void*>& allocs, int depth) {
  R.depth = depth;
  KN_HIP(hipStreamCreateWithFlags(&R.copy, hipStreamNonBlocking));
  KN_HIP(hipEventCreateWithFlags(&R.ev_packed, hipEventDisableTiming));
  R.t_of.assign((size_t)depth, 0.0);
  for (int s = 0; s < depth; ++s) {
    char* d = nullptr;
    if (int rc = kn_alloc(allocs, R.frame_bytes, &d)) return rc;
    R.dev.push_back(d);
    void* host = nullptr;
    KN_HIP(hipHostMalloc(&host, R.frame_bytes, hipHostMallocDefault));
    R.pinned.push_back(static_cast<char*>(host));
    hipEvent_t e = nullptr;
    KN_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    R.copied.push_back(e);
  }
  return KNPEMI_OK;
}
bool ring_full(const KnFrameRing& R) { return R.seq - R.tail >= R.depth; }
// frame seq at time t into slot seq % depth, which is FREE: the host has taken its previous frame, so that copy is done
// and the device frame may be overwritten.  pack(frame) enqueues the pack launch on the main stream; behind it the copy
// stream takes the frame to pinned memory.  Nothing is synchronised
template <class Pack>
int ring_record(KnDevice* own, KnFrameRing& R, double t, Pack pack) {
  const size_t slot = (size_t)(R.seq % R.depth);
  if (int rc = pack(R.dev[slot])) return rc;
  KN_HIP(hipEventRecord(R.ev_packed, own->stream));
  KN_HIP(hipStreamWaitEvent(R.copy, R.ev_packed, 0));
  KN_HIP(hipMemcpyAsync(R.pinned[slot], R.dev[slot], R.frame_bytes, hipMemcpyDeviceToHost, R.copy));
  KN_HIP(hipEventRecord(R.copied[slot], R.copy));
  R.t_of[slot] = t;
  ++R.seq;
  return KNPEMI_OK;
}
// the oldest frame in flight into `out`; 1 with nothing in flight, KNPEMI_EBUSY (wait == 0) while its copy runs
int ring_take(KnDevice* own, KnFrameRing& R, const std::string& fn, const char* layout_call, int wait, void* out, size_t bytes,
              double* t, int64_t* seq) {
  if (R.tail == R.seq) return 1;
  if (!out || bytes != R.frame_bytes) return kn_fail(KNPEMI_EINVAL, fn + ": the buffer must hold one frame (" + layout_call + ")");
  KN_HIP(hipSetDevice(own->device));
  const size_t slot = (size_t)(R.tail % R.depth);
  if (!wait) {
    const hipError_t e = hipEventQuery(R.copied[slot]);
    if (e == hipErrorNotReady) {
      (void)hipGetLastError();      // not an error: the next launch check must not see it
      return kn_fail(KNPEMI_EBUSY, fn + ": the oldest frame's copy has not finished");
    }
    KN_HIP(e);
  } else {
    KN_HIP(hipEventSynchronize(R.copied[slot]));
  }
  std::memcpy(out, R.pinned[slot], bytes);
  if (t) *t = R.t_of[slot];
  if (seq) *seq = R.tail;
  ++R.tail;
  return KNPEMI_OK;
}
// wait for the copy stream, free every slot, restart seq at 0
int ring_reset(KnDevice* own, KnFrameRing& R) {
  KN_HIP(hipSetDevice(own->device));
  KN_HIP(hipStreamSynchronize(R.copy));
  R.seq = R.tail = 0;
  return KNPEMI_OK;
}
}  // namespace

extern "C" int knpemi_snapshot_set(knpemi_handle* h, int n_watch, const int32_t* spec, int n_space_sel, const int32_t* sel_space,
                                   const int64_t* sel_off, const int32_t* sel_idx, int depth) {
  using KnSnap = knpemi_handle::KnSnap;
  const std::string fn = "knpemi_snapshot_set";
  if (!h || !spec || (n_space_sel > 0 && (!sel_space || !sel_off || !sel_idx))) return kn_fail(KNPEMI_EINVAL, fn + ": null argument");
  if (h->ode_only) return kn_fail(KNPEMI_EINVAL, fn + ": a handle of knpemi_ode_create has no fields");
  if (n_watch < 1 || n_watch > KNPEMI_SNAPSHOT_MAX_WATCH)
    return kn_fail(KNPEMI_EINVAL, fn + ": 1 to KNPEMI_SNAPSHOT_MAX_WATCH watches");
  if (depth < 1 || depth > (1 << 16)) return kn_fail(KNPEMI_EINVAL, fn + ": depth must be positive (and at most 65536)");
  if (n_space_sel < 0 || n_space_sel > KN_MAPS_MAXSPACE) return kn_fail(KNPEMI_EINVAL, fn + ": bad number of selections");
  // the space of a watch: the vertices of sub-domain s (s), or the membrane dofs of cell s (KN_MAXSUB + s)
  int space[KNPEMI_SNAPSHOT_MAX_WATCH], per_space[KN_MAPS_MAXSPACE] = {};
  KnFieldLoc loc[KNPEMI_SNAPSHOT_MAX_WATCH];
  for (int w = 0; w < n_watch; ++w) {
    const int32_t field = spec[4 * w], sub = spec[4 * w + 1], ix = spec[4 * w + 2], fl = spec[4 * w + 3];
    const std::string who = fn + ": watch " + std::to_string(w);
    bool mem = false;
    switch (field) {
      case KNPEMI_F_PHI: case KNPEMI_F_C: case KNPEMI_F_C_PREV: case KNPEMI_F_C_ELIM:
        if (int rc = kn_locate(h, field, sub, ix, &loc[w])) return rc;      // sub / idx out of range
        break;
      case KNPEMI_F_I_CH:
        if (ix < 0) return kn_fail(KNPEMI_EINVAL, who + ": bad I_ch index");
        [[fallthrough]];
      case KNPEMI_F_PHI_M:
        if (int rc = kn_locate(h, field, sub, ix, &loc[w])) return rc;      // ... and phi_M, I_ch on the ECS
        mem = true;
        break;
      case KNPEMI_F_ODE_STATE: {
        if (sub < 1 || sub >= h->n_sub) return kn_fail(KNPEMI_EINVAL, who + ": a state lives on the membrane of a cell (sub >= 1)");
        const int model = ix / KNPEMI_SNAPSHOT_STATE_STRIDE, state = ix % KNPEMI_SNAPSHOT_STATE_STRIDE;
        if (ix < 0 || model >= h->n_models[sub]) return kn_fail(KNPEMI_EINVAL, who + ": membrane model index out of range");
        const KnOdeModel& m = h->sweeps.ode[h->moff[sub] + model];
        if (!m.bound || !m.d_states) return kn_fail(KNPEMI_EINVAL, who + ": membrane model not bound (knpemi_ode_bind)");
        if (state >= m.n_states) return kn_fail(KNPEMI_EINVAL, who + ": state index out of range");
        if (m.nq != h->n_q[sub]) return kn_fail(KNPEMI_EINVAL, who + ": the state table does not cover the membrane dofs");
        loc[w] = {m.d_states + (size_t)state * m.nq, 1, (size_t)m.nq};
        mem = true;
        break;
      }
      default:
        return kn_fail(KNPEMI_EINVAL, who + ": unknown field (phi, c, c_prev, the eliminated ion's c, phi_M, I_ch or a state)");
    }
    if (fl & ~KNPEMI_SNAPSHOT_F32) return kn_fail(KNPEMI_EINVAL, who + ": unknown flag bits");
    for (int u = 0; u < w; ++u)
      if (std::equal(spec + 4 * u, spec + 4 * u + 4, spec + 4 * w)) return kn_fail(KNPEMI_EINVAL, who + " is listed twice");
    space[w] = mem ? KN_MAXSUB + sub : sub;
    ++per_space[space[w]];
    const size_t n_src = (size_t)(mem ? h->n_q[sub] : h->n_vert[sub]);
    if (loc[w].n != n_src || n_src > (size_t)INT32_MAX) return kn_fail(KNPEMI_EINVAL, who + ": field length is not the space's");
  }
  // the selections: ascending distinct items of a watched space, one list per space at most
  const int32_t* sel_of[KN_MAPS_MAXSPACE] = {};
  int sel_n[KN_MAPS_MAXSPACE] = {};
  for (int j = 0; j < n_space_sel; ++j) {
    const int sp = sel_space[j];
    const std::string who = fn + ": selection " + std::to_string(j);
    if (sp < 0 || sp >= KN_MAPS_MAXSPACE || !per_space[sp]) return kn_fail(KNPEMI_EINVAL, who + ": not a watched space");
    if (sel_of[sp]) return kn_fail(KNPEMI_EINVAL, who + ": the space has a selection already");
    const int64_t lo = sel_off[j], hi = sel_off[j + 1];
    const int sub = sp >= KN_MAXSUB ? sp - KN_MAXSUB : sp;
    const int64_t n_src = sp >= KN_MAXSUB ? h->n_q[sub] : h->n_vert[sub];
    if (lo < 0 || hi <= lo || hi - lo > n_src) return kn_fail(KNPEMI_EINVAL, who + ": empty, or longer than the space");
    for (int64_t e = lo; e < hi; ++e)
      if (sel_idx[e] < 0 || sel_idx[e] >= n_src || (e > lo && sel_idx[e] <= sel_idx[e - 1]))
        return kn_fail(KNPEMI_EINVAL, who + ": indices must be ascending, distinct and inside the space");
    sel_of[sp] = sel_idx + lo;
    sel_n[sp] = (int)(hi - lo);
  }
  // the frame: the watches in the order given, each at a multiple of KNPEMI_SNAPSHOT_ALIGN
  New<KnSnap> N;
  KnSnapTab& T = N.host;
  size_t off[KNPEMI_SNAPSHOT_MAX_WATCH], end = 0;
  for (int w = 0; w < n_watch; ++w) {
    const size_t n = sel_of[space[w]] ? (size_t)sel_n[space[w]] : loc[w].n;
    off[w] = snap_align(end);
    end = off[w] + n * ((spec[4 * w + 3] & KNPEMI_SNAPSHOT_F32) ? 4 : 8);
    N.items_of[w] = (long long)n;
  }
  N.frame_bytes = std::max<size_t>(snap_align(end), KNPEMI_SNAPSHOT_ALIGN);
  KN_HIP(hipSetDevice(h->device));
  // the table, grouped by space
  int k = 0;
  for (int sp = 0; sp < KN_MAPS_MAXSPACE; ++sp) {
    if (!per_space[sp]) continue;
    const int p = T.n_space++;
    const bool mem = sp >= KN_MAXSUB;
    const int sub = mem ? sp - KN_MAXSUB : sp;
    T.n_items[p] = sel_of[sp] ? sel_n[sp] : (mem ? h->n_q[sub] : h->n_vert[sub]);
    T.first[p] = mem ? 0 : h->voff[sub];
    T.bstart[p + 1] = T.bstart[p] + (T.n_items[p] + 255) / 256;
    T.wstart[p] = k;
    if (sel_of[sp])
      if (int rc = kn_upload(N.allocs, sel_of[sp], (size_t)sel_n[sp], &T.sel[p])) return rc;
    for (int w = 0; w < n_watch; ++w) {
      if (space[w] != sp) continue;
      KnSnapWatch& W = T.w[k];
      W = KnSnapWatch{};
      const bool f32 = spec[4 * w + 3] & KNPEMI_SNAPSHOT_F32;
      if (loc[w].stride == 1) {
        W.dense = loc[w].base;
        N.move_bytes += 8LL * T.n_items[p];
      } else {      // a slot of the vertex records: every read of the kernel stays inside the record of a vertex of `sub`
        W.slot = (int)((loc[w].base - h->dev.VR) % KN_REC);
        if (loc[w].stride != KN_REC || W.slot < 3) return kn_fail(KNPEMI_EINVAL, fn + ": field layout not understood");
        T.need_rec[p] = 1;
      }
      W.f32 = f32 ? 1 : 0;
      W.off = (long long)off[w];
      N.move_bytes += (f32 ? 4LL : 8LL) * T.n_items[p];
      N.slot_of[w] = k++;
    }
    if (T.need_rec[p]) N.move_bytes += 40LL * T.n_items[p];
    T.wstart[p + 1] = k;
  }
  T.n_watch = n_watch;
  N.n_watch = n_watch;
  N.n_blk = T.bstart[T.n_space];
  if (int rc = kn_upload(N.allocs, &T, 1, &N.tab)) return rc;
  // the ring; a return from here on frees what exists of it (recorder_free)
  if (int rc = ring_alloc(N, N.allocs, depth)) return rc;
  return recorder_install(h, &knpemi_handle::snap, N);
}

extern "C" int knpemi_snapshot_layout(knpemi_handle* h, int64_t* offset, int64_t* n_items, int64_t* frame_bytes) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  const auto& S = h->snap;
  if (S.n_watch == 0) return kn_fail(KNPEMI_EINVAL, std::string("knpemi_snapshot_layout: ") + SNAP_NONE);
  for (int w = 0; w < S.n_watch; ++w) {
    if (offset) offset[w] = (int64_t)S.host.w[S.slot_of[w]].off;
    if (n_items) n_items[w] = (int64_t)S.items_of[w];
  }
  if (frame_bytes) *frame_bytes = (int64_t)S.frame_bytes;
  return KNPEMI_OK;
}

extern "C" int knpemi_snapshot_record(knpemi_handle* h, double t) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  auto& S = h->snap;
  if (S.n_watch == 0) return kn_fail(KNPEMI_EINVAL, std::string("knpemi_snapshot_record: ") + SNAP_NONE);
  if (!std::isfinite(t)) return kn_fail(KNPEMI_EINVAL, "knpemi_snapshot_record: t must be finite");
  if (ring_full(S))
    return kn_fail(KNPEMI_EBUSY, "knpemi_snapshot_record: every slot is in flight (knpemi_snapshot_take frees the oldest)");
  KN_HIP(hipSetDevice(h->device));
  // the pack reads phi_M, I_ch and the state tables, which the ODE sweeps may write on the auxiliary streams
  if (int rc = kn_wait_ode_joins(h)) return rc;
  return ring_record(h, S, t, [&](char* frame) { return kn_launch_snapshot_pack(h, frame); });
}

extern "C" int knpemi_snapshot_take(knpemi_handle* h, int wait, void* out, size_t bytes, double* t, int64_t* seq) {
  const std::string fn = "knpemi_snapshot_take";
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  auto& S = h->snap;
  if (S.n_watch == 0) return kn_fail(KNPEMI_EINVAL, fn + ": " + SNAP_NONE);
  return ring_take(h, S, fn, "knpemi_snapshot_layout", wait, out, bytes, t, seq);
}

extern "C" int knpemi_snapshot_pending(knpemi_handle* h) { return h ? (int)(h->snap.seq - h->snap.tail) : 0; }

extern "C" int knpemi_snapshot_reset(knpemi_handle* h) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  auto& S = h->snap;
  if (S.n_watch == 0) return kn_fail(KNPEMI_EINVAL, std::string("knpemi_snapshot_reset: ") + SNAP_NONE);
  return ring_reset(h, S);
}

extern "C" int knpemi_snapshot_clear(knpemi_handle* h) { return recorder_clear(h, &knpemi_handle::snap); }

// the bytes one pack launch must move by the algorithm: 40 read per bulk item of a space with a record field, 8 per item
// of every dense watch, and the 4 or 8 written per item of every watch (the selection's indices are not counted)
extern "C" long long kn_snapshot_bytes(knpemi_handle* h) { return h ? h->snap.move_bytes : 0; }

// tools/recorder_cost.py: n pack launches back to back into the device frame of the next slot, which must be FREE; no
// copy, no frame recorded
extern "C" int kn_snapshot_pack_only(knpemi_handle* h, int n) {
  if (!h || h->snap.n_watch == 0 || n < 0) return kn_fail(KNPEMI_EINVAL, std::string("kn_snapshot_pack_only: ") + SNAP_NONE);
  auto& S = h->snap;
  if (ring_full(S)) return kn_fail(KNPEMI_EBUSY, "kn_snapshot_pack_only: every slot is in flight");
  KN_HIP(hipSetDevice(h->device));
  for (int i = 0; i < n; ++i)
    if (int rc = kn_launch_snapshot_pack(h, S.dev[(size_t)(S.seq % S.depth)])) return rc;
  return KNPEMI_OK;
}

// ---------------------------------------------------------------------------------------------------
// the DG handle's recorders (knpemi_dg_observe_*, knpemi_dg_events_*): the state, the install rule, the series routines
// and the kernels above, on the fields of a knpemi_dg; the jump seminorms are kernels_dg_record.hip's
// ---------------------------------------------------------------------------------------------------
void kn_dg_record_free(knpemi_dg* h) {
  kn_free_all(h->obs.allocs);
  kn_free_all(h->events.allocs);
  kn_free_all(h->balance.allocs);
  recorder_free(h->snap);
}

namespace {
KnEvSamples dg_samples(const knpemi_dg* h) { return {h->dev.phiM, h->dev.nq}; }

// the table, the partials and the ticket of dg_jump_kernel: once per handle, in its `allocs`
int dg_jump_alloc(knpemi_dg* h) {
  KnDgJump& J = h->jump;
  if (J.tab) return KNPEMI_OK;
  KnDgJump N;
  N.n_blk = kn_dg_jump_blocks(h->dev.n_cell, h->NV);
  int rc;
  if ((rc = kn_zeros(h->allocs, h->stream, (size_t)KN_MAXSUB * KN_DG_JSLOTS, &N.tab))
      || (rc = kn_zeros(h->allocs, h->stream, (size_t)N.n_blk * h->n_sub * KN_DG_JSLOTS, &N.part))
      || (rc = kn_zeros(h->allocs, h->stream, 4, &N.ctl)))
    return rc;
  J = N;
  return KNPEMI_OK;
}
}  // namespace

extern "C" int knpemi_dg_observe_set(knpemi_dg* h, int n_obs, const int32_t* spec, const int64_t* ptr, const int32_t* idx,
                                     const double* w, const double* denom, int capacity) {
  const std::string fn = "knpemi_dg_observe_set";
  if (!h || !spec || !ptr || !denom || !idx || !w) return kn_fail(KNPEMI_EINVAL, fn + ": null argument");
  KN_HIP(hipSetDevice(h->device));
  bool jump = false;
  for (int o = 0; o < n_obs; ++o) jump = jump || spec[4 * o] == KNPEMI_DG_JUMP;
  if (jump)
    if (int rc = dg_jump_alloc(h)) return rc;
  const kn_dg::DgDev& D = h->dev;
  auto locate = [&](int o, int field, int sub, int ix, KnFieldLoc* L) {
    const std::string who = fn + ": observable " + std::to_string(o);
    switch (field) {
      case KNPEMI_DG_C:
        if (ix < 0 || ix >= h->K) return kn_fail(KNPEMI_EINVAL, who + ": ion index out of range");
        *L = {D.rec + KN_CSLOT(ix), KN_REC, (size_t)D.n_dof};
        return KNPEMI_OK;
      case KNPEMI_DG_PHI: *L = {D.rec + 7, KN_REC, (size_t)D.n_dof}; return KNPEMI_OK;
      case KNPEMI_DG_PHI_M: *L = {D.phiM, 1, (size_t)D.nq}; return KNPEMI_OK;
      case KNPEMI_DG_JUMP:
        if (sub < 0 || sub >= h->n_sub) return kn_fail(KNPEMI_EINVAL, who + ": bad sub-domain index");
        if (ix < -1 || ix >= h->K) return kn_fail(KNPEMI_EINVAL, who + ": ion index out of range (-1: the potential)");
        if (spec[4 * o + 3] != KNPEMI_OBS_SUM) return kn_fail(KNPEMI_EINVAL, who + ": a jump seminorm is a KNPEMI_OBS_SUM entry");
        *L = {h->jump.tab + (size_t)sub * KN_DG_JSLOTS + (ix < 0 ? KN_MAXK : ix), 1, 1};
        return KNPEMI_OK;
    }
    return kn_fail(KNPEMI_EINVAL, who + ": unknown field (KNPEMI_DG_C, _PHI, _PHI_M or _JUMP)");
  };
  New<knpemi_handle::KnObserve> O;
  if (int rc = observe_build(h, fn, n_obs, spec, ptr, idx, w, denom, capacity, false, true, locate, O)) return rc;
  if (int rc = recorder_install(h, &knpemi_dg::obs, O)) return rc;
  h->obs_jump = jump;
  return KNPEMI_OK;
}

extern "C" int knpemi_dg_observe_record(knpemi_dg* h) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  if (h->obs.n_obs == 0) return kn_fail(KNPEMI_EINVAL, "knpemi_dg_observe_record: no observables set (knpemi_dg_observe_set)");
  if (!h->have_params) return kn_fail(KNPEMI_EINVAL, "knpemi_dg_observe_record: knpemi_dg_set_params has not been called");
  KN_HIP(hipSetDevice(h->device));
  if (h->obs_jump)
    if (int rc = kn_dg_launch_jump(h, h->dev, h->NV, h->n_sub, h->hex_box, h->jump)) return rc;
  return kn_launch_observe(h, h->obs);
}

extern "C" int knpemi_dg_observe_read(knpemi_dg* h, int n_rows, double* out, int64_t* rows, int64_t* overflow, int reset) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  return series_read(h, h->obs.ser, h->obs.n_obs != 0, "knpemi_dg_observe_read", "no observables set (knpemi_dg_observe_set)",
                     n_rows, out, rows, overflow, reset);
}

extern "C" int knpemi_dg_observe_clear(knpemi_dg* h) {
  if (int rc = recorder_clear(h, &knpemi_dg::obs)) return rc;
  h->obs_jump = false;
  return KNPEMI_OK;
}

extern "C" int knpemi_dg_events_set(knpemi_dg* h, double threshold, double reset, int keep) {
  const std::string fn = "knpemi_dg_events_set";
  if (!h) return kn_fail(KNPEMI_EINVAL, fn + ": null argument");
  if (keep < 0 || keep > KNPEMI_EVENTS_MAX_KEEP) return kn_fail(KNPEMI_EINVAL, fn + ": keep must be in 0..KNPEMI_EVENTS_MAX_KEEP");
  if (!(reset <= threshold)) return kn_fail(KNPEMI_EINVAL, fn + ": reset must not exceed the threshold");
  if (h->dev.nq == 0) return kn_fail(KNPEMI_EINVAL, fn + ": the mesh has no membrane facets");
  // one segment: every membrane node, in node order
  KnEvTab T{};
  bool watched[KN_MAXSUB] = {};
  T.n_watch = 1; T.gstart[1] = h->dev.nq; T.q0[0] = 0; T.sub[0] = 0;
  T.threshold[0] = threshold; T.reset[0] = reset;
  watched[0] = true;
  KN_HIP(hipSetDevice(h->device));
  New<knpemi_handle::KnEvents> E;
  int rc;
  if ((rc = events_build(T, (size_t)h->dev.nq, keep, watched, E))) return rc;
  if ((rc = recorder_install(h, &knpemi_dg::events, E))) return rc;
  if ((rc = kn_launch_events_reset(h, h->events, dg_samples(h)))) recorder_free(h->events);
  return rc;
}

extern "C" int knpemi_dg_events_record(knpemi_dg* h, double t) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  auto& E = h->events;
  if (E.n_watch == 0) return kn_fail(KNPEMI_EINVAL, "knpemi_dg_events_record: no events set (knpemi_dg_events_set)");
  if (!h->have_params) return kn_fail(KNPEMI_EINVAL, "knpemi_dg_events_record: knpemi_dg_set_params has not been called");
  if (int rc = clock_accept(E.clock, "knpemi_dg_events_record", t)) return rc;
  KN_HIP(hipSetDevice(h->device));
  if (int rc = kn_launch_events_record(h, E, dg_samples(h), E.clock.have_prev ? 0 : 1, t, E.clock.t_prev)) return rc;
  clock_advance(E.clock, t);
  return KNPEMI_OK;
}

extern "C" int knpemi_dg_events_read(knpemi_dg* h, int32_t* count, double* t_first, double* t_last, double* v_peak,
                                     double* t_peak, double* ring) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  if (h->events.n_watch == 0) return kn_fail(KNPEMI_EINVAL, "knpemi_dg_events_read: no events set (knpemi_dg_events_set)");
  return events_copy_out(h, h->events, 0, (size_t)h->dev.nq, (size_t)h->dev.nq, count, t_first, t_last, v_peak, t_peak, ring);
}

extern "C" int knpemi_dg_events_reset(knpemi_dg* h) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  auto& E = h->events;
  if (E.n_watch == 0) return kn_fail(KNPEMI_EINVAL, "knpemi_dg_events_reset: no events set (knpemi_dg_events_set)");
  KN_HIP(hipSetDevice(h->device));
  clock_restart(E.clock);
  return kn_launch_events_reset(h, E, dg_samples(h));
}

extern "C" int knpemi_dg_events_clear(knpemi_dg* h) { return recorder_clear(h, &knpemi_dg::events); }

// ---------------------------------------------------------------------------------------------------
// the per-cell ion balance of a DG run (kernels_dg_balance.hip)
// ---------------------------------------------------------------------------------------------------
extern "C" int knpemi_dg_balance_set(knpemi_dg* h, int capacity, int want_cells, int n_tags, const int32_t* facet_tag) {
  const std::string fn = "knpemi_dg_balance_set";
  if (!h) return kn_fail(KNPEMI_EINVAL, fn + ": null argument");
  const int nmf = h->dev.nq / h->NFV;
  if (capacity < 1) return kn_fail(KNPEMI_EINVAL, fn + ": capacity must be positive");
  if (n_tags < 0 || n_tags > KN_DG_MAXTAG) return kn_fail(KNPEMI_EINVAL, fn + ": 0 to " + std::to_string(KN_DG_MAXTAG) + " membrane tags");
  if (nmf > 0 && (n_tags < 1 || !facet_tag)) return kn_fail(KNPEMI_EINVAL, fn + ": the mesh has membrane facets: a tag index per facet is required");
  for (int i = 0; i < nmf; ++i)
    if (facet_tag[i] < 0 || facet_tag[i] >= n_tags)
      return kn_fail(KNPEMI_EINVAL, fn + ": tag index of membrane facet " + std::to_string(i) + " out of range");
  KN_HIP(hipSetDevice(h->device));
  New<KnDgBalance> B;
  const int K = h->K, ns = h->n_sub * K * KN_DG_BSLOTS;
  B.n_blk = kn_dg_balance_blocks(h->dev.n_cell, h->NV);
  B.n_tag = n_tags;
  B.want_cells = want_cells != 0;
  int rc;
  if ((rc = series_alloc(B.allocs, h->stream, capacity, ns + n_tags * (2 * K + 3), &B.ser))
      || (rc = kn_zeros(B.allocs, h->stream, (size_t)h->dev.n_cell * K * KN_DG_BCOLS, &B.cells))
      || (rc = kn_zeros(B.allocs, h->stream, (size_t)B.n_blk * ns, &B.part))
      || (rc = kn_zeros(B.allocs, h->stream, (size_t)B.n_blk * n_tags * KN_DG_BTAG, &B.mpart))
      || (rc = kn_zeros(B.allocs, h->stream, (size_t)KN_DG_MAXTAG * KN_DG_BTAG, &B.tagtab))
      || (rc = kn_zeros(B.allocs, h->stream, 4, &B.mctl))
      || (rc = kn_upload(B.allocs, facet_tag, (size_t)nmf, &B.facet_tag)))
    return rc;
  B.set = true;
  return recorder_install(h, &knpemi_dg::balance, B);
}

namespace {
int balance_ready(knpemi_dg* h, const std::string& fn) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  if (!h->balance.set) return kn_fail(KNPEMI_EINVAL, fn + ": no balance set (knpemi_dg_balance_set)");
  if (!h->have_params) return kn_fail(KNPEMI_EINVAL, fn + ": knpemi_dg_set_params has not been called");
  return KNPEMI_OK;
}
}  // namespace

extern "C" int knpemi_dg_balance_record_membrane(knpemi_dg* h) {
  if (int rc = balance_ready(h, "knpemi_dg_balance_record_membrane")) return rc;
  KN_HIP(hipSetDevice(h->device));
  if (int rc = kn_dg_launch_balance_membrane(h, !(h->knp_flags & KNPEMI_NO_SPLITTING))) return rc;
  h->balance.membrane = true;
  return KNPEMI_OK;
}

extern "C" int knpemi_dg_balance_record(knpemi_dg* h, double t) {
  const std::string fn = "knpemi_dg_balance_record";
  if (int rc = balance_ready(h, fn)) return rc;
  if (!h->balance.membrane)
    return kn_fail(KNPEMI_EINVAL, fn + ": no knpemi_dg_balance_record_membrane since the last record");
  if (!std::isfinite(t)) return kn_fail(KNPEMI_EINVAL, fn + ": t must be finite");
  KN_HIP(hipSetDevice(h->device));
  if (int rc = kn_dg_launch_balance_flux(h)) return rc;
  h->balance.membrane = false;
  h->balance.recorded = true;
  return KNPEMI_OK;
}

extern "C" int knpemi_dg_balance_read(knpemi_dg* h, int n_rows, double* out, int64_t* rows, int64_t* overflow, int reset) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  return series_read(h, h->balance.ser, h->balance.set, "knpemi_dg_balance_read", "no balance set (knpemi_dg_balance_set)",
                     n_rows, out, rows, overflow, reset);
}

extern "C" int knpemi_dg_balance_cells(knpemi_dg* h, double* out) {
  const std::string fn = "knpemi_dg_balance_cells";
  if (!h || !out) return kn_fail(KNPEMI_EINVAL, fn + ": null argument");
  const KnDgBalance& B = h->balance;
  if (!B.set) return kn_fail(KNPEMI_EINVAL, fn + ": no balance set (knpemi_dg_balance_set)");
  if (!B.want_cells) return kn_fail(KNPEMI_EINVAL, fn + ": the balance was set without the cell table (want_cells = 0)");
  if (!B.recorded) return kn_fail(KNPEMI_EINVAL, fn + ": no record yet (knpemi_dg_balance_record)");
  KN_HIP(hipSetDevice(h->device));
  return kn_table_download(h->stream, B.cells, out, h->dev.n_cell, h->K * KN_DG_BCOLS);      // device: [K][columns][n_cell]
}

extern "C" int knpemi_dg_balance_reset(knpemi_dg* h) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  KnDgBalance& B = h->balance;
  if (!B.set) return kn_fail(KNPEMI_EINVAL, "knpemi_dg_balance_reset: no balance set (knpemi_dg_balance_set)");
  KN_HIP(hipSetDevice(h->device));
  B.membrane = B.recorded = false;
  return series_rewind(h, B.ser);
}

extern "C" int knpemi_dg_balance_clear(knpemi_dg* h) { return recorder_clear(h, &knpemi_dg::balance); }

// ---------------------------------------------------------------------------------------------------
// field snapshots of a DG run (kernels_dg_snapshot.hip): the table is the DG handle's, the ring the conforming path's
// ---------------------------------------------------------------------------------------------------
namespace {
const char* const DG_SNAP_NONE = "no snapshots set (knpemi_dg_snapshot_set)";
}  // namespace

extern "C" int knpemi_dg_snapshot_set(knpemi_dg* h, int n_watch, const int32_t* spec, int n_space, const int32_t* space,
                                      const int64_t* list_off, const int32_t* list, int n_space_sel, const int32_t* sel_space,
                                      const int64_t* sel_off, const int32_t* sel_idx, int depth) {
  const std::string fn = "knpemi_dg_snapshot_set";
  if (!h || !spec || !space || !list_off || !list || (n_space_sel > 0 && (!sel_space || !sel_off || !sel_idx)))
    return kn_fail(KNPEMI_EINVAL, fn + ": null argument");
  if (n_watch < 1 || n_watch > KNPEMI_SNAPSHOT_MAX_WATCH)
    return kn_fail(KNPEMI_EINVAL, fn + ": 1 to KNPEMI_SNAPSHOT_MAX_WATCH watches");
  if (n_space < 1 || n_space > KNPEMI_DG_SNAPSHOT_MAX_SPACE)
    return kn_fail(KNPEMI_EINVAL, fn + ": 1 to KNPEMI_DG_SNAPSHOT_MAX_SPACE spaces");
  if (depth < 1 || depth > (1 << 16)) return kn_fail(KNPEMI_EINVAL, fn + ": depth must be positive (and at most 65536)");
  if (n_space_sel < 0 || n_space_sel > n_space) return kn_fail(KNPEMI_EINVAL, fn + ": bad number of selections");
  const kn_dg::DgDev& D = h->dev;
  // the spaces: every entry the kernel will read is checked here, against the fields' lengths
  if (list_off[0] != 0) return kn_fail(KNPEMI_EINVAL, fn + ": list_off[0] must be 0");
  long long entries[KNPEMI_DG_SNAPSHOT_MAX_SPACE] = {};      // source entries one launch reads per watch of the space
  for (int p = 0; p < n_space; ++p) {
    const int32_t mem = space[4 * p], tag = space[4 * p + 1], form = space[4 * p + 2], n = space[4 * p + 3];
    const std::string who = fn + ": space " + std::to_string(p);
    if (mem != 0 && mem != 1) return kn_fail(KNPEMI_EINVAL, who + ": the kind is 0 (cells of a sub-domain) or 1 (a membrane tag)");
    if (form != KNPEMI_DG_SNAP_BROKEN && form != KNPEMI_DG_SNAP_CELL_MEAN && form != KNPEMI_DG_SNAP_VERTEX)
      return kn_fail(KNPEMI_EINVAL, who + ": unknown form (broken, cell_mean or vertex)");
    if (mem && form == KNPEMI_DG_SNAP_CELL_MEAN) return kn_fail(KNPEMI_EINVAL, who + ": a membrane quantity has no cell_mean form");
    if (tag < 0 || (!mem && tag >= h->n_sub)) return kn_fail(KNPEMI_EINVAL, who + ": unknown tag (sub-domain index out of range)");
    for (int u = 0; u < p; ++u)
      if (std::equal(space + 4 * u, space + 4 * u + 3, space + 4 * p)) return kn_fail(KNPEMI_EINVAL, who + " is listed twice");
    if (n < 1) return kn_fail(KNPEMI_EINVAL, who + " has no items");
    const int64_t lo = list_off[p], len = list_off[p + 1] - lo;
    const int64_t n_src = mem ? D.nq : (form == KNPEMI_DG_SNAP_CELL_MEAN ? D.n_cell : D.n_dof);
    if (len < 0 || lo + len > (int64_t)INT32_MAX) return kn_fail(KNPEMI_EINVAL, who + ": bad list range");
    const int32_t* a = list + lo;
    if (form != KNPEMI_DG_SNAP_VERTEX) {
      if (len != n) return kn_fail(KNPEMI_EINVAL, who + ": the list must hold one entry per item");
      for (int64_t e = 0; e < len; ++e)
        if (a[e] < 0 || a[e] >= n_src) return kn_fail(KNPEMI_EINVAL, who + ": list entry out of range");
      entries[p] = form == KNPEMI_DG_SNAP_CELL_MEAN ? (long long)n * h->NV : n;
    } else {
      if (len < (int64_t)n + 1 || a[0] != 0 || (int64_t)a[n] != len - (n + 1))
        return kn_fail(KNPEMI_EINVAL, who + ": the list must hold vptr [n_items + 1] and then vptr[n_items] entries");
      const int32_t* v = a + n + 1;
      for (int i = 0; i < n; ++i) {
        if (a[i + 1] <= a[i] || a[i + 1] > a[n]) return kn_fail(KNPEMI_EINVAL, who + ": a vertex without entries, or vptr not increasing");
        for (int e = a[i]; e < a[i + 1]; ++e)
          if (v[e] < 0 || v[e] >= n_src || (e > a[i] && v[e] <= v[e - 1]))
            return kn_fail(KNPEMI_EINVAL, who + ": the entries of a vertex must be ascending, distinct and in range");
      }
      entries[p] = a[n];
    }
  }
  // the watches
  int space_of[KNPEMI_SNAPSHOT_MAX_WATCH], per_space[KNPEMI_DG_SNAPSHOT_MAX_SPACE] = {};
  KnSnapWatch src[KNPEMI_SNAPSHOT_MAX_WATCH];
  for (int w = 0; w < n_watch; ++w) {
    const int32_t q = spec[5 * w], tag = spec[5 * w + 1], ix = spec[5 * w + 2], form = spec[5 * w + 3], fl = spec[5 * w + 4];
    const std::string who = fn + ": watch " + std::to_string(w);
    KnSnapWatch& W = src[w];
    W = KnSnapWatch{};
    bool mem = true;
    switch (q) {
      case KNPEMI_DG_C:
        if (ix < 0 || ix >= h->K) return kn_fail(KNPEMI_EINVAL, who + ": ion index out of range");
        W.slot = KN_CSLOT(ix); mem = false;
        break;
      case KNPEMI_DG_PHI: W.slot = 7; mem = false; break;
      case KNPEMI_DG_PHI_M: W.dense = D.phiM; break;
      case KNPEMI_DG_I_CH:
        if (ix < 0 || ix >= h->K) return kn_fail(KNPEMI_EINVAL, who + ": ion index out of range");
        W.dense = D.Ich + (size_t)ix * D.nq;
        break;
      case KNPEMI_DG_ODE_STATE: {
        const KnOdeModel& m = h->sweeps.ode[0];
        if (!m.bound || !m.d_states) return kn_fail(KNPEMI_EINVAL, who + ": no membrane model bound (knpemi_dg_ode_bind)");
        if (ix < 0 || ix >= m.n_states) return kn_fail(KNPEMI_EINVAL, who + ": state index out of range");
        if (m.nq != D.nq) return kn_fail(KNPEMI_EINVAL, who + ": the state table does not cover the membrane nodes");
        W.dense = m.d_states + (size_t)ix * m.nq;
        break;
      }
      default:
        return kn_fail(KNPEMI_EINVAL, who + ": unknown quantity (KNPEMI_DG_C, _PHI, _PHI_M, _I_CH or _ODE_STATE)");
    }
    if (fl & ~KNPEMI_SNAPSHOT_F32) return kn_fail(KNPEMI_EINVAL, who + ": unknown dtype bits");
    for (int u = 0; u < w; ++u)
      if (std::equal(spec + 5 * u, spec + 5 * u + 5, spec + 5 * w)) return kn_fail(KNPEMI_EINVAL, who + " is listed twice");
    int p = 0;
    while (p < n_space && !(space[4 * p] == (mem ? 1 : 0) && space[4 * p + 1] == tag && space[4 * p + 2] == form)) ++p;
    if (p == n_space)
      return kn_fail(KNPEMI_EINVAL, who + ": unknown tag or form: no space (" + (mem ? "membrane tag " : "sub-domain ") +
                                        std::to_string(tag) + ", form " + std::to_string(form) + ") is given");
    W.f32 = (fl & KNPEMI_SNAPSHOT_F32) ? 1 : 0;
    space_of[w] = p;
    ++per_space[p];
  }
  // the selections: ascending distinct items of a watched space, one list per space at most
  const int32_t* sel_of[KNPEMI_DG_SNAPSHOT_MAX_SPACE] = {};
  int sel_n[KNPEMI_DG_SNAPSHOT_MAX_SPACE] = {};
  for (int j = 0; j < n_space_sel; ++j) {
    const int sp = sel_space[j];
    const std::string who = fn + ": selection " + std::to_string(j);
    if (sp < 0 || sp >= n_space || !per_space[sp]) return kn_fail(KNPEMI_EINVAL, who + ": not a watched space");
    if (sel_of[sp]) return kn_fail(KNPEMI_EINVAL, who + ": the space has a selection already");
    const int64_t lo = sel_off[j], hi = sel_off[j + 1], n_src = space[4 * sp + 3];
    if (lo < 0 || hi <= lo || hi - lo > n_src) return kn_fail(KNPEMI_EINVAL, who + ": empty, or longer than the space");
    for (int64_t e = lo; e < hi; ++e)
      if (sel_idx[e] < 0 || sel_idx[e] >= n_src || (e > lo && sel_idx[e] <= sel_idx[e - 1]))
        return kn_fail(KNPEMI_EINVAL, who + ": indices must be ascending, distinct and inside the space");
    sel_of[sp] = sel_idx + lo;
    sel_n[sp] = (int)(hi - lo);
  }
  // the frame: the watches in the order given, each at a multiple of KNPEMI_SNAPSHOT_ALIGN
  New<KnDgSnap> N;
  KnDgSnapTab& T = N.host;
  size_t end = 0;
  for (int w = 0; w < n_watch; ++w) {
    const int p = space_of[w];
    const size_t n = sel_of[p] ? (size_t)sel_n[p] : (size_t)space[4 * p + 3];
    src[w].off = (long long)snap_align(end);
    end = (size_t)src[w].off + n * (src[w].f32 ? 4 : 8);
    N.items_of[w] = (long long)n;
  }
  N.frame_bytes = std::max<size_t>(snap_align(end), KNPEMI_SNAPSHOT_ALIGN);
  KN_HIP(hipSetDevice(h->device));
  // the table, grouped by space; the spaces nothing watches are left out
  int k = 0;
  for (int sp = 0; sp < n_space; ++sp) {
    if (!per_space[sp]) continue;
    const int p = T.n_space++;
    const int32_t mem = space[4 * sp], form = space[4 * sp + 2], n = space[4 * sp + 3];
    const int32_t* a = list + list_off[sp];
    T.n_items[p] = sel_of[sp] ? sel_n[sp] : n;
    T.form[p] = form;
    T.bulk[p] = mem ? 0 : 1;
    T.nv[p] = h->NV;
    T.bstart[p + 1] = T.bstart[p] + (T.n_items[p] + 255) / 256;
    T.wstart[p] = k;
    const double frac = (double)T.n_items[p] / (double)n;      // of the space's entries, with a selection (an estimate)
    const long long n_read = (long long)((double)entries[sp] * frac);
    long long idx_bytes = sel_of[sp] ? 4LL * sel_n[sp] : 0;
    if (sel_of[sp])
      if (int rc = kn_upload(N.allocs, sel_of[sp], (size_t)sel_n[sp], &T.sel[p])) return rc;
    if (form == KNPEMI_DG_SNAP_VERTEX) {
      if (int rc = kn_upload(N.allocs, a, (size_t)n + 1, &T.vptr[p])) return rc;
      if (int rc = kn_upload(N.allocs, a + n + 1, (size_t)a[n], &T.vdof[p])) return rc;
      idx_bytes += 4LL * T.n_items[p] + 4LL * n_read;
    } else {
      bool run = true;      // one ascending run: first + item, no list on the device
      for (int i = 1; i < n && run; ++i) run = a[i] == a[0] + i;
      T.first[p] = a[0];
      if (!run) {
        if (int rc = kn_upload(N.allocs, a, (size_t)n, &T.src[p])) return rc;
        idx_bytes += 4LL * T.n_items[p];
      }
    }
    int n_w = 0;
    for (int w = 0; w < n_watch; ++w) {
      if (space_of[w] != sp) continue;
      T.w[k] = src[w];
      N.move_bytes += (src[w].f32 ? 4LL : 8LL) * T.n_items[p];
      N.slot_of[w] = k++;
      ++n_w;
    }
    // read: 40 bytes of every record once per space, 8 per entry and watch of a membrane space, and the index lists
    N.move_bytes += (mem ? 8LL * n_w : 40LL) * n_read + idx_bytes;
    T.wstart[p + 1] = k;
  }
  T.n_watch = n_watch;
  N.n_watch = n_watch;
  N.n_blk = T.bstart[T.n_space];
  if (int rc = kn_upload(N.allocs, &T, 1, &N.tab)) return rc;
  // the ring; a return from here on frees what exists of it (recorder_free)
  if (int rc = ring_alloc(N, N.allocs, depth)) return rc;
  return recorder_install(h, &knpemi_dg::snap, N);
}

extern "C" int knpemi_dg_snapshot_layout(knpemi_dg* h, int64_t* offset, int64_t* n_items, int64_t* frame_bytes) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  const auto& S = h->snap;
  if (S.n_watch == 0) return kn_fail(KNPEMI_EINVAL, std::string("knpemi_dg_snapshot_layout: ") + DG_SNAP_NONE);
  for (int w = 0; w < S.n_watch; ++w) {
    if (offset) offset[w] = (int64_t)S.host.w[S.slot_of[w]].off;
    if (n_items) n_items[w] = (int64_t)S.items_of[w];
  }
  if (frame_bytes) *frame_bytes = (int64_t)S.frame_bytes;
  return KNPEMI_OK;
}

extern "C" int knpemi_dg_snapshot_record(knpemi_dg* h, double t) {
  const std::string fn = "knpemi_dg_snapshot_record";
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  auto& S = h->snap;
  if (S.n_watch == 0) return kn_fail(KNPEMI_EINVAL, fn + ": " + DG_SNAP_NONE);
  if (!h->have_params) return kn_fail(KNPEMI_EINVAL, fn + ": knpemi_dg_set_params has not been called");
  if (!std::isfinite(t) || (S.clock_set && !(t > S.t_prev)))
    return kn_fail(KNPEMI_EINVAL, fn + ": t must be finite and greater than the previous record's");
  if (ring_full(S))
    return kn_fail(KNPEMI_EBUSY, fn + ": every slot is in flight (knpemi_dg_snapshot_take frees the oldest)");
  KN_HIP(hipSetDevice(h->device));
  // the membrane sweep of a DG handle runs on the main stream: the pack launch is behind it without a join
  if (int rc = ring_record(h, S, t, [&](char* frame) { return kn_dg_launch_snapshot_pack(h, S, h->dev.rec, frame); })) return rc;
  S.clock_set = true;
  S.t_prev = t;
  return KNPEMI_OK;
}

extern "C" int knpemi_dg_snapshot_take(knpemi_dg* h, int wait, void* out, size_t bytes, double* t, int64_t* seq) {
  const std::string fn = "knpemi_dg_snapshot_take";
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  if (h->snap.n_watch == 0) return kn_fail(KNPEMI_EINVAL, fn + ": " + DG_SNAP_NONE);
  return ring_take(h, h->snap, fn, "knpemi_dg_snapshot_layout", wait, out, bytes, t, seq);
}

extern "C" int knpemi_dg_snapshot_pending(knpemi_dg* h) { return h ? (int)(h->snap.seq - h->snap.tail) : 0; }

extern "C" int knpemi_dg_snapshot_reset(knpemi_dg* h) {
  if (!h) return kn_fail(KNPEMI_EINVAL, "null handle");
  auto& S = h->snap;
  if (S.n_watch == 0) return kn_fail(KNPEMI_EINVAL, std::string("knpemi_dg_snapshot_reset: ") + DG_SNAP_NONE);
  S.clock_set = false;
  return ring_reset(h, S);
}

extern "C" int knpemi_dg_snapshot_clear(knpemi_dg* h) { return recorder_clear(h, &knpemi_dg::snap); }

// the bytes one pack launch moves by the algorithm: 40 read per gathered record of a bulk space, 8 per gathered entry of
// every membrane watch, the index lists (selection, source list, vptr and vdof: 4 each) and the 4 or 8 written per item of
// every watch
extern "C" long long kn_dg_snapshot_bytes(knpemi_dg* h) { return h ? h->snap.move_bytes : 0; }

// tools/dg_snapshot_time.py: n pack launches back to back into the device frame of the next slot, which must be FREE; no
// copy, no frame recorded
extern "C" int kn_dg_snapshot_pack_only(knpemi_dg* h, int n) {
  if (!h || h->snap.n_watch == 0 || n < 0) return kn_fail(KNPEMI_EINVAL, std::string("kn_dg_snapshot_pack_only: ") + DG_SNAP_NONE);
  auto& S = h->snap;
  if (ring_full(S)) return kn_fail(KNPEMI_EBUSY, "kn_dg_snapshot_pack_only: every slot is in flight");
  KN_HIP(hipSetDevice(h->device));
  for (int i = 0; i < n; ++i)
    if (int rc = kn_dg_launch_snapshot_pack(h, S, h->dev.rec, S.dev[(size_t)(S.seq % S.depth)])) return rc;
  return KNPEMI_OK;
}
