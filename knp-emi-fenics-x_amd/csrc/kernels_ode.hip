// Membrane ODE sweep on gfx950: one lane per state component, LSODA entirely in registers.
//
// One launch fuses what the reference does in three Python stages per membrane model and step
// (examples/idealized_geometries/run_3D.py:80-111):
//   1. update_ode_variables (src/knpemi/utils.py:210-235): nodal traces of the K concentrations on
//      both sides of the membrane -> parameter columns "<ion>_e"/"<ion>_i"; V <- phi_M_prev (k > 0);
//   2. MembraneModel.step_lsoda (src/knpemi/odeSolver.py:92-127): optional stimulus write, LSODA over
//      [t, t + dt] with rtol 1e-8 / atol 1e-10, state row <- solution at t + dt;
//   3. copy-back (run_3D.py:104-109): phi_M_prev <- V, I_ch_k <- parameter columns "I_ch_<ion>".
// The currents handed to the PDEs are, as in the reference, whatever the last RHS call made by LSODA
// stored in the parameter row; lsoda_core.h reproduces ODEPACK's call
// sequence, so this is the same evaluation point.
//
// Tables are stored transposed on the device ([column][dof]) so that neighbouring threads read
// neighbouring addresses; the ODE work itself is latency/compute bound (fp64 exp/log, divergent
// step control), not HBM bound.
//
// Host side (ode_host.h): this file builds the arguments of every sweep (kn_ode_args) and decides every launch
// (launch_sweep: plug-in or shipped model, LSODA here or a fixed-step kernel of kernels_ode_fixed.hip); kn_ode_step and
// kn_ode_advance are the two entries, one per kernel shape.  All of it works on a KnSweeps, whichever handle embeds it;
// only the step that shares its launch with the potential system's rows (kn_ode_step_emi) needs the CG handle's rows.
#include <algorithm>
#include <cstdlib>

#include "ode_host.h"

OdeArgs kn_ode_args(const OdeTables& T, double t0, double dt, double rtol, double atol, const OdePde* pde) {
  OdeArgs a{};   // what no branch below sets stays zero: no stimulus, full waves (dpw), no stamps
  a.nq = T.nq; a.q0 = T.q0; a.NQtot = T.NQtot; a.model_slot = T.model_slot;
  a.states = T.states; a.params = T.params; a.mask = T.mask; a.stats = T.stats;
  a.t0 = t0; a.dt = dt; a.rtol = rtol; a.atol = atol;
  if (pde) {   // a step of the coupled problem reads traces / V from the PDE fields and writes phi_M / I_ch back
    a.flags = pde->flags; a.v_index = pde->v_index; a.n_ions = pde->n_ions;
    for (int i = 0; i < 3 * pde->n_ions; ++i) a.ion_param[i] = pde->ion_param[i];
  } else {     // a standalone advance touches its own tables only: no flags, no ions, no V column to exchange
    a.v_index = -1;
  }
  return a;
}

namespace {

// Dofs per wavefront (ode_step_body): as few as keep the sweep at one wave per SIMD (1 024 SIMDs; the stats slots of the
// handle's sweeps are sized for that), all 64 / LANES of them otherwise.  KNPEMI_ODE_DPW forces a value (0: full waves).
int dofs_per_wave(const KnOdeModel& m) {
  if (m.rtc_module) return 0;   // a run-time compiled sweep is launched with full waves (launch_sweep)
  static const int forced = [] { const char* e = getenv("KNPEMI_ODE_DPW"); return e ? atoi(e) : -1; }();
  // Measured at config 2 (2 952 dofs; round 4, bench.py): 16 dofs per wave 77.5-81 us per sweep, 8: 83.1, 4: 83.1 (spike
  // window 106.7 / 110.8 / 104.6): fewer dofs per wave do NOT shorten the wave's stream measurably -- the trips of the 16
  // phase machines of a wave overlap almost completely -- and four times the waves cost more than they save.  Full waves
  // unless forced.
  if (forced <= 0) return 0;
  int full = 0;
  with_model(m.model_id, [&](auto tag) { full = ODE_BLOCK / tag.LANES; });
  return forced < full && (m.nq + forced - 1) / forced <= m.n_stat_blocks - 1 ? forced : 0;
}

// the arguments of a sweep over the tables of `slot`
OdeArgs model_args(const KnSweeps& sw, int slot, double t0, double dt, double rtol, double atol, const OdePde* pde) {
  const KnOdeModel& m = sw.ode[slot];
  const bool lsoda = m.method == KNPEMI_ODE_LSODA;
  // a fixed-step method has no tolerances, and its kernels run one thread per dof whatever dpw says
  OdeArgs a = kn_ode_args(OdeTables{m.nq, m.q0, sw.NQtot, slot, m.d_states, m.d_params, m.d_mask, m.d_stats},
                          t0, dt, lsoda ? rtol : 0.0, lsoda ? atol : 0.0, pde);
  a.n_stim = m.n_stim;
  for (int i = 0; i < 8; ++i) { a.stim_idx[i] = m.stim_idx[i]; a.stim_val[i] = m.stim_val[i]; }
  if (lsoda) a.dpw = dofs_per_wave(m);
  return a;
}

dim3 lsoda_grid(const OdeArgs& a, int lanes) {
  const int per_wave = a.dpw > 0 ? a.dpw : ODE_BLOCK / lanes;
  return dim3(((size_t)a.nq + per_wave - 1) / per_wave);
}

// 64-thread workgroups: the sweep has only n_q (10^3..10^5) threads, so spread the waves over as many CUs as possible
// instead of stacking four of them on one.  force_waves: KNPEMI_ODE_WAVES (1 or 2 resident waves per SIMD), 0: by size
int launch_lsoda_step(hipStream_t st, int model_id, const OdeDev& dv, const OdeArgs& a, const LsodaCoef* cf, int force_waves) {
  with_model(model_id, [&](auto tag) {
    using M = typename decltype(tag)::Model;
    constexpr int LANES = decltype(tag)::LANES;
    const dim3 grid = lsoda_grid(a, LANES), block(ODE_BLOCK);
    // more waves than 1.5 x the chip's 1024 SIMDs: trade registers for a second resident wave per SIMD
    const bool dense = force_waves ? force_waves == 2 : (size_t)grid.x > 1536;
    if (a.stamps) hipLaunchKernelGGL((ode_step_kernel<M, LANES, 1, true>), grid, block, 0, st, dv, a, cf);
    else if (dense) hipLaunchKernelGGL((ode_step_kernel<M, LANES, 2>), grid, block, 0, st, dv, a, cf);
    else hipLaunchKernelGGL((ode_step_kernel<M, LANES, 1>), grid, block, 0, st, dv, a, cf);
  });
  return kn_launch_check("ode_step_kernel");
}

int launch_lsoda_advance(hipStream_t st, int model_id, const OdeArgs& a, const OdeAdvArgs& v, const LsodaCoef* cf) {
  with_model(model_id, [&](auto tag) {
    using M = typename decltype(tag)::Model;
    constexpr int LANES = decltype(tag)::LANES;
    const dim3 grid = lsoda_grid(a, LANES), block(ODE_BLOCK);
    if ((size_t)grid.x > 1536) hipLaunchKernelGGL((ode_advance_kernel<M, LANES, 2>), grid, block, 0, st, a, v, cf);
    else hipLaunchKernelGGL((ode_advance_kernel<M, LANES, 1>), grid, block, 0, st, a, v, cf);
  });
  return kn_launch_check("ode_advance_kernel");
}

// The launch decision of every sweep of either handle: model source, integrator, kernel shape (v NULL: one step, which
// exchanges with the PDE fields; else the n steps v describes).  On `st`.
int launch_sweep(const KnSweeps& sw, hipStream_t st, const KnOdeModel& m, const OdeArgs& a, const OdeAdvArgs* v,
                 const LsodaCoef* cf) {
  const bool lsoda = m.method == KNPEMI_ODE_LSODA;
  const OdeDev dv = kn_ode_dev(sw);
  if (m.rtc_module) {   // plug-in compiled at bind time (kernels_rtc.hip)
    const hipFunction_t fn = m.rtc_kernel[m.method][v != nullptr];
    if (!fn) { kn_set_error("a model bound from source runs lsoda, euler or rk4"); return KNPEMI_EINVAL; }
    // LSODA: rtc_lanes lanes per dof in full waves; fixed-step: one thread per dof
    const unsigned grid = (unsigned)(((size_t)a.nq * (lsoda ? m.rtc_lanes : 1) + ODE_BLOCK - 1) / ODE_BLOCK);
    if (lsoda) return v ? kn_rtc_launch(st, fn, grid, a, *v, cf) : kn_rtc_launch(st, fn, grid, dv, a, cf);
    return v ? kn_rtc_launch(st, fn, grid, a, *v, m.n_substeps) : kn_rtc_launch(st, fn, grid, dv, a, m.n_substeps);
  }
  if (!lsoda) return v ? kn_launch_ode_fixed_advance(st, m, a, *v) : kn_launch_ode_fixed_step(st, m, dv, a);
  if (v) return launch_lsoda_advance(st, m.model_id, a, *v, cf);
  // KNPEMI_ODE_WAVES applies to the single-step launch only
  static const int force_waves = [] { const char* e = getenv("KNPEMI_ODE_WAVES"); return e ? atoi(e) : 0; }();
  return launch_lsoda_step(st, m.model_id, dv, a, cf, force_waves);
}

// the owner's copy of the LSODA coefficient tables, uploaded on first use
int lsoda_coef(KnSweeps& sw, const LsodaCoef** out) {
  if (!sw.d_lsoda_coef) {
    LsodaCoef c;
    lsoda_fill_coef(&c);
    if (int rc = kn_upload(sw.own->allocs, &c, 1, &sw.d_lsoda_coef)) return rc;
  }
  *out = static_cast<const LsodaCoef*>(sw.d_lsoda_coef);
  return KNPEMI_OK;
}

}  // namespace

// ---- one PDE step per launch (knpemi_ode_step, knpemi_dg_ode_step) -------------------------------------------------
int kn_ode_step(KnSweeps& sw, hipStream_t st, int prof_slot, int slot, double t0, double dt, double rtol, double atol,
                const OdePde& pde) {
  KnOdeModel& m = sw.ode[slot];
  if (m.nq == 0) return KNPEMI_OK;
  const LsodaCoef* cf = nullptr;
  int rc;
  if (m.method == KNPEMI_ODE_LSODA && (rc = lsoda_coef(sw, &cf))) return rc;
  OdeArgs a = model_args(sw, slot, t0, dt, rtol, atol, &pde);
  // KNPEMI_ODE_STAMPS=1: diagnostic build of the sweep with s_memtime stamps between the phases (tools/ode_stamps.py);
  // only the LSODA kernels of the shipped models have one
  static const bool want_stamps = getenv("KNPEMI_ODE_STAMPS") != nullptr;
  if (want_stamps && m.method == KNPEMI_ODE_LSODA && !m.rtc_module) {
    if (!m.d_stamps && (rc = kn_alloc(sw.own->allocs, 24 * (size_t)m.n_stat_blocks, &m.d_stamps))) return rc;
    a.stamps = m.d_stamps;
  }
  // counters accumulate over launches; kn_ode_stats() reads and resets them.  One profiling slot whatever the
  // integrator: it is "the ODE kernel" of the step for DeviceStepper's stream choice
  KnProfScope prof(sw.own->prof, prof_slot, st);
  return launch_sweep(sw, st, m, a, nullptr, cf);
}

// ---- one PDE step and the potential system's matrix per launch (knpemi_ode_step_emi) ------------------------------
namespace {

// Row-block rounds the free CUs may run under the sweep, one block per CU and round.  Measured at config 2:
// 413 row blocks on the 64 CUs that 192 sweep workgroups leave, 6.5 rounds, end under the shortest sweep of the recorded
// trajectory -- the fused launch takes 68.4 us where the sweep alone takes 67.6, 91.6 against 91.4 on average.  Nothing
// longer has been measured, so nothing longer is taken: 7.
constexpr int SWEEP_EMI_ROUNDS = 7;
// KNPEMI_FUSED_SWEEP: 0 never, 1 whenever eligible; unset: the default below
constexpr bool SWEEP_EMI_DEFAULT = true;

// Whether the sweep of `m` (n_sweep workgroups) and the EMI row blocks go into one launch.  Everything not listed takes
// the two launches: a shipped model under LSODA with the production kernel (no plug-in, no phase stamps, no forced second
// wave per SIMD), the only model of an unpartitioned handle, rows the fused kernel is instantiated for, a sweep on at most
// 3/4 of the CUs (one wave per CU each) and row blocks for at most SWEEP_EMI_ROUNDS rounds on the CUs left over.
bool sweep_emi_eligible(knpemi_handle* h, const KnOdeModel& m, int n_sweep) {
  const char* want = getenv("KNPEMI_FUSED_SWEEP");
  if (want ? atoi(want) == 0 : !SWEEP_EMI_DEFAULT) return false;
  if (m.rtc_module || m.method != KNPEMI_ODE_LSODA || getenv("KNPEMI_ODE_STAMPS") || getenv("KNPEMI_ODE_WAVES")) return false;
  if (!h->sweeps.have_pde || h->solver.dist.on || !kn_sweep_emi_rows_ok(h)) return false;
  int bound = 0;
  for (const KnOdeModel& o : h->sweeps.ode) bound += o.bound;
  if (bound != 1) return false;
  if (h->n_cus == 0 && hipDeviceGetAttribute(&h->n_cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess) {
    (void)hipGetLastError();
    h->n_cus = -1;
  }
  const int n_ode = (n_sweep + 7) & ~7;
  if (h->n_cus <= 0 || 4 * n_ode > 3 * h->n_cus) return false;
  return h->dev.nblocks <= SWEEP_EMI_ROUNDS * (h->n_cus - n_ode);
}

}  // namespace

int kn_ode_step_emi(knpemi_handle* h, int slot, double t0, double dt, double rtol, double atol, const OdePde& pde,
                    int emi_flags, int* fused) {
  *fused = 0;
  KnSweeps& sw = h->sweeps;
  KnOdeModel& m = sw.ode[slot];
  if (m.nq > 0 && m.method == KNPEMI_ODE_LSODA && !m.rtc_module) {
    OdeArgs a = model_args(sw, slot, t0, dt, rtol, atol, &pde);
    int lanes = 1;
    with_model(m.model_id, [&](auto tag) { lanes = tag.LANES; });
    const int n_sweep = (int)lsoda_grid(a, lanes).x;
    if (sweep_emi_eligible(h, m, n_sweep)) {
      const LsodaCoef* cf = nullptr;
      if (int rc = lsoda_coef(sw, &cf)) return rc;
      if (int rc = kn_launch_sweep_emi(h, m.model_id, kn_ode_dev(sw), a, cf, n_sweep, emi_flags, fused)) return rc;
      if (*fused) return KNPEMI_OK;
    }
  }
  if (int rc = kn_ode_step(sw, h->cur, KNPEMI_K_ODE, slot, t0, dt, rtol, atol, pde)) return rc;
  return kn_launch_emi_rows(h, emi_flags | KNPEMI_SKIP_MEMBRANE_RHS);
}

// ---- n steps per launch (knpemi_ode_advance) -------------------------------------------------------------------
namespace {

// Steps per launch.  A launch of a few tens of ms at most keeps a long run from holding the device for seconds; the
// first launch runs a few steps and is timed, the rest are sized from it.  KNPEMI_ODE_ADVANCE_CHUNK forces a size.
constexpr int ADV_PROBE_STEPS = 8, ADV_MAX_STEPS = 2048;
constexpr double ADV_BUDGET_MS = 25.0;

struct DevBuf {   // a temporary device allocation
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
};

}  // namespace

int kn_ode_advance(KnSweeps& sw, hipStream_t st, int slot, double t0, double dt, int n_steps, double rtol, double atol,
                   const int32_t* rec_idx, int n_rec, int every, double* history, const knpemi_ode_ss* ss,
                   int32_t* steps_taken, int32_t* failed_step) {
  KnOdeModel& m = sw.ode[slot];
  m.adv_chunk = 0;
  if (m.nq == 0 || n_steps == 0) return KNPEMI_OK;
  const bool lsoda = m.method == KNPEMI_ODE_LSODA;
  const LsodaCoef* cf = nullptr;
  int rc = KNPEMI_OK;
  if (lsoda && (rc = lsoda_coef(sw, &cf))) return rc;
  const size_t nq = (size_t)m.nq;
  if (!m.d_adv && (rc = kn_alloc(sw.own->allocs, 3 * nq, &m.d_adv))) return rc;   // still-step counters, steps_taken, failed_step
  OdeArgs a = model_args(sw, slot, t0, dt, rtol, atol, nullptr);
  OdeAdvArgs v{};
  v.n_rec = history ? n_rec : 0;
  v.every = every;
  for (int i = 0; i < v.n_rec; ++i) v.rec_idx[i] = rec_idx[i];
  v.window = ss ? ss->window : 0;
  v.ss_rtol = ss ? ss->ss_rtol : 0.0;
  v.ss_atol = ss ? ss->ss_atol : 0.0;
  v.still = m.d_adv; v.steps_taken = m.d_adv + nq; v.failed_step = m.d_adv + 2 * nq;
  KN_HIP(hipMemsetAsync(v.still, 0, nq * sizeof(int), st));
  KN_HIP(hipMemsetAsync(v.steps_taken, 0xFF, 2 * nq * sizeof(int), st));   // -1
  const size_t n_hist = v.n_rec > 0 ? (size_t)(n_steps / every) * v.n_rec * nq : 0;
  DevBuf hist;
  if (n_hist) {
    KN_HIP(hipMalloc(&hist.p, n_hist * sizeof(double)));
    v.hist = static_cast<double*>(hist.p);
  }
  const char* forced_env = getenv("KNPEMI_ODE_ADVANCE_CHUNK");
  const int forced = forced_env ? atoi(forced_env) : 0;
  int chunk = forced > 0 ? std::min(forced, ADV_MAX_STEPS) : ADV_PROBE_STEPS;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  KN_HIP(hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); kn_set_error("hipEventCreate failed"); return KNPEMI_EHIP; }
  double t = t0;
  for (int s = 0; s < n_steps && rc == KNPEMI_OK;) {
    const int c = std::min(chunk, n_steps - s);
    v.s0 = s; v.n_steps = c; a.t0 = t;
    const bool probe = s == 0 && forced <= 0;
    if (probe && hipEventRecord(e0, st) != hipSuccess) rc = KNPEMI_EHIP;
    if (rc == KNPEMI_OK) rc = launch_sweep(sw, st, m, a, &v, cf);
    if (rc == KNPEMI_OK && probe) {
      float ms = 0.0f;
      if (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
          hipEventElapsedTime(&ms, e0, e1) != hipSuccess) {
        kn_set_error("knpemi_ode_advance: timing the first launch failed");
        rc = KNPEMI_EHIP;
      } else {
        const double per_step = std::max((double)ms, 1e-3) / c;
        chunk = std::max(1, std::min(ADV_MAX_STEPS, (int)(ADV_BUDGET_MS / per_step)));
      }
    }
    for (int i = 0; i < c; ++i) t = t + dt;   // the caller's t <- t + dt, step by step
    s += c;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc) return rc;
  m.adv_chunk = chunk;
  if (n_hist) KN_HIP(hipMemcpyAsync(history, hist.p, n_hist * sizeof(double), hipMemcpyDeviceToHost, st));
  std::vector<int32_t> flags(2 * nq);
  if ((rc = kn_to_host(st, flags.data(), v.steps_taken, 2 * nq))) return rc;
  if (steps_taken) std::copy(flags.begin(), flags.begin() + nq, steps_taken);
  if (failed_step) std::copy(flags.begin() + nq, flags.end(), failed_step);
  size_t n_failed = 0;
  for (size_t q = 0; q < nq; ++q) n_failed += flags[nq + q] >= 0;
  if (n_failed) {
    kn_set_error(kn_ode_failure(lsoda, std::to_string(n_failed) + " membrane dof(s)"));
    return KNPEMI_EODE;
  }
  return KNPEMI_OK;
}

// ---- upkeep of a slot: one body under the entry points of both handles (ode_host.h) ---------------------------------
int kn_ode_check_shipped(const KnSweeps& sw, int slot, int model_id, int n_states, int n_params, const std::string& who) {
  if (model_id < 0 || model_id > 2) return kn_fail(KNPEMI_EINVAL, who + ": unknown model id");
  int ns = 0, np = 0;
  with_model(model_id, [&](auto tag) { ns = decltype(tag)::Model::NS; np = decltype(tag)::Model::NP; });
  if (n_states != ns || n_params != np) return kn_fail(KNPEMI_EINVAL, who + ": state/parameter count does not match the model");
  if (sw.ode[slot].bound) return kn_fail(KNPEMI_EINVAL, who + ": model already bound");
  return KNPEMI_OK;
}

int kn_ode_check_exchange(const KnSweeps& sw, int slot, const int32_t* ion_param, int v_index, const std::string& who) {
  const KnOdeModel& m = sw.ode[slot];
  for (int i = 0; i < 3 * sw.n_ions; ++i)
    if (ion_param[i] < 0 || ion_param[i] >= m.n_params) return kn_fail(KNPEMI_EINVAL, who + ": parameter index out of range");
  if (v_index < 0 || v_index >= m.n_states) return kn_fail(KNPEMI_EINVAL, who + ": bad V index");
  return KNPEMI_OK;
}

int kn_ode_alloc_tables(KnSweeps& sw, hipStream_t st, int slot, int q0, int nq, int model_id, int n_states, int n_params) {
  KnOdeModel& m = sw.ode[slot];
  std::vector<void*>& owner = sw.own->allocs;
  m.q0 = q0; m.nq = nq; m.model_id = model_id; m.n_states = n_states; m.n_params = n_params;
  int rc;
  if ((rc = kn_zeros(owner, st, (size_t)n_states * nq, &m.d_states))) return rc;
  if ((rc = kn_zeros(owner, st, (size_t)n_params * nq, &m.d_params))) return rc;
  // one slot per workgroup of the sweep (a forced KNPEMI_ODE_DPW runs fewer dofs per wave, up to one wave per SIMD)
  m.n_stat_blocks = std::max((int)(((size_t)nq * n_states + 63) / 64), std::min(nq, 1024)) + 1;
  if ((rc = kn_zeros(owner, st, 3 * (size_t)m.n_stat_blocks, &m.d_stats))) return rc;
  m.bound = 1;
  return KNPEMI_OK;
}

int kn_ode_set_tables(KnSweeps& sw, hipStream_t st, int slot, const double* states, const double* params) {
  const KnOdeModel& m = sw.ode[slot];
  if (m.nq == 0) return KNPEMI_OK;
  int rc;
  if (states && (rc = kn_table_upload(st, states, m.d_states, m.nq, m.n_states))) return rc;
  if (params && (rc = kn_table_upload(st, params, m.d_params, m.nq, m.n_params))) return rc;
  return KNPEMI_OK;
}

int kn_ode_get_tables(KnSweeps& sw, hipStream_t st, int slot, double* states, double* params) {
  const KnOdeModel& m = sw.ode[slot];
  if (m.nq == 0) return KNPEMI_OK;
  int rc;
  if (states && (rc = kn_table_download(st, m.d_states, states, m.nq, m.n_states))) return rc;
  if (params && (rc = kn_table_download(st, m.d_params, params, m.nq, m.n_params))) return rc;
  return KNPEMI_OK;
}

int kn_ode_stats(KnSweeps& sw, hipStream_t st, int slot, const std::string& where, unsigned long long out[3]) {
  const KnOdeModel& m = sw.ode[slot];
  std::vector<unsigned long long> part(3 * (size_t)m.n_stat_blocks);
  KN_HIP(hipMemcpyAsync(part.data(), m.d_stats, part.size() * sizeof(part[0]), hipMemcpyDeviceToHost, st));
  KN_HIP(hipMemsetAsync(m.d_stats, 0, part.size() * sizeof(part[0]), st));
  KN_HIP(hipStreamSynchronize(st));
  out[0] = out[1] = out[2] = 0;
  for (size_t i = 0; i < part.size(); ++i) out[i % 3] += part[i];
  if (out[2]) return kn_fail(KNPEMI_EODE, kn_ode_failure(m.method == KNPEMI_ODE_LSODA, where));
  return KNPEMI_OK;
}

// ---- diagnostics: the sweep's math helpers over an array (knpemi_debug_math) ------------------------------------
__global__ void debug_math_kernel(int op, int n, const double* __restrict__ a, const double* __restrict__ b,
                                  double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = op == 0 ? kn_div(a[i], b[i]) : (op == 1 ? kn_exp(a[i]) : (op == 2 ? kn_powr(a[i], b[i]) : kn_log(a[i])));
}

extern "C" int knpemi_debug_math(int op, int n, const double* a, const double* b, double* out) {
  if (op < 0 || op > 3 || n < 0 || !a || !out || ((op == 0 || op == 2) && !b)) {
    kn_set_error("knpemi_debug_math: bad arguments");
    return KNPEMI_EINVAL;
  }
  if (n == 0) return KNPEMI_OK;
  double* d = nullptr;
  KN_HIP(hipMalloc(reinterpret_cast<void**>(&d), 3 * sizeof(double) * (size_t)n));
  int rc = KNPEMI_OK;
  auto check = [&](hipError_t e) { if (e != hipSuccess && rc == KNPEMI_OK) { kn_set_error(hipGetErrorString(e)); rc = KNPEMI_EHIP; } };
  check(hipMemcpy(d, a, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  check(hipMemcpy(d + n, (op == 1 || op == 3) ? a : b, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  if (rc == KNPEMI_OK) {
    hipLaunchKernelGGL(debug_math_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, op, n, d, d + n, d + 2 * (size_t)n);
    if (kn_launch_check("debug_math_kernel")) rc = KNPEMI_EHIP;
    check(hipMemcpy(out, d + 2 * (size_t)n, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  }
  (void)hipFree(d);
  return rc;
}
