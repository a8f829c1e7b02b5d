// Host side of the membrane ODE sweeps: what the translation units that launch or own a sweep share.  Host only: it
// adds no device code to a file that includes it (the kernels are in ode_kernel.h and fixed_step.h).
//
// Where a launch is decided: kernels_ode.hip, launch_sweep -- plug-in or shipped model, LSODA or a
// fixed-step method, one step or n steps.  Its arguments come from kn_ode_args, the one place that fills an OdeArgs.
#pragma once

#include "knpemi_internal.h"
#include "membrane_models.h"

// ---- launch arguments ---------------------------------------------------------------------------------------------
// the tables of a sweep, as a slot of KnSweeps describes them
struct OdeTables {
  int nq, q0, NQtot, model_slot;
  double* states;
  double* params;
  const unsigned char* mask;   // stimulus mask or NULL
  unsigned long long* stats;
};
// what a sweep exchanges with the PDE fields; a standalone advance has none of it
struct OdePde {
  int flags, v_index, n_ions;
  const int32_t* ion_param;    // [3 * n_ions]
};
// every field of an OdeArgs is set here or value-initialised; `pde` NULL: a standalone advance
OdeArgs kn_ode_args(const OdeTables& T, double t0, double dt, double rtol, double atol, const OdePde* pde);
inline OdeDev kn_ode_dev(const KnSweeps& sw) { return OdeDev{sw.rec, sw.q2e, sw.q2i, sw.phiM, sw.Ich}; }

// ---- shipped models -----------------------------------------------------------------------------------------------
template <class M, int L>
struct OdeModelTag {
  using Model = M;
  static constexpr int LANES = L;   // lanes per dof of the LSODA sweep (lsoda_core.h)
};
// calls f(OdeModelTag<Model, LANES>{}) for the shipped model `model_id`
template <class F>
void with_model(int model_id, F&& f) {
  switch (model_id) {
    case KNPEMI_MODEL_HH_SI: f(OdeModelTag<ModelHHSI, 4>{}); break;
    case KNPEMI_MODEL_HH_MV: f(OdeModelTag<ModelHHMV, 4>{}); break;
    default: f(OdeModelTag<ModelGlial, 1>{}); break;
  }
}

// ---- the sweeps ---------------------------------------------------------------------------------------------------
// kernels_ode.hip: one entry per kernel shape, integrator and model source chosen inside.  On the caller's stream `st`;
// the step is bracketed into the owner's profiling slot prof_slot (< 0: none).
int kn_ode_step(KnSweeps& sw, hipStream_t st, int prof_slot, int slot, double t0, double dt, double rtol, double atol,
                const OdePde& pde);
int kn_ode_advance(KnSweeps& sw, hipStream_t st, int slot, double t0, double dt, int n_steps, double rtol, double atol,
                   const int32_t* rec_idx, int n_rec, int every, double* history, const knpemi_ode_ss* ss,
                   int32_t* steps_taken, int32_t* failed_step);
// The step of model `slot` and the potential system's A, P and volume part of b (knpemi_assemble_emi with emi_flags |
// KNPEMI_SKIP_MEMBRANE_RHS), both on h->cur.  *fused = 1: one launch held both (kernels_sweep_emi.hip; the eligibility rule
// is in kernels_ode.hip), 0: kn_ode_step and kn_launch_emi_rows, one after the other.
int kn_ode_step_emi(knpemi_handle* h, int slot, double t0, double dt, double rtol, double atol, const OdePde& pde,
                    int emi_flags, int* fused);
// kernels_sweep_emi.hip: the rows of the handle are of a kind the fused launch is instantiated for; the launch itself, for
// a sweep of n_sweep workgroups (*launched = 0 and nothing enqueued: not instantiated, or the LDS of both does not fit)
bool kn_sweep_emi_rows_ok(const knpemi_handle* h);
int kn_launch_sweep_emi(knpemi_handle* h, int model_id, const OdeDev& dv, const OdeArgs& a, const void* coef, int n_sweep,
                        int emi_flags, int* launched);
// kernels_ode_fixed.hip: the fixed-step kernels of the shipped models (m.method, m.n_substeps)
int kn_launch_ode_fixed_step(hipStream_t st, const KnOdeModel& m, const OdeDev& dv, const OdeArgs& a);
int kn_launch_ode_fixed_advance(hipStream_t st, const KnOdeModel& m, const OdeArgs& a, const OdeAdvArgs& v);

// kernels_rtc.hip: a kernel of a plug-in, ODE_BLOCK threads per workgroup; `params` is the kernel's parameter list
// laid out as the compiler lays it out
int kn_rtc_launch(hipStream_t st, hipFunction_t fn, unsigned grid, void* params, size_t bytes);
template <class A, class B, class C>
int kn_rtc_launch(hipStream_t st, hipFunction_t fn, unsigned grid, const A& a, const B& b, const C& c) {
  struct { A a; B b; C c; } p{a, b, c};
  return kn_rtc_launch(st, fn, grid, &p, sizeof(p));
}

// ---- upkeep of a slot, one body under knpemi_ode_* and knpemi_dg_ode_* (kernels_ode.hip) -----------------------------
// `who` starts the error texts: the entry point.
// a shipped model may be bound to `slot`: known id, the counts are Model::NS and Model::NP, slot still free
int kn_ode_check_shipped(const KnSweeps& sw, int slot, int model_id, int n_states, int n_params, const std::string& who);
// what a step exchanges with the PDE fields: the 3 * n_ions parameter columns of the ions and V's state column
int kn_ode_check_exchange(const KnSweeps& sw, int slot, const int32_t* ion_param, int v_index, const std::string& who);
// binds `slot`: its nq dofs from q0 on, zeroed states and parameters, the statistics partials
int kn_ode_alloc_tables(KnSweeps& sw, hipStream_t st, int slot, int q0, int nq, int model_id, int n_states, int n_params);
// host tables [dof][column], either may be NULL
int kn_ode_set_tables(KnSweeps& sw, hipStream_t st, int slot, const double* states, const double* params);
int kn_ode_get_tables(KnSweeps& sw, hipStream_t st, int slot, double* states, double* params);
// reads, resets and sums the per-workgroup partials: out = {rhs evaluations, steps, failures}; KNPEMI_EODE, out filled,
// when a dof failed (`where` e.g. "at least one membrane dof")
int kn_ode_stats(KnSweeps& sw, hipStream_t st, int slot, const std::string& where, unsigned long long out[3]);
// the message of a failed sweep; `where` e.g. "3 membrane dof(s)"
inline std::string kn_ode_failure(bool lsoda, const std::string& where) {
  return lsoda ? "LSODA failed on " + where + " (odeSolver.py:121 `assert success`)"
               : "the fixed-step integrator left a non-finite state on " + where;
}
