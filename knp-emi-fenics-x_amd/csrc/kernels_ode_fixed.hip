// Membrane ODE sweep with a fixed-step integrator (forward Euler, RK4, Rush-Larsen; fixed_step.h) on gfx950.
//
// The launch fuses what the LSODA sweep fuses (kernels_ode.hip: traces -> parameter columns, V <- phi_M, stimulus,
// integration, phi_M / I_ch write-back) and takes the same OdeDev / OdeArgs, plus the number of sub-steps.  It lives
// in a translation unit of its own so that the code generation of the LSODA kernels does not depend on it.
//
// Layout: one thread per membrane dof, 64-thread workgroups spread over the CUs.  The sub-steps are straight-line
// code, the same for every dof: the sweep is as long as ONE dof's chain of dependent fp64 instructions times the
// number of sub-steps, whatever the number of dofs up to one wave per SIMD (config 2: 47 waves on 1 024 SIMDs), and
// the six independent exponentials of an HH right-hand side overlap within the lane.
#include "knpemi_internal.h"
#include "membrane_models.h"
#include "fixed_step.h"

namespace {

template <class M, int METHOD>
void launch_step(hipStream_t st, const OdeDev& dv, const OdeArgs& a, int n_sub) {
  dim3 grid(((size_t)a.nq + ODE_BLOCK - 1) / ODE_BLOCK), block(ODE_BLOCK);
  hipLaunchKernelGGL((ode_fixed_step_kernel<M, METHOD>), grid, block, 0, st, dv, a, n_sub);
}

template <class M, int METHOD>
void launch_advance(hipStream_t st, const OdeArgs& a, const OdeAdvArgs& v, int n_sub) {
  dim3 grid(((size_t)a.nq + ODE_BLOCK - 1) / ODE_BLOCK), block(ODE_BLOCK);
  hipLaunchKernelGGL((ode_fixed_advance_kernel<M, METHOD>), grid, block, 0, st, a, v, n_sub);
}

// dv == nullptr: the multi-step launch
template <class M>
void launch_method(hipStream_t st, int method, const OdeDev* dv, const OdeArgs& a, const OdeAdvArgs* v, int n_sub) {
  switch (method) {
    case KNPEMI_ODE_EULER:
      if (dv) launch_step<M, KN_FS_EULER>(st, *dv, a, n_sub); else launch_advance<M, KN_FS_EULER>(st, a, *v, n_sub);
      break;
    case KNPEMI_ODE_RK4:
      if (dv) launch_step<M, KN_FS_RK4>(st, *dv, a, n_sub); else launch_advance<M, KN_FS_RK4>(st, a, *v, n_sub);
      break;
    default:
      if (dv) launch_step<M, KN_FS_RUSH_LARSEN>(st, *dv, a, n_sub);
      else launch_advance<M, KN_FS_RUSH_LARSEN>(st, a, *v, n_sub);
      break;
  }
}

int launch_builtin(hipStream_t st, const KnOdeModel& m, const OdeDev* dv, const OdeArgs& a, const OdeAdvArgs* v) {
  switch (m.model_id) {
    case KNPEMI_MODEL_HH_SI: launch_method<ModelHHSI>(st, m.method, dv, a, v, m.n_substeps); break;
    case KNPEMI_MODEL_HH_MV: launch_method<ModelHHMV>(st, m.method, dv, a, v, m.n_substeps); break;
    default: launch_method<ModelGlial>(st, m.method, dv, a, v, m.n_substeps); break;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    kn_set_error(std::string(dv ? "ode_fixed_step_kernel: " : "ode_fixed_advance_kernel: ") + hipGetErrorString(e));
    return KNPEMI_EHIP;
  }
  return KNPEMI_OK;
}

}  // namespace

int kn_launch_ode_fixed_step(knpemi_handle* h, int slot, double t0, double dt, int flags, const int32_t* ion_param,
                             int v_index) {
  KnOdeModel& m = h->ode[slot];
  if (m.nq == 0) return KNPEMI_OK;
  const KnDev& D = h->dev;
  const OdeDev dv{D.VR, D.q2e, D.q2i, D.phiM, D.Ich};
  OdeArgs a{};
  a.nq = m.nq; a.q0 = h->qoff[m.sub]; a.n_stim = m.n_stim; a.flags = flags; a.v_index = v_index;
  a.model_slot = slot; a.NQtot = h->dev.NQtot; a.n_ions = h->K;
  for (int i = 0; i < 3 * KN_MAXK; ++i) a.ion_param[i] = i < 3 * h->K ? ion_param[i] : 0;
  for (int i = 0; i < 8; ++i) { a.stim_idx[i] = m.stim_idx[i]; a.stim_val[i] = m.stim_val[i]; }
  a.t0 = t0; a.dt = dt;
  a.states = m.d_states; a.params = m.d_params; a.mask = m.d_mask; a.stats = m.d_stats;
  // the same profiling slot as the LSODA sweep: it is "the ODE kernel" of the step for DeviceStepper's stream choice
  KnProfScope prof(h, KNPEMI_K_ODE);
  if (m.rtc_function) return kn_rtc_fixed_launch(h, m, &dv, &a);
  return launch_builtin(h->cur, m, &dv, a, nullptr);
}

int kn_launch_ode_fixed_advance(knpemi_handle* h, const KnOdeModel& m, const void* args, const void* adv) {
  if (m.rtc_function) return kn_rtc_fixed_advance_launch(h, m, args, adv);
  return launch_builtin(h->cur, m, nullptr, *static_cast<const OdeArgs*>(args), static_cast<const OdeAdvArgs*>(adv));
}
