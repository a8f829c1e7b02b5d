// Membrane ODE sweep with a fixed-step integrator (forward Euler, RK4, Rush-Larsen; fixed_step.h) on gfx950.
//
// The launch fuses what the LSODA sweep fuses (kernels_ode.hip: traces -> parameter columns, V <- phi_M, stimulus,
// integration, phi_M / I_ch write-back) and takes the same OdeDev / OdeArgs, plus the number of sub-steps.  It lives
// in a translation unit of its own so that the code generation of the LSODA kernels does not depend on it, and holds
// the kernels of the shipped models only: the caller (kernels_ode.hip, launch_sweep) has built the arguments and has
// decided that this is the launch to make.
//
// Layout: one thread per membrane dof, 64-thread workgroups spread over the CUs.  The sub-steps are straight-line
// code, the same for every dof: the sweep is as long as ONE dof's chain of dependent fp64 instructions times the
// number of sub-steps, whatever the number of dofs up to one wave per SIMD (config 2: 47 waves on 1 024 SIMDs), and
// the six independent exponentials of an HH right-hand side overlap within the lane.
#include "ode_host.h"
#include "fixed_step.h"

namespace {

// dv == nullptr: the multi-step launch
template <class M, int METHOD>
void launch_kernel(hipStream_t st, const OdeDev* dv, const OdeArgs& a, const OdeAdvArgs* v, int n_sub) {
  dim3 grid(((size_t)a.nq + ODE_BLOCK - 1) / ODE_BLOCK), block(ODE_BLOCK);
  if (dv) hipLaunchKernelGGL((ode_fixed_step_kernel<M, METHOD>), grid, block, 0, st, *dv, a, n_sub);
  else hipLaunchKernelGGL((ode_fixed_advance_kernel<M, METHOD>), grid, block, 0, st, a, *v, n_sub);
}

int launch(hipStream_t st, const KnOdeModel& m, const OdeDev* dv, const OdeArgs& a, const OdeAdvArgs* v) {
  with_model(m.model_id, [&](auto tag) {
    using M = typename decltype(tag)::Model;
    switch (m.method) {
      case KNPEMI_ODE_EULER: launch_kernel<M, KN_FS_EULER>(st, dv, a, v, m.n_substeps); break;
      case KNPEMI_ODE_RK4: launch_kernel<M, KN_FS_RK4>(st, dv, a, v, m.n_substeps); break;
      default: launch_kernel<M, KN_FS_RUSH_LARSEN>(st, dv, a, v, m.n_substeps); break;
    }
  });
  return kn_launch_check(dv ? "ode_fixed_step_kernel" : "ode_fixed_advance_kernel");
}

}  // namespace

int kn_launch_ode_fixed_step(hipStream_t st, const KnOdeModel& m, const OdeDev& dv, const OdeArgs& a) {
  return launch(st, m, &dv, a, nullptr);
}

int kn_launch_ode_fixed_advance(hipStream_t st, const KnOdeModel& m, const OdeArgs& a, const OdeAdvArgs& v) {
  return launch(st, m, nullptr, a, &v);
}
