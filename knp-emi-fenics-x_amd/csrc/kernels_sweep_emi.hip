// The membrane ODE sweep and the assembly of the potential system in ONE launch.
//
// Of everything a time step launches, only A_emi, P_emi and the volume part of b_emi do not depend on the sweep's output:
// they are formed from the concentrations the previous step left.  A small sweep is the instruction stream of one wave per
// workgroup on a fifth of the chip (config 2: 185 waves on 1 024 SIMDs) and the rest of the chip idles for its whole length.
// Running the row kernel on another stream beside it costs a cross-queue fork and join that exceed the row kernel's own
// length at that size (KNPEMI_OVERLAP_THRESHOLD_MS); one grid that holds both has no queues to order.
//
// Grid: n_ode + D.nblocks workgroups of KN_BLOCK threads.
//   [0, n_ode)            wave 0 runs ode_step_body, as the ode_step_kernel workgroup of that index does; waves 1..3 return
//                         at once, so the sweep keeps its one wave per CU (kernels_ode.hip on why four on one lose).
//                         n_ode is the sweep's grid rounded up to a multiple of 8; a padding workgroup returns untouched.
//   [n_ode, n_ode + nb)   row block blockIdx.x - n_ode of emi_rows_v2 (emi_rows.h) without the membrane Robin term
//                         (KNPEMI_SKIP_MEMBRANE_RHS), which needs the sweep's phi_M and I_ch and stays a launch of its own.
//                         n_ode % 8 == 0 keeps a row block on the XCD (blockIdx.x % 8) the stand-alone kernel gives it.
// The kernel is compiled for the sweep (one wave per SIMD, the whole register file, the flags of kernels_ode.o): a row
// block then needs a CU of its own and never shares one with a sweep wave; the row blocks go round on the CUs the sweep
// leaves free.  The sweep's static LDS is allocated for every workgroup: the launcher checks static + dynamic <= 160 KiB.
#include "emi_rows.h"
#include "ode_host.h"

namespace {

template <class M, int LANES, int LPR, bool UT>
__global__ __launch_bounds__(KN_BLOCK) void sweep_emi_kernel(OdeDev dv, OdeArgs a, const LsodaCoef* __restrict__ cf, int n_sweep,
                                                             int n_ode, KnDev D, const KnConsts* __restrict__ Cp, int acc_n,
                                                             int rec_n, int want_p, int splitting) {
  if ((int)blockIdx.x < n_ode) {
    // (both conditions are uniform over a wave)
    if (threadIdx.x >= ODE_BLOCK || (int)blockIdx.x >= n_sweep) return;
    ode_step_body<M, LANES, 1, false, true>(dv, a, cf);
  } else {
    emi_rows_block<3, LPR, UT>(D, *Cp, acc_n, rec_n, want_p, splitting, (int)blockIdx.x - n_ode);
  }
}

constexpr size_t LDS_PER_CU = 160 * 1024;

// *fits: the workgroup's LDS -- the static part is the sweep's (work columns, coefficient tables, row copy; asked once),
// the dynamic part the row block's -- fits a CU, and a CU holds ONE workgroup of the kernel (registers or LDS; the HH
// models' sweep takes 262 registers, a row block compiled with it as many): a row block then never lands on a sweep
// wave's CU, where it would take issue slots from the stream the step waits for.  The glial sweep fits 255 registers:
// two workgroups per CU unless the row block's LDS forbids it, so that model is mostly declined here.
template <auto KERNEL>
int prepare_kernel(size_t dyn, bool* fits) {
  static size_t static_lds = 0, asked_dyn = 0;
  static int per_cu = 0;
  const void* fn = reinterpret_cast<const void*>(KERNEL);
  if (static_lds == 0) {
    hipFuncAttributes attr;
    KN_HIP(hipFuncGetAttributes(&attr, fn));
    static_lds = attr.sharedSizeBytes;
  }
  *fits = static_lds + dyn <= LDS_PER_CU;
  if (!*fits) return KNPEMI_OK;
  if (int rc = kn_set_lds_limit(fn, dyn)) return rc;
  if (per_cu == 0 || asked_dyn != dyn) {
    KN_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, KN_BLOCK, dyn));
    asked_dyn = dyn;
  }
  *fits = per_cu == 1;
  return KNPEMI_OK;
}

}  // namespace

bool kn_sweep_emi_rows_ok(const knpemi_handle* h) {
  // tetrahedra with four lanes per row (knpemi_create's choice for them), lattice and general; by kind: a quadrilateral
  // has four vertices too, and runs the two launches as triangles do
  return h->cell_kind == KNPEMI_TETRAHEDRON && h->lpr == 4 && h->dev.nblocks > 0;
}

int kn_launch_sweep_emi(knpemi_handle* h, int model_id, const OdeDev& dv, const OdeArgs& a, const void* coef, int n_sweep,
                        int emi_flags, int* launched) {
  *launched = 0;
  if (!kn_sweep_emi_rows_ok(h)) return KNPEMI_OK;
  const KnDev& D = h->dev;
  const KnRowShape shape = kn_rows_shape(h, KN_ROWS_EMI);
  const int want_p = (emi_flags & KNPEMI_WANT_P) ? 1 : 0;
  const int split = ((emi_flags & KNPEMI_NO_SPLITTING) ? 0 : 1) | 2;   // 2: without the membrane Robin term
  const int n_ode = (n_sweep + 7) & ~7;
  const dim3 grid((unsigned)n_ode + (unsigned)D.nblocks), block(KN_BLOCK);
  const LsodaCoef* cf = static_cast<const LsodaCoef*>(coef);
  int rc = KNPEMI_OK;
  with_model(model_id, [&](auto tag) {
    using M = typename decltype(tag)::Model;
    constexpr int LANES = decltype(tag)::LANES;
    auto go = [&](auto ut) {
      constexpr auto kernel = sweep_emi_kernel<M, LANES, 4, decltype(ut)::value>;
      bool fits = false;
      if ((rc = prepare_kernel<kernel>(shape.lds, &fits)) || !fits) return;
      h->lds_bytes_emi = shape.lds;
      KnProfScope prof(h->prof, KNPEMI_K_ODE, h->cur);
      hipLaunchKernelGGL(kernel, grid, block, shape.lds, h->cur, dv, a, cf, n_sweep, n_ode, D, h->d_consts, shape.acc_n,
                         shape.rec_n, want_p, split);
      *launched = 1;
    };
    if (shape.geo == 2) go(std::true_type{});
    else go(std::false_type{});
  });
  if (rc || !*launched) return rc;
  return kn_launch_check("sweep_emi_kernel");
}
