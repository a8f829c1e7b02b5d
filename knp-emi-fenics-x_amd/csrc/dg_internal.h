// Shared declarations of the DG variant's kernels: kernels_dg.hip (broken P1 on simplices, the C ABI) and
// kernels_dg_hex.hip (broken Q1 on hexahedra).
#pragma once

#include "knpemi_internal.h"
#include "kn_pick.h"

namespace kn_dg {

#ifndef KN_DG_BLOCK
#define KN_DG_BLOCK 64
#endif
#ifndef KN_DG_ROUND
#define KN_DG_ROUND KN_DG_BLOCK
#endif
constexpr int DG_BLOCK = KN_DG_BLOCK;   // threads (= rows) per workgroup
constexpr int DG_RPITCH = 10;           // doubles per staged record in LDS
constexpr int DG_ROUND = KN_DG_ROUND;   // rows whose image is in LDS at a time

struct DgConsts {
  int n_sub, K;
  double F, psi, C_M, dt, inv_dt, C_phi, gamma;
  double z[KN_MAXK];
  double elim[KN_MAXK];              // -(z_k / z_K)
  double D[KN_MAXSUB][KN_MAXK];
  double kap[KN_MAXSUB][KN_MAXK];    // F psi z_k^2 D_k
  double sig[KN_MAXSUB][KN_MAXK];    // F z_k D_k
  double az2D[KN_MAXSUB][KN_MAXK];   // D_k z_k^2
  double rho_term[KN_MAXSUB];        // -(1 / z_K) rho_z rho^s
};

struct DgDev {
  int n_cell, n_dof, nq;             // nq: membrane nodes
  int nquad;                         // points of the degree-6 membrane rule
  long long nnz;
  double* rec;
  const int* nbr;
  const unsigned* finfo;
  const int* mfid;                   // [n_cell][nv] membrane facet of local facet f (-1)
  const double* box_h;               // box meshes of hexahedra: [n_cell][3] edge lengths along the local axes, else NULL
  const unsigned char* cell_sub;
  const int* rowptr;
  double* A_emi;
  double* b_emi;
  double* A_knp;                     // [K-1][nnz]
  double* b_knp;                     // [K-1][n_dof]
  double* phiM;                      // [nq]
  double* Ich;                       // [KN_MAXK][nq]
  const double* fsrc;                // [K-1][n_dof] or NULL
  const double* qtab;                // weights, then shape values [nquad][nf]
  const int* q2e;
  const int* q2i;
};

struct DofRec {
  double x[3], c[KN_MAXK], phi;
};

__device__ __forceinline__ DofRec load_rec(const double* rec, int dof) {
  const double2* p = reinterpret_cast<const double2*>(rec + (size_t)dof * KN_REC);
  const double2 a = p[0], b = p[1], c = p[2], d = p[3];
  DofRec r;
  r.x[0] = a.x; r.x[1] = a.y; r.x[2] = b.x;
  r.c[3] = b.y; r.c[0] = c.x; r.c[1] = c.y; r.c[2] = d.x; r.phi = d.y;
  return r;
}

// The workgroup's own records are staged in LDS by one coalesced pass (lane t loads record row0 + t) and read from there
// by the NV lanes of each cell; 10-double pitch keeps the 16-byte reads of a wave on distinct banks.

__device__ __forceinline__ void stage_rec(double* lrec, const double* rec, int dof, int t) {
  const double2* p = reinterpret_cast<const double2*>(rec + (size_t)dof * KN_REC);
  double2* q = reinterpret_cast<double2*>(lrec + t * DG_RPITCH);
  const double2 a = p[0], b = p[1], c = p[2], d = p[3];
  q[0] = a; q[1] = b; q[2] = c; q[3] = d;
}

__device__ __forceinline__ DofRec lds_rec(const double* lrec, int t) {
  const double2* p = reinterpret_cast<const double2*>(lrec + t * DG_RPITCH);
  const double2 a = p[0], b = p[1], c = p[2], d = p[3];
  DofRec r;
  r.x[0] = a.x; r.x[1] = a.y; r.x[2] = b.x;
  r.c[3] = b.y; r.c[0] = c.x; r.c[1] = c.y; r.c[2] = d.x; r.phi = d.y;
  return r;
}


// 1 / a and 1 / sqrt(a) from the hardware estimates plus two Newton steps (relative error ~1e-16): a fraction of the
// instruction count of the IEEE division / square-root sequences, and the results are only compared at 1e-10.
__device__ __forceinline__ double fast_rcp(double a) {
  double r = __builtin_amdgcn_rcp(a);
  r = fma(fma(-a, r, 1.0), r, r);
  return fma(fma(-a, r, 1.0), r, r);
}
__device__ __forceinline__ double fast_rsqrt(double a) {
  double y = __builtin_amdgcn_rsq(a);
  y = y * fma(-0.5 * a * y, y, 1.5);
  return y * fma(-0.5 * a * y, y, 1.5);
}

// Workgroups are dealt to the 8 XCDs round robin; give every XCD a contiguous run of cells so that the neighbour
// records a workgroup reads are mostly the ones its XCD's L2 already holds.  Bijection on [0, 8 * chunk).
__device__ __forceinline__ int dg_block_index(int b, int chunk) { return (b & 7) * chunk + (b >> 3); }

}  // namespace kn_dg

// The jump seminorms of a record (kernels_dg_record.hip): per sub-domain the K concentrations at slots 0 .. K - 1 and the
// potential at slot KN_MAXK of `tab`, which dg_jump_kernel fills and a KNPEMI_DG_JUMP observable reads.  Allocated in the
// owner's `allocs` by the first knpemi_dg_observe_set that defines one.
#define KN_DG_JSLOTS (KN_MAXK + 1)
struct KnDgJump {
  double* tab = nullptr;               // [KN_MAXSUB][KN_DG_JSLOTS]
  double* part = nullptr;              // [n_blk][n_sub * KN_DG_JSLOTS] workgroup partials
  unsigned long long* ctl = nullptr;   // [4]: the ticket of record_tail.h
  int n_blk = 0;
};
int kn_dg_jump_blocks(int n_cell, int NV);
// one launch on the owner's main stream: every sub-domain, every field
int kn_dg_launch_jump(KnDevice* own, const kn_dg::DgDev& D, int NV, int n_sub, int box, const KnDgJump& J);

struct knpemi_dg : KnDevice {
  int NV = 0, K = 0, n_sub = 0;
  int NFC = 0, NFV = 0;            // facets per cell, vertices per facet (hexahedra: 6 and 4)
  int hex_box = 0;                 // hexahedra: every cell is an orthogonal parallelepiped (box-mesh kernels)
  kn_dg::DgDev dev{};
  kn_dg::DgConsts consts{};
  kn_dg::DgConsts* d_consts = nullptr;
  int have_params = 0;
  std::vector<int> h_rowptr, h_colind, h_q2e, h_q2i;
  double* d_fsrc = nullptr;
  const int* d_colind = nullptr;
  // (prof: brackets of the two assembly kernels, 0 = EMI, 1 = KNP, on the main stream -- knpemi_dg_profile)
  // membrane ODE sweep over the membrane nodes: one slot, offset 0 (view: knpemi_dg_create), and what that slot exchanges
  // with the fields, fixed at knpemi_dg_ode_bind: V's state column and the ions' parameter columns
  KnSweeps sweeps{this};
  int sweep_v = 0;
  int32_t sweep_ion_param[3 * KN_MAXK] = {0};
  // device solves (knpemi_dg_solve_emi / knpemi_dg_solve_knp): the Krylov + AMG code of the CG path on the DG systems
  std::vector<int> aux_of;         // continuous P1 dof (sub-domain, mesh vertex) of every broken dof
  int n_aux = 0;
  KnSolver solver{this};           // views and configuration: dg_solver, on first use
  double* d_csol = nullptr;        // [K-1][n_dofs] solved concentrations; != NULL: the solver is set up
  int extrapolate = 0;             // knpemi_dg_set_extrapolation
  // The recorders (knpemi_record.hip: knpemi_dg_observe_*, knpemi_dg_events_*): the state, the kernels and the series
  // routines of the CG path's, each freed by its clear, both by kn_dg_record_free.
  knpemi_handle::KnObserve obs;
  knpemi_handle::KnEvents events;
  KnDgJump jump;
  bool obs_jump = false;           // the installed observables read `jump.tab`: a record launches dg_jump_kernel first
};
void kn_dg_record_free(knpemi_dg* h);   // every recorder's device memory (knpemi_record.hip); knpemi_dg_destroy

// The DG kernels are built for 3, 4 and 8 vertices per cell and KS = K - 1 = 1..3 solved ions; the launchers pick the
// instantiation with kn_pick and answer anything else (unreachable with a handle knpemi_dg_create made) with this
inline int kn_dg_not_built(const char* kernel, int NV, int KS) {
  return kn_fail(KNPEMI_EINVAL, std::string(kernel) + ": not built for " + std::to_string(NV) + " vertices per cell and " +
                                    std::to_string(KS) + " solved ion(s)");
}

// Q1 hexahedra (kernels_dg_hex.hip): one launch each, on `st`; KS = K - 1 solved ions; box != 0: every cell is an
// orthogonal parallelepiped (the closed-frame kernels), 0: general trilinear cells
int kn_dg_hex_launch_emi(hipStream_t st, const kn_dg::DgDev& D, const kn_dg::DgConsts* d_consts, int splitting, int box);
int kn_dg_hex_launch_knp(hipStream_t st, const kn_dg::DgDev& D, const kn_dg::DgConsts* d_consts, int KS, int splitting, int box);
