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

// -- simplices: the affine geometry of a cell (kernels_dg.hip, kernels_dg_balance.hip)
template <int NV>
struct Geo {
  double g[NV][NV - 1];   // gradients of the barycentric coordinates
  double vol;
};

template <int GD>
__device__ __forceinline__ double dot(const double (&a)[GD], const double (&b)[GD]) {
  double s = a[0] * b[0];
#pragma unroll
  for (int d = 1; d < GD; ++d) s += a[d] * b[d];
  return s;
}

template <int NV>
__device__ __forceinline__ void geometry(const double (&X)[NV][NV - 1], Geo<NV>& G) {
  if constexpr (NV == 3) {
    const double e1x = X[1][0] - X[0][0], e1y = X[1][1] - X[0][1];
    const double e2x = X[2][0] - X[0][0], e2y = X[2][1] - X[0][1];
    const double det = e1x * e2y - e1y * e2x, inv = fast_rcp(det);
    G.g[1][0] = e2y * inv; G.g[1][1] = -e2x * inv;
    G.g[2][0] = -e1y * inv; G.g[2][1] = e1x * inv;
    G.g[0][0] = -(G.g[1][0] + G.g[2][0]); G.g[0][1] = -(G.g[1][1] + G.g[2][1]);
    G.vol = 0.5 * fabs(det);
  } else {
    double e[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int d = 0; d < 3; ++d) e[a][d] = X[a + 1][d] - X[0][d];
    double cr[3][3];   // cr[a] = e[a+1] x e[a+2]
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int b = (a + 1) % 3, c = (a + 2) % 3;
      cr[a][0] = e[b][1] * e[c][2] - e[b][2] * e[c][1];
      cr[a][1] = e[b][2] * e[c][0] - e[b][0] * e[c][2];
      cr[a][2] = e[b][0] * e[c][1] - e[b][1] * e[c][0];
    }
    const double det = e[0][0] * cr[0][0] + e[0][1] * cr[0][1] + e[0][2] * cr[0][2], inv = fast_rcp(det);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      G.g[1][d] = cr[0][d] * inv; G.g[2][d] = cr[1][d] * inv; G.g[3][d] = cr[2][d] * inv;
      G.g[0][d] = -(G.g[1][d] + G.g[2][d] + G.g[3][d]);
    }
    G.vol = fabs(det) * (1.0 / 6.0);
  }
}

// -- hexahedra: the frame aligned with a facet (kernels_dg_hex.hip says what it is; kernels_dg_balance.hip)
constexpr double HX_G0 = 0.21132486540518711775, HX_G1 = 0.78867513459481288225;   // 2-point Gauss on [0, 1]

struct Vec3 {
  double x, y, z;
};
__device__ __forceinline__ Vec3 cross(const Vec3& a, const Vec3& b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ double dot3(const Vec3& a, const Vec3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// tangents, surface element, outward unit normal of T and the depth-frame numbers of T and N at facet point p
struct FacetFrame {
  double A, aTs, aTt, cT, aNs, aNt, cN, N[4], ds[4], dt[4];
};
__device__ __forceinline__ void hx_shapes(int p, double (&N)[4], double (&ds)[4], double (&dt)[4]) {
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const double ws = ((m ^ p) & 1) ? HX_G0 : HX_G1, wt = (((m ^ p) >> 1) & 1) ? HX_G0 : HX_G1;
    N[m] = ws * wt;
    ds[m] = (m & 1) ? wt : -wt;
    dt[m] = (m >> 1) ? ws : -ws;
  }
}
__device__ __forceinline__ void hx_frame(int p, const double (&xm)[4][3], const double (&dT)[4][3], const double (&dN)[4][3],
                                         bool have_n, FacetFrame& F) {
  hx_shapes(p, F.N, F.ds, F.dt);
  Vec3 ts{0, 0, 0}, tt{0, 0, 0}, eT{0, 0, 0}, eN{0, 0, 0};
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    ts.x += F.ds[m] * xm[m][0]; ts.y += F.ds[m] * xm[m][1]; ts.z += F.ds[m] * xm[m][2];
    tt.x += F.dt[m] * xm[m][0]; tt.y += F.dt[m] * xm[m][1]; tt.z += F.dt[m] * xm[m][2];
    eT.x += F.N[m] * dT[m][0]; eT.y += F.N[m] * dT[m][1]; eT.z += F.N[m] * dT[m][2];
    eN.x += F.N[m] * dN[m][0]; eN.y += F.N[m] * dN[m][1]; eN.z += F.N[m] * dN[m][2];
  }
  const Vec3 cr = cross(ts, tt);
  const double a2 = dot3(cr, cr), ra = fast_rsqrt(a2);
  F.A = a2 * ra;
  const double detT = dot3(cr, eT);
  const double nu = detT > 0.0 ? -ra : ra;            // n = nu cr points away from T
  const Vec3 n{nu * cr.x, nu * cr.y, nu * cr.z};
  const double riT = fast_rcp(detT);
  F.cT = dot3(cr, n) * riT;
  F.aTs = dot3(cross(tt, eT), n) * riT;
  F.aTt = dot3(cross(eT, ts), n) * riT;
  F.cN = F.aNs = F.aNt = 0.0;
  if (have_n) {
    const double riN = fast_rcp(dot3(cr, eN));
    F.cN = dot3(cr, n) * riN;
    F.aNs = dot3(cross(tt, eN), n) * riN;
    F.aNt = dot3(cross(eN, ts), n) * riN;
  }
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

// The per-cell ion balance (kernels_dg_balance.hip; knpemi_dg_balance_*).  Per cell and ion the table holds KN_DG_BCOLS
// numbers; dg_balance_membrane_kernel writes mem, m_old and src between the assembly and the solve of the concentrations,
// dg_balance_flux_kernel the rest at the end of the step, and appends the series row
//   [n_sub][K][mass, outflow, penalty, defect_max] [n_tag][K j^e | K j^i | capacitive, channel, area].
#define KN_DG_BCOLS 8                      // mem cons pen drift m_old m_new src defect
#define KN_DG_BSLOTS 4                     // per sub-domain and ion: sum m_new, sum out, sum |pen|, max |defect|
#define KN_DG_BTAG (2 * KN_MAXK + 3)       // per membrane tag: j^e and j^i of the KN_MAXK ions, int I_cap, int I_ch,tot, area
#define KN_DG_MAXTAG 8
struct KnDgBalance {
  std::vector<void*> allocs;
  knpemi_handle::KnSeries ser;         // ctl[2] is the ticket of the flux launch
  double* cells = nullptr;             // [K][KN_DG_BCOLS][n_cell]: consecutive lanes (cells) write consecutive addresses
  double* part = nullptr;              // [n_blk][n_sub * K * KN_DG_BSLOTS] workgroup partials of the flux launch
  double* mpart = nullptr;             // [n_blk][n_tag * KN_DG_BTAG] ... of the membrane launch
  double* tagtab = nullptr;            // [n_tag * KN_DG_BTAG] the membrane launch's sums, read by the flux launch's row
  unsigned long long* mctl = nullptr;  // [4]: the ticket of the membrane launch
  const int* facet_tag = nullptr;      // [n_mem_facets] index into the tags
  int n_blk = 0, n_tag = 0, want_cells = 0;
  bool set = false;
  bool membrane = false;               // a membrane launch came since the last record
  bool recorded = false;               // the table is complete: a record has been enqueued
};
int kn_dg_balance_blocks(int n_cell, int NV);
struct knpemi_dg;
int kn_dg_launch_balance_membrane(knpemi_dg* h, int splitting);
int kn_dg_launch_balance_flux(knpemi_dg* h);

// Field snapshots of a DG run (kernels_dg_snapshot.hip; knpemi_dg_snapshot_*).  A space is (sub-domain or membrane tag,
// form); every workgroup of the pack launch belongs to one space (bstart), the watches of space p are w[wstart[p] ..
// wstart[p + 1]).  Space p stores n_items[p] items; with a selection sel[p] lane i takes item sel[p][i], else item i.
//   form KNPEMI_DG_SNAP_BROKEN     an item is one source entry: the broken dof (bulk[p]) or the membrane node src[p][item],
//                                  or first[p] + item where the list is one ascending run (src[p] == NULL);
//        KNPEMI_DG_SNAP_CELL_MEAN  an item is a cell (src / first as above): its nv[p] dofs cell * nv .. in local order;
//        KNPEMI_DG_SNAP_VERTEX     an item is a mesh vertex: the entries vdof[p][vptr[p][item] .. vptr[p][item + 1]), ascending.
// A bulk watch takes slot `slot` (3 .. 7) of the dof records, a membrane watch reads `dense` (phi_M, a row of I_ch, a column
// of the state table).  The value of an item is its entries summed in list order, starting from the first, divided by their
// number (one IEEE division; none for the broken form); f32: (float) of it.
struct KnDgSnapTab {
  int n_space, n_watch;
  int bstart[KNPEMI_DG_SNAPSHOT_MAX_SPACE + 1];
  int wstart[KNPEMI_DG_SNAPSHOT_MAX_SPACE + 1];
  int n_items[KNPEMI_DG_SNAPSHOT_MAX_SPACE];
  int form[KNPEMI_DG_SNAPSHOT_MAX_SPACE];
  int bulk[KNPEMI_DG_SNAPSHOT_MAX_SPACE];
  int first[KNPEMI_DG_SNAPSHOT_MAX_SPACE];
  int nv[KNPEMI_DG_SNAPSHOT_MAX_SPACE];
  const int* sel[KNPEMI_DG_SNAPSHOT_MAX_SPACE];
  const int* src[KNPEMI_DG_SNAPSHOT_MAX_SPACE];
  const int* vptr[KNPEMI_DG_SNAPSHOT_MAX_SPACE];
  const int* vdof[KNPEMI_DG_SNAPSHOT_MAX_SPACE];
  KnSnapWatch w[KNPEMI_SNAPSHOT_MAX_WATCH];
};
// the recorder: the table, its lists and the ring (KnFrameRing), created by the first knpemi_dg_snapshot_set -- a run that
// does not save opens no copy stream; recorder_free(KnDgSnap&) (knpemi_record.hip) frees what is not in `allocs`
struct KnDgSnap : KnFrameRing {
  int n_watch = 0, n_blk = 0;
  KnDgSnapTab host{};                  // the table as uploaded
  int slot_of[KNPEMI_SNAPSHOT_MAX_WATCH] = {};       // watch of knpemi_dg_snapshot_set -> entry of the table
  long long items_of[KNPEMI_SNAPSHOT_MAX_WATCH] = {};
  KnDgSnapTab* tab = nullptr;
  long long move_bytes = 0;            // what one launch must move by the algorithm (kn_dg_snapshot_bytes)
  bool clock_set = false;              // a frame has been recorded since the set-up or the last reset, at t_prev
  double t_prev = 0.0;
  std::vector<void*> allocs;
};
// one pack launch on the owner's main stream into `frame` (a device frame of the ring)
int kn_dg_launch_snapshot_pack(KnDevice* own, const KnDgSnap& S, const double* rec, char* frame);

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
  KnDgBalance balance;
  KnDgSnap snap;
  int knp_flags = 0;              // flags of the last knpemi_dg_assemble_knp: the balance's membrane launch follows its splitting
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
