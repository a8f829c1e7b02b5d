// Internal data structures shared by the host-side builder/API and the gfx950 kernels.
// Not part of the C ABI (see include/knpemi_hip.h).
#pragma once

#include <hip/hip_runtime.h>
#include "block_spmv.h"
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/knpemi_hip.h"
#include "monitor_table.h"

#define KN_MAXK KNPEMI_MAX_IONS
#define KN_MAXSUB KNPEMI_MAX_SUB
#define KN_REC 8          // doubles per vertex record: x y z c3 | c0 c1 c2 phi  (ion k lives in slot KN_CSLOT(k);
                          // K = 3: c2 is the eliminated ion and slot 3 is unused, as in every reference driver)
#define KN_CSLOT(k) ((k) < 3 ? 4 + (k) : 3)
#define KN_BLOCK 256          // threads per row-kernel workgroup (rows per block = KN_BLOCK / lanes-per-row)
#define KN_SLICE 64       // rows per sliced-ELL slice == wavefront width on gfx950
// consecutive rows per chunk of a row block (kernels_assemble.hip: BlkRows).  Measured at 995 k tets / 166 k hexahedra:
// 16-row chunks give the simplex kernels fewer, longer output pieces (emi_rows 46.6 -> 43.3 us, knp_rows 45.8 -> 44.7 us;
// 266 instead of 233 distinct vertices per block), the hexahedral ones lose with them (blocks closed early by the bound on
// the distinct vertices are half empty: knp_rows_hex 61 -> 71 us); 4-row chunks lose everywhere.
#define KN_CHUNK_SIMPLEX 16
#define KN_CHUNK_HEX 8

// Per-sub-domain constants folded on the host from knpemi_params (double arithmetic identical
// to what the kernels would do per cell).
struct KnSubConst {
  double kap[KN_MAXK];   // F * psi * z_k^2 * D_k^s      (emiWeakForm.py:103)
  double sig[KN_MAXK];   // F * z_k * D_k^s              (emiWeakForm.py:217)
  double D[KN_MAXK];     // D_k^s
  double zpsiD[KN_MAXK]; // z_k * psi * D_k^s            (knpWeakForm.py:141)
  double az2D[KN_MAXK];  // D_k^s z_k^2                  (knpWeakForm.py:97)
  double rho_term;       // -(1/z_K) * rho_z * rho^s     (utils.py:249)
};

struct KnConsts {
  int n_sub, K;
  int voff[KN_MAXSUB + 1];   // global vertex offset of each sub-domain
  int qoff[KN_MAXSUB + 1];   // global Q-dof offset
  KnSubConst sc[KN_MAXSUB];
  double dt, inv_dt, F, psi, C_M, C_phi;
  double z[KN_MAXK];
  double elim_coef[KN_MAXK]; // -(z_k / z_K)            (utils.py:258)
  int splitting;
};

// Device views (raw pointers; owned by knpemi_handle).
struct KnDev {
  int Ntot, nctot, NQtot, nftot;
  int nblocks;                // row blocks; a block never straddles two sub-domains
  const int* blk_rng;         // [nblocks][KN_BLOCK / lpr / chunk][6] chunks of consecutive rows (BlkRows)
  const int* blk_sub;         // [nblocks] sub-domain of the block
  const int4* blk_info;       // [nblocks][4]: {first row, rows, sub, 0} {EMI seg length, offset into ent_loc,
                              //   Laplacian seg length, offset into blk_uverts} {slice entry bases / 64}
                              //   {4 x uint8 slice steps, #distinct vertices, 0, 0}
  const int* blk_uverts;      // concatenated per-block sorted lists of the distinct vertices its rows touch
  const uint16_t* ent_loc;    // [nnzL] position of every Laplacian entry's vertex in its block's list, stored in the
                              //   order of the blocks' concatenated Laplacian segments
  const int4* row_info;       // [Ntot]: offsets in the block's concatenated segments {EMI row start, (that + lapoff[g]) |
                              //          n_membrane_entries << 16, Laplacian row start, first membrane entry}
  double* VR;                 // [Ntot][KN_REC]
  double* csol;               // [K-1][Ntot]  solver output c (block order handled by offsets)
  double* fsrc;               // [K-1][N_0] optional ECS source term (NULL when unused)
  const int* cells;           // [nctot][NV] global vertex ids
  // sliced ELL of (row, incident cell) pairs
  const int64_t* sl_ptr;      // [4*nblocks+1] entry offsets (multiples of KN_SLICE); slice 4*b + w
                              // holds the 64/lpr rows blk_row0[b] + (64/lpr)*w .. of block b; lane
                              // r*lpr + j of step p reads pair p*lpr + j of row r of the slice
  const uint32_t* pair_sl;    // simplices: NV x uint8 slots of the cell's vertices in the row's Laplacian
                              // segment (byte 0 = the row's own vertex); 0xFFFFFFFF marks padding.  Lattice tetrahedra
                              // (tet_tab != NULL): slots are 5 bits, bits 5-7 of byte 0 hold the cell's shape, bits
                              // 5-6 of bytes 1-3 the canonical vertex number of the vertex in that byte
  const double* tet_tab;      // lattice tetrahedra of a uniform grid (knpemi_create): [8 shapes][4][4] gradient dot
                              // products of the canonical vertices, then [8] cell volumes; NULL otherwise
  const int* pair_cell;       // hexahedra, quadrilaterals: cell*8 + local index, -1 = padding
  const uint32_t* pair_slots; // hexahedra: 8 x uint8 slots in two consecutive words per entry; quadrilaterals: 4 in one word
  // EMI CSR (monolithic) and Laplacian-pattern CSR (KNP blocks share it per sub-domain)
  const int* rowptr; const int* colind; const uint8_t* lapoff;
  const int* rowptrL; const int* colindL;
  double* A_emi; double* P_emi; double* b_emi;
  double* A_knp; double* b_knp;          // block order (sub, ion)
  const int* krowptr; const int* kcolind; // monolithic block-diagonal KNP pattern (Krylov solve, export)
  int64_t nnz, nnzL;
  // membrane
  const int* mptr;            // [M+1]
  const int* mentry;          // facet*8 + local vertex a
  const uint64_t* mslots;     // bytes 0..3 own-side slot of col b, bytes 4..7 other-side slot
  const int* mrow;            // [M] global row of each membrane row
  // per membrane entry e = (row, facet, local vertex): model slot (-1: none), Q dofs of the facet, facet-mass row
  const int* me_model;        // [E]
  const int* me_q;            // [E][NF]
  const double* me_mass;      // [E][NF], filled once by membrane_mass_kernel
  const int* gam_pos;         // [nftot][2 sides][NF] -> entry e
  const int* fe; const int* fi; const int* fq;   // [nftot][NF] global ids
  const int* fmodel;          // [nftot] global model slot or -1
  const int* q2e; const int* q2i;                // [NQtot] global vertex ids
  const double* P_mass;       // [nnz - pmass0] static ICS mass entries of P_emi (rows of the cell sub-domains)
  int64_t pmass0;             // rowptr[first cell-side row]
  double* gam_e;              // [E][K-1] membrane partial integrals of b_knp, in entry order
  double* gpre;               // [E][(1 + NF)(K-1)] early form: phi-independent part + facet matrix (knp_membrane_pre_kernel)
  double* phiM;               // [NQtot]
  double* Ich;                // [n_model_slots][K][stride NQtot] (indexed by global q)
  int M;
  // membrane quadrature tables (degree 6): weights and shape values
  const double* qtab;         // [nq] weights, then [nq][NF] shape values, then (quads) [nq][NF][2] derivatives
  int nq_gamma;
};

// Table of the watched sub-domains of the membrane events (kernels_events.hip), read by the record kernel: lane i of the
// grid belongs to segment w with gstart[w] <= i < gstart[w + 1], its dof is q0[w] + i - gstart[w] of sub-domain sub[w]
struct KnEvTab {
  int n_watch;
  int gstart[KN_MAXSUB + 1];
  int q0[KN_MAXSUB];
  int sub[KN_MAXSUB];
  double threshold[KN_MAXSUB];   // indexed by the sub-domain
  double reset[KN_MAXSUB];
};

// Table of the watches of a recorder with per-item fields and a series row: the ion fluxes (kernels_flux.hip; an item is a
// cell, a watch a sub-domain) and the membrane exchange (kernels_exchange.hip; an item is a membrane facet, a watch a cell),
// read by the record kernel.  Workgroup b belongs to watch w with bstart[w] <= b < bstart[w + 1] and takes one chunk
// (KN_FLUX_CHUNK cells; kn_exchange_chunk() facets, both sides of each) of the count[w] items of sub-domain sub[w], from
// first[w] + (b - bstart[w]) * chunk on.  A workgroup's partial has KN_FLUX_SLOTS / KN_EX_SLOTS doubles at fixed places:
//   fluxes    ion k at k (2 gdim + 1) .. ({sum vol J_diff}, {sum vol J_drift}, max |J|), the current at
//             KN_MAXK (2 gdim + 1) .. ({sum vol i}, max |i|);
//   exchange  ion k at 3 k .. (int j_k^e, int j_k^i, int I_ch,k), then at 3 KN_MAXK .. int I_cap, int I_ch,tot, the area.
// Column q of the series row is slot col_slot[q] of watch col_watch[q], folded over that watch's workgroups in their
// order by sum or (col_max[q]; the fluxes' maxima only) maximum.  The per-item fields of watch w start at fbase[w]
// doubles: [component][count[w]], the selected ions in ascending order (fluxes: {J_diff}, {J_drift}; exchange: j^e, j^i,
// I_ch,k), then the current (fluxes: {i_diff}, {i_drift}; exchange: I_cap and the area).
// Partitioned runs (knpemi_<name>_set_partitioned): count[w] may be 0 (no workgroup then) and item i of watch w has the
// byte ibase[w] + i of the recorded mask; the other kernels do not read ibase.
#define KN_FLUX_CHUNK 256
#define KN_FLUX_SLOTS 32        // >= KN_MAXK (2 * 3 + 1) + 3 + 1
#define KN_EX_SLOTS 16          // >= 3 KN_MAXK + 3
#define KN_WATCH_MAXCOLS (KN_MAXSUB * KN_FLUX_SLOTS)
#define KN_WATCH_CURRENT 0x100  // bit 8 of a watch's ion mask
struct KnWatchTab {
  int n_watch, n_cols;
  int bstart[KN_MAXSUB + 1];
  int sub[KN_MAXSUB];
  int first[KN_MAXSUB];
  int count[KN_MAXSUB];
  int mask[KN_MAXSUB];
  int ibase[KN_MAXSUB];
  long long fbase[KN_MAXSUB];
  uint8_t col_watch[KN_WATCH_MAXCOLS], col_slot[KN_WATCH_MAXCOLS], col_max[KN_WATCH_MAXCOLS];
};

// Table of the field maps (kernels_maps.hip), read by the record and the reset kernel.  Watches are grouped by space: the
// vertices of a sub-domain, or the membrane dofs of a cell.  Workgroup b belongs to space p with bstart[p] <= b <
// bstart[p + 1] and takes 256 consecutive items of its n_items[p]; a lane serves the watches wstart[p] .. wstart[p + 1] - 1
// of its item.  A bulk lane reads slots 3 .. 7 of its vertex record (vertex first[p] + item) once when need_rec[p]; a watch
// with dense == NULL takes slot `slot` of it, any other reads dense[item] (the solver's c, phi_M).  State arrays are
// per watch, [n_items] each, NULL where the statistic is not selected (v_prev: with the integral or the threshold only --
// peak and trough do not depend on it).  A series watch has the item weights `weight` and the slots 2 j, 2 j + 1 (measure, n)
// of its workgroups' partials, j its number among the series watches of the space; column q of the row folds slot
// col_slot[q] over the workgroups of space col_space[q].  Partitioned (knpemi_maps_set_partitioned): `weight` is lumped from
// the items' cells (facets) this rank records, and n counts the items with owned[item] != 0.
#define KN_MAPS_MAXSPACE (2 * KN_MAXSUB)
#define KN_MAPS_SLOTS (2 * KNPEMI_MAPS_MAX_PER_SPACE)
#define KN_MAPS_MAXCOLS (2 * KNPEMI_MAPS_MAX_WATCH)
struct KnMapWatch {
  const double* dense;
  int slot, flags, ser;          // ser: j of a series watch, else -1
  double thr, sgn;
  double *v_prev, *v_max, *t_max, *v_min, *t_min, *integral, *t_arrival, *exposure, *excess;
  int* count;
  const double* weight;
  const uint8_t* owned;          // partitioned series watch: 1 where this rank's n counts the item; NULL: every item
};
struct KnMapTab {
  int n_space, n_watch, n_cols;
  int bstart[KN_MAPS_MAXSPACE + 1];
  int wstart[KN_MAPS_MAXSPACE + 1];
  int n_items[KN_MAPS_MAXSPACE];
  int first[KN_MAPS_MAXSPACE];
  int need_rec[KN_MAPS_MAXSPACE];
  uint8_t col_space[KN_MAPS_MAXCOLS], col_slot[KN_MAPS_MAXCOLS];
  KnMapWatch w[KNPEMI_MAPS_MAX_WATCH];
};

// Table of the field snapshots (kernels_snapshot.hip), read by the pack kernel.  Spaces, bstart, wstart, first and need_rec
// as in KnMapTab; n_items[p] is the number of items the space STORES: with a selection sel[p] (ascending item indices,
// device memory) lane i reads item sel[p][i], without one (NULL) item i, and writes position i of every watch of the space.
// A watch reads dense[item] (the solver's c, phi_M, I_ch, a row of a state table) or, dense == NULL, slot `slot` of the
// vertex record, and stores the double, or with f32 (float)v, at byte `off` of the frame (a multiple of
// KNPEMI_SNAPSHOT_ALIGN).
struct KnSnapWatch {
  const double* dense;
  int slot, f32;
  long long off;
};
struct KnSnapTab {
  int n_space, n_watch;
  int bstart[KN_MAPS_MAXSPACE + 1];
  int wstart[KN_MAPS_MAXSPACE + 1];
  int n_items[KN_MAPS_MAXSPACE];
  int first[KN_MAPS_MAXSPACE];
  int need_rec[KN_MAPS_MAXSPACE];
  const int* sel[KN_MAPS_MAXSPACE];
  KnSnapWatch w[KNPEMI_SNAPSHOT_MAX_WATCH];
};

// The ring of a snapshot recorder, on either handle (knpemi_record.hip: ring_*): `depth` slots -- a device frame, a pinned
// host frame and a "copied" event each -- fed by a copy stream of its own.  Slot seq % depth takes frame seq; the frames
// [tail, seq) are IN FLIGHT, so a slot is FREE exactly when seq - tail < depth.  The device frames live in the recorder's
// `allocs`; the stream, the events and the pinned frames do not: ring_free frees them.
struct KnFrameRing {
  int depth = 0;
  size_t frame_bytes = 0;
  hipStream_t copy = nullptr;
  hipEvent_t ev_packed = nullptr;      // the pack launch's end on the main stream; the copy stream waits for it
  std::vector<char*> dev, pinned;      // [depth] frames
  std::vector<hipEvent_t> copied;      // [depth]
  std::vector<double> t_of;            // [depth] the time of the frame a slot holds
  int64_t seq = 0, tail = 0;
};

// (the table of the membrane monitors, KnMonTab: monitor_table.h, shared with the run-time compiled monitor programs)

struct KnOdeModel {
  int bound = 0, model_id = -1, n_states = 0, n_params = 0, nq = 0;
  int q0 = 0;                   // offset of its dofs in phiM / Ich
  double* d_states = nullptr;   // [n_states][nq]
  double* d_params = nullptr;   // [n_params][nq]
  uint8_t* d_mask = nullptr;    // [nq] or NULL
  int n_stim = 0;
  int stim_idx[8] = {};
  double stim_val[8] = {};
  unsigned long long* d_stats = nullptr; // [n_stat_blocks][3]: rhs evals, steps, failures per workgroup of the sweep
  int n_stat_blocks = 0;
  unsigned long long* d_stamps = nullptr;   // diagnostic phase stamps (KNPEMI_ODE_STAMPS)
  // model compiled at bind time from the plug-in's HIP source (kernels_rtc.hip); NULL for the shipped models
  hipModule_t rtc_module = nullptr;
  // its kernels, [KNPEMI_ODE_* method][0: one step, 1: n steps]; NULL: the plug-in cannot run that method (Rush-Larsen)
  hipFunction_t rtc_kernel[4][2] = {};
  int rtc_lanes = 1;
  int* d_adv = nullptr;                   // [3][nq] knpemi_ode_advance: still-step counters, steps_taken, failed_step
  int adv_chunk = 0;                      // steps per launch the last knpemi_ode_advance chose
  // integrator of the slot (knpemi_ode_set_method): KNPEMI_ODE_LSODA or a fixed-step scheme with n_substeps sub-steps
  int method = 0, n_substeps = 0;
  // the monitor program of a plug-in (knpemi_monitor_bind_source; kernels_rtc.hip): [0] series only, [1] with fields;
  // NULL: the slot has no monitor of its own (shipped models: the library's kernel)
  hipFunction_t mon_kernel[2] = {};
  int n_monitored = 0;
};

// blocks of the dense coarsest-level inverse, passed to the kernels by value: block b covers the unknowns start[b] ..
// start[b] + size[b] - 1, its row-major size[b] x size[b] inverse begins at off[b] (doubles)
struct KnDenseBlocks { int nb = 0; int start[8] = {0}; int size[8] = {0}; int off[8] = {0}; };

// geometry of the cells of a uniform hexahedral mesh (edge vectors e_t = x[1 << t] - x[0] of every cell): g = |det J| J^-1 J^-T,
// J = [e_0 e_1 e_2]; passed to the hexahedral row kernels by value
struct KnHexGeo { double g[3][3]; double det; int skew; };

// Algebraic multigrid hierarchy (kernels_amg.hip)
struct KnAmgCsr { int n = 0, m = 0, nnz = 0; int* rp = nullptr; int* ci = nullptr; double* v = nullptr; };
struct KnAmgLevel {
  int n = 0, nc = 0;                 // size, size of the next coarser level (0: dense coarsest level)
  int avg_row = 0, p_row = 0, r_row = 0;
  double omega = 0.0;                // Jacobi damping 4 / (3 rho)
  KnAmgCsr A, P, R;
  // merged transfer operators of the fused cycle (kernels_fused.hip): Rm = R (I - omega A D^-1), Pm = (I - omega D^-1 A) P,
  // built from the operator the hierarchy was set up with; frozen_v: that operator's values on the finest level (the
  // coarser levels' A.v are frozen copies already)
  KnAmgCsr Rm, Pm;
  double* frozen_v = nullptr;
  double* dinv = nullptr;
  // explicit inverse on the coarsest level as up to 8 dense diagonal blocks (amg_host.h: dense_inverse_blocks; the
  // aggregates of every level are numbered component by component, so the independent ion systems are contiguous ranges)
  double* dense_inv = nullptr;
  KnDenseBlocks dense_blk;
  double *x = nullptr, *r = nullptr, *t = nullptr;
};
struct KnAmgAsync;     // a rebuild running on a host thread (kernels_amg.hip)
// How a hierarchy is built: set by the owner of the system (knpemi_api.hip: kn_solver_attach; kernels_dg.hip: dg_solver)
// and, for what depends on the run, at the build (kernels_krylov.hip: amg_upkeep); read by the set-up and carried whole
// into a background rebuild.
struct KnAmgConfig {
  bool negative_strength = false;    // strength of connection from -a_ij only (classical) instead of |a_ij|
  double theta = 0.08;               // strength threshold
  bool want_fused = false;           // also build the merged operators of the fused cycle (single rank, point smoother)
  bool want_cycle = false;           // point-Jacobi hierarchy of a rank's diagonal block: the whole cycle that way
  // Optional aggregates of the finest level (auxiliary-space variant, DG systems: the broken dofs of a (sub-domain,
  // mesh vertex) form one aggregate, so the first coarse level is the continuous P1 space of the sub-domains and the
  // strength-based aggregation only starts there).  first_na == 0: aggregate every level by strength.
  std::vector<int> first_agg;
  int first_na = 0;
  // split_first: the given aggregates are split into the connected components of their strong couplings (-a_ij >=
  // split_theta sqrt(a_ii a_jj) between two dofs of ONE given aggregate): the interior penalty of a stretched cell
  // ties coincident dofs together across the facets along the long direction a hundred times more strongly than across
  // the others, and the low-energy error of the DG systems is continuous only across the former.
  bool split_first = false;
  double split_theta = 0.1;
  bool positive_conflict = false;    // aggregation keeps strongly positively coupled unknowns apart (aggregate_apart)
  // Block-smoothed hierarchies (DG): the levels below the finest run through the merged transfer operators of the fused
  // cycle (kn_fused_subcycle)
  bool sub_fused = false;
  double filter_theta = 0.0;         // > 0: prolongator smoothing with the filtered operator (weak entries lumped)
  bool first_tentative = false;      // the prolongator of the given aggregates is not smoothed
  // Optional block-Jacobi smoother on the finest level: `block` consecutive unknowns (the dofs of a DG cell) form a
  // block whose inverse is refreshed from the current values before every solve (kn_amg_refresh).  0: point Jacobi.
  int block = 0;
};
struct KnAmg {
  KnAmgConfig cfg;
  KnAmgAsync* async = nullptr;
  bool rebuild_wanted = false;       // the hierarchy has aged (iteration count doubled): rebuild it in the background
  int solves = 0;                    // solves with this hierarchy's system (KNPEMI_AMG_REBUILD_EVERY test hook)
  std::vector<KnAmgLevel> lev;
  std::vector<void*> allocs;
  bool built = false, singular = false;
  int n = 0;
  double op_complexity = 1.0;
  bool fused_ok = false;             // cfg.want_fused and the merged operators exist: every level but the last has Rm / Pm,
                                     // the last one a dense inverse
  bool sub_fused_ok = false;         // cfg.sub_fused and the merged operators below the finest level exist
  bool cycle_ok = false;             // cfg.want_cycle and the merged operators exist
  int its_ref = -1;                  // iterations of the first solve after the build (rebuild trigger)
  int its_last = 4;                  // iterations of the last fused solve: size of the next solve's first chunk
  int builds = 0;
  double* zero_sc = nullptr;         // 32 zeroed doubles: the "not done" flag the fused kernels look at
  double* binv = nullptr;            // [n / cfg.block][cfg.block][cfg.block]
  double omega_block = 1.0;          // damping 4 / (3 rho(B^-1 A))
};
void kn_amg_free(KnAmg& G);
void kn_amg_async_join(KnAmg& G);    // ends (waits for) a background rebuild; before the hierarchy or its handle goes away
// Distributed solves (knpemi_set_distributed, knpemi_dg_set_distributed: kn_dist_enable)
struct KnDist {
  bool on = false;
  std::vector<uint8_t> h_owned_emi, h_owned_knp;   // host masks in the unknown order of the two systems
  uint8_t* d_owned_emi = nullptr;
  uint8_t* d_owned_knp = nullptr;
  double* d_red = nullptr;                         // caller's reduction buffer (>= 8 doubles)
  knpemi_allreduce_fn allreduce = nullptr;
  knpemi_halo_fn halo = nullptr;
  void* ctx = nullptr;
  double n_owned_global = 0.0;                     // owned EMI unknowns summed over the ranks
  // Coarse space of the distributed EMI preconditioner (knpemi_set_distributed_coarse): hat functions over k slices (along
  // the longest axis) of every sub-domain of every rank.  nc = world * n_sub * (k + 1) <= KN_COARSE_MAX.
  int rank = -1, world = 0, nc = 0, nl = 0, k = 1;   // nl = n_sub * (k + 1) local nodes, nc = world * nl
  bool coarse_built = false;
  double* d_coarse_inv = nullptr;                  // [nc][nc] (A_c + alpha 1 1^T)^-1, the same on every rank
  double* d_coarse_z = nullptr;                    // [nl] this rank's coarse corrections
  int* d_agg_of = nullptr;                         // [Ntot] lower local node of every unknown, -1 for ghosts
  double* d_agg_w = nullptr;                       // [Ntot] its weight in the upper node
  int* d_agg_ptr = nullptr;                        // [nl + 1]
  int* d_agg_idx = nullptr;                        // unknowns of every node ...
  double* d_agg_wt = nullptr;                      // ... and their weights
};
#define KN_COARSE_MAX 64
#define KN_COARSE_OFF 8                            // coarse vector sits behind the 8 scalars of the reduction buffer

// The device solves (kernels_krylov.hip, kernels_fused.hip, kernels_amg.hip): everything they read and keep, and nothing
// else.  knpemi_handle and knpemi_dg each embed one; the owner fills the views, the hooks and the AMG configuration
// (knpemi_create; kernels_dg.hip: dg_solver), the solver files never see the owner's type.
struct KnDevice;
struct KnSysView { int n = 0; const int* rowptr = nullptr; const int* colind = nullptr; double* A = nullptr; double* b = nullptr; };
struct KnSolver {
  explicit KnSolver(KnDevice* owner) : own(owner) {}
  KnDevice* own;                       // device, main stream, `allocs` (what the solves allocate lives as long as the owner), prof
  // views of the owner's two systems: the potential, and the block-diagonal system of the `ks` solved ions
  KnSysView emi, knp;
  int ks = 0;
  double* csol = nullptr;              // [ks][emi.n] the concentrations, the iterate and the result of kn_solve_knp
  double* phi = nullptr;               // the potential, iterate and result of kn_solve_emi: phi[i * phi_stride]
  int phi_stride = 1;
  // What the owner does around a solve, as data it supplies.  An empty hook stands for the plain form on the right.
  std::function<int(double* x)> knp_load;          // csol into the solver's order of the unknowns          x = csol
  std::function<int(const double* x)> knp_store;   // ... and the solution out of it (idempotent)           csol = x
  // The fused CG's write-back of the potential (idempotent): x minus its mean -- the `np` block sums `part` times inv_n,
  // which also goes to *mean_out -- into phi, with whatever the owner forms in the same launch.  The owner sets or clears
  // it before a solve and finds in phi_stored whether that solve has run it.           phi[i * phi_stride] = x[i] - mean
  std::function<int(const double* x, const double* part, int np, double inv_n, double* mean_out)> phi_store;
  bool phi_stored = false;
  uint64_t emi_key = 0, knp_key = 0;   // the part of a fused-graph key that depends on what the hooks launch
  double* kry = nullptr; size_t kry_n = 0;           // Krylov workspace (kernels_krylov.hip)
  int kry_ones_masked = 0;                           // the workspace's `ones` vector currently holds the ownership mask
  void* kry_pinned = nullptr;                        // pinned host buffer the solvers' scalars are read through
  // state of the fused loops published by the device into mapped host memory (kernels_fused.hip: publish_state)
  double* pub_host = nullptr; double* pub_host_dev = nullptr; unsigned long long* pub_count = nullptr;
  unsigned long long pub_expected = 0;
  KnBlockCols bcols;                 // block structure of a DG problem's systems, else empty
  int spmv_lpr[2] = {0, 0};          // lanes per row of the Krylov SpMV of the two systems (from the average row length)
  double* fused_part = nullptr; size_t fused_part_n = 0;   // block partials of the dot products fused into the solver kernels
  double* guess_old[2] = {nullptr, nullptr};         // previous solutions (EMI, KNP) for knpemi_extrapolate_guess
  int guess_have[2] = {0, 0};                        // previous solutions stored so far (0, 1, 2)
  KnAmg amg_emi, amg_knp;
  // captured iteration bodies of the plain Krylov loops (kernels_krylov.hip: run_chunk); key = configuration they were
  // captured for.  Both kinds of graph are captured by kn_capture and freed by kn_solver_free.
  struct KnGraph { hipGraphExec_t exec = nullptr; uint64_t key = 0; };
  KnGraph graph_emi, graph_knp;
  // captured chunks of the fused loops (kernels_fused.hip: run_chunk_graph), keyed by everything their kernel arguments hold
  std::unordered_map<uint64_t, hipGraphExec_t> fused_graphs;
  // graph replay or direct launches for the chunks of the fused loops, decided per system from timed solves (choose_mode)
  struct FusedMode { bool decided = false, graph = true; int solves = 0; double t[2] = {0.0, 0.0}; int n[2] = {0, 0}; };
  FusedMode fused_mode[2];
  int pc_emi = KNPEMI_PC_AMG, pc_knp = KNPEMI_PC_AMG;
  int knp_min_it = 0;                  // KNPEMI_OPT_KNP_MIN_IT (ksp_min_it of the concentration solve, pdeSolver.py:101)
  int emi_norm_pre = 0;                // KNPEMI_OPT_EMI_NORM: 1 = CG tests the preconditioned residual norm (KSPCG's default)
  int knp_method = 0;                  // KNPEMI_OPT_KNP_METHOD: 0 BiCGStab on the true residual, 1 GMRES(30) as PETSc runs it
  double* gm_V = nullptr; size_t gm_n = 0;   // Krylov basis of the GMRES solve
  double* gm_state = nullptr;                // its Hessenberg column, rotations, triangular factor, dot-product partial sums
  KnDist dist;
};
int kn_amg_setup(KnSolver& sv, KnAmg& G, int n, const int* d_rowptr, const int* d_colind, const double* d_vals,
                 bool singular, const uint8_t* h_owned = nullptr);
// G.rebuild_wanted: start the rebuild of an aged hierarchy on a host thread from a snapshot of the operator, or swap a
// finished one in; G stays usable throughout
int kn_amg_rebuild_step(KnSolver& sv, KnAmg& G, int n, const int* d_rowptr, const int* d_colind, const double* d_vals,
                        bool singular);
int kn_amg_apply(KnSolver& sv, KnAmg& G, const double* vals, const double* dinv0, const double* r, double* scratch,
                 double* out);
int kn_amg_refresh(KnSolver& sv, KnAmg& G, const double* vals);   // block inverses of the current finest operator
// fused solver loops (kernels_fused.hip): the iteration of kn_solve_emi / kn_solve_knp in 6 / 13 launches
struct KnFusedSys {
  int n; const int* rowptr; const int* colind; const double* vals;   // the system of the current time step
  double* sc; double* work;   // the solver's device scalars and vector workspace (kernels_krylov.hip layout)
  size_t N;                   // stride of the workspace vectors
};
int kn_fused_subcycle(KnSolver& sv, KnAmg& G, int l0, const double* r0 = nullptr, double* out0 = nullptr);
// pre / post: what the caller has to run before the first residual / after the last iteration (both become part of the
// captured graph of a chunk; post must be idempotent, it follows every chunk).  The CG's are single launches of its own
// file that read KnSolver::phi; its post is KnSolver::phi_store where the owner has set one.
int kn_fused_cg(KnSolver& sv, KnAmg& G, const KnFusedSys& S, const double* b, double rtol, double atol, int maxit,
                int* iters, double* rr, double* bb);
int kn_fused_bicgstab(KnSolver& sv, KnAmg& G, const KnFusedSys& S, const double* b, double rtol, double atol, int maxit,
                      int* iters, double* rr, double* bb, const std::function<int()>& pre, const std::function<int()>& post);
int kn_fused_gmres(KnSolver& sv, KnAmg& G, const KnFusedSys& S, const double* b, double rtol, double atol, int maxit,
                   int* iters, double* rr, double* bb, const std::function<int()>& pre, const std::function<int()>& post);
void kn_fused_graphs_free(KnSolver& sv);
// captures what `enqueue` launches on the owner's stream into *out (nullptr on failure): the one capture path of the Krylov loops
int kn_capture(KnSolver& sv, const std::function<int()>& enqueue, hipGraphExec_t* out);
// frees the solver state that is not in the owner's `allocs`: AMG hierarchies (background rebuilds joined), pinned and
// published host buffers, captured graphs -- knpemi_destroy and knpemi_dg_destroy, before kn_device_close
void kn_solver_free(KnSolver& sv);

// The membrane ODE sweeps (kernels_ode.hip, kernels_ode_fixed.hip, the bind halves of kernels_rtc.hip): everything they read
// and keep, and nothing else.  knpemi_handle and knpemi_dg each embed one; the owner fills the view (knpemi_create,
// knpemi_ode_create, knpemi_dg_create) and maps its models to slots, the sweep files never see the owner's type.  The
// stream and the profiling slot of a launch are the caller's and come with every call.
struct KnSweeps {
  explicit KnSweeps(KnDevice* owner) : own(owner) {}
  KnDevice* own;                       // device, `allocs` (what a bind allocates lives as long as the owner), prof
  // view of the PDE side a sweep exchanges with (OdeDev is built from it: kn_ode_dev, ode_host.h)
  const double* rec = nullptr;         // [..][KN_REC] vertex (DG: dof) records
  const int* q2e = nullptr; const int* q2i = nullptr;   // [NQtot] record of every membrane dof on either side
  double* phiM = nullptr;              // [NQtot]
  double* Ich = nullptr;               // [slot][ion][NQtot]
  int NQtot = 0, n_ions = 0;
  bool have_pde = false;               // there are fields to read traces and V from (not: knpemi_ode_create)
  std::vector<KnOdeModel> ode;         // the slots; knpemi_handle: [moff[n_sub]], knpemi_dg: one, offset 0
  const void* d_lsoda_coef = nullptr;  // LsodaCoef tables, uploaded by the first LSODA sweep (kernels_ode.hip)
  std::vector<void*> rtc_modules;      // hipModule_t of run-time compiled membrane models and monitor programs
};
// unloads the modules; the device memory is in the owner's `allocs` -- knpemi_destroy and knpemi_dg_destroy, before kn_device_close
inline void kn_sweeps_free(KnSweeps& sw) {
  for (void* m : sw.rtc_modules) (void)hipModuleUnload(static_cast<hipModule_t>(m));
  sw.rtc_modules.clear();
}

// ghost refresh of a solver vector without Python (comm_rccl.hip)
struct KnVecPlan {
  bool set = false;
  const int32_t* send_idx = nullptr; const int32_t* recv_idx = nullptr;
  int n_send = 0, n_recv = 0;
  double* send_buf = nullptr; double* recv_buf = nullptr;
  std::vector<int32_t> peer;
  std::vector<int64_t> send_off, send_cnt, recv_off, recv_cnt;
};

// error plumbing ------------------------------------------------------------------------------
void kn_set_error(const std::string& msg);
#define KN_HIP(call)                                                                     \
  do {                                                                                   \
    hipError_t e_ = (call);                                                              \
    if (e_ != hipSuccess) {                                                              \
      kn_set_error(std::string(#call) + ": " + hipGetErrorString(e_));                   \
      return KNPEMI_EHIP;                                                                \
    }                                                                                    \
  } while (0)
inline int kn_fail(int code, const std::string& msg) {
  kn_set_error(msg);
  return code;
}
// after a kernel launch: KNPEMI_OK, or KNPEMI_EHIP with "<what>: <HIP's message>" (what: the kernel's name, or the text
// the caller wants in front of HIP's)
inline int kn_launch_check(const std::string& what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? KNPEMI_OK : kn_fail(KNPEMI_EHIP, what + ": " + hipGetErrorString(e));
}
// before a launch with `bytes` of dynamic LDS: above 64 KiB the kernel's limit has to be raised first
inline int kn_set_lds_limit(const void* kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return KNPEMI_OK;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  return e == hipSuccess ? KNPEMI_OK
                         : kn_fail(KNPEMI_EHIP, std::string("hipFuncSetAttribute(max dynamic LDS): ") + hipGetErrorString(e));
}
// knpemi_debug_linalg: the device copies of the caller's arrays (upload of every given slot, copy-back of the slots
// marked `out`, free), and the checks its dispatchers share.  The dispatch of an op lives in the translation unit that owns
// the kernel: kernels_krylov.hip (the entry itself) and kernels_amg.hip (kn_debug_linalg_amg, ops >= KNPEMI_LINALG_AMG_SPMV).
struct KnDebugBufs {
  const knpemi_debug_linalg_args& A;
  const char* opname;
  void* d[KNPEMI_LINALG_MAX_BUF] = {};
  KnDebugBufs(const knpemi_debug_linalg_args& a, const char* name) : A(a), opname(name) {}
  ~KnDebugBufs() { for (void* p : d) if (p) (void)hipFree(p); }
  KnDebugBufs(const KnDebugBufs&) = delete;
  KnDebugBufs& operator=(const KnDebugBufs&) = delete;
  int bad(const std::string& what) const { return kn_fail(KNPEMI_EINVAL, std::string("knpemi_debug_linalg(") + opname + "): " + what); }
  // slot s holds at least `count` elements of `elem` bytes (required), or is absent (optional)
  int need(int s, const char* name, size_t count, size_t elem, bool optional = false) const {
    if (!A.buf[s]) return optional ? KNPEMI_OK : bad(std::string(name) + " (buf[" + std::to_string(s) + "]) is null");
    if (A.bytes[s] < count * elem)
      return bad(std::string(name) + " (buf[" + std::to_string(s) + "]) holds " + std::to_string(A.bytes[s]) + " bytes, " +
                 std::to_string(count * elem) + " needed");
    return KNPEMI_OK;
  }
  const int* hi(int s) const { return static_cast<const int*>(A.buf[s]); }
  // row pointers of `rows` rows into an entry array of slot `s_entries` (elements of `elem` bytes)
  int check_rowptr(int s, const char* name, int rows, int s_entries, size_t elem) const {
    if (int rc = need(s, name, (size_t)rows + 1, sizeof(int))) return rc;
    const int* rp = hi(s);
    if (rp[0] < 0) return bad(std::string(name) + "[0] is negative");
    for (int i = 0; i < rows; ++i) if (rp[i + 1] < rp[i]) return bad(std::string(name) + " decreases at row " + std::to_string(i));
    if ((size_t)rp[rows] * elem > A.bytes[s_entries]) return bad(std::string(name) + " runs past the entries of buf[" + std::to_string(s_entries) + "]");
    return KNPEMI_OK;
  }
  // the first `count` entries of slot s lie in [lo, hi)
  int check_range(int s, const char* name, size_t count, int lo, int hi_) const {
    if (int rc = need(s, name, count, sizeof(int))) return rc;
    for (size_t i = 0; i < count; ++i)
      if (hi(s)[i] < lo || hi(s)[i] >= hi_) return bad(std::string(name) + "[" + std::to_string(i) + "] = " + std::to_string(hi(s)[i]) + " is out of range");
    return KNPEMI_OK;
  }
  int upload() {
    for (int s = 0; s < KNPEMI_LINALG_MAX_BUF; ++s) {
      if (!A.buf[s]) continue;
      KN_HIP(hipMalloc(&d[s], A.bytes[s] ? A.bytes[s] : 8));      // (an empty array is still a non-null pointer)
      if (A.bytes[s]) KN_HIP(hipMemcpy(d[s], A.buf[s], A.bytes[s], hipMemcpyHostToDevice));
    }
    return KNPEMI_OK;
  }
  int download() {
    KN_HIP(hipDeviceSynchronize());
    for (int s = 0; s < KNPEMI_LINALG_MAX_BUF; ++s)
      if (d[s] && A.out[s]) KN_HIP(hipMemcpy(A.buf[s], d[s], A.bytes[s], hipMemcpyDeviceToHost));
    return KNPEMI_OK;
  }
  template <class T> T* p(int s) const { return static_cast<T*>(d[s]); }
};
int kn_debug_linalg_amg(int op, const knpemi_debug_linalg_args& A);

// Read-back of the diagnostic builds (KN_ROW_STAMPS, KN_DG_STAMPS, KN_HX_STAMPS): `symbol` is a __device__ array of 1024
// slots, slot_stride counters apart, of which the first n_phases hold the ticks the kernel added up per phase.  On every
// `every`-th launch (`launch` counts them from 1): synchronise, print the averages per unit (`n_units` workgroups or waves a
// launch) under `label`, zero the counters.
inline void kn_stamps_report(const void* symbol, int slot_stride, int n_phases, int every, int launch, int n_units,
                             const char* label, const char* kernel, const char* units, const char* unit) {
  if (launch % every != 0) return;
  std::vector<unsigned long long> acc((size_t)1024 * slot_stride);
  const size_t bytes = acc.size() * sizeof(unsigned long long);
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(acc.data(), symbol, bytes);
  const double n = (double)every * n_units;
  std::vector<double> ph(n_phases, 0.0);
  double total = 0.0;
  for (int sl = 0; sl < 1024; ++sl) for (int i = 0; i < n_phases; ++i) ph[i] += (double)acc[(size_t)sl * slot_stride + i];
  for (int i = 0; i < n_phases; ++i) total += ph[i];
  fprintf(stderr, "%s %s, %s per %s, %d launches of %d %ss: total %.1f\n", label, kernel, units, unit, every, n_units, unit, total / n);
  for (int i = 0; i < n_phases; ++i) fprintf(stderr, "%s   phase %*d: %8.1f\n", label, n_phases > 9 ? 2 : 1, i, ph[i] / n);
  std::fill(acc.begin(), acc.end(), 0ull);
  (void)hipMemcpyToSymbol(symbol, acc.data(), bytes);
}

// The device base of both handles (knpemi_handle here, knpemi_dg in kernels_dg.hip): what they own in the same way, and the
// one set of helpers for it.  Host only.
void kn_comm_free(void* comm);   // comm_rccl.hip

// per-kernel event profiling (knpemi_profile, knpemi_dg_profile): begin/end event pairs around the launches of kernel k
struct KnProf {
  uint32_t mask = 0;                               // bit k: the launches of kernel k are bracketed
  // every stride-th one only (an event pair around a kernel on the critical path costs the step several microseconds)
  int stride = 1;
  unsigned count[KNPEMI_N_KERNELS] = {};           // launches seen since the stride was set
  std::vector<hipEvent_t> ev[KNPEMI_N_KERNELS];    // begin/end pairs
  size_t used[KNPEMI_N_KERNELS] = {};              // events of ev[k] recorded since the last read
};
// RAII bracket around one kernel launch on stream `st`; no-op unless the kernel's bit is set in the mask (k < 0: no slot)
struct KnProfScope {
  KnProf& p; int k; hipStream_t st; bool on;
  KnProfScope(KnProf& p_, int k_, hipStream_t st_) : p(p_), k(k_), st(st_), on(k_ >= 0 && ((p_.mask >> k_) & 1u)) {
    if (on && p.stride > 1 && (p.count[k]++ % p.stride) != 0) on = false;
    if (!on) return;
    auto& v = p.ev[k];
    if (p.used[k] + 2 > v.size()) {
      hipEvent_t a, b;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { on = false; return; }
      v.push_back(a); v.push_back(b);
    }
    (void)hipEventRecord(v[p.used[k]], st);
  }
  ~KnProfScope() {
    if (!on) return;
    (void)hipEventRecord(p.ev[k][p.used[k] + 1], st);
    p.used[k] += 2;
  }
};
// launches and summed time of the finished brackets of kernel k, which are forgotten; the caller has synchronised
inline int kn_prof_read(KnProf& p, int k, int64_t* launches, double* total_ms) {
  double sum = 0.0;
  for (size_t i = 0; i + 1 < p.used[k]; i += 2) {
    float ms = 0.f;
    KN_HIP(hipEventElapsedTime(&ms, p.ev[k][i], p.ev[k][i + 1]));
    sum += ms;
  }
  if (launches) *launches = (int64_t)(p.used[k] / 2);
  if (total_ms) *total_ms = sum;
  p.used[k] = 0;
  return KNPEMI_OK;
}

struct KnDevice {
  int device = 0;
  hipStream_t stream = nullptr;          // main stream
  hipEvent_t ev0 = nullptr, ev1 = nullptr;   // timer pair (knpemi_timer_*, knpemi_dg_time_kernel)
  std::vector<void*> allocs;             // everything hipMalloc'ed for the handle's lifetime
  double* d_stage = nullptr; size_t stage_len = 0;   // staging buffer for strided field I/O
  void* comm = nullptr;                  // RCCL communicator (comm_rccl.hip), NULL until knpemi_comm_init / knpemi_dg_comm_init
  int comm_world = 1;
  KnProf prof;
};
// device-count check, hipSetDevice, the non-blocking main stream and the timer pair; `who` starts the error texts
inline int kn_device_open(KnDevice* h, int device, const std::string& who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return kn_fail(KNPEMI_EHIP, who + ": no HIP device visible (the hot path has no CPU fallback)");
  if (device < 0 || device >= ndev) return kn_fail(KNPEMI_EINVAL, who + ": bad device index");
  KN_HIP(hipSetDevice(device));
  h->device = device;
  KN_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  KN_HIP(hipEventCreate(&h->ev0));
  KN_HIP(hipEventCreate(&h->ev1));
  return KNPEMI_OK;
}
inline void kn_free_all(std::vector<void*>& owner) {
  for (void* p : owner) (void)hipFree(p);
  owner.clear();
}
// The one teardown order: synchronise, free `allocs`, free the communicator (kn_device_release), then destroy the events and
// the stream.  What only one kind of handle owns is freed by that handle's destroy before these steps, and so is the
// solver state of either (kn_solver_free), whose graphs and mapped buffers belong to that stream.
inline void kn_device_release(KnDevice* h) {
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  kn_free_all(h->allocs);
  kn_comm_free(h->comm);
  h->comm = nullptr;
}
inline void kn_device_close(KnDevice* h) {
  kn_device_release(h);
  for (auto& v : h->prof.ev) for (hipEvent_t e : v) (void)hipEventDestroy(e);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->stream) (void)hipStreamDestroy(h->stream);
}

// Device memory: n (at least one) elements, recorded in `owner` -- a handle's `allocs`, or a list that is freed at another
// time (KnObserve::allocs, KnAmg::allocs).
template <class T>
int kn_alloc(std::vector<void*>& owner, size_t n, T** out) {
  void* p = nullptr;
  KN_HIP(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
  owner.push_back(p);
  *out = static_cast<T*>(p);
  return KNPEMI_OK;
}
template <class T>
int kn_zeros(std::vector<void*>& owner, hipStream_t st, size_t n, T** out) {
  if (int rc = kn_alloc(owner, n, out)) return rc;
  // zero on the handle's own (non-blocking) stream: a null-stream hipMemset is not ordered with it
  KN_HIP(hipMemsetAsync(*out, 0, std::max<size_t>(n, 1) * sizeof(T), st));
  KN_HIP(hipStreamSynchronize(st));
  return KNPEMI_OK;
}
template <class T, class U>
int kn_upload(std::vector<void*>& owner, const T* src, size_t n, U** out) {
  T* p = nullptr;
  if (int rc = kn_alloc(owner, n, &p)) return rc;
  if (n) KN_HIP(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
  *out = p;
  return KNPEMI_OK;
}
template <class T, class U>
int kn_upload(std::vector<void*>& owner, const std::vector<T>& v, U** out) { return kn_upload(owner, v.data(), v.size(), out); }
// synchronous copies on stream `st`: ordered with the work enqueued on it, done when they return
template <class T>
int kn_to_host(hipStream_t st, T* host, const T* dev, size_t n) {
  KN_HIP(hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, st));
  KN_HIP(hipStreamSynchronize(st));
  return KNPEMI_OK;
}
template <class T>
int kn_to_device(hipStream_t st, T* dev, const T* host, size_t n) {
  KN_HIP(hipMemcpyAsync(dev, host, n * sizeof(T), hipMemcpyHostToDevice, st));
  KN_HIP(hipStreamSynchronize(st));
  return KNPEMI_OK;
}
// The membrane ODE tables: host tables are row-major [dof][column], device tables [column][dof]: dst[c][r] = src[r][c]
inline void kn_transpose(const double* src, double* dst, int rows, int cols) {
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) dst[(size_t)c * rows + r] = src[(size_t)r * cols + c];
}
inline int kn_table_upload(hipStream_t st, const double* host, double* dev, int nq, int cols) {
  std::vector<double> t((size_t)nq * cols);
  kn_transpose(host, t.data(), nq, cols);
  return kn_to_device(st, dev, t.data(), t.size());
}
inline int kn_table_download(hipStream_t st, const double* dev, double* host, int nq, int cols) {
  std::vector<double> t((size_t)nq * cols);
  if (int rc = kn_to_host(st, t.data(), dev, t.size())) return rc;
  kn_transpose(t.data(), host, cols, nq);
  return KNPEMI_OK;
}

// Hexahedra come in tensor-product vertex order (bit a of a local vertex = its coordinate along axis a): whether the cell
// with the vertices cell8[0..7], vertex v at x[v * x_stride .. + 2], is in one of the 48 such orders (left-handed ones
// included) and not degenerate.  The trilinear map of a cell given in another order (e.g. the counter-clockwise order of
// other formats) folds over, i.e. its Jacobian determinant changes sign between the corners.
inline bool kn_hex_tensor_order(const double* x, int x_stride, const int* cell8) {
  int pos = 0, neg = 0;
  for (int j = 0; j < 8; ++j) {
    double e[3][3];
    for (int a = 0; a < 3; ++a) {
      const double* x0 = x + (size_t)cell8[j] * x_stride;
      const double* x1 = x + (size_t)cell8[j ^ (1 << a)] * x_stride;
      const double sgn = ((j >> a) & 1) ? -1.0 : 1.0;
      for (int k = 0; k < 3; ++k) e[a][k] = sgn * (x1[k] - x0[k]);
    }
    const double det = e[0][0] * (e[1][1] * e[2][2] - e[1][2] * e[2][1]) - e[0][1] * (e[1][0] * e[2][2] - e[1][2] * e[2][0]) +
                       e[0][2] * (e[1][0] * e[2][1] - e[1][1] * e[2][0]);
    pos += det > 0.0;
    neg += det < 0.0;
  }
  return pos == 8 || neg == 8;
}

// The same for Q1 quadrilaterals, vertex v at x[v * x_stride .. + 1]: one of the 8 tensor orders, and the bilinear map does
// not fold -- the Jacobian determinant at the four corners has one sign.  A cell in counter-clockwise order, a non-convex
// and a degenerate one fail.
inline bool kn_quad_tensor_order(const double* x, int x_stride, const int* cell4) {
  int pos = 0, neg = 0;
  for (int j = 0; j < 4; ++j) {
    double e[2][2];
    for (int a = 0; a < 2; ++a) {
      const double* x0 = x + (size_t)cell4[j] * x_stride;
      const double* x1 = x + (size_t)cell4[j ^ (1 << a)] * x_stride;
      const double sgn = ((j >> a) & 1) ? -1.0 : 1.0;
      for (int k = 0; k < 2; ++k) e[a][k] = sgn * (x1[k] - x0[k]);
    }
    const double det = e[0][0] * e[1][1] - e[0][1] * e[1][0];
    pos += det > 0.0;
    neg += det < 0.0;
  }
  return pos == 4 || neg == 4;
}

struct knpemi_handle : KnDevice {
  hipStream_t aux = nullptr;             // auxiliary stream (EMI matrix assembly beside the ODE sweep)
  hipStream_t aux2 = nullptr;            // second auxiliary stream (ODE sweeps of further membrane models)
  hipEvent_t ev_join2 = nullptr;
  hipEvent_t ev_pre_fork = nullptr, ev_pre = nullptr;   // early membrane integrals on the auxiliary stream
  int pre_pending = 0;
  hipStream_t cur = nullptr;             // stream the row-kernel launchers enqueue on (stream or aux)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int gdim = 0, cell_kind = 0, NV = 0, NF = 0, n_sub = 0, K = 0;
  std::vector<int> n_vert, n_cell, n_q, n_facet, n_models;
  std::vector<int> voff, coff, qoff, foff, moff;
  KnConsts consts{};
  KnConsts* d_consts = nullptr;        // device copy read by the kernels
  KnDev dev{};
  int have_params = 0;
  int lpr = 1;                         // lanes per row of the row kernels (1, 2, 4 or 8)
  bool hex_affine = false;             // every hexahedron is a parallelepiped / every quadrilateral a parallelogram (constant Jacobian)
  bool tet_uniform = false;            // tetrahedra: every cell a lattice tetrahedron of a uniform grid (dev.tet_tab)
  bool hex_uniform = false;            // ... and all of them are the same one: the geometry below is a constant of the mesh
  KnHexGeo hex_geo{};
  int lds_doubles_emi = 0, lds_doubles_knp = 0; // per-block LDS segment sizes (doubles)
  int lds_uniq_max = 0;                         // most distinct vertices touched by one row block
  // what knpemi_debug_layout reports: longest row of the EMI / Laplacian pattern, most pairs on one lane, most membrane
  // entries on one row; dynamic LDS of the latest EMI / KNP row launch (0: not launched yet)
  int lay_row_max = 0, lay_rowL_max = 0, lay_np_max = 0, lay_ne_max = 0;
  size_t lds_bytes_emi = 0, lds_bytes_knp = 0;
  KnSweeps sweeps{this};       // the membrane ODE sweeps; slot of (sub-domain, model): moff[sub] + model
  bool ode_only = false;       // knpemi_ode_create: membrane models without a mesh (no PDE fields)
  int n_cus = 0;               // compute units of the device, asked on first use (kernels_ode.hip: sweep_emi_eligible); -1: unknown
  // host copies of patterns for export
  std::vector<int> h_rowptr, h_colind, h_rowptrL, h_colindL;
  int comm_rank = 0;
  KnVecPlan vec_plan[2];                             // [KNPEMI_B_EMI], [KNPEMI_B_KNP]
  KnSolver solver{this};               // the device solves of the two systems (views and hooks: knpemi_api.hip, kn_solver_attach)
  int fuse_update = 0;                 // KNPEMI_OPT_FUSE_UPDATE
  int fuse_membrane = 0;               // KNPEMI_OPT_FUSE_MEMBRANE
  // Membrane-facet integrals of b_knp formed by the launch that writes the potential back (kn_launch_emi_writeback_membrane),
  // reused by knpemi_assemble_knp while current.  One rule, in host code that graph replay cannot skip: every entry point
  // that may write an input (phi, c_prev, the eliminated ion, phi_M, I_ch, parameters) bumps inputs_gen, the caller of the
  // folding launch stamps gam_gen / gam_split, the assembly compares (kn_inputs_changed, kn_gam_formed, kn_gam_current).
  uint64_t inputs_gen = 1;
  uint64_t gam_gen = 0;                // inputs_gen gam_e was formed at; 0 = never
  int gam_split = 1;
  int fold_membrane = 1;               // KNPEMI_OPT_FOLD_MEMBRANE: form them in the write-back launch of the potential
  int emi_flags = 0;                   // flags of the last knpemi_assemble_emi (the splitting scheme the step runs with)
  int lds_gam_max = 0;                 // most membrane entries of one row block
  bool blocks_clustered = false;       // row blocks are clusters of row chunks (default), not consecutive rows
  // The recorders (knpemi_record.hip); each is freed by its knpemi_*_clear, all of them by kn_record_free.
  // A series buffer: the rows a record kernel appends (record_tail.h) until the host reads them.
  struct KnSeries {
    unsigned long long* ctl = nullptr;   // [4]: rows written, rows dropped (buffer full), ticket of the last workgroup
    double* rows = nullptr;              // [capacity][n_cols]
    int capacity = 0, n_cols = 0;
  };
  // A partitioned record's place among the ranks (knpemi_*_set_partitioned): the caller's [world][n_cols] exchange buffer,
  // summed over the ranks by `allreduce` (or the library's communicator when it is null) between the record launch, which
  // writes this rank's slots, and the combine launch.  xbuf == nullptr: not partitioned.
  struct KnRankSlots {
    double* xbuf = nullptr;
    int rank = 0, world = 1;
    knpemi_allreduce_fn allreduce = nullptr;
    void* ctx = nullptr;
  };
  // The time of the previous record of a recorder that integrates over the interval between two records.
  struct KnRecordClock {
    bool have_prev = false;              // a record has been enqueued since the set-up / the last reset ...
    double t_prev = 0.0;                 // ... at this time
  };
  // Per-item fields: allocated at the first record that writes them, read back while a record since the set-up / the last
  // reset has written them.
  struct KnItemFields {
    double* fld = nullptr;
    size_t fld_len = 0;
    bool fld_valid = false;
  };
  // observables (knpemi_observe_set, kernels_observe.hip)
  struct KnObserve {
    int n_obs = 0, n_blk = 0;
    int4* blk = nullptr;                 // [n_blk] {observable, first entry, end entry, 0}
    int* blk_ptr = nullptr;              // [n_obs + 1] first block of every observable
    int* op = nullptr;                   // [n_obs]
    int* stride = nullptr;               // [n_obs]
    const double** base = nullptr;       // [n_obs] field addresses (kn_locate)
    double* denom = nullptr;             // [n_obs] divisor of a sum (1, n for a nodal mean, the measure for an average)
    int* idx = nullptr;                  // [entries]
    double* w = nullptr;                 // [entries]
    double* part = nullptr;              // [n_blk] block partials
    KnSeries ser;
    KnRankSlots slots;                   // knpemi_observe_set_partitioned: [world][n_obs]
    std::vector<void*> allocs;
  } obs;
  // membrane events (knpemi_events_set, kernels_events.hip)
  struct KnEvents {
    int n_watch = 0, keep = 0, n_grid = 0;
    bool watched[KN_MAXSUB] = {};
    KnRecordClock clock;
    KnEvTab* tab = nullptr;
    // state over the concatenated membrane dofs ([NQtot]; the ring [keep][NQtot])
    double* v_prev = nullptr;
    uint8_t* armed = nullptr;
    int* count = nullptr;
    double *t_first = nullptr, *t_last = nullptr, *v_peak = nullptr, *t_peak = nullptr, *ring = nullptr;
    std::vector<void*> allocs;
  } events;
  // ion fluxes and current density per cell (knpemi_flux_set, kernels_flux.hip) and membrane ion exchange per cell
  // (knpemi_exchange_set, kernels_exchange.hip): a watch table, workgroup partials, per-item fields and a series
  struct KnWatched {
    int n_watch = 0, n_blk = 0;
    KnWatchTab host{};                   // the table as uploaded
    int watch_of[KN_MAXSUB] = {};        // sub-domain -> watch, -1: not watched
    KnWatchTab* tab = nullptr;
    double* part = nullptr;              // [n_blk][slots] workgroup partials
    KnSeries ser;
    KnItemFields fields;
    // partitioned runs (knpemi_<name>_set_partitioned): one byte per item in watch order (1: this rank's sums and maxima
    // count it), and the rank's slots of [world][n_cols]
    uint8_t* recorded = nullptr;
    KnRankSlots slots;
    std::vector<void*> allocs;
  } flux, exchange;
  // field maps (knpemi_maps_set, kernels_maps.hip): per-item state arrays of every watch and, with a series watch, workgroup
  // partials and a series
  struct KnMaps {
    int n_watch = 0, n_blk = 0;
    KnRecordClock clock;
    KnMapTab host{};                     // the table as uploaded
    int slot_of[KNPEMI_MAPS_MAX_WATCH] = {};   // watch of knpemi_maps_set -> entry of the table (grouped by space)
    int items_of[KNPEMI_MAPS_MAX_WATCH] = {};  // ... and its number of items
    KnMapTab* tab = nullptr;
    double* part = nullptr;              // [n_blk][KN_MAPS_SLOTS] workgroup partials (series watches only)
    KnSeries ser;
    KnRankSlots slots;                   // knpemi_maps_set_partitioned: [world][n_cols], every column a sum
    std::vector<void*> allocs;
  } maps;
  // membrane monitors (knpemi_monitor_set, kernels_monitor.hip): a watch table, the columns and points of the series row,
  // workgroup partials, per-dof fields and a series
  struct KnMon {
    int n_watch = 0, n_blk = 0;
    KnMonTab host{};                     // the table as uploaded
    int slot_of[KN_MON_MAXW] = {};       // watch -> model slot (moff[sub] + model)
    hipFunction_t fn[KN_MON_MAXW][2] = {};   // watch -> the kernels of its plug-in's monitor program, NULL: the library's
    KnMonTab* tab = nullptr;
    int4* cols = nullptr;                // [n_cols] {kind, watch, quantity, point}
    int* pt_q = nullptr;                 // [n_pts][4] dofs of a point within its watch, -1: unused
    int* pt_watch = nullptr;             // [n_pts]
    double* pt_w = nullptr;              // [n_pts][4]
    double* pt_val = nullptr;            // [n_pts][4][KN_MON_MAX] what the last workgroup evaluates at the points' dofs
    double* part = nullptr;              // [n_blk][KN_MON_SLOTS] workgroup partials
    KnSeries ser;
    KnItemFields fields;                 // per dof
    // partitioned runs (knpemi_monitor_set_partitioned): the rank's slots of [world][n_cols] and, per column, the fold
    // over the ranks (KNPEMI_OBS_SUM / _MIN / _MAX) and the divisor of its sum (the global weight sum of an average, else 1)
    KnRankSlots slots;
    int* col_op = nullptr;               // [n_cols]
    double* col_denom = nullptr;         // [n_cols]
    std::vector<void*> allocs;
  } mon;
  // field snapshots (knpemi_snapshot_set, kernels_snapshot.hip): the table, the selections, and the ring (KnFrameRing);
  // recorder_free(KnSnap&) (knpemi_record.hip) frees what of the ring is not in `allocs`.
  struct KnSnap : KnFrameRing {
    int n_watch = 0, n_blk = 0;
    KnSnapTab host{};                    // the table as uploaded
    int slot_of[KNPEMI_SNAPSHOT_MAX_WATCH] = {};       // watch of knpemi_snapshot_set -> entry of the table
    long long items_of[KNPEMI_SNAPSHOT_MAX_WATCH] = {};
    KnSnapTab* tab = nullptr;
    long long move_bytes = 0;            // what one launch must move by the algorithm (kn_snapshot_bytes)
    std::vector<void*> allocs;
  } snap;
  int knp_flags = 0;                 // flags of the last knpemi_assemble_knp: the splitting scheme the exchange records with
};

// The main stream waits for the membrane ODE sweeps on the auxiliary streams: what follows reads phi_M, I_ch or the models'
// tables.  (An ODE-only handle has no side streams and no events.)
static inline int kn_wait_ode_joins(knpemi_handle* h) {
  if (h->ev_join) KN_HIP(hipStreamWaitEvent(h->stream, h->ev_join, 0));
  if (h->ev_join2) KN_HIP(hipStreamWaitEvent(h->stream, h->ev_join2, 0));
  return KNPEMI_OK;
}

inline void kn_inputs_changed(knpemi_handle* h) { ++h->inputs_gen; }
inline void kn_gam_formed(knpemi_handle* h, int split) { h->gam_gen = h->inputs_gen; h->gam_split = split; }
inline bool kn_gam_current(const knpemi_handle* h, int split) { return h->gam_gen == h->inputs_gen && h->gam_split == split; }

void kn_comm_destroy(knpemi_handle* h);   // comm_rccl.hip
int kn_comm_create(int device, int rank, int world, const char* id_bytes, size_t len, void** out);
int kn_comm_sendrecv(void* comm, int world, int device, hipStream_t stream, const double* send_buf_dev, double* recv_buf_dev,
                     int n_parts, const int32_t* peer, const int64_t* send_off, const int64_t* send_cnt,
                     const int64_t* recv_off, const int64_t* recv_cnt);
int kn_gamma_quadrature(int NF, std::vector<double>* out);   // degree-6 membrane-facet rule (knpemi_api.hip)
// where a field of knpemi_set_field / knpemi_get_field lives on the device (knpemi_api.hip)
struct KnFieldLoc { double* base; int stride; size_t n; };
int kn_locate(knpemi_handle* h, int field, int sub, int idx, KnFieldLoc* loc);
void kn_record_free(knpemi_handle* h);    // every recorder's device memory (knpemi_record.hip)

// kernel launchers (kernels_*.hip) ------------------------------------------------------------
int kn_launch_emi_rows(knpemi_handle* h, int flags);
// Launch shape of a row block, of either system (KN_ROWS_EMI, KN_ROWS_KNP) on simplices, hexahedra and quadrilaterals:
// accumulator doubles per solved field, staged records, fused membrane integrals (KNP with KNPEMI_OPT_FUSE_MEMBRANE, else 0),
// the geometry variant -- 2: lattice cells (tetrahedra or boxes of a uniform grid: records without coordinates), 1: affine
// hexahedra / quadrilaterals, 0: general -- and the dynamic LDS bytes (records of gdim coordinates and the S fields, or the
// S + 1 values of the lattice cells).  One rule for the six row kernels and for the row blocks of the fused launch
// (kernels_sweep_emi.hip).
enum { KN_ROWS_EMI = 0, KN_ROWS_KNP = 1 };
struct KnRowShape { int acc_n = 0, rec_n = 0, gam_n = 0, geo = 0; size_t lds = 0; };
KnRowShape kn_rows_shape(const knpemi_handle* h, int system);
int kn_launch_knp_rows(knpemi_handle* h, int flags);
int kn_launch_knp_membrane_pre(knpemi_handle* h, int flags);
int kn_launch_emi_membrane_rhs(knpemi_handle* h, int flags);
int kn_launch_knp_membrane(knpemi_handle* h, int flags);
int kn_launch_emi_writeback_membrane(knpemi_handle* h, const double* x, const double* part, int np, double inv_n, double* mean_out);
int kn_launch_membrane_mass(knpemi_handle* h, int n_entries, const int* d_entry_row, double* d_out);
int kn_launch_update_pde(knpemi_handle* h);
// the observables of either handle on the owner's main stream: the table holds the field addresses, so the launch needs
// nothing else of the handle
int kn_launch_observe(KnDevice* own, const knpemi_handle::KnObserve& O);
int kn_launch_observe_combine(knpemi_handle* h);
// the combine launch of a partitioned record (kernels_observe.hip): op / denom of the observables, or op == nullptr and
// col_max of a watch table (sums and maxima from 0; both NULL: every column a sum).  keep_nan: minimum and maximum keep a NaN
// as the monitors' mon_min / mon_max do (fmin / fmax, the observables' fold, drop it)
int kn_launch_record_combine(knpemi_handle* h, const char* who, int n_cols, int capacity, int world, int rank, const int* op,
                             const double* denom, const uint8_t* col_max, double* xbuf, unsigned long long* ctl, double* rows,
                             bool keep_nan = false);
// the membrane events of either handle on the owner's main stream; the view of the samples is the owner's: phi_M over its
// concatenated membrane dofs (knpemi_handle: dev.phiM, dev.NQtot; knpemi_dg: the membrane nodes)
struct KnEvSamples { const double* phiM; int nq_tot; };
int kn_launch_events_record(KnDevice* own, const knpemi_handle::KnEvents& E, const KnEvSamples& V, int first, double t,
                            double t_prev);
int kn_launch_events_reset(KnDevice* own, const knpemi_handle::KnEvents& E, const KnEvSamples& V);
int kn_launch_maps_record(knpemi_handle* h, double t, double t_prev);
int kn_launch_maps_reset(knpemi_handle* h);
int kn_launch_snapshot_pack(knpemi_handle* h, char* frame);
int kn_launch_flux(knpemi_handle* h, int write_fields);
int kn_launch_exchange(knpemi_handle* h, int write_fields);
int kn_launch_monitor(knpemi_handle* h, double t, int write_fields);
// one watch, fields only, no series row: d_tab a device copy of a table with one watch, fld its [bits of mask][nq] output
// fn: the fields kernel of a plug-in's monitor program, NULL: the library's kernel (a shipped model)
int kn_launch_monitor_eval(knpemi_handle* h, const KnMonTab* d_tab, int nq, double t, double* fld, hipFunction_t fn);
// kernels_rtc.hip: the monitor program of a plug-in (knpemi_monitor_bind_source) and the launch of one of its kernels
int kn_rtc_monitor_bind(KnSweeps& sw, KnOdeModel& m, int n_monitored, const char* monitor_source);
struct OdeDev;
int kn_rtc_launch_monitor(hipStream_t st, hipFunction_t fn, unsigned grid, unsigned block, const OdeDev& dv,
                          const KnMonArgs& a);
int kn_rtc_bind(KnSweeps& sw, KnOdeModel& m, int n_states, int n_params, const char* rhs_source);
// (the membrane ODE sweeps: ode_host.h)
int kn_solve_emi(KnSolver& sv, double rtol, double atol, int maxit, int* iters, double* relres);
int kn_solve_knp(KnSolver& sv, double rtol, double atol, int maxit, int* iters, double* relres);
int kn_extrapolate_guess(KnSolver& sv, int which);
// Distributed solves on or (owned_emi == nullptr) off for either handle: uploads the two ownership masks (the caller's
// unknown orders), counts the owned unknowns of the potential system over the ranks, keeps the hooks.  `who`: the entry point
int kn_dist_enable(KnSolver& sv, const uint8_t* owned_emi, std::vector<uint8_t>&& owned_knp, void* reduce_buf_dev,
                   knpemi_allreduce_fn allreduce, knpemi_halo_fn halo, void* ctx, const char* who);
int kn_launch_knp_order(knpemi_handle* h, double* x, int to_blocks);
int kn_launch_knp_writeback_update(knpemi_handle* h, const double* x);
int kn_launch_halo(knpemi_handle* h, int kind, int pack, const int32_t* idx, int n, double* buf);
int kn_launch_field_scatter(hipStream_t st, const double* src, double* dst, int n, int dst_stride);
int kn_launch_field_gather(hipStream_t st, const double* src, int src_stride, double* dst, int n);
int kn_launch_trace(knpemi_handle* h, const double* ue, const double* ui, int sub, double* qe, double* qi);
int kn_launch_vec_index(hipStream_t st, double* vec, const int32_t* idx, int n, double* buf, int gather);
// knpemi_vec_gather / _scatter and knpemi_dg_vec_gather / _scatter: buf[i] = vec[idx[i]] (gather) or the reverse, on the
// handle's main stream; `who`: the entry point (knpemi_api.hip)
int kn_vec_index(KnDevice* h, const char* who, const void* vec_dev, const int32_t* idx_dev, int n, const void* buf_dev, int gather);
