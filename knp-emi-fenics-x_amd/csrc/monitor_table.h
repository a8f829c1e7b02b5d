// The table and the launch arguments of the membrane monitors' record kernel (monitor_kernel.h).  Plain types only and no
// include: the header is compiled by hipcc into the library (through knpemi_internal.h) and at run time by hipRTC into the
// monitor program of a plug-in model (kernels_rtc.hip).
#pragma once

// Table of the membrane monitors (monitor_kernel.h), read by the record kernel.  A watch is one bound (sub-domain,
// model) slot: workgroup b belongs to watch w with bstart[w] <= b < bstart[w + 1] and takes 256 consecutive dofs of the
// watch's nq, one per lane.  The tables are the slot's own, [column][dof].  pde: the lane works on a private copy of its
// parameter row in which columns ion_e[k] / ion_i[k] hold the traces of ion k (vertex records of q2e / q2i) and on a
// state in which component v_index is phi_M; else row and state are as the tables hold them.  mask: the quantities
// written as per-dof fields, [selected quantity][nq] from fbase doubles on; rmask: the quantities some reduction column
// needs.  A workgroup's partial has KN_MON_SLOTS doubles: quantity i at 3 i .. (sum of weight * value, minimum, maximum
// over the dofs with weight > 0).  Column c of the series row is cols[c] = {kind, watch, quantity, point}: kind
// KNPEMI_MON_POINT sums pt_w * value over the up to 4 dofs pt_q[4 point ..] of the point (-1: unused), the other kinds
// fold a slot over the watch's workgroups in their order (the average divides the integral by wsum, the sum of weights).
#define KN_MON_MAX 32
#define KN_MON_MAXW 16
#define KN_MON_SLOTS (3 * KN_MON_MAX)
struct KnMonWatch {
  int model_id, nq, q0, n_ions, v_index, pde;
  unsigned mask, rmask;
  int ion_e[4], ion_i[4];     // [KNPEMI_MAX_IONS]
  const double* states;
  const double* params;
  const double* weight;
  double wsum;
  long long fbase;
};
struct KnMonTab {
  int n_watch, n_cols, n_pts;
  int bstart[KN_MON_MAXW + 1];
  KnMonWatch w[KN_MON_MAXW];
};

// A record is one launch per run of consecutive watches that share a program -- the library's kernel for the shipped
// models, the hipRTC program of a plug-in's monitor for the slots bound from it; a table of shipped models is ONE launch.
// Workgroup blockIdx.x of a launch is workgroup blk0 + blockIdx.x of the record; the workgroup that draws the last of the
// record's n_blk_total tickets writes the row.  Partitioned (slot != NULL; knpemi_monitor_set_partitioned): it writes the
// folded columns -- the average undivided -- into slot[0 .. n_cols) and claims no row: the caller sums the exchange buffer
// over the ranks and record_combine_kernel (kernels_observe.hip) folds the ranks' slots, divides and appends the row.  A
// watch may then have nq == 0 (no workgroup; its columns fold to the operation's identity).
struct KnMonArgs {
  const KnMonTab* tab;
  const int* cols;             // [n_cols][4] {kind, watch, quantity, point}
  const int* pt_watch;         // [n_pts]
  const int* pt_q;             // [n_pts][4]
  const double* pt_w;          // [n_pts][4]
  double* pt_val;              // [n_pts][4][KN_MON_MAX]
  double* part;                // [n_blk_total][KN_MON_SLOTS]
  unsigned long long* ctl;     // the series buffer's counters; NULL: no series row (knpemi_monitor_eval)
  double* rows;
  double* fld;
  double* slot;                // partitioned: this rank's n_cols slots of the exchange buffer; NULL: append the row to `rows`
  int capacity, blk0, n_blk_total;
  double t;
};
