/* knpemi_hip.h -- C ABI of libknpemi_hip.so, the MI355X (gfx950) implementation of the
 * per-time-step hot path of adajel/knp-emi-fenics-x.
 *
 * The reference has no FFI of its own: its hot path is reached through Python calls into
 * DOLFINx/PETSc/numbalsoda.  Each entry point below names the reference call it replaces
 * (paths relative to the reference repository root).  Conventions:
 *   - every function returns 0 on success and a negative KNPEMI_E* code on failure; nothing
 *     throws across the boundary; knpemi_last_error() returns the message of the last failure
 *     on the calling thread;
 *   - the caller owns every host buffer; the library owns all device memory behind the
 *     opaque handle and frees it in knpemi_destroy();
 *   - a handle is not thread-safe; handles on different devices are independent;
 *   - kernels are enqueued on the handle's HIP stream; getters that copy to the host and
 *     knpemi_sync() block until that stream is idle.
 *   - all floating point data is IEEE binary64, all indices are int32.
 */
#ifndef KNPEMI_HIP_H
#define KNPEMI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KNPEMI_OK 0
#define KNPEMI_EINVAL (-1)   /* bad argument / unsupported configuration */
#define KNPEMI_EHIP (-2)     /* HIP runtime error (no device, launch failure, ...) */
#define KNPEMI_ENOMEM (-3)
#define KNPEMI_ESOLVE (-5)   /* Krylov solver did not converge (ksp_error_if_not_converged, pdeSolver.py:20,27) */
#define KNPEMI_EODE (-4)     /* LSODA reported failure on at least one membrane dof
                                (`assert success`, src/knpemi/odeSolver.py:121) */

/* cell kinds (CG-1 on each): triangle / tetrahedron = P1, hexahedron = Q1, quadrilateral = Q1 in 2-D (what
 * dolfinx.mesh.create_rectangle(..., CellType.quadrilateral) gives; the conforming systems only, knpemi_dg_create
 * refuses it)
 * (src/knpemi/emiWeakForm.py:66, examples/idealized_geometries/make_mesh_2D.py:53-55,
 *  make_mesh_3D.py:100-102) */
#define KNPEMI_TRIANGLE 0
#define KNPEMI_TETRAHEDRON 1
#define KNPEMI_HEXAHEDRON 2
#define KNPEMI_QUADRILATERAL 3

/* membrane models shipped as device code (the reference's numba cfunc plug-ins):
 *   HH_SI  examples/idealized_geometries/mm_hh.py:139-227          (4 states, 22 parameters)
 *   HH_MV  examples/local_astrocyte_depolarization/mm_hh.py:130-201 (4 states, 22 parameters)
 *   GLIAL  examples/local_astrocyte_depolarization/mm_glial.py:133-205 (1 state, 23 parameters) */
#define KNPEMI_MODEL_HH_SI 0
#define KNPEMI_MODEL_HH_MV 1
#define KNPEMI_MODEL_GLIAL 2

#define KNPEMI_MAX_IONS 4   /* ionic species K = 2..4, the last one eliminated (knpWeakForm.py:53,92,131) */
#define KNPEMI_MAX_SUB 8
#define KNPEMI_MAX_MODELS 4   /* membrane models per cellular sub-domain */

/* Fields addressable with knpemi_set_field / knpemi_get_field.  `sub` is the sub-domain index
 * (0 = ECS), `idx` the ion index k or, for I_CH, model*KNPEMI_MAX_IONS + k.  Lengths are the
 * number of vertices of the sub-mesh (bulk fields) or of membrane dofs of Q_sub (PHI_M, I_CH):
 * exactly `Function.x.array` of the reference objects named on the right. */
#define KNPEMI_F_PHI 0      /* phi[tag]                      emiWeakForm.py:68   */
#define KNPEMI_F_C 1        /* c[tag][k], k < K-1            knpWeakForm.py:65   */
#define KNPEMI_F_C_PREV 2   /* c_prev[tag][k], k < K-1       knpWeakForm.py:67   */
#define KNPEMI_F_C_ELIM 3   /* ion_list[-1]['c_tag']         knpWeakForm.py:77   */
#define KNPEMI_F_PHI_M 4    /* phi_M_prev[tag]               emiWeakForm.py:78   */
#define KNPEMI_F_I_CH 5     /* mem_model['I_ch_k'][ion]      utils.py:137-141    */
#define KNPEMI_F_SOURCE 6   /* ion['f_source'] (ECS only)    knpWeakForm.py:164-166 */

/* matrices / vectors */
#define KNPEMI_A_EMI 0      /* a  of emi_system   emiWeakForm.py:138-167 */
#define KNPEMI_P_EMI 1      /* p  of emi_system   emiWeakForm.py:169-198 */
#define KNPEMI_A_KNP 2      /* a (= p) of knp_system  knpWeakForm.py:123-143,319 */
#define KNPEMI_B_EMI 0      /* L of emi_system    emiWeakForm.py:201-241 */
#define KNPEMI_B_KNP 1      /* L of knp_system    knpWeakForm.py:146-216 */

/* assemble flags */
#define KNPEMI_WANT_P 1       /* also fill P_EMI (fused with A_EMI, one pass) */
#define KNPEMI_NO_SPLITTING 2 /* splitting_scheme=False (emiWeakForm.py:234-236, knpWeakForm.py:201-206) */
/* Overlap of the ODE sweep with the EMI matrix assembly (they are independent: only the membrane
 * Robin term of b_emi needs the ODE output phi_M_prev / I_ch).
 *   KNPEMI_SKIP_MEMBRANE_RHS: knpemi_assemble_emi leaves that term out; add it later with
 *                             knpemi_assemble_emi_membrane_rhs (same flags for splitting);
 *   KNPEMI_ON_AUX_STREAM:     knpemi_assemble_emi runs on the handle's auxiliary stream, ordered after
 *                             everything enqueued so far; knpemi_join() orders the main stream after it. */
#define KNPEMI_SKIP_MEMBRANE_RHS 4
#define KNPEMI_ON_AUX_STREAM 8

typedef struct knpemi_handle knpemi_handle;

/* Flattened topology of the mixed-dimensional problem.  Replaces what the reference builds with
 * scifem.extract_submesh (run_3D.py:156-158), dolfinx function spaces (emiWeakForm.py:63-79) and
 * scifem.compute_interface_data (emiWeakForm.py:39-42).  All per-sub arrays have n_sub entries;
 * entry 0 is the ECS.  Vertices on a membrane exist once in the ECS sub-mesh and once in the
 * cell's sub-mesh.  Facet vertex a of facet f is the same physical point in facet_e, facet_i
 * and facet_q ("+" = ECS side, "-" = cell side; emiWeakForm.py:25-26). */
typedef struct {
  int32_t gdim;                      /* 2 or 3 */
  int32_t cell_kind;                 /* KNPEMI_TRIANGLE | TETRAHEDRON | HEXAHEDRON | QUADRILATERAL (gdim 2) */
  int32_t n_sub;                     /* sub-domains, ECS first */
  int32_t n_ions;                    /* K = 2..4; the last ion is eliminated (run_3D.py:255-256) */
  const int32_t* n_vert;             /* [n_sub] vertices (owned + ghost) of each sub-mesh */
  const int32_t* n_cell;             /* [n_sub] */
  const double* const* x;            /* [n_sub] -> n_vert*gdim, row-major */
  const int32_t* const* cells;       /* [n_sub] -> n_cell*nv sub-mesh vertex ids (hexahedra and quadrilaterals: local vertex j at
                                        the reference point whose coordinate along axis a is bit a of j; any of the 48 (8)
                                        such orders of a cell, left-handed ones included; a cell whose Jacobian determinant
                                        changes sign between its corners -- counter-clockwise order, non-convex, degenerate --
                                        is refused) */
  const int32_t* n_q;                /* [n_sub] membrane dofs of Q_sub (0 for the ECS) */
  const int32_t* n_facet;            /* [n_sub] membrane facets of the cell (0 for the ECS) */
  const int32_t* const* facet_e;     /* [n_sub] -> n_facet*nf ECS sub-mesh vertex ids */
  const int32_t* const* facet_i;     /* [n_sub] -> n_facet*nf cell sub-mesh vertex ids */
  const int32_t* const* facet_q;     /* [n_sub] -> n_facet*nf dofs of Q_sub */
  const int32_t* const* facet_model; /* [n_sub] -> n_facet index of the membrane model whose
                                        tag the facet carries (mm['ode'].tag), -1 = none */
  const int32_t* const* q_to_e;      /* [n_sub] -> n_q ECS vertex of each Q dof (utils.py:150-207) */
  const int32_t* const* q_to_i;      /* [n_sub] -> n_q cell vertex of each Q dof */
  const int32_t* n_models;           /* [n_sub] membrane models of the cell (len(mem_models)) */
  /* Optional.  Hexahedra: the three edge vectors e_t = x[1 << t] - x[0] (row t) shared by EVERY cell of a uniform box mesh
   * as its generator knows them (make_mesh_3D.py:100-102: dolfinx.mesh.create_box on a uniform grid), all zero = unknown.
   * When every cell matches it (or, unknown, the first cell) to 1e-9 the row kernels use it as the geometry of every cell
   * and stage no coordinates; a generator that supplies it gives every rank of a partitioned run the same bits.
   * Tetrahedra: the edge vectors of the uniform GRID the mesh was split from (BASELINE configs 2, 3, 5: six Kuhn tetrahedra
   * per grid cell).  When the vertices of every cell are corners of one grid cell (lattice coordinates within 1e-6 of
   * integers) and no Laplacian row is longer than 31, the row kernels take gradient products and volumes from a table of
   * the (at most eight) cell shapes and stage no coordinates; there is no fall-back to the first cell: all zero, or a cell
   * that does not fit, keeps the general kernels.
   * Quadrilaterals: ignored (there is no uniform-cell variant of their row kernels). */
  double uniform_cell[9];
} knpemi_problem_desc;

/* Physical parameters: the `physical_params` / `ion_list` dictionaries (run_3D.py:180-256). */
typedef struct {
  double dt, F, psi, C_M;
  double z[KNPEMI_MAX_IONS];                            /* ion['z'] */
  double D[KNPEMI_MAX_SUB][KNPEMI_MAX_IONS];            /* ion['D'][tag] */
  double rho_z;                                         /* rho['z'] (utils.py:249) */
  double rho[KNPEMI_MAX_SUB];                           /* rho[tag] */
  double C_phi;                                         /* physical_parameters['C_phi'], its own entry in the reference
                                                           (run_2D.py:187,208; emiWeakForm.py:164,231-236): the membrane
                                                           coupling and Robin datum of the EMI forms.  <= 0: C_M / dt */
} knpemi_params;

const char* knpemi_last_error(void);
int knpemi_device_count(void);

/* Build the device problem: uploads the topology, derives vertex->cell adjacency, CSR patterns
 * and row-relative scatter slots.  Replaces LinearProblem construction (pdeSolver.py:46-66,
 * 121-139: sparsity pattern + FFCx JIT). */
int knpemi_create(const knpemi_problem_desc* desc, int device, knpemi_handle** out);
void knpemi_destroy(knpemi_handle* h);
int knpemi_set_params(knpemi_handle* h, const knpemi_params* p);
int knpemi_sync(knpemi_handle* h);

/* Function I/O (`Function.x.array[:] = ...` / reading it back). */
int knpemi_set_field(knpemi_handle* h, int field, int sub, int idx, const double* host, size_t n);
int knpemi_get_field(knpemi_handle* h, int field, int sub, int idx, double* host, size_t n);

/* Assembly: the matrix/vector assembly inside problem_emi.solve() / problem_knp.solve()
 * (run_3D.py:355-356 -> dolfinx assemble_matrix/assemble_vector over FFCx kernels). */
int knpemi_assemble_emi(knpemi_handle* h, int flags);
int knpemi_assemble_knp(knpemi_handle* h, int flags);
int knpemi_assemble_emi_membrane_rhs(knpemi_handle* h, int flags);
/* The membrane-facet integrals of b_knp (knpWeakForm.py:168-214) in two parts.  Everything of the integrand that does
 * not depend on the potential -- the rational factors alpha_k, C_k g_k with phi_M and I_ch from the ODE step -- is
 * integrated by knpemi_assemble_knp_membrane_early(flags [| KNPEMI_ON_AUX_STREAM]) as soon as the ODE sweep has
 * finished, i.e. BESIDE the EMI solve; knpemi_assemble_knp(flags | KNPEMI_MEMBRANE_EARLY) then only applies the small
 * facet matrices to the jump of the potential just solved for.  Same integrals as the one-part form (1e-15 apart:
 * another summation order), one kernel less between the two solves.  Measured on MI355X it does not pay at the
 * BASELINE sizes: the membrane rows of the KNP row kernel get longer (facet -> vertex -> record loads per entry) by more
 * than the facet kernel's 13-19 us (config 2: 0.187 -> 0.193 ms per step; 995 k tets: 0.262 -> 0.275), so the
 * stepper keeps the one-part form by default. */
#define KNPEMI_MEMBRANE_EARLY 16
int knpemi_assemble_knp_membrane_early(knpemi_handle* h, int flags);
int knpemi_join(knpemi_handle* h);

/* CSR access.  A_EMI/P_EMI: square, unknown order [phi_0, phi_1, ...] (pdeSolver.py:42).
 * A_KNP: block diagonal, unknown order [c[0][0], c[0][1], c[1][0], ...] (pdeSolver.py:117). */
int knpemi_csr_dims(knpemi_handle* h, int which, int64_t* n_rows, int64_t* nnz);
int knpemi_get_csr_pattern(knpemi_handle* h, int which, int32_t* rowptr, int32_t* colind);
int knpemi_get_csr_values(knpemi_handle* h, int which, double* vals);
int knpemi_get_rhs(knpemi_handle* h, int which, double* b);
/* Caller-supplied values of an operator / right-hand side, in the layout of knpemi_get_csr_values / knpemi_get_rhs
 * (petsc4py Mat.setValuesCSR / Vec.setArray on `problem.A` / `problem.b`, pdeSolver.py:56-66 expose both objects).
 * Synchronous. */
int knpemi_set_csr_values(knpemi_handle* h, int which, const double* vals);
int knpemi_set_rhs(knpemi_handle* h, int which, const double* b);
/* Device-resident views for on-GPU consumers (solvers, RCCL halo exchange through torch). */
int knpemi_device_csr(knpemi_handle* h, int which, const int32_t** rowptr, const int32_t** colind,
                      const double** vals);
int knpemi_device_rhs(knpemi_handle* h, int which, const double** b);
/* Write a solver result back into the bulk fields: x has the unknown order of the system
 * (`which` = KNPEMI_B_EMI -> phi, KNPEMI_B_KNP -> c).  on_device != 0: x is a device pointer (one launch, nothing
 * synchronised).  With KNPEMI_OPT_FUSE_UPDATE the KNP write-back is followed by (device: fused with) the end-of-step
 * update knpemi_update_pde, on both paths. */
int knpemi_set_solution(knpemi_handle* h, int which, const double* x, int on_device);
int knpemi_get_solution(knpemi_handle* h, int which, double* x);

/* Linear solves on the device (adjacent to the hot path): the KSP solve inside
 * problem_emi.solve() / problem_knp.solve() with the iterative options of pdeSolver.py:24-35,99-110.
 * EMI: preconditioned CG on A_EMI x = B_EMI with the constant null space projected out (:74-78);
 * KNP: right-preconditioned BiCGStab on the block-diagonal system.  Both start from the current fields
 * (ksp_initial_guess_nonzero), stop at ||r|| <= max(atol, rtol ||b||) and write the solution back into
 * phi / c.  Returns KNPEMI_ESOLVE when maxit is reached. */
enum { KNPEMI_PC_JACOBI = 0, KNPEMI_PC_AMG = 1 };
int knpemi_solve_emi(knpemi_handle* h, double rtol, double atol, int maxit, int* iters, double* relres);
int knpemi_solve_knp(knpemi_handle* h, double rtol, double atol, int maxit, int* iters, double* relres);
/* Replace the initial guess of the next solve of `which` (the current phi / c, i.e. the previous solution:
 * ksp_initial_guess_nonzero, pdeSolver.py:26,101) by the extrapolation of the last solutions: 3 x_n - 3 x_(n-1) + x_(n-2)
 * once three are known, 2 x_n - x_(n-1) after two; the first call only records x_n.  Call once per time step, before
 * the solve. */
int knpemi_extrapolate_guess(knpemi_handle* h, int which);
/* Preconditioner of the device solve of system `which` (KNPEMI_B_EMI / KNPEMI_B_KNP): the counterpart of
 * pc_type / pc_hypre_type in pdeSolver.py:27-34,102-109.  KNPEMI_PC_AMG: smoothed-aggregation V(1,1) cycle,
 * strength threshold `theta` (<= 0: default 0.08); the hierarchy is (re)built at the next solve and kept for
 * the following time steps (rebuilt when the iteration count has doubled).  Default: AMG for both. */
int knpemi_solver_setup(knpemi_handle* h, int which, int precond, double theta);
/* levels / operator complexity / number of builds of the AMG hierarchy of `which` (0 levels: not built). */
int knpemi_solver_info(knpemi_handle* h, int which, int* levels, double* op_complexity, int* builds);

/* Membrane ODEs: MembraneModel (src/knpemi/odeSolver.py:6-188).  `states`/`params` are the
 * row-major [n_q][n_states|n_params] tables `MembraneModel.states/.parameters`. */
int knpemi_ode_bind(knpemi_handle* h, int sub, int model, int model_id, int n_states, int n_params);
/* A membrane model that brings its own right-hand side (the reference accepts any module with a numba cfunc
 * `rhs_numba(t, states, values, parameters)`, odeSolver.py:96, e.g. examples/benchmark/mm_glial.py:127-215).
 * `rhs_source` is HIP source that defines
 *     __device__ void rhs(double t, const double* states, double* values, double* parameters);
 * with the cfunc's semantics (parameters is the in/out row of the dof: what the last call stores in I_ch_* is handed
 * to the PDEs).  It is compiled for gfx950 with hipRTC under the sweep kernel of the shipped models; one lane per
 * state component for 1, 2, 4 or 8 states, one thread per dof otherwise.  knpemi_ode_compile_source only compiles
 * (no device needed) and returns the compiler's messages. */
int knpemi_ode_bind_source(knpemi_handle* h, int sub, int model, int n_states, int n_params, const char* rhs_source);
int knpemi_ode_compile_source(int n_states, int n_params, const char* rhs_source, char* log, size_t log_len);
int knpemi_ode_set_tables(knpemi_handle* h, int sub, int model, const double* states,
                          const double* params);
int knpemi_ode_get_tables(knpemi_handle* h, int sub, int model, double* states, double* params);
/* stimulus_mask[n_q] (may be NULL = everywhere) and (param index, value) pairs written into the
 * masked rows before every step (odeSolver.py:98-112). */
int knpemi_ode_set_stimulus(knpemi_handle* h, int sub, int model, const uint8_t* stimulus_mask,
                            int n_pairs, const int32_t* param_idx, const double* values);
/* One fused launch of update_ode_variables (utils.py:210-235: with KNPEMI_ODE_SET_TRACES the
 * concentration traces go into the "<ion>_e"/"<ion>_i" parameter columns, with KNPEMI_ODE_SET_V
 * V <- phi_M_prev, i.e. the k > 0 branch of utils.py:233), MembraneModel.step_lsoda
 * (odeSolver.py:92-127) and the copy-back of run_3D.py:104-109 (phi_M_prev <- V, I_ch_k <-
 * currents).  ion_param[3*K] = parameter indices of "<ion>_e", "<ion>_i", "I_ch_<ion>" for each
 * ion (ode.parameter_indices), v_index = ode.state_indices('V'). */
#define KNPEMI_ODE_SET_V 1
#define KNPEMI_ODE_SET_TRACES 2
/* run the sweep on the auxiliary stream (fork after what is queued on the main stream; knpemi_join waits for it):
 * lets a caller keep the LONGER of {ODE sweep, EMI matrix assembly} on the main stream, so that the work that follows
 * the join does not pay the cross-stream signal latency */
#define KNPEMI_ODE_ON_AUX_STREAM 4
/* the same on a second auxiliary stream: the sweeps of different membrane models (neuron, glia, ...) are independent
 * of each other and each fills a fraction of the chip only, so they run side by side */
#define KNPEMI_ODE_ON_AUX2_STREAM 8
int knpemi_ode_step(knpemi_handle* h, int sub, int model, double t0, double dt, double rtol,
                    double atol, int flags, const int32_t* ion_param, int v_index);
/* knpemi_ode_step and knpemi_assemble_emi(emi_flags | KNPEMI_SKIP_MEMBRANE_RHS), both on the main stream (no auxiliary-stream
 * flag in either set of flags: KNPEMI_EINVAL).  A, P and the volume part of b_emi depend on the concentrations only, not
 * on what the sweep writes, and a small sweep leaves most of the chip idle: where the problem is eligible ONE launch holds
 * the sweep's workgroups and the row blocks (*fused = 1), else the two launches follow each other (*fused = 0); the results
 * are bit for bit the same.  Eligible: a model that ships with the library, integrated by LSODA; the only model of the
 * handle; no partition; tetrahedra; a sweep of at most 3/4 of the device's compute units in workgroups, and row blocks for
 * at most 7 rounds on the units left over.  KNPEMI_FUSED_SWEEP=0 in the environment: never fused.
 * Either way the membrane Robin term of b_emi is pending: call knpemi_assemble_emi_membrane_rhs(emi_flags) next.  The
 * profiling bracket of the fused launch is KNPEMI_K_ODE. */
int knpemi_ode_step_emi(knpemi_handle* h, int sub, int model, double t0, double dt, double rtol,
                        double atol, int flags, const int32_t* ion_param, int v_index, int emi_flags, int* fused);
/* RHS evaluations / internal steps / failed dofs summed over all knpemi_ode_step launches since
 * the previous call (the counters are reset by this call). */
int knpemi_ode_stats(knpemi_handle* h, int sub, int model, int64_t* n_rhs, int64_t* n_steps,
                     int32_t* n_failed);

/* Membrane models without a mesh: the reference's MembraneModel(ode, ct, tag, Q) steps its model over the dofs of any
 * CG-1 space on its own (odeSolver.py:8-50; its calibration tool builds an interval mesh for nothing else).  Creates a
 * handle with n_models membrane models of nq[i] dofs each and no PDE problem.  Model i is addressed as sub = 1 + i,
 * model = 0 (n_models <= KNPEMI_MAX_SUB - 1).  knpemi_ode_bind, knpemi_ode_bind_source, knpemi_ode_set_tables,
 * knpemi_ode_get_tables, knpemi_ode_set_stimulus, knpemi_ode_step, knpemi_ode_stats, knpemi_ode_advance, the
 * knpemi_events_* calls and knpemi_destroy work on it as on a PDE handle; no other entry point takes it.
 * knpemi_ode_step refuses the flags that read PDE fields (KNPEMI_ODE_SET_TRACES, KNPEMI_ODE_SET_V: KNPEMI_EINVAL); its
 * phi_M write-back goes to a buffer of the handle, and there are no ions (ion_param is read for 0 ions; pass any
 * non-NULL pointer). */
int knpemi_ode_create(int device, int n_models, const int32_t* nq, knpemi_handle** out);
/* Steady-state mode of knpemi_ode_advance: after a step, a dof is still when |y_j - y_j(previous step)| <=
 * ss_atol + ss_rtol |y_j| for every state component j; after `window` consecutive still steps it is steady and frozen. */
typedef struct knpemi_ode_ss {
  double ss_rtol, ss_atol;
  int32_t window;
} knpemi_ode_ss;
/* n_steps successive MembraneModel.step_lsoda(dt) calls (odeSolver.py:92-127, i.e. n_steps knpemi_ode_step launches
 * with flags = 0 over [t, t + dt], t <- t + dt from t0), bit for bit, with the LSODA state kept in registers from one
 * step to the next; the reference's calibration tool makes exactly this loop.  The run is split into launches of a
 * bounded length (the first one is timed and sizes the rest; KNPEMI_ODE_ADVANCE_CHUNK=n in the environment forces n
 * steps per launch).  Works on PDE handles too; the tables are current on the device afterwards (knpemi_ode_get_tables),
 * phi_M / I_ch of a PDE handle are not written.  The stimulus of knpemi_ode_set_stimulus is applied at every step.
 *   rec_idx[n_rec] (n_rec <= 8): state components recorded after every `every`-th step into the host buffer
 *     history[n_steps / every][n_rec][nq] (history may be NULL: nothing recorded);
 *   ss: steady-state mode, or NULL for a plain run.  steps_taken[q] = the number of steps after which dof q became
 *     steady, -1 if it did not; frozen dofs keep their state, later records repeat it;
 *   failed_step[q]: the step on which LSODA failed for dof q (the dof is frozen at its last good state), -1 if none.
 *     Any failure returns KNPEMI_EODE (`assert success`, odeSolver.py:121) after every output is written.
 * steps_taken / failed_step are int32[nq] or NULL.  RHS evaluations, internal steps and failures are added to the
 * counters knpemi_ode_stats reads. */
int knpemi_ode_advance(knpemi_handle* h, int sub, int model, double t0, double dt, int n_steps, double rtol, double atol,
                       const int32_t* rec_idx, int n_rec, int every, double* history, const knpemi_ode_ss* ss,
                       int32_t* steps_taken, int32_t* failed_step);
/* The integrator of a membrane model slot: LSODA (default), or a fixed-step scheme with n_substeps equal sub-steps
 * per knpemi_ode_step / knpemi_ode_advance interval -- forward Euler, classical RK4, first-order Rush-Larsen (gates by
 * their exponential update, everything else by Euler).  This is the family the reference's drivers still carry a knob
 * for: `n_steps_ODE = 25` in physical_parameters (examples/idealized_geometries/run_2D.py:176,205, run_3D.py:178,207),
 * the sub-step count of its former splitting solver, which nothing reads since the move to LSODA.
 * State of the slot; knpemi_ode_step and knpemi_ode_advance dispatch on it and ignore rtol / atol for a fixed-step
 * method.  n_substeps in 1..10000 (ignored for KNPEMI_ODE_LSODA), anything else KNPEMI_EINVAL.  Works on PDE handles
 * and on handles of knpemi_ode_create.  A model bound from source (knpemi_ode_bind_source) brings a right-hand side only,
 * no gate rates: KNPEMI_ODE_RUSH_LARSEN on it is KNPEMI_EINVAL.
 * Currents: a fixed-step method evaluates the right-hand side once more at (t0 + dt, y(t0 + dt)) and hands out those
 * currents (LSODA: those of its last internal evaluation).  A dof whose state is not finite after the interval counts
 * as failed in knpemi_ode_stats / knpemi_ode_advance exactly as an LSODA failure does. */
#define KNPEMI_ODE_LSODA 0
#define KNPEMI_ODE_EULER 1
#define KNPEMI_ODE_RK4 2
#define KNPEMI_ODE_RUSH_LARSEN 3
int knpemi_ode_set_method(knpemi_handle* h, int sub, int model, int method, int n_substeps);
int knpemi_ode_get_method(knpemi_handle* h, int sub, int model, int* method, int* n_substeps);
/* Diagnostics (no reference counterpart): the steps per launch the last knpemi_ode_advance of this model chose. */
int knpemi_ode_advance_chunk(knpemi_handle* h, int sub, int model);

/* Diagnostics (no reference counterpart): with KNPEMI_ODE_STAMPS=1 in the environment the sweep runs a stamped build of
 * the kernel; per workgroup 12 cycle sums (loop head, TOP, PRED, RHS, CORR, ERR up to the order selection, prologue, -,
 * order selection, new coefficients + rescaling, rest of ERR, -) and 12 counts.  Returns
 * the number of workgroups copied (<= max_blocks). */
int knpemi_debug_ode_stamps(knpemi_handle* h, int sub, int model, uint64_t* out, int max_blocks);

/* Diagnostics (no reference counterpart): evaluates one of the ODE sweep's device math helpers (csrc/lsoda_core.h) over
 * host arrays on the current device, so that tests can bound their error against the C library: op 0: kn_div(a, b),
 * 1: kn_exp(a), 2: kn_powr(a, b), 3: kn_log(a).  a, b, out: n doubles each (b is ignored by ops 1 and 3). */
int knpemi_debug_math(int op, int n, const double* a, const double* b, double* out);

/* Diagnostics (no reference counterpart): runs ONE kernel of the device solves (csrc/kernels_krylov.hip, csrc/block_spmv.h,
 * the device half of csrc/kernels_amg.hip) on host arrays, on the current device and the default stream, without a
 * handle: upload, launch through the launch helper the solves themselves call (so grid, lanes per row and kernel choice
 * are the solver's), check, copy back, free.  Tests hold each kernel to a plain reference of the same operation this way.
 *
 * buf[s]: host array of slot s (NULL: the kernel gets a null pointer where the slot is optional "?"), bytes[s] its size,
 * out[s] != 0: copied back after the launch.  Every given array is uploaded first, so in/out arrays keep what the kernel
 * leaves alone.  Index arrays (row pointers, columns, block columns, node lists) are checked against the sizes of the
 * arrays they index before anything is launched.  n: rows / entries (> 0).  Slots (i = int32, d = double, u = uint8):
 *  SPMV          ip: lanes per row (4, 16), columns.  0 rowptr i, 1 colind i, 2 vals d, 3 x d, 4 dinv? d, 5 b? d,
 *                6 owned? u, 7 y d, 8 dinv_out? d
 *  BLOCK_SPMV    n = rows; ip: NV, nbmax, unknowns of one system, kernel (-1: the process default, 0: row-wise, 1: cell-wise
 *                where it is built).  0 rowptr i, 1 bcol i, 2 vals d, 3 x d, 4 b? d, 5 owned? u, 6 y d
 *  DOTS          ip: nd, op (0 STORE3, 1 CG_INIT, 2 CG_PAP, 3 CG_RHO, 4 BI_RHO, 5 BI_ALPHA, 6 BI_OMEGA, 7 MEAN, 8 START),
 *                d0, d1, d2, through red (0 / 1); dp: scale.  0..5 a0 b0 a1? b1? a2? b2? d, 6 sc d [16], 7 red? d [3].
 *                The partial sums and the ticket live in one process-wide buffer that is kept between calls.
 *  VEC           ip: op (0 RESID, 1 SHIFT, 2 CG_XR, 3 CG_P, 4 JACOBI, 5 BI_P, 6 BI_S, 7 COPY, 8 COPY_SHIFT).  0 sc d [16],
 *                1 a d, 2 b? d, 3 c? d, 4 d? d
 *  BICG_UPDATE   0 sc, 1 x, 2 r, 3 p, 4 s, 5 sres, 6 t, 7 dinv? (all d)
 *  BICG_INIT     0 p d, 1 v d, 2 sc d [16]
 *  MASK          ip: as_ones.  0 owned u, 1 a d
 *  GHOST_IDENTITY 0 rowptr i, 1 colind i, 2 owned u, 3 vals d
 *  DIAG_INV      0 rowptr i, 1 colind i, 2 vals d, 3 dinv d
 *  SCATTER_SHIFT ip: stride.  0 src d, 1 dst d [n * stride], 2 sc d [16]
 *  EXTRAPOLATE   ip: stride, have.  0 cur d [n * stride], 1 old d, 2 old2? d
 *  KNP_ORDER     n = vertices of all sub-domains; ip: ks, n_sub, to_blocks, voff[0 .. n_sub].  0 x d [ks n], 1 csol d [ks n]
 *  COARSE_RESTRICT n = length of r; ip: nl, rank, world.  0 r d, 1 agg_ptr i [nl + 1], 2 agg_idx i, 3 agg_wt d,
 *                4 red d [8 + world nl]
 *  COARSE_SOLVE  n = nl; ip: rank, nc.  0 inv d [nc nc], 1 red d [8 + nc], 2 zc d
 *  COARSE_PROLONG ip: mode, pick, length of zc.  0 agg_of i, 1 agg_w d, 2 zc? d, 3 z d
 *  AMG_SPMV      ip: mode (0 AX, 1 PRE, 2 ADD, 3 JAC, 4 RES), avg_row (picks 4 / 16 / 64 lanes), columns; dp: w.
 *                0 rowptr i, 1 colind i, 2 vals d, 3 x? d, 4 r? d, 5 dinv? d, 6 y d, 7 xout? d
 *  AMG_BLOCK_INV n = cells; ip: block size (3, 4, 8), nbmax, cells per system.  0 rowptr i, 1 colind i, 2 vals d,
 *                3 bcol? i, 4 binv d
 *  AMG_BLOCK_APPLY ip: block size; dp: w.  0 binv d, 1 v d, 2 x? d, 3 y d
 *  AMG_DENSE     ip: nb, start[8], size[8], off[8].  0 Minv d, 1 r d, 2 x d
 * KNPEMI_EINVAL (the message names the argument) for a null or short required array, n <= 0, an index out of range, or
 * a lane count or block size that is not built; KNPEMI_EHIP without a device. */
#define KNPEMI_LINALG_SPMV 0
#define KNPEMI_LINALG_BLOCK_SPMV 1
#define KNPEMI_LINALG_DOTS 2
#define KNPEMI_LINALG_VEC 3
#define KNPEMI_LINALG_BICG_UPDATE 4
#define KNPEMI_LINALG_BICG_INIT 5
#define KNPEMI_LINALG_MASK 6
#define KNPEMI_LINALG_GHOST_IDENTITY 7
#define KNPEMI_LINALG_DIAG_INV 8
#define KNPEMI_LINALG_SCATTER_SHIFT 9
#define KNPEMI_LINALG_EXTRAPOLATE 10
#define KNPEMI_LINALG_KNP_ORDER 11
#define KNPEMI_LINALG_COARSE_RESTRICT 12
#define KNPEMI_LINALG_COARSE_SOLVE 13
#define KNPEMI_LINALG_COARSE_PROLONG 14
#define KNPEMI_LINALG_AMG_SPMV 20
#define KNPEMI_LINALG_AMG_BLOCK_INV 21
#define KNPEMI_LINALG_AMG_BLOCK_APPLY 22
#define KNPEMI_LINALG_AMG_DENSE 23
#define KNPEMI_LINALG_MAX_BUF 10
typedef struct knpemi_debug_linalg_args {
  int32_t n;
  int32_t ip[28];
  double dp[2];
  void* buf[KNPEMI_LINALG_MAX_BUF];
  uint64_t bytes[KNPEMI_LINALG_MAX_BUF];
  int32_t out[KNPEMI_LINALG_MAX_BUF];
} knpemi_debug_linalg_args;
int knpemi_debug_linalg(int op, const knpemi_debug_linalg_args* args);

/* Diagnostics (no reference counterpart): `links` dependent trivial kernels on the handle's stream, `reps` times, launched
 * one by one or replayed from a captured hipGraph; *us_per_kernel = host wall time per kernel.  kind 0: an empty one-wave
 * kernel, 1: y = x + 1 over n doubles, 2: the one-block start kernel of the fused Krylov loops.  What a dependent launch
 * costs inside THIS process and on THIS stream, next to tools/probes/kernel_chain.hip which measures a bare process. */
int knpemi_debug_launch_chain(knpemi_handle* h, int kind, int n, int links, int reps, int use_graph, double* us_per_kernel);

/* Diagnostics (no reference counterpart): which geometry specialisations knpemi_create selected for the row kernels.
 * *flags: bit 0 = lattice tetrahedra of a uniform grid (shape table, no coordinates staged), bit 1 = hexahedra that are all
 * parallelepipeds or quadrilaterals that are all parallelograms (closed-form rows; KNPEMI_HEX_GENERAL=1 /
 * KNPEMI_QUAD_GENERAL=1 force the quadrature kernels), bit 2 = ... and all the same box (uniform hexahedral kernels; never
 * set for quadrilaterals). */
int knpemi_debug_geometry(knpemi_handle* h, int* flags);

/* Diagnostics (no reference counterpart): the sizes of the row-kernel layout knpemi_create built, so that a test can tell
 * which code a mesh reaches.  Fills out[0 .. min(n, 9)): 8 = row blocks (workgroups of a row kernel), 0 = longest row of the EMI pattern (membrane coupling included),
 * 1 = lanes per row, 2 = most (row, cell) pairs on one lane (more than 8: the loop after the prefetched pairs runs),
 * 3 = most distinct vertices of one row block (more than 768: the staging loop for oversized blocks runs), 4 = most
 * membrane entries on one row, 5 / 6 = dynamic LDS bytes of the latest EMI / KNP row launch (0 before the first),
 * 7 = longest row of the Laplacian pattern (the one the 8-bit pair slots index; more than 31 excludes the lattice path). */
int knpemi_debug_layout(knpemi_handle* h, int* out, int n);

/* End-of-step update: update_pde_variables (utils.py:238-295): c_prev <- c, eliminated ion from
 * electroneutrality, phi_M_prev <- tr(phi_i) - tr(phi_e). */
int knpemi_update_pde(knpemi_handle* h);

/* Observables: linear functionals and min/max reductions of the nodal fields, recorded on the device into a
 * time-series buffer (knpemi.observables).  The reference evaluates fields at points of a checkpoint of every step
 * (scifem.evaluate_function, examples/idealized_geometries/make_figures.py:24-117) and takes means / maxima of the
 * downloaded arrays (local_astrocyte_depolarization/run_stim_duration.py:239-246).
 * Observable o reads the field spec[4o + 0] of sub-domain spec[4o + 1], index spec[4o + 2] (the ids of
 * knpemi_set_field) and applies op spec[4o + 3] to the entries ptr[o] .. ptr[o + 1] - 1 of (idx, w):
 *   KNPEMI_OBS_SUM: (sum_e w[e] u[idx[e]]) / denom[o]   (points, integrals, means),
 *   KNPEMI_OBS_MIN / KNPEMI_OBS_MAX: min / max_e u[idx[e]]   (w and denom unused).
 * capacity: rows of n_obs doubles the device buffer holds.  Replaces any previous table and clears the buffer. */
#define KNPEMI_OBS_SUM 0
#define KNPEMI_OBS_MIN 1
#define KNPEMI_OBS_MAX 2
int knpemi_observe_set(knpemi_handle* h, int n_obs, const int32_t* spec, const int64_t* ptr, const int32_t* idx,
                       const double* w, const double* denom, int capacity);
/* Enqueue the evaluation of every observable as one row on the main stream (after the end-of-step update:
 * knpemi_update_pde, or the fused write-back of knpemi_solve_knp).  The row index is a counter in device memory that
 * the launch advances; a full buffer writes nothing and counts the overflow.  Sums are formed in a fixed order: two
 * identical runs give bit-identical rows.  Nothing is synchronised. */
int knpemi_observe_record(knpemi_handle* h);
/* Synchronise and copy out min(n_rows, device row count) rows (out: [n_rows][n_obs], may be NULL when n_rows is 0),
 * the device row count and the overflow count; reset != 0 empties the buffer afterwards (the reference's host loop
 * keeps its time series in Python lists: make_figures.py:24-117). */
int knpemi_observe_read(knpemi_handle* h, int n_rows, double* out, int64_t* rows, int64_t* overflow, int reset);
/* Drop the table and the buffer (knpemi_observe_record then fails with KNPEMI_EINVAL). */
int knpemi_observe_clear(knpemi_handle* h);
/* The same table on one rank of a cell-partitioned run (knpemi.observables, DeviceStepper.observe(halo=...)): every rank
 * passes the same observables in the same order, with the entries of what it counts -- the points it took, the integral
 * weights of the cells it records, its owned vertices -- and the GLOBAL denominators.  An observable may have no entries
 * here (ptr[o + 1] == ptr[o]), and a rank may have none at all.  xbuf_dev: the caller's device buffer of world * n_obs
 * doubles (zeroed here).  knpemi_observe_record then enqueues on the main stream:
 *   1. the partial pass: this rank's fold of every observable, without the denominator, into xbuf[rank * n_obs + o]
 *      (the op's identity without entries);
 *   2. the sum of the first world * n_obs doubles of xbuf over the ranks: allreduce(ctx, world * n_obs) when given,
 *      else knpemi_comm_allreduce on the handle's communicator (knpemi_comm_init; required then).  Every slot has one
 *      non-zero contributor, so the sum is an exact all-gather;
 *   3. record_combine_kernel: the slots folded in rank order, sums divided by denom, the row appended as above, the
 *      other ranks' slots zeroed for the next record.
 * Every rank appends the same row; knpemi_observe_read stays rank-local.  Points, minima and maxima equal those of one
 * rank holding the whole mesh bit for bit; sums agree to rounding (a different order of summation). */
int knpemi_observe_set_partitioned(knpemi_handle* h, int n_obs, const int32_t* spec, const int64_t* ptr,
                                   const int32_t* idx, const double* w, const double* denom, int capacity, int rank,
                                   int world, void* xbuf_dev, int (*allreduce)(void* ctx, int n), void* ctx);

/* Membrane events: per membrane dof, when phi_M crossed a threshold upwards, how often, and its running peak
 * (knpemi.events).  The reference has no such output: its users checkpoint phi_M at every step
 * (examples/idealized_geometries/run_3D.py:57-60, 376) and post-process the checkpoints on the host (make_figures.py:
 * 67-89 reads one point of each back); an activation map, a spike count per dof or a conduction velocity needs every one
 * of those arrays.  Here every membrane dof of a watched cell keeps on the device
 *   v_prev (the sample of the previous record), armed (u8: a crossing may be counted), count (i32: upward crossings),
 *   t_first / t_last (time of the first / latest crossing, NaN while count == 0), v_peak / t_peak (largest sample and
 *   the time of its first occurrence), ring[keep] (the latest `keep` crossing times: crossing n, 1-based, in slot
 *   (n - 1) % keep, NaN where unused).
 * knpemi_events_set watches the n_watch cell sub-domains sub[w] (1 <= sub[w] < n_sub, each at most once) with
 * threshold[w] and reset[w] <= threshold[w] (reset == NULL: the thresholds) and ring length 0 <= keep <=
 * KNPEMI_EVENTS_MAX_KEEP; anything else is KNPEMI_EINVAL.  Replaces any previous table and clears all state.  `keep`
 * bounds only how many crossing TIMES a dof remembers; count, t_first and t_last are exact however often it fires.
 * Works on handles of knpemi_ode_create too (sub = 1 + i): the samples are then the handle's phi_M write-back buffer,
 * which knpemi_ode_step fills.  knpemi_ode_advance does not write phi_M, so nothing is recorded during it. */
#define KNPEMI_EVENTS_MAX_KEEP 64
int knpemi_events_set(knpemi_handle* h, int n_watch, const int32_t* sub, const double* threshold, const double* reset,
                      int keep);
/* Enqueue one record at time t on the main stream (after the end-of-step update as knpemi_observe_record, or after
 * knpemi_ode_step on the main stream): one launch over the dofs of every watched sub-domain, nothing synchronised.  This
 * replaces the reference's per-step checkpoint of phi_M (run_3D.py:376) as the input of firing statistics.
 * With sample v = phi_M[q] and t_prev the time of the previous record:
 *   first record after the set-up or a reset: v_prev <- v, armed <- (v < threshold), v_peak <- v, t_peak <- t;
 *   later records, in this order (a non-finite v only replaces v_prev):
 *     1. !armed && v < reset: armed <- 1;
 *     2. armed && v >= threshold: t_c = t_prev + (t - t_prev) * ((threshold - v_prev) / (v - v_prev)); count += 1,
 *        t_last <- t_c, t_first <- t_c at the first crossing, ring slot written, armed <- 0;
 *     3. v > v_peak: v_peak <- v, t_peak <- t;
 *     4. v_prev <- v.
 * KNPEMI_EINVAL before knpemi_events_set, and when t is not finite or not greater than the previous record's t. */
int knpemi_events_record(knpemi_handle* h, double t);
/* Synchronise and copy out the maps of watched sub-domain `sub`: n_q[sub] entries each, ring as [keep][n_q[sub]] in slot
 * order; every pointer may be NULL.  This is what the reference's users compute from the downloaded checkpoints of all
 * steps.  KNPEMI_EINVAL before knpemi_events_set and for a sub-domain that is not watched. */
int knpemi_events_read(knpemi_handle* h, int sub, int32_t* count, double* t_first, double* t_last, double* v_peak,
                       double* t_peak, double* ring);
/* All state back to "before the first record" (a second run from the same start; the reference would delete its
 * checkpoint files); the table stays.  Enqueue only. */
int knpemi_events_reset(knpemi_handle* h);
/* Drop the table and the state buffers (knpemi_events_record then fails with KNPEMI_EINVAL); knpemi_destroy does the
 * same. */
int knpemi_events_clear(knpemi_handle* h);

/* Ion fluxes and current density per cell (knpemi.fluxes).  The reference writes these quantities in its
 * manufactured-solution scripts (tests/run_mms.py:270-301: J_k = -D_k grad c_k - z_k D_k psi c_k grad phi, total flux
 * F sum_k z_k J_k); its drivers have no such output, a user differentiates downloaded checkpoints on the host.
 * Definitions, for a cell T of sub-domain s and every ion k = 0 .. K-1, the eliminated one included:
 *   c_k, g(u): value and gradient, at the cell's centroid, of the P1 / Q1 interpolant of the nodal field.  Simplices: the
 *     mean of the vertex values and the constant gradient.  Hexahedra (tensor vertex order, x[1 << t]): the mean of the
 *     eight values; the reference derivative along t is 1/4 sum_v +-u_v with the sign from bit t of v, mapped by the
 *     Jacobian at the centre.
 *   J_diff = -D_k^s g(c_k),  J_drift = -z_k psi D_k^s c_k g(phi),  J = J_diff + J_drift;
 *   current density i = F sum_k z_k J_k, split the same way into i_diff and i_drift;
 *   vol_T = |det| / d! on simplices, |det J(centre)| on hexahedra (midpoint rule); the orientation of a cell does not
 *     matter.
 * The fields are those of the device's vertex records: phi, c_prev of the solved ions and the eliminated ion's c, i.e.
 * the new state once knpemi_update_pde / the fused write-back of knpemi_solve_knp has run.
 * Series row: for every watched sub-domain in the order given, for every selected ion in ascending order
 *   sum_T vol_T J_diff (gdim values), sum_T vol_T J_drift (gdim), max_T |J| (Euclidean norm),
 * then, with the current selected, sum_T vol_T i (gdim) and max_T |i|.  On simplices the sums are the exact integrals of
 * the discrete flux. */
/* Watch the n_watch sub-domains sub[w] (0 <= sub[w] < n_sub, each at most once, the ECS included): bits 0 .. K-1 of
 * ion_mask[w] select the ions, bit 8 the current (run_mms.py:270-301 evaluates all of them).  capacity: rows the device
 * buffer holds.  Replaces any previous table and clears the buffer.  KNPEMI_EINVAL: a bad or repeated sub-domain, one
 * without cells, an empty mask, mask bits at or above K (other than bit 8), capacity < 1. */
int knpemi_flux_set(knpemi_handle* h, int n_watch, const int32_t* sub, const int32_t* ion_mask, int capacity);
/* Enqueue one record on the main stream (after the end-of-step update, as knpemi_observe_record): ONE launch over the
 * cells of every watched sub-domain appends the series row (run_mms.py:270-301 for the integrand) and, with
 * write_fields != 0, writes the per-cell vectors (buffers allocated at the first such record).  The row index is a
 * counter in device memory that the launch advances; a full buffer writes nothing and counts the overflow.  Sums are
 * formed in a fixed order: two identical runs give bit-identical rows, and the row does not depend on write_fields.
 * KNPEMI_EINVAL before knpemi_flux_set and before knpemi_set_params. */
int knpemi_flux_record(knpemi_handle* h, int write_fields);
/* Synchronise and copy out min(n_rows, device row count) rows of the series (run_mms.py:270-301 per row), the device row
 * count and the overflow count; reset != 0 empties the buffer afterwards. */
int knpemi_flux_read(knpemi_handle* h, int n_rows, double* out, int64_t* rows, int64_t* overflow, int reset);
/* Synchronise and copy out one per-cell field of the last record made with fields (run_mms.py:270-301: J_k, or the
 * total flux for ion == -1): part 0 = diffusive, 1 = drift, as [gdim][n_cell[sub]] (component-major, the device layout);
 * n = gdim * n_cell[sub].  KNPEMI_EINVAL for a sub-domain, ion or current that is not watched, a bad part or length,
 * and before any record with fields. */
int knpemi_flux_fields(knpemi_handle* h, int sub, int ion, int part, double* host, size_t n);
/* A new series (run_mms.py:270-301 has none: it evaluates once): the buffer is emptied and the per-cell fields count as
 * not yet recorded; the table stays.  Enqueue only. */
int knpemi_flux_reset(knpemi_handle* h);
/* Drop the table and the buffers (knpemi_flux_record then fails with KNPEMI_EINVAL; the quantities of
 * run_mms.py:270-301 are no longer evaluated); knpemi_destroy does the same. */
int knpemi_flux_clear(knpemi_handle* h);
/* knpemi_flux_set on one rank of a cell-partitioned run (knpemi.fluxes, DeviceStepper.fluxes(halo=...); the integrand is
 * that of run_mms.py:270-301).  Every rank passes the same watches and capacity.  recorded: one byte per local cell, the
 * cells of sub[0] first, then those of sub[1], ...: 1 = this rank records the cell (every cell of the global mesh is
 * recorded by exactly one rank; the others hold it in their ghost layer, with valid records after the bulk halo).  A
 * watched sub-domain may have no local cell.  rank, world, xbuf_dev (world * n_cols doubles, zeroed here), allreduce and
 * ctx as in knpemi_observe_set_partitioned.  knpemi_flux_record then enqueues on the main stream
 *   1. the record launch: the per-cell vectors of EVERY local cell with write_fields, and this rank's sums and maxima
 *      over its recorded cells, folded in workgroup order, into xbuf[rank * n_cols + q] (zeros without local cells);
 *   2. the sum of xbuf over the ranks: allreduce(ctx, world * n_cols) when given, else knpemi_comm_allreduce on the
 *      handle's communicator (required then).  Every slot has one non-zero contributor: an exact all-gather;
 *   3. record_combine_kernel: the slots of every column folded in rank order -- sums summed, maxima maximised from 0 --
 *      the row appended or counted as dropped, the other ranks' slots zeroed for the next record.
 * Every rank appends the same row, and repeated runs the same bits.  Maxima equal those of one rank holding the whole
 * mesh bit for bit; sums agree to rounding (a different order of summation).  knpemi_flux_read, _fields (the local
 * cells), _reset and _clear are unchanged.  KNPEMI_EINVAL as knpemi_flux_set, and for a NULL mask or buffer, a bad rank
 * or world, and no hook with no communicator; a refused call leaves the previous table alone. */
int
knpemi_flux_set_partitioned(knpemi_handle* h, int n_watch, const int32_t* sub, const int32_t* ion_mask, int capacity,
                            const uint8_t* recorded, int rank, int world, void* xbuf_dev,
                            int (*allreduce)(void* ctx, int n), void* ctx);

/* Membrane ion exchange per cell (knpemi.exchange): what crosses the membranes.  The membrane term of the reference's KNP
 * right-hand side (knpWeakForm.py:168-214) is minus the transmembrane molar flux of each ion, tested against the facet
 * functions; the reference integrates it into b and keeps nothing else of it.  Definitions, at a point of a membrane facet
 * of cell sub-domain s, on side e (ECS) or i (cell), for every ion k = 0 .. K-1, the eliminated one included:
 *   j_k^side = (I_ch,k + alpha_k^side (I_cap - S I_ch,tot)) / (F z_k)   [mol / (m^2 s)], positive out of the cell;
 *   I_cap = C_M (phi_M - phi_M_prev) / dt with phi_M = phi_i - phi_e of the potential the device holds;
 *   alpha_k^side = D_k z_k^2 c_k / sum_j D_j z_j^2 c_j with D and c (c_prev, the eliminated ion's c) of that side;
 *   I_ch,tot = sum_j I_ch,j; S = 1 with the splitting scheme, 0 without (the flags of the last knpemi_assemble_knp;
 *   splitting before the first).
 * Integrals use the degree-6 facet rule of the assembly; a facet without a membrane model contributes nothing.  The sum of
 * block (s, k) of the membrane part of b_knp is -int j_k^i dS, that of block (0, k) +sum_cells int j_k^e dS.
 * Series row: for every watched cell in the order given, for every selected ion in ascending order
 *   int j_k^e dS, int j_k^i dS [mol/s], int I_ch,k dS [A],
 * then, with the current columns selected, int I_cap dS, int I_ch,tot dS [A] and the membrane area. */
/* Watch the n_watch cell sub-domains sub[w] (1 <= sub[w] < n_sub, each at most once): bits 0 .. K-1 of ion_mask[w]
 * select the ions, bit 8 the current columns (knpWeakForm.py:168-214 holds all of them).  capacity: rows the device buffer
 * holds.  Replaces any previous table and clears the buffer; a refused call leaves the table alone.  KNPEMI_EINVAL: the
 * ECS (sub-domain 0), an unknown or repeated cell, one without membrane facets, an empty mask, mask bits at or above K
 * (other than bit 8), capacity < 1. */
int knpemi_exchange_set(knpemi_handle* h, int n_watch, const int32_t* sub, const int32_t* ion_mask, int capacity);
/* Enqueue one record on the main stream: ONE launch over the membrane facets of every watched cell, both sides, appends
 * the series row (knpWeakForm.py:168-214 for the integrand) and, with write_fields != 0, writes the per-facet means
 * (buffers allocated at the first such record).  It reads what the membrane part of knpemi_assemble_knp reads; in a time
 * step it belongs directly behind that call and before the KNP solve, the only moment the device holds the new potential,
 * the old c_prev, the post-ODE phi_M_prev and the new I_ch together.  The row index is a counter in device memory that the
 * launch advances; a full buffer writes nothing and counts the overflow.  Sums are formed in a fixed order: two identical
 * runs give bit-identical rows, and the row does not depend on write_fields.  KNPEMI_EINVAL before knpemi_exchange_set
 * and before knpemi_set_params. */
int knpemi_exchange_record(knpemi_handle* h, int write_fields);
/* Synchronise and copy out min(n_rows, device row count) rows of the series (knpWeakForm.py:168-214 per row), the device
 * row count and the overflow count; reset != 0 empties the buffer afterwards. */
int knpemi_exchange_read(knpemi_handle* h, int n_rows, double* out, int64_t* rows, int64_t* overflow, int reset);
/* Synchronise and copy out one per-facet field of the last record made with fields (knpWeakForm.py:168-214: the
 * integrand's mean over the facet, integral / area): for ion >= 0 part 0 = j^e, 1 = j^i, 2 = I_ch,ion; for ion == -1
 * part 0 = I_cap, 1 = the facet's area.  n = n_facet[sub]; facets in the order of the problem description.  A facet
 * without a membrane model holds zeros, its area included.  KNPEMI_EINVAL for a cell, ion or current that is not watched,
 * a bad part or length, and before any record with fields. */
int knpemi_exchange_fields(knpemi_handle* h, int sub, int ion, int part, double* host, size_t n);
/* A new series (knpWeakForm.py:168-214 keeps none): the buffer is emptied and the per-facet fields count as not yet
 * recorded; the table stays.  Enqueue only. */
int knpemi_exchange_reset(knpemi_handle* h);
/* Drop the table and the buffers (knpemi_exchange_record then fails with KNPEMI_EINVAL; the fluxes of
 * knpWeakForm.py:168-214 are no longer kept); knpemi_destroy does the same. */
int knpemi_exchange_clear(knpemi_handle* h);
/* knpemi_exchange_set on one rank of a cell-partitioned run (knpemi.exchange, DeviceStepper.exchange(halo=...); the
 * integrand is that of knpWeakForm.py:168-214).  Every rank passes the same watches and capacity.  recorded: one byte per
 * local membrane facet, the facets of sub[0] first, then those of sub[1], ...: 1 = this rank records the facet (every
 * facet of the global membrane is recorded by exactly one rank; the ghost layer's facets have valid inputs after the bulk
 * halo and their membrane dofs are integrated redundantly).  A watched cell may have no local facet.  The other arguments
 * and the three stages of knpemi_exchange_record -- record launch into xbuf[rank * n_cols + q] with the per-facet means
 * of EVERY local facet, sum over the ranks, record_combine_kernel -- are those of knpemi_flux_set_partitioned; every
 * column is a sum.  Every rank appends the same row; knpemi_exchange_read, _fields (the local facets), _reset and _clear
 * are unchanged.  KNPEMI_EINVAL as knpemi_exchange_set, and for a NULL mask or buffer, a bad rank or world, and no hook
 * with no communicator; a refused call leaves the previous table alone. */
int
knpemi_exchange_set_partitioned(knpemi_handle* h, int n_watch, const int32_t* sub, const int32_t* ion_mask, int capacity,
                                const uint8_t* recorded, int rank, int world, void* xbuf_dev,
                                int (*allreduce)(void* ctx, int n), void* ctx);

/* Field maps: per vertex of a bulk field, or per membrane dof, the running peak, trough, time integral, arrival time,
 * exposure and excess over a level, kept on the device over a whole run (knpemi.maps).  The reference's astrocyte study
 * normalises the glial membrane potential in space by its maximum and minimum over the run
 * (examples/local_astrocyte_depolarization/results/compare_1D_3D.py:89-105, compare_tort.py:114-130,
 * make_figures.py:336-352) and plots ECS concentrations in space at chosen times (make_figures.py:135); its users get
 * such maps by checkpointing every field at every step and post-processing on the host.
 * A watch is a field -- KNPEMI_F_PHI, KNPEMI_F_C (idx: a solved ion), KNPEMI_F_C_ELIM or KNPEMI_F_PHI_M -- of sub-domain
 * `sub`, an optional threshold thr, a direction s = +1 ("beyond" = at or above) or -1 (KNPEMI_MAPS_BELOW: at or below)
 * and a selection of the statistics KNPEMI_MAPS_PEAK, _TROUGH, _INTEGRAL, _THRESHOLD.  Its items are the vertices of
 * the sub-domain, or the membrane dofs of cell `sub` for phi_M.
 * State per item after the set-up or a reset: v_prev, v_max, t_max, v_min, t_min, t_arrival are NaN; integral, exposure,
 * excess and count (int32) are 0.
 * One record at time t (previous record's time t_prev, D = t - t_prev) with sample v, for each item, in this order:
 *   v not finite: v_prev <- v.  Nothing else changes.
 *   v_prev not finite (the first record, or the record after a non-finite sample): no interval is accounted for; peak
 *     and trough are updated as in step 3; with the threshold statistic and s (v - thr) >= 0: count += 1, and
 *     t_arrival <- t when count == 1 (a field already beyond the level counts as arrived at the first sight of it);
 *     v_prev <- v.
 *   otherwise, with a = s (v_prev - thr) and b = s (v - thr):
 *     1. integral:  integral += 0.5 D (v_prev + v)   (trapezoid);
 *     2. threshold, with theta = a / (a - b) where used:
 *          onset (a < 0 <= b): t_c = t_prev + D theta; count += 1; t_arrival <- t_c when count == 1;
 *            exposure += (1 - theta) D; excess += 0.5 (1 - theta) D b;
 *          stays beyond (a >= 0 && b >= 0): exposure += D; excess += 0.5 D (a + b);
 *          offset (a >= 0 > b): exposure += theta D; excess += 0.5 theta D a;
 *     3. peak and trough: !(v <= v_max) -> v_max <- v, t_max <- t.  !(v >= v_min) -> v_min <- v, t_min <- t (strict
 *        improvement, or the first value);
 *     4. v_prev <- v.
 * A statistic that is not selected keeps its initial value, has no array and costs no memory traffic.
 * Series: every watch with KNPEMI_MAPS_SERIES (needs KNPEMI_MAPS_THRESHOLD) contributes two columns per record, in watch
 * order: the sum of the item weights over the items with s (v - thr) >= 0 (the measure of the region beyond the level)
 * and the number of such items (a double, exact). */
#define KNPEMI_MAPS_MAX_WATCH 32
#define KNPEMI_MAPS_MAX_PER_SPACE 8
#define KNPEMI_MAPS_PEAK 1
#define KNPEMI_MAPS_TROUGH 2
#define KNPEMI_MAPS_INTEGRAL 4
#define KNPEMI_MAPS_THRESHOLD 8
#define KNPEMI_MAPS_SERIES 16
#define KNPEMI_MAPS_BELOW 32
#define KNPEMI_MAP_V_MAX 0
#define KNPEMI_MAP_T_MAX 1
#define KNPEMI_MAP_V_MIN 2
#define KNPEMI_MAP_T_MIN 3
#define KNPEMI_MAP_INTEGRAL 4
#define KNPEMI_MAP_T_ARRIVAL 5
#define KNPEMI_MAP_EXPOSURE 6
#define KNPEMI_MAP_EXCESS 7
#define KNPEMI_MAP_COUNT 8
/* Set the n_watch watches spec[w] = {field, sub, idx, flags} (1 <= n_watch <= KNPEMI_MAPS_MAX_WATCH, at most
 * KNPEMI_MAPS_MAX_PER_SPACE on the vertices of one sub-domain or the membrane of one cell) with the levels threshold[w]
 * (read with KNPEMI_MAPS_THRESHOLD only; may be NULL without one) -- the maps of compare_1D_3D.py:89-105 are peak and
 * trough of phi_M.  weight: the item weights (lumped nodal measures) of the series watches, concatenated in watch order;
 * capacity: rows of the series buffer.  Without a series watch both are ignored and no buffer exists.  Replaces any
 * previous table and puts all state to "before the first record"; a refused call leaves the previous table in place.
 * KNPEMI_EINVAL: null arguments, an unknown field, sub / idx out of range, phi_M on the ECS, a watch listed twice (the
 * same spec and level), no statistic, KNPEMI_MAPS_THRESHOLD with a non-finite level, KNPEMI_MAPS_SERIES or
 * KNPEMI_MAPS_BELOW without KNPEMI_MAPS_THRESHOLD, a series watch with weight == NULL or capacity < 1, too many watches,
 * a handle of knpemi_ode_create. */
int knpemi_maps_set(knpemi_handle* h, int n_watch, const int32_t* spec, const double* threshold, const double* weight,
                    int capacity);
/* Enqueue one record at time t on the main stream (behind the end-of-step update, as knpemi_events_record): ONE launch
 * over the items of every watched space applies the rules above -- this replaces the per-step checkpoints behind
 * make_figures.py:336-352 -- and, with a series watch, appends the series row (a full buffer writes nothing and counts
 * the overflow; sums are formed in a fixed order, two identical runs give identical bits).  KNPEMI_EINVAL before
 * knpemi_maps_set, and when t is not finite or not greater than the previous record's t. */
int knpemi_maps_record(knpemi_handle* h, double t);
/* Synchronise and copy out one map of watch `watch` (its index in knpemi_maps_set): which = KNPEMI_MAP_V_MAX ...
 * KNPEMI_MAP_EXCESS as n doubles, KNPEMI_MAP_COUNT as n int32; n = the number of items of the watch.  These are the
 * arrays compare_tort.py:114-130 takes the maximum and minimum of over all checkpoints.  KNPEMI_EINVAL before
 * knpemi_maps_set, for a bad watch, which or length, and for a statistic that was not selected. */
int knpemi_maps_read(knpemi_handle* h, int watch, int which, void* host, size_t n);
/* Synchronise and copy out min(n_rows, device row count) rows of the series (the region beyond the level over time, read
 * off the frames of make_figures.py:135 in the reference), the device row count and the overflow count; reset != 0
 * empties the buffer afterwards.  KNPEMI_EINVAL before knpemi_maps_set and without a series watch. */
int knpemi_maps_series_read(knpemi_handle* h, int n_rows, double* out, int64_t* rows, int64_t* overflow, int reset);
/* All state back to "before the first record", the series rewound (a second run from the same start; the reference
 * would delete the checkpoints of compare_1D_3D.py:89-105); the table stays.  Enqueue only. */
int knpemi_maps_reset(knpemi_handle* h);
/* Drop the table, the state and the buffer (knpemi_maps_record then fails with KNPEMI_EINVAL; the maps of
 * make_figures.py:336-352 are no longer kept); knpemi_destroy does the same. */
int knpemi_maps_clear(knpemi_handle* h);
/* knpemi_maps_set with at least one series watch on one rank of a cell-partitioned run (knpemi.maps,
 * DeviceStepper.track(halo=...); the curve is the region beyond the level over time of make_figures.py:135).  Every rank
 * passes the same watches, levels and capacity.  weight: as in knpemi_maps_set, but lumped from the cells (membrane
 * facets) this rank records only -- every cell of the global mesh is recorded by exactly one rank -- so the ranks' measures
 * add up to the global one and a rank's weights may all be zero.  owned: one byte per item of every series watch,
 * concatenated as weight: 1 = the rank owns the item and its n column counts it (every item is owned by exactly one rank).
 * rank, world, xbuf_dev (world * n_cols doubles, zeroed here), allreduce and ctx as in knpemi_observe_set_partitioned.  The
 * per-item maps of every watch are kept for EVERY local item as without a partition.  knpemi_maps_record then enqueues the
 * record launch, which writes the rank's (measure, n) columns into xbuf[rank * n_cols + q] (zeros without local items)
 * instead of a row, the sum of xbuf over the ranks, and record_combine_kernel, which sums the slots of every column in rank
 * order and appends the row or counts it as dropped.  Every rank appends the same row; n equals that of one rank holding the
 * whole mesh exactly, the measure to rounding (another order of summation).  knpemi_maps_read, _series_read, _reset and
 * _clear are unchanged.  KNPEMI_EINVAL as knpemi_maps_set, and without a series watch, for a NULL mask or buffer, a bad
 * rank or world, and no hook with no communicator; a refused call leaves the previous table alone. */
int knpemi_maps_set_partitioned(knpemi_handle* h, int n_watch, const int32_t* spec, const double* threshold,
                                const double* weight, int capacity, const uint8_t* owned, int rank, int world, void* xbuf_dev,
                                int (*allreduce)(void* ctx, int n), void* ctx);

/* Membrane monitors: the named intermediates of a membrane model's right-hand side -- Nernst potentials, conductances,
 * the currents split by mechanism, the gates' steady states and time constants -- evaluated per membrane dof from what
 * the device holds (knpemi.monitor; csrc/membrane_monitors.h lists the quantities of the shipped models).  The
 * reference's figure scripts restate the models' formulas and constants by hand and evaluate them from checkpoints of
 * every step (examples/local_astrocyte_depolarization/make_figures.py:169-195, 279-327: E_K, E_Na, E_Cl, i_kir, i_pump at
 * a glial membrane point; examples/idealized_geometries/make_figures.py:146-149: E_Na, E_K;
 * calibrate_initial_conditions/run_calibration.py:148-212: the Kir and pump currents at rest).
 * The state a monitor sees.  On a handle of knpemi_create it is the state the next sweep would start from: the monitor
 * works on a private copy of the dof's parameter row in which the <ion>_e / <ion>_i columns hold the traces of the
 * concentrations the vertex records hold now (as KNPEMI_ODE_SET_TRACES writes them) and on a state in which V is phi_M of
 * the dof (as KNPEMI_ODE_SET_V); the gates come from the state table, every other column, the stimulus columns included,
 * is as the parameter table holds it, and t is the record's time.  On a handle of knpemi_ode_create there are no fields:
 * row and state are as the tables hold them.  Nothing is written to a table, to phi_M, to I_ch or to a vertex record.  A
 * non-finite value is stored as it is and makes the columns it enters non-finite.
 * A watch is one bound model slot (sub, model) with a mask of its quantities (bit i: quantity i of the catalogue).
 * Column kinds of the series row: KNPEMI_MON_POINT, sum_j w_j v(q_j) over the up to 4 dofs of the membrane facet that
 * holds a point; and over the dofs q of the watch with weight w_q > 0 (w_q: the integral of the dof's hat function over
 * the facets that carry the model) KNPEMI_MON_INTEGRAL = sum_q w_q v_q, KNPEMI_MON_AVERAGE = that / sum_q w_q,
 * KNPEMI_MON_MIN and KNPEMI_MON_MAX. */
#define KNPEMI_MON_MAX 32
#define KNPEMI_MON_MAX_WATCH 16
#define KNPEMI_MON_POINT 0
#define KNPEMI_MON_INTEGRAL 1
#define KNPEMI_MON_AVERAGE 2
#define KNPEMI_MON_MIN 3
#define KNPEMI_MON_MAX_OP 4
/* The catalogue of shipped model model_id (KNPEMI_MODEL_*): the number of quantities (0 for an unknown id) and the name
 * of quantity i (NULL out of range) -- the names the files E_K_*.txt ... of make_figures.py:279-327 carry. */
int knpemi_monitor_count(int model_id);
const char* knpemi_monitor_name(int model_id, int i);
/* The monitor of a plug-in model: `__device__ void monitor(double t, const double* states, const double* parameters,
 * double* monitored)` as HIP source, n_monitored (1 .. KNPEMI_MON_MAX) quantities -- what a Gotran-generated module's
 * `monitor` computes and make_figures.py:169-195 restates by hand.  It is compiled with hipRTC as a program of its own,
 * under the record kernel's body (the program of the sweeps is compiled from the same text as before), and from then on
 * slot (sub, model) -- bound with knpemi_ode_bind_source -- can be watched and evaluated like a shipped model, with
 * quantity i = monitored[i]; `states` and `parameters` are the state a monitor sees.  A record launches once per run of
 * consecutive watches that share a program.  knpemi_monitor_compile_source compiles only and needs no device (the compiler's
 * messages go to log, which may be NULL).  KNPEMI_EINVAL: null arguments, a slot that is not bound from source or has a
 * monitor already, sizes out of range, a source that does not compile (knpemi_last_error holds the messages). */
int knpemi_monitor_bind_source(knpemi_handle* h, int sub, int model, int n_monitored, const char* monitor_source);
int knpemi_monitor_compile_source(int n_states, int n_params, int n_monitored, const char* monitor_source, char* log,
                                  size_t log_len);
/* Set the watches spec[w] = {sub, model, mask, v_index} (1 <= n_watch <= KNPEMI_MON_MAX_WATCH; v_index: the state
 * component that is V, -1: none) with ion_param[w][2 k], [2 k + 1] = the parameter columns <ion k>_e, <ion k>_i (read on
 * a handle of knpemi_create; K ions per watch) and the dense dof weights `weights`, concatenated in watch order (n_q of
 * the sub-domain each).  The row has n_cols >= 0 columns col_spec[c] = {kind, watch, quantity, point}; point p (of n_pts)
 * belongs to watch pt_watch[p] and has the dofs pt_q[4 p ..] (local to the sub-domain, -1: unused) with the weights
 * pt_w[4 p ..] -- the glial membrane point of make_figures.py:169-195.  capacity: rows of the series buffer.  Replaces
 * any previous table.  KNPEMI_EINVAL: null arguments, a slot that is unbound or bound from source without a monitor, a mask that is empty or
 * has bits at or beyond the model's count, a sub-domain without membrane dofs, a watch listed twice, a v_index or
 * parameter column out of range, a column with an unknown kind, watch, point or a quantity its watch does not select, a
 * reduction over weights that sum to nothing, a dof out of range; a refused call leaves the previous table alone. */
int knpemi_monitor_set(knpemi_handle* h, int n_watch, const int32_t* spec, const int32_t* ion_param, const double* weights,
                       int n_cols, const int32_t* col_spec, int n_pts, const int32_t* pt_watch, const int32_t* pt_q,
                       const double* pt_w, int capacity);
/* Enqueue one record at time t on the main stream: ONE launch over the dofs of the watched slots evaluates the selected
 * quantities, with fields != 0 writes them per dof, and appends the series row (a full buffer writes nothing and counts
 * the overflow; sums are formed in a fixed order, two identical runs give identical bits) -- this replaces the per-step
 * checkpoints behind make_figures.py:279-327.  KNPEMI_EINVAL before knpemi_monitor_set and for a non-finite t. */
int knpemi_monitor_record(knpemi_handle* h, double t, int fields);
/* Synchronise and copy out min(n_rows, device row count) rows (the time series compare_tort.py plots), the device row
 * count and the overflow count; reset != 0 empties the buffer afterwards. */
int knpemi_monitor_read(knpemi_handle* h, int n_rows, double* out, int64_t* rows, int64_t* overflow, int reset);
/* Synchronise and copy out quantity `quantity` of watch `watch` per dof (n = n_q of its sub-domain) as the latest record
 * with fields wrote it (the spatial profiles of make_figures.py:336-352 for a monitored quantity).  KNPEMI_EINVAL before
 * such a record, for a bad watch, a quantity the watch does not select, or a wrong length. */
int knpemi_monitor_fields(knpemi_handle* h, int watch, int quantity, double* out, size_t n);
/* A new series, stream-ordered; the fields of the old one are forgotten.  The table stays. */
int knpemi_monitor_reset(knpemi_handle* h);
/* Drop the table and the buffers; knpemi_destroy does the same. */
int knpemi_monitor_clear(knpemi_handle* h);
/* knpemi_monitor_set on one rank of a cell-partitioned run (knpemi.monitor, DeviceStepper.monitor(halo=...); the
 * quantities are those of make_figures.py:279-327).  Every rank passes the same watches, columns, points and capacity.
 * weights: the dof weights integrated over the membrane facets this rank records only (every facet of the global
 * membrane is recorded by exactly one rank, which holds all of its dofs with current values: the ghost layer's membrane
 * dofs are integrated redundantly); they may sum to nothing, and a watched slot may have no local dof.  wsum_global[w]: the
 * sum of watch w's weights over the ranks, the same bits on every rank, the divisor of its averages.  A point is taken by
 * one rank; every other rank passes -1 for its four dofs.  rank, world, xbuf_dev (world * n_cols doubles, zeroed here),
 * allreduce and ctx as in knpemi_observe_set_partitioned.  knpemi_monitor_record then enqueues on the main stream
 *   1. the record launch(es): the per-dof values of EVERY local dof with fields, and this rank's columns -- sums and
 *      extrema over its dofs with weight > 0 folded in workgroup order, the averages undivided, a point it does not take 0
 *      -- into xbuf[rank * n_cols + c] (the operations' identities without a local dof);
 *   2. the sum of xbuf over the ranks (allreduce, else knpemi_comm_allreduce): an exact all-gather;
 *   3. record_combine_kernel: the slots of every column folded in rank order -- points, integrals and averages summed from
 *      0, minima and maxima from +-inf, keeping a NaN as the record kernel does -- the averages divided by wsum_global, the
 *      row appended or counted as dropped, the other ranks' slots zeroed for the next record.
 * Every rank appends the same row.  Points, minima and maxima equal those of one rank holding the whole mesh bit for bit;
 * integrals and averages agree to rounding (another order of summation).  knpemi_monitor_read, _fields (the local dofs),
 * _reset and _clear are unchanged.  KNPEMI_EINVAL as knpemi_monitor_set -- but for local weights that sum to nothing, a
 * slot without local dofs and a point without dofs, which are accepted -- and for a NULL wsum_global or buffer, a global
 * weight sum that is negative or not finite, n_cols < 1, a bad rank or world, no hook with no communicator, a handle of
 * knpemi_ode_create; a refused call leaves the previous table alone. */
int knpemi_monitor_set_partitioned(knpemi_handle* h, int n_watch, const int32_t* spec, const int32_t* ion_param,
                                   const double* weights, int n_cols, const int32_t* col_spec, int n_pts,
                                   const int32_t* pt_watch, const int32_t* pt_q, const double* pt_w, int capacity,
                                   const double* wsum_global, int rank, int world, void* xbuf_dev,
                                   int (*allreduce)(void* ctx, int n), void* ctx);
/* Evaluate the quantities in `mask` of slot (sub, model) at time t now: one launch, synchronise, copy out
 * out[bits set][n_q], n = their product (the rest currents of run_calibration.py:148-212).  states / params: host tables
 * [n_q][columns] to evaluate instead of the slot's device tables (both or neither; they are copied to scratch memory,
 * the slot's tables stay as they are).  ion_param ([2 K], as in knpemi_monitor_set) != NULL on a handle of knpemi_create:
 * the traces and phi_M are taken from the fields as in a record; NULL: row and state as the tables hold them.  Works on
 * both kinds of handle. */
int knpemi_monitor_eval(knpemi_handle* h, int sub, int model, double t, uint32_t mask, const double* states,
                        const double* params, const int32_t* ion_param, int v_index, double* out, size_t n);

/* Field snapshots: every watched field packed into ONE contiguous frame on the device, copied to pinned host memory by a
 * stream of its own and handed to the host when the copy is done (knpemi.snapshots).  The reference's astrocyte study
 * writes every field every save_frequency steps (examples/local_astrocyte_depolarization/run_stim_duration.py:52-90,
 * 446-460, 487-494: results_sub_<tag>.xdmf, results_mem_<tag>.xdmf and the ADIOS2 checkpoints); with the fields resident
 * on the device that took one knpemi_get_field per field -- a strided gather and a blocking copy each -- on the stepping
 * thread.  Here the main stream never waits for the host, and no frame is dropped or overwritten.
 * A watch is spec[w] = {field, sub, idx, flags}: KNPEMI_F_PHI, _C, _C_PREV, _C_ELIM, _PHI_M, _I_CH as knpemi_set_field
 * takes them, or KNPEMI_F_ODE_STATE with idx = model * KNPEMI_SNAPSHOT_STATE_STRIDE + state: state component `state`
 * (< KNPEMI_SNAPSHOT_STATE_STRIDE) of the bound model slot (sub, model), as the device's state table holds it.  flags:
 * KNPEMI_SNAPSHOT_F32 stores (float)v, round-to-nearest-even (numpy: np.float32(v)); otherwise the double is stored
 * as it is, bit for bit.  Watches group by space -- the vertices of sub-domain `sub` (phi, c, c_prev, the eliminated
 * ion), or the membrane dofs of cell `sub` (phi_M, I_ch, states).  A space may carry a selection, an ascending list of
 * distinct item indices (the box plotting/plot_roi.py clips to): every watch of the space then stores only those items,
 * in list order.
 * Frame layout: the watches in the order given, watch w at byte offset[w], a multiple of KNPEMI_SNAPSHOT_ALIGN (the 256
 * bytes one wavefront stores of a float watch, so every wavefront's store covers whole 128-byte lines), n_items[w] values
 * of 4 or 8 bytes; the bytes between two watches are not defined.  knpemi_snapshot_layout reports it.
 * Ring: `depth` slots, each a device frame, a pinned host frame and a "copied" event; a slot is FREE or IN FLIGHT. */
#define KNPEMI_F_ODE_STATE 7
#define KNPEMI_SNAPSHOT_MAX_WATCH 64
#define KNPEMI_SNAPSHOT_STATE_STRIDE 256
#define KNPEMI_SNAPSHOT_F32 1
#define KNPEMI_SNAPSHOT_ALIGN 256
#define KNPEMI_EBUSY (-6)    /* knpemi_snapshot_record: the slot is in flight; knpemi_snapshot_take: the copy has not finished */
/* Set the n_watch watches (1 <= n_watch <= KNPEMI_SNAPSHOT_MAX_WATCH) and the n_space_sel >= 0 selections: selection j
 * belongs to space sel_space[j] (sub-domain s: s for its vertices, KNPEMI_MAX_SUB + s for its membrane dofs) and lists
 * sel_idx[sel_off[j] .. sel_off[j + 1]).  depth: slots of the ring.  Creates the copy stream and the events; replaces any
 * previous table (frames in flight are dropped); a refused call leaves the previous table in place -- what replaces the
 * set-up of the writers in run_stim_duration.py:446-460.  KNPEMI_EINVAL: null arguments, an unknown field or flag, sub,
 * idx, model slot or state out of range, a slot that is not bound, phi_M, I_ch or a state on the ECS, a watch listed twice,
 * a selection that is empty, unsorted, repeated or out of range, of a space nothing watches, or the second of one space,
 * depth < 1, too many watches, a handle of knpemi_ode_create. */
int knpemi_snapshot_set(knpemi_handle* h, int n_watch, const int32_t* spec, int n_space_sel, const int32_t* sel_space,
                        const int64_t* sel_off, const int32_t* sel_idx, int depth);
/* offset[w], n_items[w] (n_watch each; either may be NULL) and the frame's size in bytes: what a reader of a frame needs
 * instead of the function-space bookkeeping behind run_stim_duration.py:52-90.  KNPEMI_EINVAL before knpemi_snapshot_set. */
int knpemi_snapshot_layout(knpemi_handle* h, int64_t* offset, int64_t* n_items, int64_t* frame_bytes);
/* Enqueue frame number seq (0, 1, ... since the set-up or the last reset) at time t into slot seq % depth: ONE pack
 * launch on the main stream behind whatever it holds, an event, and behind that event on the copy stream the copy of the
 * frame to pinned host memory and the slot's "copied" event -- the checkpoint write of run_stim_duration.py:487-494
 * without a host synchronisation.  A slot that is IN FLIGHT: nothing is enqueued, nothing changes, KNPEMI_EBUSY.
 * KNPEMI_EINVAL before knpemi_snapshot_set and for a non-finite t. */
int knpemi_snapshot_record(knpemi_handle* h, double t);
/* Hand out the oldest frame IN FLIGHT: wait == 0 polls its "copied" event and returns KNPEMI_EBUSY, touching nothing,
 * while the copy runs; wait != 0 waits for that one event (no stream is synchronised).  Then the pinned frame is copied
 * to out (bytes must be the frame's size), the slot becomes FREE and *t, *seq (may be NULL) are the frame's.  Returns 1
 * -- not an error, nothing written -- with nothing in flight.  This is the read of a checkpoint the reference's figure
 * scripts do (make_figures.py:135). */
int knpemi_snapshot_take(knpemi_handle* h, int wait, void* out, size_t bytes, double* t, int64_t* seq);
/* The number of frames IN FLIGHT (0 before knpemi_snapshot_set): the checkpoints of run_stim_duration.py:487-494 not yet
 * on the host. */
int knpemi_snapshot_pending(knpemi_handle* h);
/* Wait for the copy stream, free every slot and restart seq at 0 (a second run from the same start; the reference would
 * delete the checkpoints of run_stim_duration.py:487-494); the table stays. */
int knpemi_snapshot_reset(knpemi_handle* h);
/* Synchronise both streams and drop the table, the ring, the copy stream and the events (knpemi_snapshot_record then
 * fails with KNPEMI_EINVAL; the writers of run_stim_duration.py:446-460 are closed); knpemi_destroy does the same. */
int knpemi_snapshot_clear(knpemi_handle* h);

/* Options of a handle (device-resident loops).
 * KNPEMI_OPT_FUSE_UPDATE (0/1): update_pde_variables follows problem_knp.solve() directly in the reference's loop
 *   (run_3D.py:356,362); with this option the write-back kernel of knpemi_solve_knp -- and of
 *   knpemi_set_solution(KNPEMI_B_KNP, device pointer) -- also performs that update (same arithmetic, one launch
 *   fewer per step), and the caller does not call knpemi_update_pde.
 * KNPEMI_OPT_FUSE_MEMBRANE (0/1, default 0): 1 evaluates the membrane-facet integrals of b_knp
 *   (knpWeakForm.py:178-214) inside the KNP row kernel -- each row block integrates the (facet, local vertex) entries
 *   of its rows before it sums them, same arithmetic and order as the stand-alone facet kernel, bit-identical b_knp --
 *   instead of in a launch of their own that hands them over through HBM.  Measured on MI355X it does not pay: the
 *   degree-6 facet quadrature lands on the few row blocks that own membrane rows, so the row kernel's tail grows by as
 *   much as (24,794 dofs: 17.0 + 16.3 us apart, 34.2 us fused) or more than (219,542 dofs: 59.3 + 18.7 us apart,
 *   107 us fused) the stand-alone kernel costs spread over all CUs.  Kept as an option for small, launch-bound cases.
 *   It needs row blocks of consecutive rows (the membrane entries of a block are then one range): create the handle
 *   with KNPEMI_BLOCK_CLASSIC=1 in the environment, otherwise the option is refused with KNPEMI_EINVAL. */
#define KNPEMI_OPT_FUSE_UPDATE 1
#define KNPEMI_OPT_FUSE_MEMBRANE 2
/* KNPEMI_OPT_PROFILE_STRIDE (n >= 1, default 1): knpemi_profile brackets every n-th launch of a selected kernel only. */
#define KNPEMI_OPT_PROFILE_STRIDE 3
/* KNPEMI_OPT_KNP_MIN_IT (n >= 0, default 0): knpemi_solve_knp performs at least n iterations before a residual below
 * the target ends it (`ksp_min_it`: 5 in the reference's iterative options of the concentration solve, pdeSolver.py:101;
 * knpemi.pdeSolver.create_solver_knp sets it).  A residual that has vanished exactly still ends the solve. */
#define KNPEMI_OPT_KNP_MIN_IT 4
/* KNPEMI_OPT_FOLD_MEMBRANE (0/1, default 1): the launch that writes the potential back at the end of knpemi_solve_emi
 * (single rank, fused loop) or of knpemi_set_solution(KNPEMI_B_EMI, on_device) also forms the membrane-facet integrals of
 * b_knp (knpWeakForm.py:168-214) for that potential, so knpemi_assemble_knp launches the row kernel only: one dependent
 * launch fewer between the two solves.  The integrals are used only while no entry point that may change one of their
 * inputs (phi, concentrations, phi_M, I_ch, parameters, the FUSE_* / FOLD options) has been called since; 0 keeps the
 * facet kernel a launch of its own (what bench.py times as the facet-assembly kernel).  Writes through knpemi_vec_scatter
 * or the knpemi_device_csr / knpemi_device_rhs pointers are not seen: a caller who writes fields that way must call
 * knpemi_set_field or toggle this option before the next assembly. */
#define KNPEMI_OPT_FOLD_MEMBRANE 5
/* KNPEMI_OPT_KNP_METHOD (default 0): 0 = right-preconditioned BiCGStab, convergence on the true residual (fewest launches per
 * V-cycle); 1 = what PETSc's defaults make of the reference's `ksp_type gmres` (pdeSolver.py:100): GMRES with restart 30, left
 * preconditioning, classical Gram-Schmidt, convergence on the preconditioned residual norm relative to |M^-1 b|; the
 * iteration count and KNPEMI_OPT_KNP_MIN_IT then count GMRES iterations as `ksp_min_it` / getIterationNumber() do.
 * Single rank, AMG preconditioner (the fused loops); otherwise the option is ignored. */
#define KNPEMI_OPT_KNP_METHOD 6
/* KNPEMI_OPT_EMI_NORM (default 0): convergence test of the potential solve's CG: 0 = true residual |b - A x| <= max(atol,
 * rtol |b|); 1 = what PETSc's defaults make of the reference's `ksp_type cg` (pdeSolver.py:60-72; KSPCG: left preconditioning,
 * KSP_NORM_PRECONDITIONED): |M^-1 r| <= max(atol, rtol |M^-1 b|), the residual norm reported is that one.  Single rank,
 * AMG preconditioner (the fused loop); otherwise the option is ignored. */
#define KNPEMI_OPT_EMI_NORM 7
int knpemi_set_option(knpemi_handle* h, int option, int value);

/* Nodal trace of an (ECS, cell) pair of bulk functions onto Q_sub: interpolate_to_membrane
 * (utils.py:150-207).  u_e has n_vert[0] entries, u_i n_vert[sub]; q_e, q_i receive n_q[sub]. */
int knpemi_trace(knpemi_handle* h, int sub, const double* u_e, const double* u_i, double* q_e,
                 double* q_i);

/* Multi-GPU forward halo (owner -> ghost) of dof fields; replaces
 * Function.x.scatter_forward() (utils.py:100,199,204,254,293).  idx_dev / buf_dev are DEVICE pointers
 * (the caller moves buf between GPUs, e.g. torch.distributed send/recv over RCCL).
 * kind 0 (bulk): idx = global vertex ids (sub-mesh vertex + offset of its sub-domain), 5 doubles per
 *   entry: the K concentrations (solved ones as c_prev, the eliminated one last) and phi;
 * kind 1 (membrane): idx = global Q-dof ids, 1 + 3*n_model_slots doubles per entry: phi_M_prev and
 *   the I_ch_k (KNPEMI_MAX_IONS slots per model) of every membrane model. */
int knpemi_halo_width(knpemi_handle* h, int kind);
int knpemi_halo_pack(knpemi_handle* h, int kind, const int32_t* idx_dev, int n, double* buf_dev);
int knpemi_halo_unpack(knpemi_handle* h, int kind, const int32_t* idx_dev, int n, const double* buf_dev);

/* Distributed solves on a partitioned problem (one handle per rank; the reference runs its KSP solves on the MPI
 * communicator of the mesh, pdeSolver.py:24-35,74-78,99-110).  The library knows which local vertices this rank owns;
 * the caller supplies the two communication steps, both ordered on knpemi_stream(h):
 *   allreduce(ctx, n): sum the first n doubles of `reduce_buf_dev` over all ranks, in place;
 *   halo(ctx, vec_dev, which): forward halo (owner -> ghost) of a device vector in the unknown order of system `which`
 *     (KNPEMI_B_EMI: one value per local vertex; KNPEMI_B_KNP: the block order [sub-domain][ion][vertex]).
 * knpemi_solve_emi / knpemi_solve_knp then run the same Krylov methods on the global system: SpMV over the owned rows
 * after a halo of its argument, dot products over the owned entries summed with `allreduce`, and each rank's
 * smoothed-aggregation V-cycle on its own diagonal block as the preconditioner (block Jacobi over the ranks).
 * `owned` is a host array with one byte per local vertex (global numbering of this handle: sub-mesh vertex + offset
 * of its sub-domain), 1 = owned.  owned == NULL switches back to the single-rank solves. */
typedef int (*knpemi_allreduce_fn)(void* ctx, int n);
typedef int (*knpemi_halo_fn)(void* ctx, void* vec_dev, int which);
int knpemi_set_distributed(knpemi_handle* h, const uint8_t* owned, void* reduce_buf_dev, knpemi_allreduce_fn allreduce,
                           knpemi_halo_fn halo, void* ctx);
/* gather / scatter of entries of a device vector (the pack / unpack of the halo of a solver vector) */
/* Two-level variant of the distributed EMI preconditioner: next to every rank's AMG cycle a coarse space of one
 * piecewise-constant function per chunk of consecutive vertices of every sub-domain of every rank (as many chunks as
 * fit 64 functions in all) -- A_c = Phi^T A Phi is built with <= 64 SpMVs when the hierarchy is (re)built, every
 * application costs one all-reduce of <= 64 doubles.  Call after knpemi_set_distributed; the reduction buffer then
 * needs 8 + 64 doubles.  world <= 1 switches it off. */
int knpemi_set_distributed_coarse(knpemi_handle* h, int rank, int world);
int knpemi_vec_gather(knpemi_handle* h, const void* vec_dev, const int32_t* idx_dev, int n, void* buf_dev);
int knpemi_vec_scatter(knpemi_handle* h, void* vec_dev, const int32_t* idx_dev, int n, const void* buf_dev);

/* ---- RCCL transport inside the library (the reference: MPI inside DOLFINx / PETSc, Function.x.scatter_forward() and the
 * parallel KSP of pdeSolver.py:24-35) ----------------------------------------------------------------------------------
 * One process per GPU.  Rank 0 obtains a unique id (128 bytes), the caller distributes it over whatever rendezvous it
 * has, every rank calls knpemi_comm_init (collective).  knpemi_comm_sendrecv posts, in ONE RCCL group on the handle's
 * stream, for every part p: send_buf[send_off[p], +send_cnt[p]) -> peer[p] and recv_buf[recv_off[p], +recv_cnt[p]) <-
 * peer[p] (device buffers, counts in doubles): with knpemi_halo_pack before and knpemi_halo_unpack after it this is the
 * forward halo of a step, stream-ordered, no host synchronisation, no Python.  knpemi_comm_allreduce sums n doubles of a
 * device buffer over the ranks.  knpemi_comm_allreduce_hook / knpemi_comm_halo_hook have the signatures of
 * knpemi_allreduce_fn / knpemi_halo_fn and take the handle as ctx: passed to knpemi_set_distributed (after
 * knpemi_comm_set_vector_plan for both systems) they keep the distributed Krylov solves inside the library.
 * RCCL is resolved at run time (the copy already loaded in the process, else /opt/rocm/lib/librccl.so). */
int knpemi_comm_unique_id(char* out, size_t len);
int knpemi_comm_init(knpemi_handle* h, int rank, int world, const char* id_bytes, size_t len);
int knpemi_comm_sendrecv(knpemi_handle* h, const double* send_buf_dev, double* recv_buf_dev, int n_parts,
                         const int32_t* peer, const int64_t* send_off, const int64_t* send_cnt, const int64_t* recv_off,
                         const int64_t* recv_cnt);
int knpemi_comm_allreduce(knpemi_handle* h, double* buf_dev, int n);
int knpemi_comm_set_vector_plan(knpemi_handle* h, int which, const int32_t* send_idx_dev, int n_send,
                                const int32_t* recv_idx_dev, int n_recv, double* send_buf_dev, double* recv_buf_dev,
                                int n_parts, const int32_t* peer, const int64_t* send_off, const int64_t* send_cnt,
                                const int64_t* recv_off, const int64_t* recv_cnt);
int knpemi_comm_allreduce_hook(void* ctx, int n);
int knpemi_comm_halo_hook(void* ctx, void* vec_dev, int which);

/* Per-kernel HIP-event profiling on the handle's stream: every launch of a kernel whose bit is set
 * in `kernel_mask` is bracketed by an event pair; knpemi_profile_read() synchronises, returns the
 * number of bracketed launches and their summed duration, and resets the accumulator. */
#define KNPEMI_K_ODE 0           /* ode_step_kernel      */
#define KNPEMI_K_EMI_ROWS 1      /* emi_rows_kernel      */
#define KNPEMI_K_KNP_ROWS 2      /* knp_rows_kernel      */
#define KNPEMI_K_KNP_MEMBRANE 3  /* knp_membrane_kernel  */
#define KNPEMI_K_UPDATE 4        /* update_pde_kernel    */
#define KNPEMI_K_EMI_MEMBRANE 5  /* emi_membrane_rhs_kernel */
#define KNPEMI_K_SNAPSHOT 6      /* snapshot_pack_kernel */
#define KNPEMI_N_KERNELS 7
int knpemi_profile(knpemi_handle* h, uint32_t kernel_mask);
int knpemi_profile_read(knpemi_handle* h, int kernel, int64_t* launches, double* total_ms);

/* Stream-event timing of a region on the handle's stream (bench.py / rocprof cross-check). */
int knpemi_timer_start(knpemi_handle* h);
int knpemi_timer_stop_ms(knpemi_handle* h, double* ms);
/* HIP stream (hipStream_t) the handle enqueues on, for external event timing / ordering. */
void* knpemi_stream(knpemi_handle* h);

/* ---- DG(P1) + symmetric interior penalty variant -------------------------------------
 * The reference's README (README.md:5-7) describes a "DG fem method" and its 2D mesh script keeps the "interior
 * facets are tagged 0" convention of that method (examples/idealized_geometries/make_mesh_2D.py:88-90), but the
 * code under src/knpemi is continuous Galerkin on sub-meshes: there is NO reference interface these entry points
 * replace.  They provide the same step on ONE mesh with broken P1 functions: the volume terms of
 * emiWeakForm.py:138-241 / knpWeakForm.py:123-166 cell by cell, interior-penalty and upwind terms on the interior
 * facets of every sub-domain, and the reference's membrane terms (emiWeakForm.py:160-165,228-239,
 * knpWeakForm.py:168-214) on the tagged facets, with phi_M and I_ch living at the vertices of each membrane facet.
 * Triangles and tetrahedra (broken P1) and hexahedra (broken Q1: the cell type of the reference's own 3-D idealized
 * mesh, make_mesh_3D.py:100-102; volume terms by the 2 x 2 x 2 Gauss rule, facet terms by the 2 x 2 rule with every
 * quantity taken at the point, membrane terms by the reference's quadrilateral rules).  Dof (cell c, local vertex j)
 * = c * nv + j; membrane node (facet f, vertex a) = f * nf + a; CSR rows hold one nv-wide block per cell (the cell
 * itself and its facet neighbours, in increasing cell order).  The K - 1 concentration systems share the pattern of
 * the potential system. */
typedef struct knpemi_dg knpemi_dg;

typedef struct {
  int32_t cell_kind;            /* KNPEMI_TRIANGLE | KNPEMI_TETRAHEDRON | KNPEMI_HEXAHEDRON (broken Q1; local vertex j at the
                                   reference point whose coordinate along axis a is bit a of j) */
  int32_t n_sub;                /* sub-domains, ECS = 0 */
  int32_t n_ions;               /* K = 2..4, the last one eliminated */
  int64_t n_cells, n_vertices, n_mem_facets;
  const double* x;              /* [n_vertices][gdim] */
  const int32_t* cells;         /* [n_cells][nv] vertex ids */
  const int32_t* cell_sub;      /* [n_cells] sub-domain index of every cell */
  const int32_t* mem_facets;    /* [n_mem_facets][nf] vertex ids of the membrane facets: every one separates an ECS
                                   cell from a cell of a sub-domain > 0; every other facet between two cells must
                                   lie inside one sub-domain */
} knpemi_dg_desc;

typedef struct {
  double dt, F, psi, C_M;
  double gamma;                                         /* interior penalty parameter (10 is a safe default) */
  double z[KNPEMI_MAX_IONS];
  double D[KNPEMI_MAX_SUB][KNPEMI_MAX_IONS];
  double rho_z;
  double rho[KNPEMI_MAX_SUB];
} knpemi_dg_params;

#define KNPEMI_DG_C 0         /* previous-step concentration of ion idx < K (the eliminated ion last)  [n_dofs] */
#define KNPEMI_DG_PHI 1       /* potential                                                            [n_dofs] */
#define KNPEMI_DG_PHI_M 2     /* phi_M_prev at the membrane nodes                                     [n_mem_nodes] */
#define KNPEMI_DG_I_CH 3      /* channel current of ion idx < K at the membrane nodes                 [n_mem_nodes] */
#define KNPEMI_DG_SOURCE 4    /* source term of solved ion idx < K - 1 (used in ECS cells only)       [n_dofs] */

int knpemi_dg_create(const knpemi_dg_desc* desc, int device, knpemi_dg** out);
void knpemi_dg_destroy(knpemi_dg* h);
int knpemi_dg_set_params(knpemi_dg* h, const knpemi_dg_params* p);
int knpemi_dg_dims(knpemi_dg* h, int64_t* n_dofs, int64_t* nnz, int64_t* n_mem_nodes);
int knpemi_dg_get_pattern(knpemi_dg* h, int32_t* rowptr, int32_t* colind);
/* dofs of the ECS cell / of the intracellular cell that sit at every membrane node */
int knpemi_dg_get_membrane_dofs(knpemi_dg* h, int32_t* dof_e, int32_t* dof_i);
int knpemi_dg_set_field(knpemi_dg* h, int field, int idx, const double* host, size_t n);
int knpemi_dg_get_field(knpemi_dg* h, int field, int idx, double* host, size_t n);
/* flags: KNPEMI_NO_SPLITTING.  assemble_emi fills A_emi, b_emi from the concentrations, phi_M (and I_ch without the
 * splitting scheme); assemble_knp fills the K - 1 matrices and right-hand sides from the concentrations, the potential,
 * phi_M and I_ch.  One kernel launch each. */
int knpemi_dg_assemble_emi(knpemi_dg* h, int flags);
int knpemi_dg_assemble_knp(knpemi_dg* h, int flags);
/* which: 0 = potential system, 1 + k = concentration system of solved ion k */
int knpemi_dg_get_values(knpemi_dg* h, int which, double* vals);
int knpemi_dg_get_rhs(knpemi_dg* h, int which, double* b);
int knpemi_dg_device_system(knpemi_dg* h, int which, const int32_t** rowptr, const int32_t** colind, const double** vals,
                            const double** b);
/* End of step (utils.py:238-295): c_prev <- c_new ([K-1][n_dofs], host or device pointer), eliminated ion from
 * electroneutrality dof by dof, phi_M <- phi_i - phi_e at the membrane nodes. */
int knpemi_dg_update(knpemi_dg* h, const double* c_new, int on_device);
/* Device solves of the DG systems (the KSP solves of pdeSolver.py:24-35,74-78,99-110 with the iterative options,
 * SURVEY section 8 f1 for the f4 variant): CG on the potential system with the constants projected out, BiCGStab on the
 * K - 1 concentration systems, both preconditioned by the library's smoothed-aggregation AMG whose first coarse level is
 * the continuous P1 space of every sub-domain (auxiliary space) under a damped-Jacobi smoother on the broken dofs.
 * Start from the current potential / the previous concentrations, stop at ||r|| <= max(atol, rtol ||b||),
 * KNPEMI_ESOLVE at maxit.  solve_emi writes the potential field; solve_knp keeps the solution on the device and, with
 * update != 0, runs knpemi_dg_update on it; knpemi_dg_get_solution copies it out ([K-1][n_dofs]).  Single rank. */
int knpemi_dg_solve_emi(knpemi_dg* h, double rtol, double atol, int maxit, int* iters, double* relres);
/* On a cell partition (knpemi.dg.DGSlab; the reference's parallel KSP, SURVEY section 8 e + f1, for the f4 variant): the two
 * solves become solves of the global systems exactly as knpemi_set_distributed arranges for the CG path -- owned rows
 * only, halo of every SpMV argument, all-reduced dot products, per-rank auxiliary-space AMG.  `owned`: one byte per local
 * broken dof, 1 = dof of an owned cell (NULL: back to single-rank solves); vector orders for `halo`: KNPEMI_B_EMI one value
 * per dof, KNPEMI_B_KNP [solved ion][dof]. */
int knpemi_dg_set_distributed(knpemi_dg* h, const uint8_t* owned, void* reduce_buf_dev, knpemi_allreduce_fn allreduce,
                              knpemi_halo_fn halo, void* ctx);
/* For the halo hook: knpemi_vec_gather / knpemi_vec_scatter on the DG handle's stream -- buf[i] = vec[idx[i]], and
 * vec[idx[i]] = buf[i], over the n entries of idx (doubles and int32 in device memory).  n == 0 launches nothing;
 * KNPEMI_EINVAL for a null handle, n < 0, or a null pointer with n > 0. */
int knpemi_dg_vec_gather(knpemi_dg* h, const void* vec_dev, const int32_t* idx_dev, int n, void* buf_dev);
int knpemi_dg_vec_scatter(knpemi_dg* h, void* vec_dev, const int32_t* idx_dev, int n, const void* buf_dev);
int knpemi_dg_solve_knp(knpemi_dg* h, double rtol, double atol, int maxit, int* iters, double* relres, int update);
int knpemi_dg_get_solution(knpemi_dg* h, double* c_host);
/* on != 0: both solves start from 2 x_n - x_(n-1) (the last two solutions) instead of x_n, as knpemi_extrapolate_guess
 * does for the CG path; the stopping criterion is unchanged. */
int knpemi_dg_set_extrapolation(knpemi_dg* h, int on);
/* Membrane ODE sweep over the membrane nodes with one of the built-in models (KNPEMI_MODEL_*): same kernel, tables and
 * flags as knpemi_ode_step; states / params are [n_mem_nodes][n_states | n_params] row-major on the host. */
int knpemi_dg_ode_bind(knpemi_dg* h, int model_id, int n_states, int n_params, const double* states, const double* params,
                       const int32_t* ion_param, int v_index);
int knpemi_dg_ode_step(knpemi_dg* h, double t0, double dt, double rtol, double atol, int flags);
int knpemi_dg_ode_get_tables(knpemi_dg* h, double* states, double* params);
int knpemi_dg_ode_stats(knpemi_dg* h, int64_t* n_rhs, int64_t* n_steps, int64_t* n_failed);
/* Cell-partitioned runs: every rank holds its cells plus one layer of ghost cells across the cut facets.  The ghost
 * cells' dofs (five field doubles each: the K concentrations and the potential) are refreshed from their owners once
 * per step: pack the listed dofs into a device buffer [n][5] / unpack it on the receiving side (device index lists,
 * stream-ordered; the transport is the caller's: RCCL point-to-point in knpemi/dg.py, as Function.x.scatter_forward()
 * of a DG function does under MPI in DOLFINx).  Membrane nodes of ghost cells are integrated redundantly. */
int knpemi_dg_halo_pack(knpemi_dg* h, const int32_t* idx_dev, int n, double* buf_dev);
int knpemi_dg_halo_unpack(knpemi_dg* h, const int32_t* idx_dev, int n, const double* buf_dev);
/* the library's RCCL transport for that halo, on the DG handle's stream (see knpemi_comm_init / knpemi_comm_sendrecv) */
int knpemi_dg_comm_init(knpemi_dg* h, int rank, int world, const char* id_bytes, size_t len);
int knpemi_dg_comm_sendrecv(knpemi_dg* h, const double* send_buf_dev, double* recv_buf_dev, int n_parts,
                            const int32_t* peer, const int64_t* send_off, const int64_t* send_cnt, const int64_t* recv_off,
                            const int64_t* recv_cnt);
int knpemi_dg_sync(knpemi_dg* h);
/* average duration (ms) of `reps` back-to-back launches of one assembly kernel (0 = potential, 1 = concentrations),
 * measured with HIP events on the stream the kernel is launched on */
int knpemi_dg_time_kernel(knpemi_dg* h, int which, int flags, int reps, double* avg_ms);
/* HIP event brackets of the assembly kernels inside a running time loop (as knpemi_profile): on = n >= 1 brackets
 * every n-th launch of each kernel, 0 switches them off;
 * profile_read synchronises, returns the number of bracketed launches of kernel `which` and their summed duration,
 * and resets the accumulator */
int knpemi_dg_profile(knpemi_dg* h, int on);
int knpemi_dg_profile_read(knpemi_dg* h, int which, int64_t* launches, double* total_ms);
/* HIP stream the handle enqueues on */
void* knpemi_dg_stream(knpemi_dg* h);

/* Observables of a DG run (knpemi.dg_recording.DGObservables): linear functionals and min / max reductions of the broken
 * fields, and the jump seminorms the interior penalty controls, recorded on the device into a time-series buffer.  The
 * table, the kernel, the buffer and the capacity / dropped-row / reset semantics are those of knpemi_observe_set ..
 * knpemi_observe_clear; what differs is where a field lives.  Observable o reads the field spec[4o + 0]:
 *   KNPEMI_DG_C with ion index spec[4o + 2] < K (the eliminated ion last; valid after knpemi_dg_update), KNPEMI_DG_PHI:
 *     indices are broken dofs c * nv + j;
 *   KNPEMI_DG_PHI_M: indices are membrane nodes f * nf + a;
 *   KNPEMI_DG_JUMP: the jump seminorm of sub-domain spec[4o + 1] and of the concentration of ion spec[4o + 2] < K, or of the
 *     potential with spec[4o + 2] == -1,
 *         J_s(u) = sum over the interior facets F with both cells in s of  int_F (1 / h_F) [u]^2 dS,
 *     1 / h_F the penalty weight of the assembly (simplices: the mean of the two cells' |grad lambda_opposite|; hexahedra:
 *     point by point on the 2 x 2 Gauss rule the mean of the two cells' |grad xi_normal|).  Every facet counts once,
 *     membrane and boundary facets never; a sub-domain without interior facets gives 0.  One KNPEMI_OBS_SUM entry with index
 *     0 whose weight scales the value; no square root is taken.
 * spec[4o + 1] is read for KNPEMI_DG_JUMP only.  Validated on the host: every index in range, every weight and
 * denominator finite, every op known -- anything else is KNPEMI_EINVAL by name, and the previous table keeps recording. */
#define KNPEMI_DG_JUMP 5
int knpemi_dg_observe_set(knpemi_dg* h, int n_obs, const int32_t* spec, const int64_t* ptr, const int32_t* idx,
                          const double* w, const double* denom, int capacity);
/* Enqueue the evaluation of every observable as one row on the handle's stream, behind whatever knpemi_dg_update and the
 * membrane sweep have enqueued: dg_jump_kernel first when a jump seminorm is defined (one launch, every sub-domain and all
 * K + 1 fields), then the observe launch.  Sums are formed in a fixed order: two identical runs give bit-identical rows.
 * Nothing is synchronised.  KNPEMI_EINVAL before knpemi_dg_observe_set, after knpemi_dg_observe_clear and before
 * knpemi_dg_set_params. */
int knpemi_dg_observe_record(knpemi_dg* h);
/* As knpemi_observe_read. */
int knpemi_dg_observe_read(knpemi_dg* h, int n_rows, double* out, int64_t* rows, int64_t* overflow, int reset);
/* Drop the table and the buffer (knpemi_dg_observe_record then fails with KNPEMI_EINVAL); knpemi_dg_destroy does the same. */
int knpemi_dg_observe_clear(knpemi_dg* h);

/* Membrane events of a DG run (knpemi.dg_recording.DGMembraneEvents): the per-dof state of knpemi_events_set for every
 * membrane node (facet f, vertex a) = f * nf + a, one threshold and one reset <= threshold for all of them, ring length
 * 0 <= keep <= KNPEMI_EVENTS_MAX_KEEP; anything else is KNPEMI_EINVAL.  Replaces any previous table and clears all state. */
int knpemi_dg_events_set(knpemi_dg* h, double threshold, double reset, int keep);
/* Enqueue one record at time t on the handle's stream (after knpemi_dg_update or knpemi_dg_ode_step): one launch over the
 * membrane nodes, nothing synchronised, by the rules stated at knpemi_events_record.  KNPEMI_EINVAL before
 * knpemi_dg_events_set, before knpemi_dg_set_params, and when t is not finite or not greater than the previous record's t. */
int knpemi_dg_events_record(knpemi_dg* h, double t);
/* Synchronise and copy out the maps: n_mem_nodes entries each, ring as [keep][n_mem_nodes] in slot order; every pointer
 * may be NULL.  KNPEMI_EINVAL before knpemi_dg_events_set. */
int knpemi_dg_events_read(knpemi_dg* h, int32_t* count, double* t_first, double* t_last, double* v_peak, double* t_peak,
                          double* ring);
/* All state back to "before the first record"; the table stays.  Enqueue only. */
int knpemi_dg_events_reset(knpemi_dg* h);
/* Drop the table and the state buffers (knpemi_dg_events_record then fails with KNPEMI_EINVAL); knpemi_dg_destroy does the
 * same. */
int knpemi_dg_events_clear(knpemi_dg* h);

/* The per-cell ion balance of a DG run (knpemi.dg_balance.DGIonBalance): what the scheme conserves cell by cell.  Testing
 * the system of solved ion k with the indicator of a cell T leaves
 *     (m_T,k(new) - m_T,k(old)) / dt + out_T,k = mem_T,k + src_T,k  (+ the cell's share of the solve's residual),
 * m_T,k = int_T c_k, out_T,k the numerical outflow of the assembly through the interior facets of T in its three parts
 *     cons  = - int_F {D_k grad c_k} . n_T,   pen = int_F (gamma / h_F) {D_k} [c_k],   drift = int_F beta_F c_k^up
 * (beta_F = -z_k psi {D_k grad phi} . n_T, upwind side T when beta_F > 0; every ingredient as the assembly kernels take it;
 * membrane and boundary facets contribute nothing), mem_T,k the integral over the cell's membrane facets of
 *     j_k^s = (I_ch,k + alpha_k^s (I_cap - S I_ch,tot)) / (F z_k),  I_cap = C_M ([phi] - phi_M) / dt,
 * counted positive INTO T (s: the cell's own side; S = 1 with the splitting scheme; the assembly's degree-6 facet rule), and
 * src_T,k = int_T f_k on ECS cells.  cons, pen, drift, mem and the masses are kept for all K ions, src and the defect
 *     defect_T,k = (m_new - m_old) / dt + cons + pen + drift - mem - src
 * for the K - 1 solved ones (0 for the eliminated ion).
 *
 * knpemi_dg_balance_set installs the recorder: a series buffer of `capacity` rows, the cell table, and for every membrane
 * facet the index facet_tag[f] < n_tags (<= 8) of its tag (NULL allowed without membrane facets).  want_cells == 0: the
 * end-of-step launch does not write its columns of the cell table and knpemi_dg_balance_cells is refused.  Anything else is
 * KNPEMI_EINVAL by name, and the previous recorder keeps recording.
 * A row: [n_sub][K](sum_T m_new, sum_T out, sum_T |pen|, max_T |defect|), then [n_tags](K x sum_F int j_k^e, K x sum_F int
 * j_k^i, int I_cap, int I_ch,tot, area). */
int knpemi_dg_balance_set(knpemi_dg* h, int capacity, int want_cells, int n_tags, const int32_t* facet_tag);
/* Between knpemi_dg_assemble_knp and the solve of the concentrations (old concentrations, new potential, old phi_M, I_ch on
 * the device): one launch on the handle's stream writes mem, m_old and src of every cell and the membrane tags' sums; the
 * splitting scheme is that of the last knpemi_dg_assemble_knp.  Nothing is synchronised.  KNPEMI_EINVAL before
 * knpemi_dg_balance_set and before knpemi_dg_set_params. */
int knpemi_dg_balance_record_membrane(knpemi_dg* h);
/* At the end of the step, after knpemi_dg_update (new concentrations): one launch writes the outflow parts, m_new and the
 * defect (dt: that of knpemi_dg_set_params) and appends the row; t, the time of the record, must be finite -- the row carries
 * no time, the caller keeps it.  Sums are formed in a fixed order without floating-point atomics: two identical runs give
 * bit-identical rows and tables.  KNPEMI_EINVAL, by name: before knpemi_dg_balance_set, before knpemi_dg_set_params, and
 * when no knpemi_dg_balance_record_membrane came since the last record. */
int knpemi_dg_balance_record(knpemi_dg* h, double t);
/* As knpemi_observe_read. */
int knpemi_dg_balance_read(knpemi_dg* h, int n_rows, double* out, int64_t* rows, int64_t* overflow, int reset);
/* Synchronise and copy out the cell table of the last record: [n_cells][K][mem, cons, pen, drift, m_old, m_new, src, defect].
 * KNPEMI_EINVAL before the first record and when the recorder was set with want_cells == 0. */
int knpemi_dg_balance_cells(knpemi_dg* h, double* out);
/* A new series; a pending knpemi_dg_balance_record_membrane is forgotten.  Enqueue only. */
int knpemi_dg_balance_reset(knpemi_dg* h);
/* Drop the recorder (knpemi_dg_balance_record then fails with KNPEMI_EINVAL); knpemi_dg_destroy does the same. */
int knpemi_dg_balance_clear(knpemi_dg* h);

/* Field snapshots of a DG run (knpemi.dg_snapshots.DGSnapshots): the frames, the ring, the copy stream and the rules of
 * knpemi_snapshot_* above, on the fields of a DG handle.  A DG field is broken -- a mesh vertex carries one dof per cell that
 * touches it -- so a watch also names a FORM, and a space is (sub-domain or membrane tag, form):
 *   KNPEMI_DG_SNAP_BROKEN     bulk: one value per dof (cell, local vertex), in the cell order of the sub-domain; membrane: one
 *                             per membrane node (facet, a) of the tag;
 *   KNPEMI_DG_SNAP_CELL_MEAN  bulk only: one value per cell, the nodal values summed in local-vertex order 0 .. nv - 1 and
 *                             divided by nv (the integral mean on simplices and on parallelepiped hexahedra);
 *   KNPEMI_DG_SNAP_VERTEX     one value per mesh vertex the space touches, in increasing vertex id: the coincident dofs
 *                             (membrane: the nodes of the tag at that vertex) summed in increasing order and divided by
 *                             their number -- what results_sub_<tag>.xdmf / results_mem_<tag>.xdmf of the reference hold
 *                             (run_stim_duration.py:52-90).
 * A sum starts from its first entry; then additions in list order and one IEEE double division: a frame is a bit-exact
 * function of the fields.
 * A watch is spec[w] = {quantity, tag, ion-or-state, form, dtype}: KNPEMI_DG_C (ion < K, the eliminated one last) and
 * KNPEMI_DG_PHI over sub-domain index `tag`; KNPEMI_DG_PHI_M, KNPEMI_DG_I_CH (ion < K) and KNPEMI_DG_ODE_STATE (a state
 * column of the table bound with knpemi_dg_ode_bind) over the membrane tag with index `tag`; dtype 0 stores the double,
 * KNPEMI_SNAPSHOT_F32 (float)v.  The handle knows neither the tags of the membrane facets nor the mesh vertices, so the
 * caller gives the spaces: space[p] = {kind (0: cells of a sub-domain, 1: a membrane tag), tag, form, n_items} and the list
 * list[list_off[p] .. list_off[p + 1]) -- broken: the n_items dofs (nodes); cell_mean: the n_items cells; vertex: vptr
 * [n_items + 1] (vptr[0] = 0, increasing) followed by the vptr[n_items] dofs (nodes), ascending within a vertex.  Every
 * entry is checked against the fields' lengths.  Selection j belongs to space sel_space[j] (an index into `space`) and
 * lists ascending distinct items, as in knpemi_snapshot_set.  Frame layout as there; knpemi_dg_snapshot_layout reports it.
 * The first call creates the copy stream and the ring (knpemi_dg_create does not).  A refused call names the reason
 * (KNPEMI_EINVAL: null arguments, an unknown quantity, form or dtype, a watch whose (kind, tag, form) is no given space, an
 * ion or state out of range, a state watch before knpemi_dg_ode_bind, a watch or space listed twice, a list entry out of
 * range, a bad selection, depth < 1, too many watches or spaces) and leaves the previous recorder recording. */
#define KNPEMI_DG_ODE_STATE 6
#define KNPEMI_DG_SNAP_BROKEN 0
#define KNPEMI_DG_SNAP_CELL_MEAN 1
#define KNPEMI_DG_SNAP_VERTEX 2
#define KNPEMI_DG_SNAPSHOT_MAX_SPACE 40
int knpemi_dg_snapshot_set(knpemi_dg* h, int n_watch, const int32_t* spec, int n_space, const int32_t* space,
                           const int64_t* list_off, const int32_t* list, int n_space_sel, const int32_t* sel_space,
                           const int64_t* sel_off, const int32_t* sel_idx, int depth);
/* As knpemi_snapshot_layout. */
int knpemi_dg_snapshot_layout(knpemi_dg* h, int64_t* offset, int64_t* n_items, int64_t* frame_bytes);
/* As knpemi_snapshot_record: ONE pack launch on the handle's stream, then the copy on the copy stream; nothing waits for the
 * host.  KNPEMI_EINVAL, by name: before knpemi_dg_snapshot_set, before knpemi_dg_set_params, and when t is not finite or
 * does not exceed the previous record's.  A slot IN FLIGHT: KNPEMI_EBUSY, nothing enqueued, nothing changed. */
int knpemi_dg_snapshot_record(knpemi_dg* h, double t);
/* As knpemi_snapshot_take. */
int knpemi_dg_snapshot_take(knpemi_dg* h, int wait, void* out, size_t bytes, double* t, int64_t* seq);
/* The number of frames IN FLIGHT (0 before knpemi_dg_snapshot_set). */
int knpemi_dg_snapshot_pending(knpemi_dg* h);
/* Wait for the copy stream, free every slot, restart seq at 0 and forget the previous record's time; the table stays. */
int knpemi_dg_snapshot_reset(knpemi_dg* h);
/* Synchronise both streams and drop the table, the ring, the copy stream and the events (knpemi_dg_snapshot_record then
 * fails with KNPEMI_EINVAL); knpemi_dg_destroy does the same. */
int knpemi_dg_snapshot_clear(knpemi_dg* h);

#ifdef __cplusplus
}
#endif
#endif /* KNPEMI_HIP_H */
