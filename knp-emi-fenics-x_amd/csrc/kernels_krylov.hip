// Device-resident Krylov solves for the two sub-problems (the row next to the
// hot path).  The reference hands its systems to PETSc (src/knpemi/pdeSolver.py:13-38,88-113): CG +
// hypre BoomerAMG for the symmetric positive semi-definite EMI system with the constant null space
// attached (:74-78), GMRES + BoomerAMG for the non-symmetric block-diagonal KNP system, both with a
// non-zero initial guess (the previous solution).  Here: CG with the right-hand side and the solution
// projected onto zero mean, and right-preconditioned BiCGStab, both preconditioned with a smoothed-aggregation
// V-cycle (kernels_amg.hip; Jacobi selectable), working in place on the assembled device CSR.
//
// All vectors and scalars stay on the device; the host reads back one residual norm per chunk of iterations
// (one iteration with AMG) to test convergence.  A dot product, its block partials and the scalar update it
// feeds are one launch with a fixed summation order, so the solves are bit-reproducible.
#include <cmath>
#include <cstdio>

#include "knpemi_internal.h"

namespace {

constexpr int RED_BLOCKS = 512, RED_THREADS = 256;

// sc[] layout (device scalars)
enum { S_RHO = 0, S_RHO_OLD, S_PAP, S_ALPHA, S_BETA, S_OMEGA, S_RR, S_BB, S_TS, S_TT, S_MEAN, S_FLAG, S_RV, S_N };
// S_FLAG: breakdown events of the current chunk of iterations (bit set, stored as a double): a vanishing denominator never
// reaches a division -- the quotient is replaced by 0 and the event is recorded, so a breakdown surfaces as a flag the host
// acts on (converged / restart / error with the scalars in the message), not as a NaN that has already overwritten x.
enum { F_RHO_ZERO = 1, F_RV_ZERO = 2, F_OMEGA_ZERO = 4, F_PAP_ZERO = 8 };

// y = A * (x .* dinv?), or (dinv == NULL, b != NULL) the residual y = b - A x : LPR lanes per row, four independent
// index -> value -> gather chains per lane and trip
template <bool SCALED, int LPR>
__global__ __launch_bounds__(256) void spmv_kernel(int n, const int* __restrict__ rowptr, const int* __restrict__ colind,
                                                   const double* __restrict__ vals, const double* __restrict__ x,
                                                   const double* __restrict__ dinv, double* __restrict__ y,
                                                   const double* __restrict__ b = nullptr,
                                                   const uint8_t* __restrict__ owned = nullptr,
                                                   double* __restrict__ dinv_out = nullptr) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int row = t / LPR, l = t % LPR;
  double acc = 0.0, diag = 0.0;
  // partitioned problem: only the rows of owned unknowns are assembled completely; ghost rows give 0
  const bool live = row < n && (!owned || owned[row]);
  if (live) {
    const int a = rowptr[row], e = rowptr[row + 1];
    double acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
    int j = a + l;
    for (; j + 3 * LPR < e; j += 4 * LPR) {
      const int c0 = colind[j], c1 = colind[j + LPR], c2 = colind[j + 2 * LPR], c3 = colind[j + 3 * LPR];
      const double v0 = vals[j], v1 = vals[j + LPR], v2 = vals[j + 2 * LPR], v3 = vals[j + 3 * LPR];
      if (SCALED) {
        acc += v0 * (x[c0] * dinv[c0]); acc1 += v1 * (x[c1] * dinv[c1]);
        acc2 += v2 * (x[c2] * dinv[c2]); acc3 += v3 * (x[c3] * dinv[c3]);
      } else {
        acc += v0 * x[c0]; acc1 += v1 * x[c1]; acc2 += v2 * x[c2]; acc3 += v3 * x[c3];
        diag = c0 == row ? v0 : c1 == row ? v1 : c2 == row ? v2 : c3 == row ? v3 : diag;
      }
    }
    for (; j < e; j += LPR) {
      const int c = colind[j];
      acc += vals[j] * (SCALED ? x[c] * dinv[c] : x[c]);
      if (!SCALED && c == row) diag = vals[j];
    }
    acc = (acc + acc1) + (acc2 + acc3);
  }
#pragma unroll
  for (int m = LPR / 2; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
  if (!SCALED && dinv_out) {   // the inverse diagonal as a by-product of the first residual (diag_inv_kernel's rule)
#pragma unroll
    for (int m = LPR / 2; m >= 1; m >>= 1) diag += __shfl_xor(diag, m);
    if (row < n && l == 0) dinv_out[row] = diag != 0.0 ? 1.0 / diag : 1.0;
  }
  if (row < n && l == 0) y[row] = live ? ((!SCALED && b) ? b[row] - acc : acc) : 0.0;
}

// a[i] = 0 on ghost entries (partitioned problems)
__global__ void mask_kernel(int n, const uint8_t* __restrict__ owned, double* __restrict__ a, int as_ones) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (as_ones) a[i] = owned[i] ? 1.0 : 0.0;
  else if (!owned[i]) a[i] = 0.0;
}

// ghost rows of the operator become identity rows: the rank-local V-cycle then leaves ghost entries at zero
__global__ void ghost_identity_kernel(int n, const int* __restrict__ rowptr, const int* __restrict__ colind,
                                      const uint8_t* __restrict__ owned, double* __restrict__ vals) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n || owned[row]) return;
  for (int j = rowptr[row]; j < rowptr[row + 1]; ++j) vals[j] = colind[j] == row ? 1.0 : 0.0;
}

__global__ void diag_inv_kernel(int n, const int* __restrict__ rowptr, const int* __restrict__ colind,
                                const double* __restrict__ vals, double* __restrict__ dinv) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  double d = 1.0;
  for (int j = rowptr[row]; j < rowptr[row + 1]; ++j)
    if (colind[j] == row) d = vals[j];
  dinv[row] = d != 0.0 ? 1.0 / d : 1.0;
}

// second-stage scalar algebra of the algorithm step `op`
enum { OP_STORE3 = 0, OP_CG_INIT, OP_CG_PAP, OP_CG_RHO, OP_BI_RHO, OP_BI_ALPHA, OP_BI_OMEGA, OP_MEAN, OP_START };

__device__ __forceinline__ void raise_flag(double* __restrict__ sc, int bit) { sc[S_FLAG] = (double)((int)sc[S_FLAG] | bit); }

__device__ __forceinline__ void apply_dot_op(double* __restrict__ sc, int op, int nd, double v0, double v1, double v2, int d0,
                                             int d1, int d2, double scale) {
  switch (op) {
    case OP_STORE3: sc[d0] = v0; if (nd > 1) sc[d1] = v1; if (nd > 2) sc[d2] = v2; break;
    case OP_MEAN: sc[S_MEAN] = v0 * scale; break;
    case OP_START: sc[S_RR] = v0; sc[S_BB] = v1; sc[S_FLAG] = 0.0; break;                        // r.r, b.b of a new solve
    case OP_CG_INIT: sc[S_RHO] = v0; sc[S_RR] = v1; if (nd > 2) sc[S_BB] = v2; break;          // r.z, r.r[, b.b]
    case OP_CG_PAP:                                                                          // p.Ap
      sc[S_PAP] = v0;
      if (v0 != 0.0) sc[S_ALPHA] = sc[S_RHO] / v0;
      else { sc[S_ALPHA] = 0.0; raise_flag(sc, F_PAP_ZERO); }                                // p = 0: nothing left to correct
      break;
    case OP_CG_RHO:                                                                          // r.z, r.r
      sc[S_BETA] = sc[S_RHO] != 0.0 ? v0 / sc[S_RHO] : 0.0;
      sc[S_RHO] = v0; sc[S_RR] = v1;
      break;
    case OP_BI_RHO:                                                                          // rhat.r
      // rho_(i-1) = 0 or omega_(i-1) = 0 with a residual left is BiCGStab's breakdown: beta = 0 restarts the recurrence
      // from p = r (the host re-bases rhat as well when it sees the flag)
      if (sc[S_RHO] != 0.0 && sc[S_OMEGA] != 0.0) sc[S_BETA] = (v0 / sc[S_RHO]) * (sc[S_ALPHA] / sc[S_OMEGA]);
      else { sc[S_BETA] = 0.0; raise_flag(sc, sc[S_RHO] != 0.0 ? F_OMEGA_ZERO : F_RHO_ZERO); }
      sc[S_RHO] = v0;
      break;
    case OP_BI_ALPHA:                                                                        // rhat.v
      sc[S_RV] = v0;
      if (v0 != 0.0) sc[S_ALPHA] = sc[S_RHO] / v0;
      else { sc[S_ALPHA] = 0.0; raise_flag(sc, F_RV_ZERO); }
      break;
    case OP_BI_OMEGA:                                                                        // t.s, t.t
      sc[S_TS] = v0; sc[S_TT] = v1;
      sc[S_OMEGA] = v1 != 0.0 ? v0 / v1 : 0.0;      // t = 0 <=> s = 0: the half step x += alpha p was exact, r = s
      break;
  }
}

// Up to three dot products and the scalar update that consumes them in ONE launch: every block writes its
// partial sums, the last block to finish (ticket counter) adds the partials in a fixed order and applies
// `op` to the device scalars.  The summation order does not depend on which block is last, so the solves stay
// bit-reproducible.
__global__ __launch_bounds__(RED_THREADS) void dots_kernel(int n, int nd, const double* a0, const double* b0,
                                                           const double* a1, const double* b1, const double* a2,
                                                           const double* b2, double* partial, unsigned* ticket,
                                                           double* __restrict__ sc, int op, int d0, int d1, int d2,
                                                           double scale, double* __restrict__ red = nullptr) {
  __shared__ double sh[3][RED_THREADS];
  __shared__ bool last;
  double s0 = 0, s1 = 0, s2 = 0;
  const int stride = gridDim.x * blockDim.x;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n; i += 4 * stride) {     // four independent loads per vector in flight
    const double x0 = a0[i], x1 = a0[i + stride], x2 = a0[i + 2 * stride], x3 = a0[i + 3 * stride];
    const double y0 = b0[i], y1 = b0[i + stride], y2 = b0[i + 2 * stride], y3 = b0[i + 3 * stride];
    s0 += x0 * y0; s0 += x1 * y1; s0 += x2 * y2; s0 += x3 * y3;
    if (nd > 1) { s1 += a1[i] * b1[i]; s1 += a1[i + stride] * b1[i + stride]; s1 += a1[i + 2 * stride] * b1[i + 2 * stride]; s1 += a1[i + 3 * stride] * b1[i + 3 * stride]; }
    if (nd > 2) { s2 += a2[i] * b2[i]; s2 += a2[i + stride] * b2[i + stride]; s2 += a2[i + 2 * stride] * b2[i + 2 * stride]; s2 += a2[i + 3 * stride] * b2[i + 3 * stride]; }
  }
  for (; i < n; i += stride) {
    s0 += a0[i] * b0[i];
    if (nd > 1) s1 += a1[i] * b1[i];
    if (nd > 2) s2 += a2[i] * b2[i];
  }
  sh[0][threadIdx.x] = s0; sh[1][threadIdx.x] = s1; sh[2][threadIdx.x] = s2;
  __syncthreads();
  for (int w = RED_THREADS / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w)
      for (int k = 0; k < nd; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    for (int k = 0; k < nd; ++k)
      __hip_atomic_store(&partial[k * RED_BLOCKS + blockIdx.x], sh[k][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  const int nb = gridDim.x;
  for (int k = 0; k < nd; ++k) {
    double s = 0;
    for (int i = threadIdx.x; i < nb; i += RED_THREADS)
      s += __hip_atomic_load(&partial[k * RED_BLOCKS + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sh[k][threadIdx.x] = s;
  }
  __syncthreads();
  for (int w = RED_THREADS / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w)
      for (int k = 0; k < nd; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  *ticket = 0;
  const double v0 = sh[0][0], v1 = nd > 1 ? sh[1][0] : 0.0, v2 = nd > 2 ? sh[2][0] : 0.0;
  if (red) {   // partitioned problem: the sums of this rank; the scalar algebra follows the all-reduce (dots_apply_kernel)
    red[0] = v0; red[1] = v1; red[2] = v2;
    return;
  }
  apply_dot_op(sc, op, nd, v0, v1, v2, d0, d1, d2, scale);
}

__global__ void dots_apply_kernel(double* __restrict__ sc, const double* __restrict__ red, int op, int nd, int d0, int d1,
                                  int d2, double scale) {
  apply_dot_op(sc, op, nd, red[0], nd > 1 ? red[1] : 0.0, nd > 2 ? red[2] : 0.0, d0, d1, d2, scale);
}


enum { V_RESID = 0, V_SHIFT, V_CG_XR, V_CG_P, V_JACOBI, V_BI_P, V_BI_S, V_COPY, V_COPY_SHIFT };

// small fused vector updates; scalars are read from device memory
__global__ void vec_kernel(int n, int op, const double* __restrict__ sc, double* __restrict__ a, double* __restrict__ b,
                           const double* __restrict__ c, const double* __restrict__ d, const double* __restrict__ e) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  switch (op) {
    case V_RESID: a[i] = c[i] - d[i]; break;                                   // r = b - Ax
    case V_SHIFT: a[i] -= sc[S_MEAN]; break;                                   // a -= mean
    case V_CG_XR: a[i] += sc[S_ALPHA] * c[i]; b[i] -= sc[S_ALPHA] * d[i]; break;   // x += alpha p; r -= alpha q
    case V_JACOBI: a[i] = c[i] * d[i]; break;                                  // z = r .* dinv
    case V_CG_P: a[i] = c[i] + sc[S_BETA] * a[i]; break;                       // p = z + beta p
    case V_BI_P: a[i] = c[i] + sc[S_BETA] * (a[i] - sc[S_OMEGA] * d[i]); break;  // p = r + beta (p - omega v)
    case V_BI_S: a[i] = c[i] - sc[S_ALPHA] * d[i]; break;                      // s = r - alpha v
    case V_COPY: a[i] = c[i]; break;
    case V_COPY_SHIFT: a[i] = c[i] - sc[S_MEAN]; break;                        // copy and shift in one pass
  }
}

// dst[i * stride] = src[i] - mean: the solution made orthogonal to the constants on its way into the vertex records
__global__ void scatter_shift_kernel(const double* __restrict__ src, double* __restrict__ dst, int n, int stride,
                                     const double* __restrict__ sc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[(size_t)i * stride] = src[i] - sc[S_MEAN];
}

// dinv != NULL: p, s are the unpreconditioned directions (Jacobi applied here); else they are M^-1 p, M^-1 s
__global__ void bicg_update_kernel(int n, const double* __restrict__ sc, double* __restrict__ x, double* __restrict__ r,
                                   const double* __restrict__ p, const double* __restrict__ s, const double* __restrict__ sres,
                                   const double* __restrict__ t, const double* __restrict__ dinv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double d = dinv ? dinv[i] : 1.0;
  x[i] += sc[S_ALPHA] * (p[i] * d) + sc[S_OMEGA] * (s[i] * d);
  r[i] = sres[i] - sc[S_OMEGA] * t[i];
}

// KNP unknowns: `csol` is ion-major over the global vertex numbering ([k][g]); the solver works in the
// reference's block order [sub-domain][ion][vertex] (pdeSolver.py:117).  to_blocks: x = csol, else csol = x.
__global__ void knp_order_kernel(int ntot, int ks, int n_sub, const KnConsts* __restrict__ Cp, double* __restrict__ x,
                                 double* __restrict__ csol, int to_blocks) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ks * ntot) return;
  const int k = i / ntot, g = i - k * ntot;
  int sd = 0;
  for (int t = 1; t < n_sub; ++t) sd += g >= Cp->voff[t];
  const int v0 = Cp->voff[sd], nv = Cp->voff[sd + 1] - v0;
  const size_t xb = (size_t)ks * v0 + (size_t)k * nv + (g - v0);
  if (to_blocks) x[xb] = csol[i];
  else csol[i] = x[xb];
}

// cur <- 2 cur - old (linear extrapolation of the last two solutions), old <- the value cur had; `have` = 0: only store.
// have >= 2 with old2 != NULL: quadratic extrapolation 3 cur - 3 old + old2 through the last three solutions.
__global__ void extrapolate_kernel(int n, double* __restrict__ cur, int stride, double* __restrict__ old, double* __restrict__ old2,
                                   int have) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double c = cur[(size_t)i * stride];
  if (have >= 2 && old2) cur[(size_t)i * stride] = 3.0 * (c - old[i]) + old2[i];
  else if (have >= 1) cur[(size_t)i * stride] = 2.0 * c - old[i];
  if (old2) old2[i] = old[i];
  old[i] = c;
}

// ---- coarse space of the distributed EMI preconditioner ---------------------------------------------------------
// Coarse functions (knpemi_set_distributed_coarse): per rank and sub-domain the k + 1 hat functions over k slices of the
// owned vertices' extent along its longest axis (piecewise linear along the axis, a partition of unity on the owned
// vertices; the two half hats that meet at a cut between ranks are separate functions, so the space contains the
// continuous piecewise-linear functions across the cuts).  agg_of[i] = the lower node of unknown i (-1: ghost), agg_w[i]
// its weight in the upper node; per node the list of its unknowns and their weights (agg_ptr / agg_idx / agg_wt).
// restriction: one workgroup per local node sums the weighted r over its list in a fixed order (reproducible) and writes
// its entry of the coarse vector in the reduction buffer; the all-reduce fills in the other ranks' entries.
__global__ __launch_bounds__(256) void coarse_restrict_kernel(const double* __restrict__ r, const int* __restrict__ agg_ptr,
                                                              const int* __restrict__ agg_idx, const double* __restrict__ agg_wt,
                                                              int nl, int rank, int world, double* __restrict__ red) {
  __shared__ double sh[256];
  const int a = blockIdx.x;
  double acc = 0.0;
  for (int t = agg_ptr[a] + threadIdx.x; t < agg_ptr[a + 1]; t += 256) acc += agg_wt[t] * r[agg_idx[t]];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int m = 128; m > 0; m >>= 1) {
    if ((int)threadIdx.x < m) sh[threadIdx.x] += sh[threadIdx.x + m];
    __syncthreads();
  }
  if (threadIdx.x == 0) red[KN_COARSE_OFF + rank * nl + a] = sh[0];
  if (a == 0)   // the other ranks' entries start from zero
    for (int j = threadIdx.x; j < world * nl; j += 256)
      if (j / nl != rank) red[KN_COARSE_OFF + j] = 0.0;
}

// z_c = A_c^+ r_c, this rank's rows only
__global__ void coarse_solve_kernel(const double* __restrict__ inv, const double* __restrict__ red, int nl, int rank, int nc,
                                    double* __restrict__ zc) {
  const int a = threadIdx.x;
  if (a >= nl) return;
  const double* row = inv + (size_t)(rank * nl + a) * nc;
  double v = 0.0;
  for (int j = 0; j < nc; ++j) v += row[j] * red[KN_COARSE_OFF + j];
  zc[a] = v;
}

// prolongation: z += (1 - w) z_c[node] + w z_c[node + 1] on the owned unknowns (mode 0); mode 1: z = coarse function `pick`
__global__ void coarse_prolong_kernel(int n, const int* __restrict__ agg_of, const double* __restrict__ agg_w,
                                      const double* __restrict__ zc, double* __restrict__ z, int mode, int pick) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int a = agg_of[i];
  const double w = a >= 0 ? agg_w[i] : 0.0;
  // w == 0 (one node per rank and sub-domain, or a vertex on the lower node itself): zc[a + 1] may lie past the nl entries
  // coarse_solve_kernel writes -- it must not be read, 0 * (stale NaN) would poison z
  if (mode == 0) { if (a >= 0) z[i] += w > 0.0 ? (1.0 - w) * zc[a] + w * zc[a + 1] : zc[a]; }
  else z[i] = a < 0 ? 0.0 : (a == pick ? 1.0 - w : (a + 1 == pick ? w : 0.0));
}

struct Ctx {
  KnSolver& sv;
  int n;
  const int* rowptr; const int* colind; const double* vals;
  double* sc; double* partial;
  // partitioned problem (knpemi_set_distributed): mask of owned unknowns of this system, which system
  const uint8_t* owned = nullptr;
  int which = 0;
  int comm_rc = 0;     // first failure of a communication hook
  int lpr = 16;        // lanes per row of the SpMV (spmv_lanes)
};

// lanes per row from the average row length (read once per system and handle)
int spmv_lanes(KnSolver& sv, int which, const int* rowptr, int n) {
  int& l = sv.spmv_lpr[which == KNPEMI_B_KNP ? 1 : 0];
  if (l == 0) {
    int nnz = 0;
    if (hipMemcpy(&nnz, rowptr + n, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return 16;
    l = n > 0 && nnz / n <= 24 ? 4 : 16;
  }
  return l;
}

inline dim3 grid1(int n) { return dim3((n + 255) / 256); }

// The launches of the plain kernels, on a stream and plain arguments: the solves below call them through their Ctx, and
// knpemi_debug_linalg calls them on a caller's arrays, so the geometry a test sees is the geometry a solve runs.

// lpr: 4, else 16 lanes per row
void spmv_launch(hipStream_t st, int n, int lpr, const int* rowptr, const int* colind, const double* vals, const double* x,
                 const double* dinv, double* y, const double* b, const uint8_t* owned, double* dinv_out) {
  dim3 g(((size_t)n * lpr + 255) / 256);
  if (lpr == 4) {
    if (dinv) hipLaunchKernelGGL((spmv_kernel<true, 4>), g, dim3(256), 0, st, n, rowptr, colind, vals, x, dinv, y,
                                 (const double*)nullptr, owned);
    else hipLaunchKernelGGL((spmv_kernel<false, 4>), g, dim3(256), 0, st, n, rowptr, colind, vals, x, dinv, y, b,
                            owned, dinv_out);
    return;
  }
  if (dinv) hipLaunchKernelGGL((spmv_kernel<true, 16>), g, dim3(256), 0, st, n, rowptr, colind, vals, x, dinv, y,
                               (const double*)nullptr, owned);
  else hipLaunchKernelGGL((spmv_kernel<false, 16>), g, dim3(256), 0, st, n, rowptr, colind, vals, x, dinv, y, b,
                          owned, dinv_out);
}

// partial: 3 * RED_BLOCKS partial sums and, behind them, the ticket counter (zero before the first launch)
void dots_launch(hipStream_t st, int n, int nd, const double* a0, const double* b0, const double* a1, const double* b1,
                 const double* a2, const double* b2, double* partial, double* sc, int op, int d0, int d1, int d2, double scale,
                 double* red) {
  // 16 entries per thread: every block costs ~50 ns at the ticket counter, whatever it sums
  const int nb = std::min(RED_BLOCKS, (n + 16 * RED_THREADS - 1) / (16 * RED_THREADS));
  hipLaunchKernelGGL(dots_kernel, dim3(nb), dim3(RED_THREADS), 0, st, n, nd, a0, b0, a1, b1, a2, b2, partial,
                     reinterpret_cast<unsigned*>(partial + 3 * RED_BLOCKS), sc, op, d0, d1, d2, scale, red);
}

void dots_apply_launch(hipStream_t st, double* sc, const double* red, int op, int nd, int d0, int d1, int d2, double scale) {
  hipLaunchKernelGGL(dots_apply_kernel, dim3(1), dim3(1), 0, st, sc, red, op, nd, d0, d1, d2, scale);
}

void mask_launch(hipStream_t st, int n, const uint8_t* owned, double* a, int as_ones) {
  hipLaunchKernelGGL(mask_kernel, grid1(n), dim3(256), 0, st, n, owned, a, as_ones);
}

void vec_launch(hipStream_t st, int n, int op, const double* sc, double* a, double* b, const double* cc, const double* d) {
  hipLaunchKernelGGL(vec_kernel, grid1(n), dim3(256), 0, st, n, op, sc, a, b, cc, d, (const double*)nullptr);
}

void ghost_identity_launch(hipStream_t st, int n, const int* rowptr, const int* colind, const uint8_t* owned, double* vals) {
  hipLaunchKernelGGL(ghost_identity_kernel, grid1(n), dim3(256), 0, st, n, rowptr, colind, owned, vals);
}

void diag_inv_launch(hipStream_t st, int n, const int* rowptr, const int* colind, const double* vals, double* dinv) {
  hipLaunchKernelGGL(diag_inv_kernel, grid1(n), dim3(256), 0, st, n, rowptr, colind, vals, dinv);
}

void scatter_shift_launch(hipStream_t st, const double* src, double* dst, int n, int stride, const double* sc) {
  hipLaunchKernelGGL(scatter_shift_kernel, grid1(n), dim3(256), 0, st, src, dst, n, stride, sc);
}

void bicg_update_launch(hipStream_t st, int n, const double* sc, double* x, double* r, const double* p, const double* s,
                        const double* sres, const double* t, const double* dinv) {
  hipLaunchKernelGGL(bicg_update_kernel, grid1(n), dim3(256), 0, st, n, sc, x, r, p, s, sres, t, dinv);
}

void knp_order_launch(hipStream_t st, int ntot, int ks, int n_sub, const KnConsts* consts, double* x, double* csol, int to_blocks) {
  hipLaunchKernelGGL(knp_order_kernel, grid1(ks * ntot), dim3(256), 0, st, ntot, ks, n_sub, consts, x, csol, to_blocks);
}

void extrapolate_launch(hipStream_t st, int n, double* cur, int stride, double* old, double* old2, int have) {
  hipLaunchKernelGGL(extrapolate_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, cur, stride, old, old2, have);
}

void coarse_restrict_launch(hipStream_t st, const double* r, const int* agg_ptr, const int* agg_idx, const double* agg_wt, int nl,
                            int rank, int world, double* red) {
  hipLaunchKernelGGL(coarse_restrict_kernel, dim3(nl), dim3(256), 0, st, r, agg_ptr, agg_idx, agg_wt, nl, rank, world, red);
}

void coarse_solve_launch(hipStream_t st, const double* inv, const double* red, int nl, int rank, int nc, double* zc) {
  hipLaunchKernelGGL(coarse_solve_kernel, dim3(1), dim3(KN_COARSE_MAX), 0, st, inv, red, nl, rank, nc, zc);
}

void coarse_prolong_launch(hipStream_t st, int n, const int* agg_of, const double* agg_w, const double* zc, double* z, int mode,
                           int pick) {
  hipLaunchKernelGGL(coarse_prolong_kernel, grid1(n), dim3(256), 0, st, n, agg_of, agg_w, zc, z, mode, pick);
}

void spmv(Ctx& c, const double* x, double* y, const double* dinv, const double* b = nullptr, double* dinv_out = nullptr) {
  if (c.owned) {   // the argument's ghost entries take their owners' values first
    const KnDist& d = c.sv.dist;
    if (int e = d.halo(d.ctx, const_cast<double*>(x), c.which)) c.comm_rc = c.comm_rc ? c.comm_rc : e;
  }
  if (c.sv.bcols.bcol && !dinv && !dinv_out) {   // DG systems: block columns instead of one column index per entry
    launch_block_spmv<double>(c.sv.own->stream, c.sv.bcols, c.n, c.rowptr, c.vals, x, b, y, c.owned);
    return;
  }
  spmv_launch(c.sv.own->stream, c.n, c.lpr, c.rowptr, c.colind, c.vals, x, dinv, y, b, c.owned, dinv_out);
}

void dots(Ctx& c, int nd, const double* a0, const double* b0, const double* a1, const double* b1, const double* a2,
          const double* b2, int op, int d0 = 0, int d1 = 0, int d2 = 0, double scale = 1.0) {
  double* red = c.owned ? c.sv.dist.d_red : nullptr;
  dots_launch(c.sv.own->stream, c.n, nd, a0, b0, a1, b1, a2, b2, c.partial, c.sc, op, d0, d1, d2, scale, red);
  if (red) {   // every vector is zero on its ghost entries, so the local sums run over the owned unknowns only
    const KnDist& d = c.sv.dist;
    if (int e = d.allreduce(d.ctx, nd)) c.comm_rc = c.comm_rc ? c.comm_rc : e;
    dots_apply_launch(c.sv.own->stream, c.sc, red, op, nd, d0, d1, d2, scale);
  }
}

void mask(const Ctx& c, double* a, int as_ones = 0) {
  if (c.owned) mask_launch(c.sv.own->stream, c.n, c.owned, a, as_ones);
}

void vec(const Ctx& c, int op, double* a, double* b, const double* cc, const double* d) {
  vec_launch(c.sv.own->stream, c.n, op, c.sc, a, b, cc, d);
}

// the solver's scalars on the host: through a pinned buffer (a copy into pageable memory is staged by the runtime)
int read_scalars(const Ctx& c, double* host, int count) {
  KnSolver& sv = c.sv;
  if (!sv.kry_pinned) KN_HIP(hipHostMalloc(&sv.kry_pinned, 64 * sizeof(double), hipHostMallocDefault));
  KN_HIP(hipMemcpyAsync(sv.kry_pinned, c.sc, count * sizeof(double), hipMemcpyDeviceToHost, sv.own->stream));
  KN_HIP(hipStreamSynchronize(sv.own->stream));
  for (int i = 0; i < count; ++i) host[i] = static_cast<double*>(sv.kry_pinned)[i];
  return KNPEMI_OK;
}

// BiCGStab start: p = v = 0, rho = alpha = omega = 1, everything else 0 (one launch instead of two fills and a copy)
__global__ void bicg_init_kernel(int n, double* __restrict__ p, double* __restrict__ v, double* __restrict__ sc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { p[i] = 0.0; v[i] = 0.0; }
  if (i < S_N) sc[i] = (i == S_RHO || i == S_ALPHA || i == S_OMEGA) ? 1.0 : 0.0;
}

void bicg_init_launch(hipStream_t st, int n, double* p, double* v, double* sc) {
  hipLaunchKernelGGL(bicg_init_kernel, grid1(std::max(n, (int)S_N)), dim3(256), 0, st, n, p, v, sc);
}

// Run `chunk` iterations of `body`: captured once into a hipGraph (the launch-bound inner loop of small
// systems: ~20 launches of a few microseconds per iteration) and replayed; the graph is keyed on everything its
// kernel arguments depend on.  KNPEMI_NO_GRAPH=1 launches the kernels directly.
template <class Body>
int run_chunk(KnSolver& sv, KnSolver::KnGraph& g, uint64_t key, int chunk, Body&& body) {
  static const bool no_graph_env = getenv("KNPEMI_NO_GRAPH") != nullptr;
  auto loop = [&]() -> int {
    int rc = KNPEMI_OK;
    for (int k = 0; k < chunk && !rc; ++k) rc = body();
    return rc;
  };
  if (no_graph_env || sv.dist.on) return loop();   // the communication hooks cannot be captured
  if (!g.exec || g.key != key) {
    if (g.exec) { (void)hipGraphExecDestroy(g.exec); g.exec = nullptr; }
    if (int rc = kn_capture(sv, loop, &g.exec)) return rc;
    g.key = key;
  }
  KN_HIP(hipGraphLaunch(g.exec, sv.own->stream));
  return KNPEMI_OK;
}

// KNPEMI_NO_FUSED=1: the plain loops (one launch per operation) instead of kernels_fused.hip
inline bool use_fused() {
  static const bool off = getenv("KNPEMI_NO_FUSED") != nullptr;
  return !off;
}

// KNPEMI_AMG_REBUILD_EVERY=k (test hook): the hierarchy is declared aged at every k-th solve of its system
inline int rebuild_every() {
  static const int k = getenv("KNPEMI_AMG_REBUILD_EVERY") ? atoi(getenv("KNPEMI_AMG_REBUILD_EVERY")) : 0;
  return k;
}

inline bool debug_krylov() {
  static const bool on = getenv("KNPEMI_DEBUG_KRYLOV") != nullptr;
  return on;
}

inline uint64_t graph_key(const KnSolver& sv, const KnAmg& G, bool amg, int chunk, int n) {
  uint64_t k = reinterpret_cast<uint64_t>(sv.kry);
  k = k * 1000003u + (uint64_t)G.builds;
  k = k * 1000003u + (amg ? 1u : 0u);
  k = k * 1000003u + (uint64_t)chunk;
  k = k * 1000003u + (uint64_t)n;
  return k | 1u;
}

// the solver's scalars for an error message
std::string describe_scalars(const double* sc, int it) {
  char buf[320];
  snprintf(buf, sizeof buf,
           "[iteration %d: |r|^2 = %.6e, |b|^2 = %.6e, rho = %.6e, alpha = %.6e, beta = %.6e, omega = %.6e, rhat.v = %.6e, "
           "t.s = %.6e, t.t = %.6e, p.Ap = %.6e, breakdown flags = %d]",
           it, sc[S_RR], sc[S_BB], sc[S_RHO], sc[S_ALPHA], sc[S_BETA], sc[S_OMEGA], sc[S_RV], sc[S_TS], sc[S_TT], sc[S_PAP],
           (int)sc[S_FLAG]);
  return buf;
}

// A solve that starts from non-finite data is an input error, not a breakdown: say which operand it is before the first
// iteration has overwritten the iterate (|b| from the right-hand side alone; |r0| = |b - A x0| brings in the matrix and
// the initial guess).
int check_start(const char* who, const double* sc) {
  if (!std::isfinite(sc[S_BB])) {
    kn_set_error(std::string(who) + ": the right-hand side contains non-finite values");
    return KNPEMI_EINVAL;
  }
  if (!std::isfinite(sc[S_RR])) {
    kn_set_error(std::string(who) + ": the initial residual b - A x0 is not finite (matrix values or initial guess)");
    return KNPEMI_EINVAL;
  }
  return KNPEMI_OK;
}

// Hierarchy upkeep at the head of an AMG-preconditioned solve: the first build (also after a size change, and on a
// partitioned problem once the hierarchy has aged), else the background rebuild of an aged one; then the block inverses
// of the finest level.  `owned`: the rank's mask of the system's unknowns (partitioned problems).
int amg_upkeep(KnSolver& sv, KnAmg& G, int n, const int* rowptr, const int* colind, const double* vals, bool singular,
               const std::vector<uint8_t>& owned) {
  const KnDist& dist = sv.dist;
  int rc;
  if (!G.built || G.n != n) {
    KnAmgConfig& C = G.cfg;   // the owner's choices, and what follows from the partition
    C.negative_strength = true;
    C.want_fused = !dist.on && use_fused();
    C.want_cycle = dist.on && use_fused() && !getenv("KNPEMI_DIST_PLAIN_CYCLE");
    if ((rc = kn_amg_setup(sv, G, n, rowptr, colind, vals, singular, dist.on ? owned.data() : nullptr))) return rc;
    G.its_ref = -1;
    ++G.builds;
  } else if (!dist.on) {
    if (rebuild_every() > 0 && ++G.solves % rebuild_every() == 0) G.rebuild_wanted = true;
    if (G.rebuild_wanted && (rc = kn_amg_rebuild_step(sv, G, n, rowptr, colind, vals, singular))) return rc;
  }
  return kn_amg_refresh(sv, G, vals);
}

// frozen hierarchy: rebuild at the next solve once it has visibly aged (`it`: iterations of the solve just finished)
void amg_age(KnSolver& sv, KnAmg& G, int it) {
  if (G.its_ref < 0) G.its_ref = it;
  else if (it > 2 * G.its_ref + 4) { if (sv.dist.on) G.built = false; else G.rebuild_wanted = true; }
}

}  // namespace

int kn_capture(KnSolver& sv, const std::function<int()>& enqueue, hipGraphExec_t* out) {
  *out = nullptr;
  hipGraph_t graph = nullptr;
  KN_HIP(hipStreamBeginCapture(sv.own->stream, hipStreamCaptureModeThreadLocal));
  const int rc = enqueue();
  hipError_t e = hipStreamEndCapture(sv.own->stream, &graph);
  if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
  if (e != hipSuccess) { kn_set_error(std::string("hipStreamEndCapture: ") + hipGetErrorString(e)); return KNPEMI_EHIP; }
  e = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e != hipSuccess) { *out = nullptr; kn_set_error(std::string("hipGraphInstantiate: ") + hipGetErrorString(e)); return KNPEMI_EHIP; }
  return KNPEMI_OK;
}

void kn_solver_free(KnSolver& sv) {
  if (sv.own->stream) (void)hipStreamSynchronize(sv.own->stream);   // nothing in flight replays a graph or publishes its state
  for (KnAmg* G : {&sv.amg_emi, &sv.amg_knp}) {
    kn_amg_async_join(*G);
    kn_amg_free(*G);
  }
  if (sv.kry_pinned) (void)hipHostFree(sv.kry_pinned);
  if (sv.pub_host) (void)hipHostFree(sv.pub_host);
  kn_fused_graphs_free(sv);
  for (KnSolver::KnGraph* g : {&sv.graph_emi, &sv.graph_knp})
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
}

int kn_dist_enable(KnSolver& sv, const uint8_t* owned_emi, std::vector<uint8_t>&& owned_knp, void* reduce_buf_dev,
                   knpemi_allreduce_fn allreduce, knpemi_halo_fn halo, void* ctx, const char* who) {
  KnDist& d = sv.dist;
  sv.amg_emi.built = false;      // the preconditioner changes with the ownership
  sv.amg_knp.built = false;
  if (!owned_emi) { d.on = false; return KNPEMI_OK; }
  if (!reduce_buf_dev || !allreduce || !halo)
    return kn_fail(KNPEMI_EINVAL, std::string(who) + ": reduction buffer and both communication hooks are required");
  const int n = sv.emi.n;
  hipStream_t st = sv.own->stream;
  d.h_owned_emi.assign(owned_emi, owned_emi + n);
  d.h_owned_knp = std::move(owned_knp);
  int rc;
  if ((rc = kn_upload(sv.own->allocs, d.h_owned_emi, &d.d_owned_emi))) return rc;
  if ((rc = kn_upload(sv.own->allocs, d.h_owned_knp, &d.d_owned_knp))) return rc;
  d.d_red = static_cast<double*>(reduce_buf_dev);
  d.allreduce = allreduce; d.halo = halo; d.ctx = ctx;
  // number of owned unknowns of the EMI system over all ranks (mean of the constant null space)
  double cnt = 0.0;
  for (int i = 0; i < n; ++i) cnt += owned_emi[i] ? 1.0 : 0.0;
  KN_HIP(hipMemcpyAsync(d.d_red, &cnt, sizeof(double), hipMemcpyHostToDevice, st));
  if (allreduce(ctx, 1)) return kn_fail(KNPEMI_EHIP, std::string(who) + ": allreduce hook failed");
  KN_HIP(hipMemcpyAsync(&cnt, d.d_red, sizeof(double), hipMemcpyDeviceToHost, st));
  KN_HIP(hipStreamSynchronize(st));
  d.n_owned_global = cnt;
  d.on = true;
  return KNPEMI_OK;
}

// Workspace: 10 vectors of the larger system + ones + scalars + partials (allocated on first use).
static int ensure_work(KnSolver& sv, size_t n) {
  if (sv.kry_n >= n) return KNPEMI_OK;
  const size_t doubles = 11 * n + 64 + 3 * RED_BLOCKS + 2;   // + ticket counter of dots_kernel
  if (int rc = kn_zeros(sv.own->allocs, sv.own->stream, doubles, &sv.kry)) return rc;
  sv.kry_n = n;
  const std::vector<double> ones(n, 1.0);
  return kn_to_device(sv.own->stream, sv.kry + 10 * n, ones.data(), n);
}

// r_c = Phi^T r into the reduction buffer (all-reduced): every rank ends up with the whole coarse vector
static void coarse_restrict(Ctx& c, const double* r) {
  KnSolver& sv = c.sv;
  KnDist& d = sv.dist;
  coarse_restrict_launch(sv.own->stream, r, d.d_agg_ptr, d.d_agg_idx, d.d_agg_wt, d.nl, d.rank, d.world, d.d_red);
  if (int e = d.allreduce(d.ctx, KN_COARSE_OFF + d.nc)) c.comm_rc = c.comm_rc ? c.comm_rc : e;
}

// Coarse operator A_c = Phi^T A Phi of the partitioned EMI system (one column per coarse function: an SpMV of it and a
// restriction), then on the host the inverse of A_c + alpha 1 1^T (A_c has the constants in its kernel;
// the residuals it is applied to have zero mean) with empty aggregates decoupled.
static int coarse_setup(Ctx& c, double* work_phi, double* work_y) {
  KnSolver& sv = c.sv;
  KnDist& d = sv.dist;
  const int nc = d.nc, nl = d.nl;
  if (!d.d_coarse_inv) {
    int rc;
    if ((rc = kn_alloc(sv.own->allocs, (size_t)KN_COARSE_MAX * KN_COARSE_MAX, &d.d_coarse_inv))) return rc;
    if ((rc = kn_alloc(sv.own->allocs, KN_COARSE_MAX + 1, &d.d_coarse_z))) return rc;
    // (KNPEMI_DEBUG_POISON_COARSE: all-ones bytes = NaN, for the test that no entry past the nl written ones is read)
    KN_HIP(hipMemset(d.d_coarse_z, getenv("KNPEMI_DEBUG_POISON_COARSE") ? 0xFF : 0, (KN_COARSE_MAX + 1) * sizeof(double)));
  }
  std::vector<double> Ac((size_t)nc * nc, 0.0), col(nc);
  for (int j = 0; j < nc; ++j) {
    const int rj = j / nl, aj = j % nl;
    // phi_j: 1 on the owned unknowns of aggregate aj of rank rj (ghost copies are filled by the SpMV's halo), 0 elsewhere
    coarse_prolong_launch(sv.own->stream, c.n, d.d_agg_of, d.d_agg_w, nullptr, work_phi, 1, rj == d.rank ? aj : -2);
    spmv(c, work_phi, work_y, nullptr);
    coarse_restrict(c, work_y);
    if (int rc = kn_to_host(sv.own->stream, col.data(), d.d_red + KN_COARSE_OFF, nc)) return rc;
    if (c.comm_rc) { kn_set_error("coarse space set-up: a communication hook failed"); return KNPEMI_EHIP; }
    for (int i = 0; i < nc; ++i) Ac[(size_t)i * nc + j] = col[i];
  }
  // symmetrise (rounding), decouple empty aggregates, shift the constants' kernel, invert (Gauss-Jordan, nc <= 64)
  double tr = 0.0;
  for (int i = 0; i < nc; ++i) tr += Ac[(size_t)i * nc + i];
  const double alpha = tr > 0 ? tr / ((double)nc * nc) : 1.0;
  std::vector<double> M((size_t)nc * nc), inv((size_t)nc * nc, 0.0);
  std::vector<char> empty(nc, 0);
  for (int i = 0; i < nc; ++i) empty[i] = !(Ac[(size_t)i * nc + i] > 0.0);
  for (int i = 0; i < nc; ++i)
    for (int j = 0; j < nc; ++j) {
      double v = 0.5 * (Ac[(size_t)i * nc + j] + Ac[(size_t)j * nc + i]);
      if (empty[i] || empty[j]) v = i == j ? 1.0 : 0.0;
      else v += alpha;
      M[(size_t)i * nc + j] = v;
    }
  for (int i = 0; i < nc; ++i) inv[(size_t)i * nc + i] = 1.0;
  for (int k = 0; k < nc; ++k) {
    int piv = k;
    for (int i = k + 1; i < nc; ++i) if (std::fabs(M[(size_t)i * nc + k]) > std::fabs(M[(size_t)piv * nc + k])) piv = i;
    if (!(std::fabs(M[(size_t)piv * nc + k]) > 0.0)) { kn_set_error("coarse space set-up: singular coarse operator"); return KNPEMI_EINVAL; }
    if (piv != k)
      for (int j = 0; j < nc; ++j) { std::swap(M[(size_t)k * nc + j], M[(size_t)piv * nc + j]); std::swap(inv[(size_t)k * nc + j], inv[(size_t)piv * nc + j]); }
    const double dk = 1.0 / M[(size_t)k * nc + k];
    for (int j = 0; j < nc; ++j) { M[(size_t)k * nc + j] *= dk; inv[(size_t)k * nc + j] *= dk; }
    for (int i = 0; i < nc; ++i) {
      if (i == k) continue;
      const double f = M[(size_t)i * nc + k];
      if (f == 0.0) continue;
      for (int j = 0; j < nc; ++j) { M[(size_t)i * nc + j] -= f * M[(size_t)k * nc + j]; inv[(size_t)i * nc + j] -= f * inv[(size_t)k * nc + j]; }
    }
  }
  for (int i = 0; i < nc; ++i)
    if (empty[i]) for (int j = 0; j < nc; ++j) inv[(size_t)i * nc + j] = inv[(size_t)j * nc + i] = 0.0;   // nothing to correct there
  KN_HIP(hipMemcpy(d.d_coarse_inv, inv.data(), inv.size() * sizeof(double), hipMemcpyHostToDevice));
  d.coarse_built = true;
  return KNPEMI_OK;
}

// z += Phi A_c^+ Phi^T r  (additive two-level correction next to the per-rank AMG)
static void coarse_correct(Ctx& c, const double* r, double* z) {
  KnSolver& sv = c.sv;
  KnDist& d = sv.dist;
  coarse_restrict(c, r);
  coarse_solve_launch(sv.own->stream, d.d_coarse_inv, d.d_red, d.nl, d.rank, d.nc, d.d_coarse_z);
  coarse_prolong_launch(sv.own->stream, c.n, d.d_agg_of, d.d_agg_w, d.d_coarse_z, z, 0, 0);
}

// Jacobi-PCG on A_emi x = b_emi, x = phi (KnSolver::phi: a component of the records, gathered into a contiguous vector first).
int kn_solve_emi(KnSolver& sv, double rtol, double atol, int maxit, int* iters, double* relres) {
  const KnSysView& D = sv.emi;
  const int n = D.n;
  sv.phi_stored = false;
  int rc = ensure_work(sv, (size_t)std::max(1, sv.ks) * D.n);
  if (rc) return rc;
  const size_t N = sv.kry_n;
  double *x = sv.kry, *r = x + N, *z = r + N, *p = z + N, *q = p + N, *b = q + N, *dinv = b + N, *ones = sv.kry + 10 * N;
  Ctx c{sv, n, D.rowptr, D.colind, D.A, sv.kry + 11 * N, sv.kry + 11 * N + 64};
  c.lpr = spmv_lanes(sv, KNPEMI_B_EMI, D.rowptr, n);
  const KnDist& dist = sv.dist;
  bool has_ghosts = false;
  double n_mean = (double)n;
  if (dist.on) {   // partitioned problem: this rank's rows of the global system
    c.owned = dist.d_owned_emi;
    c.which = KNPEMI_B_EMI;
    n_mean = dist.n_owned_global;
    for (uint8_t o : dist.h_owned_emi) has_ghosts |= !o;
    ghost_identity_launch(sv.own->stream, n, c.rowptr, c.colind, c.owned, D.A);
  }
  if (sv.kry_ones_masked != (dist.on ? 1 : 0)) {   // `ones` counts the owned unknowns
    if (dist.on) mask(c, ones, 1);
    else {
      std::vector<double> one(n, 1.0);
      KN_HIP(hipMemcpy(ones, one.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    }
    sv.kry_ones_masked = dist.on ? 1 : 0;
  }
  // x0 = current phi (ksp_initial_guess_nonzero), b = b_emi projected onto zero mean (constant null space).  With the
  // fused loop these launches open the captured graph of the solve's first chunk (kernels_fused.hip), hence the lambda.
  auto pre = [&]() -> int {
    if (int e = kn_launch_field_gather(sv.own->stream, sv.phi, sv.phi_stride, x, n)) return e;
    if (dist.on) {
      vec(c, V_COPY, b, nullptr, D.b, nullptr);
      mask(c, b);
      dots(c, 1, b, ones, nullptr, nullptr, nullptr, nullptr, OP_MEAN, 0, 0, 0, 1.0 / n_mean);
      vec(c, V_SHIFT, b, nullptr, nullptr, nullptr);
      mask(c, b);
    } else {   // single rank: the mean of b_emi itself, then copy and shift in one pass (same arithmetic)
      dots(c, 1, D.b, ones, nullptr, nullptr, nullptr, nullptr, OP_MEAN, 0, 0, 0, 1.0 / n_mean);
      vec(c, V_COPY_SHIFT, b, nullptr, D.b, nullptr);
    }
    // (single rank: the inverse diagonal comes out of the first residual below)
    if (dist.on) diag_inv_launch(sv.own->stream, n, c.rowptr, c.colind, c.vals, dinv);
    return KNPEMI_OK;
  };
  // solution orthogonal to constants, then into the phi component of the vertex records (ghosts included: they take
  // their owners' values first); idempotent
  auto post = [&]() -> int {
    dots(c, 1, x, ones, nullptr, nullptr, nullptr, nullptr, OP_MEAN, 0, 0, 0, 1.0 / n_mean);
    if (dist.on) {
      if (int e = dist.halo(dist.ctx, x, KNPEMI_B_EMI)) c.comm_rc = c.comm_rc ? c.comm_rc : e;
      vec(c, V_SHIFT, x, nullptr, nullptr, nullptr);
      if (int e = kn_launch_field_scatter(sv.own->stream, x, sv.phi, n, sv.phi_stride)) return e;
    } else if (n > 0) {
      scatter_shift_launch(sv.own->stream, x, sv.phi, n, sv.phi_stride, c.sc);
    }
    return KNPEMI_OK;
  };
  KnAmg& G = sv.amg_emi;
  const bool amg = sv.pc_emi == KNPEMI_PC_AMG;
  // (the diagonal block of a rank that has ghosts has lost couplings: it is non-singular)
  if (amg && (rc = amg_upkeep(sv, G, n, D.rowptr, D.colind, D.A, !has_ghosts, dist.h_owned_emi))) return rc;
  // two-level variant on a partitioned mesh: the ranks' AMG cycles do not see each other, a coarse space of one
  // constant per (rank, sub-domain) carries the error across the cuts (knpemi_set_distributed_coarse)
  const bool coarse = dist.on && amg && sv.dist.nc > 0;
  if (coarse && (!sv.dist.coarse_built || G.its_ref < 0)) {
    if ((rc = coarse_setup(c, p, q))) return rc;               // p, q are free before the first search direction
  }
  auto precond = [&]() -> int {
    if (amg) {
      int e = kn_amg_apply(sv, G, D.A, dinv, r, q, z);      // q = A p is free here
      if (e) return e;
      if (coarse) coarse_correct(c, r, z);
      return KNPEMI_OK;
    }
    vec(c, V_JACOBI, z, nullptr, r, dinv);
    return KNPEMI_OK;
  };
  const int chunk = amg ? 1 : 8;   // a V-cycle costs ~15 launches: test convergence after every iteration
  double sc[S_N];
  const bool fused = amg && G.fused_ok && !dist.on && use_fused();
  int it = 0;
  if (fused) {   // residual, target and the loop in 2 + (2 levels - 1) launches per iteration (kernels_fused.hip)
    const KnFusedSys S{n, c.rowptr, c.colind, c.vals, c.sc, sv.kry, N};
    if ((rc = kn_fused_cg(sv, G, S, D.b, rtol, atol, maxit, &it, &sc[S_RR], &sc[S_BB]))) return rc;
  } else {
    if ((rc = pre())) return rc;
    spmv(c, x, r, nullptr, b, dist.on ? nullptr : dinv);         // r = b - A x
    dots(c, 2, r, r, b, b, nullptr, nullptr, OP_START);
    if ((rc = read_scalars(c, sc, S_N))) return rc;
    if ((rc = check_start("EMI CG", sc))) return rc;
  }
  const double bnorm = std::sqrt(sc[S_BB]);
  const double target = std::max(atol, rtol * (bnorm > 0 ? bnorm : 1.0));
  double rn = std::sqrt(sc[S_RR]);
  if (!fused && rn > target) {   // the (extrapolated) initial guess is not good enough: first search direction
    if ((rc = precond())) return rc;
    vec(c, V_COPY, p, nullptr, z, nullptr);
    dots(c, 2, r, z, r, r, nullptr, nullptr, OP_CG_INIT);      // r.z, r.r
  }
  auto iteration = [&]() -> int {
    spmv(c, p, q, nullptr);
    dots(c, 1, p, q, nullptr, nullptr, nullptr, nullptr, OP_CG_PAP);
    vec(c, V_CG_XR, x, r, p, q);
    if (int e = precond()) return e;
    dots(c, 2, r, z, r, r, nullptr, nullptr, OP_CG_RHO);
    vec(c, V_CG_P, p, nullptr, z, nullptr);
    return KNPEMI_OK;
  };
  const uint64_t gkey = graph_key(sv, G, amg, chunk, n);
  while (!fused && rn > target && it < maxit) {
    const int todo = std::min(chunk, maxit - it);
    if (todo == chunk) { if ((rc = run_chunk(sv, sv.graph_emi, gkey, chunk, iteration))) return rc; }
    else for (int k = 0; k < todo; ++k) if ((rc = iteration())) return rc;
    it += todo;
    if ((rc = read_scalars(c, sc, S_N))) return rc;
    rn = std::sqrt(sc[S_RR]);
    if (debug_krylov()) fprintf(stderr, "[knpemi] emi cg it %d |r| %.3e target %.3e alpha %.3e beta %.3e\n", it, rn, target, sc[S_ALPHA], sc[S_BETA]);
    if (!std::isfinite(rn)) { kn_set_error("EMI CG broke down (non-finite residual) " + describe_scalars(sc, it)); return KNPEMI_ESOLVE; }
  }
  if (!fused && (rc = post())) return rc;
  if (c.comm_rc) { kn_set_error("EMI solve: a communication hook failed"); return KNPEMI_EHIP; }
  if (iters) *iters = it;
  if (relres) *relres = bnorm > 0 ? rn / bnorm : rn;
  if ((rc = kn_launch_check("krylov (emi)"))) return rc;
  if (amg) amg_age(sv, G, it);
  if (rn > target) { kn_set_error("EMI CG did not converge (ksp_error_if_not_converged)"); return KNPEMI_ESOLVE; }
  return KNPEMI_OK;
}

// Jacobi-BiCGStab on the block-diagonal KNP system; x = c (csol, converted to the block order).
int kn_solve_knp(KnSolver& sv, double rtol, double atol, int maxit, int* iters, double* relres) {
  const KnSysView& D = sv.knp;
  const int n = D.n;
  int rc = ensure_work(sv, (size_t)std::max(1, sv.ks) * sv.emi.n);
  if (rc) return rc;
  if (!D.rowptr) { kn_set_error("KNP monolithic pattern missing"); return KNPEMI_EINVAL; }
  const size_t N = sv.kry_n;
  double *x = sv.kry, *r = x + N, *rhat = r + N, *p = rhat + N, *v = p + N, *s = v + N, *t = s + N, *dinv = t + N;
  double *phat = sv.kry + 8 * N, *shat = sv.kry + 9 * N;
  Ctx c{sv, n, D.rowptr, D.colind, D.A, sv.kry + 11 * N, sv.kry + 11 * N + 64};
  c.lpr = spmv_lanes(sv, KNPEMI_B_KNP, D.rowptr, n);
  const KnDist& dist = sv.dist;
  if (dist.on) {
    c.owned = dist.d_owned_knp;
    c.which = KNPEMI_B_KNP;
    ghost_identity_launch(sv.own->stream, n, c.rowptr, c.colind, c.owned, D.A);
    mask(c, D.b);      // the ghost rows of the right-hand side are not assembled
  }
  // x0 = previous concentrations in the solver's order (first launch of the solve: with the fused loop it opens the
  // captured graph of the first chunk)
  auto pre = [&]() -> int {
    if (sv.knp_load) return sv.knp_load(x);
    vec(c, V_COPY, x, nullptr, sv.csol, nullptr);
    return KNPEMI_OK;
  };
  // the solution back into csol, or wherever the owner takes it; idempotent
  auto post = [&]() -> int {
    if (sv.knp_store) return sv.knp_store(x);
    vec(c, V_COPY, sv.csol, nullptr, x, nullptr);
    return KNPEMI_OK;
  };
  const bool fused_planned = sv.pc_knp == KNPEMI_PC_AMG && !dist.on && use_fused();
  if (!fused_planned && (rc = pre())) return rc;
  KnAmg& G = sv.amg_knp;
  const bool amg = sv.pc_knp == KNPEMI_PC_AMG;
  if (dist.on) {
    diag_inv_launch(sv.own->stream, n, c.rowptr, c.colind, c.vals, dinv);
    // Jacobi: the scaled SpMV A (dinv .* p) reads dinv on ghost columns, where the identity rows above left 1: take the
    // owners' 1 / a_ii instead, so that the recurrence residual stays b - A x (x is updated with the owners' dinv)
    if (!amg) if (int e = dist.halo(dist.ctx, dinv, KNPEMI_B_KNP)) c.comm_rc = c.comm_rc ? c.comm_rc : e;
  }
  if (amg && (rc = amg_upkeep(sv, G, n, D.rowptr, D.colind, D.A, false, dist.h_owned_knp))) return rc;
  double sc[S_N];
  const bool fused = amg && G.fused_ok && !dist.on && use_fused();
  int it = 0, restarts = 0;
  if (fused) {   // residual, target and 3 + 2 cycles launches per iteration (kernels_fused.hip)
    const KnFusedSys S{n, c.rowptr, c.colind, c.vals, c.sc, sv.kry, N};
    if (sv.knp_method == 1) {      // GMRES(30) as PETSc runs the reference's options (KNPEMI_OPT_KNP_METHOD)
      if ((rc = kn_fused_gmres(sv, G, S, D.b, rtol, atol, maxit, &it, &sc[S_RR], &sc[S_BB], pre, post))) return rc;
    } else
    if ((rc = kn_fused_bicgstab(sv, G, S, D.b, rtol, atol, maxit, &it, &sc[S_RR], &sc[S_BB], pre, post))) return rc;
  } else {
    if (fused_planned && (rc = pre())) return rc;      // (the hierarchy did not qualify for the fused loop after all)
    spmv(c, x, r, nullptr, D.b, dist.on ? nullptr : dinv);   // r = b - A x
    vec(c, V_COPY, rhat, nullptr, r, nullptr);
    bicg_init_launch(sv.own->stream, n, p, v, c.sc);
    dots(c, 2, r, r, D.b, D.b, nullptr, nullptr, OP_START);
    if ((rc = read_scalars(c, sc, S_N))) return rc;
    if ((rc = check_start("KNP BiCGStab", sc))) return rc;
  }
  const double bnorm = std::sqrt(sc[S_BB]);
  const double target = std::max(atol, rtol * (bnorm > 0 ? bnorm : 1.0));
  double rn = std::sqrt(sc[S_RR]);
  const int chunk = amg ? 1 : 4;
  auto iteration = [&]() -> int {
    int rc = KNPEMI_OK;

      dots(c, 1, rhat, r, nullptr, nullptr, nullptr, nullptr, OP_BI_RHO);
      vec(c, V_BI_P, p, nullptr, r, v);
      if (amg) {
        if ((rc = kn_amg_apply(sv, G, D.A, dinv, p, t, phat))) return rc;   // t is free here
        spmv(c, phat, v, nullptr);
      } else spmv(c, p, v, dinv);                           // v = A M^-1 p
      dots(c, 1, rhat, v, nullptr, nullptr, nullptr, nullptr, OP_BI_ALPHA);
      vec(c, V_BI_S, s, nullptr, r, v);
      if (amg) {
        if ((rc = kn_amg_apply(sv, G, D.A, dinv, s, t, shat))) return rc;
        spmv(c, shat, t, nullptr);
      } else spmv(c, s, t, dinv);                           // t = A M^-1 s
      dots(c, 2, t, s, t, t, nullptr, nullptr, OP_BI_OMEGA);
      if (amg) bicg_update_launch(sv.own->stream, n, c.sc, x, r, phat, shat, s, t, nullptr);
      else bicg_update_launch(sv.own->stream, n, c.sc, x, r, p, s, s, t, dinv);
      dots(c, 1, r, r, nullptr, nullptr, nullptr, nullptr, OP_STORE3, S_RR);
    return rc;
  };
  const uint64_t gkey = graph_key(sv, G, amg, chunk, n);
  // ksp_min_it (pdeSolver.py:101).  With KNPEMI_OPT_KNP_METHOD = 1 it counts GMRES iterations; where this BiCGStab loop runs
  // instead (partitioned problems, Jacobi preconditioning) an iteration applies operator and preconditioner twice
  const int min_it = std::max(0, std::min(sv.knp_method == 1 ? (sv.knp_min_it + 1) / 2 : sv.knp_min_it, maxit));
  while (!fused && (rn > target || (it < min_it && rn != 0.0)) && it < maxit) {
    const int todo = std::min(chunk, maxit - it);
    if (todo == chunk) { if ((rc = run_chunk(sv, sv.graph_knp, gkey, chunk, iteration))) return rc; }
    else for (int k = 0; k < todo; ++k) if ((rc = iteration())) return rc;
    it += todo;
    if ((rc = read_scalars(c, sc, S_N))) return rc;
    rn = std::sqrt(sc[S_RR]);
    if (!std::isfinite(rn)) {
      kn_set_error("KNP BiCGStab broke down (non-finite residual) " + describe_scalars(sc, it));
      return KNPEMI_ESOLVE;
    }
    const int flag = (int)sc[S_FLAG];
    if ((flag & (F_RHO_ZERO | F_OMEGA_ZERO | F_RV_ZERO)) && rn > target) {
      // a true breakdown (rhat has become orthogonal to the recurrence, or the stabilising step vanished) with a
      // residual left: restart from the current iterate with rhat = r, as PETSc's KSPBCGS does
      if (++restarts > 3) {
        kn_set_error("KNP BiCGStab broke down repeatedly " + describe_scalars(sc, it));
        return KNPEMI_ESOLVE;
      }
      vec(c, V_COPY, rhat, nullptr, r, nullptr);
      bicg_init_launch(sv.own->stream, n, p, v, c.sc);
    }
  }
  if (dist.on) if (int e = dist.halo(dist.ctx, x, KNPEMI_B_KNP)) c.comm_rc = c.comm_rc ? c.comm_rc : e;
  if (c.comm_rc) { kn_set_error("KNP solve: a communication hook failed"); return KNPEMI_EHIP; }
  if (!fused && (rc = post())) return rc;
  if (iters) *iters = it;
  if (relres) *relres = bnorm > 0 ? rn / bnorm : rn;
  if ((rc = kn_launch_check("krylov (knp)"))) return rc;
  if (amg) amg_age(sv, G, it);
  if (rn > target) { kn_set_error("KNP BiCGStab did not converge (ksp_error_if_not_converged)"); return KNPEMI_ESOLVE; }
  return KNPEMI_OK;
}

// x in the reference's block order (pdeSolver.py:117) <-> csol (ion-major over the global vertex numbering)
int kn_launch_knp_order(knpemi_handle* h, double* x, int to_blocks) {
  const KnDev& D = h->dev;
  const int n = (h->K - 1) * D.Ntot;
  if (n == 0) return KNPEMI_OK;
  knp_order_launch(h->stream, D.Ntot, h->K - 1, h->n_sub, h->d_consts, x, D.csol, to_blocks);
  return kn_launch_check("knp_order_kernel");
}

// Initial guess of the next solve: instead of the previous solution (ksp_initial_guess_nonzero) the extrapolation of the
// last solutions -- 3 x_n - 3 x_(n-1) + x_(n-2) once three are known, 2 x_n - x_(n-1) before -- written into phi / csol
// in place.  Only the starting point changes; the solves still stop on the same residual criterion.
int kn_extrapolate_guess(KnSolver& sv, int which) {
  const int slot = which == KNPEMI_B_EMI ? 0 : 1;
  const int n = slot == 0 ? sv.emi.n : sv.knp.n;
  if (n == 0) return KNPEMI_OK;
  // order 2 (default) extrapolates through the last three solutions: 5.3 instead of 5.85 CG iterations per step while the
  // cell fires at config 2, 3.5 instead of 3.8 over the first 72 steps; KNPEMI_EXTRAPOLATE_ORDER=1: 2 x_n - x_(n-1)
  static const int order = getenv("KNPEMI_EXTRAPOLATE_ORDER") ? atoi(getenv("KNPEMI_EXTRAPOLATE_ORDER")) : 2;
  if (!sv.guess_old[slot]) {
    if (int rc = kn_alloc(sv.own->allocs, 2 * (size_t)n, &sv.guess_old[slot])) return rc;
    sv.guess_have[slot] = slot == 0 ? -1 : 0;
  }
  // the potential a run starts with is a guess, not a solution of the system (the concentrations it starts with are the
  // initial condition, i.e. the first point of the trajectory): no history from it -- 2 x_1 - x_0 with that x_0 cost the
  // second and third solves of a run twice their iterations
  if (sv.guess_have[slot] < 0) { sv.guess_have[slot] = 0; return KNPEMI_OK; }
  double* cur = slot == 0 ? sv.phi : sv.csol;
  extrapolate_launch(sv.own->stream, n, cur, slot == 0 ? sv.phi_stride : 1, sv.guess_old[slot],
                     order >= 2 ? sv.guess_old[slot] + n : (double*)nullptr, sv.guess_have[slot]);
  sv.guess_have[slot] = std::min(2, sv.guess_have[slot] + 1);
  return kn_launch_check("extrapolate_kernel");
}

// ---- diagnostics: one solver kernel on a caller's host arrays (knpemi_debug_linalg) ------------------------------
namespace {

// partial sums + ticket of the reductions, kept between calls as a solve keeps its workspace
double* g_debug_partial = nullptr;

int debug_partial(double** out) {
  if (!g_debug_partial) {
    const size_t bytes = (3 * RED_BLOCKS + 2) * sizeof(double);
    KN_HIP(hipMalloc(reinterpret_cast<void**>(&g_debug_partial), bytes));
    KN_HIP(hipMemset(g_debug_partial, 0, bytes));
  }
  *out = g_debug_partial;
  return KNPEMI_OK;
}

const char* debug_opname(int op) {
  static const char* names[] = {"SPMV", "BLOCK_SPMV", "DOTS", "VEC", "BICG_UPDATE", "BICG_INIT", "MASK", "GHOST_IDENTITY",
                                "DIAG_INV", "SCATTER_SHIFT", "EXTRAPOLATE", "KNP_ORDER", "COARSE_RESTRICT", "COARSE_SOLVE",
                                "COARSE_PROLONG"};
  return op >= 0 && op <= KNPEMI_LINALG_COARSE_PROLONG ? names[op] : "?";
}

// CSR pattern of n rows and ncols columns in slots 0 (rowptr), 1 (colind); the values in slot 2
int debug_check_csr(const KnDebugBufs& B, int n, int ncols) {
  int rc;
  if ((rc = B.need(2, "vals", 0, sizeof(double)))) return rc;
  if ((rc = B.check_rowptr(0, "rowptr", n, 2, sizeof(double)))) return rc;
  return B.check_range(1, "colind", (size_t)B.hi(0)[n], 0, ncols);
}

// what the block kernels read: whole cells of nv rows of equal length, a whole number of blocks each, and a block column
// for every block
int debug_check_blocks(const KnDebugBufs& B, int rows, int nv, int nbmax, int nsys) {
  int rc;
  if (nv != 3 && nv != 4 && nv != 8) return B.bad("NV (ip[0]) must be 3, 4 or 8");
  if (nbmax < 1) return B.bad("nbmax (ip[1]) must be positive");
  if (nsys <= 0 || nsys % nv || rows % nsys) return B.bad("unknowns of one system (ip[2]): a multiple of NV that divides the rows");
  const int cells = nsys / nv;
  if ((rc = B.need(2, "vals", 0, sizeof(double)))) return rc;
  if ((rc = B.check_rowptr(0, "rowptr", rows, 2, sizeof(double)))) return rc;
  if ((rc = B.check_range(1, "bcol", (size_t)cells * nbmax, -1, cells))) return rc;
  const int* rp = B.hi(0);
  for (int row = 0; row < rows; ++row) {
    const int len = rp[row + 1] - rp[row], first = row - row % nv;
    if (len % nv || len / nv > nbmax) return B.bad("row " + std::to_string(row) + ": not a whole number of blocks <= nbmax");
    if (len != rp[first + 1] - rp[first]) return B.bad("row " + std::to_string(row) + ": the rows of a cell differ in length");
    const int cl = (row % nsys) / nv;
    for (int k = 0; k < len / nv; ++k)
      if (B.hi(1)[(size_t)cl * nbmax + k] < 0) return B.bad("cell " + std::to_string(cl) + ": a block without a block column");
  }
  return KNPEMI_OK;
}

}  // namespace

extern "C" int knpemi_debug_linalg(int op, const knpemi_debug_linalg_args* args) {
  if (!args) return kn_fail(KNPEMI_EINVAL, "knpemi_debug_linalg: args is null");
  const knpemi_debug_linalg_args& A = *args;
  const bool amg_op = op >= KNPEMI_LINALG_AMG_SPMV && op <= KNPEMI_LINALG_AMG_DENSE;
  if (!amg_op && (op < 0 || op > KNPEMI_LINALG_COARSE_PROLONG)) return kn_fail(KNPEMI_EINVAL, "knpemi_debug_linalg: unknown op");
  if (A.n <= 0) return kn_fail(KNPEMI_EINVAL, "knpemi_debug_linalg: n must be positive");
  if (amg_op) return kn_debug_linalg_amg(op, A);
  KnDebugBufs B(A, debug_opname(op));
  const int n = A.n;
  const size_t N = (size_t)n, D = sizeof(double);
  const int* ip = A.ip;
  int rc = KNPEMI_OK;
  KnConsts consts{};
  // the arguments first: a refusal needs no device
  switch (op) {
    case KNPEMI_LINALG_SPMV:
      if (ip[0] != 4 && ip[0] != 16) return B.bad("lanes per row (ip[0]) must be 4 or 16");
      if (ip[1] <= 0) return B.bad("columns (ip[1]) must be positive");
      if ((rc = debug_check_csr(B, n, ip[1])) || (rc = B.need(3, "x", ip[1], D)) || (rc = B.need(4, "dinv", ip[1], D, true)) ||
          (rc = B.need(5, "b", N, D, true)) || (rc = B.need(6, "owned", N, 1, true)) || (rc = B.need(7, "y", N, D)) ||
          (rc = B.need(8, "dinv_out", N, D, true))) return rc;
      break;
    case KNPEMI_LINALG_BLOCK_SPMV:
      if (ip[3] < -1 || ip[3] > 1) return B.bad("kernel (ip[3]) must be -1, 0 or 1");
      if ((rc = debug_check_blocks(B, n, ip[0], ip[1], ip[2])) || (rc = B.need(3, "x", N, D)) || (rc = B.need(4, "b", N, D, true)) ||
          (rc = B.need(5, "owned", N, 1, true)) || (rc = B.need(6, "y", N, D))) return rc;
      break;
    case KNPEMI_LINALG_DOTS:
      if (ip[0] < 1 || ip[0] > 3) return B.bad("nd (ip[0]) must be 1, 2 or 3");
      if (ip[1] < OP_STORE3 || ip[1] > OP_START) return B.bad("op (ip[1]) is not a scalar step");
      for (int k = 2; k <= 4; ++k) if (ip[k] < 0 || ip[k] >= S_N) return B.bad("d0, d1, d2 (ip[2..4]) must be scalar slots");
      for (int k = 0; k < 2 * ip[0]; ++k) if ((rc = B.need(k, "a vector of the dot products", N, D))) return rc;
      if ((rc = B.need(6, "sc", 16, D)) || (rc = B.need(7, "red", 3, D, !ip[5]))) return rc;
      break;
    case KNPEMI_LINALG_VEC: {
      const int vop = ip[0];
      if (vop < V_RESID || vop > V_COPY_SHIFT) return B.bad("op (ip[0]) is not a vector update");
      const bool need_b = vop == V_CG_XR, need_c = vop != V_SHIFT;
      const bool need_d = vop == V_RESID || vop == V_CG_XR || vop == V_JACOBI || vop == V_BI_P || vop == V_BI_S;
      if ((rc = B.need(0, "sc", 16, D)) || (rc = B.need(1, "a", N, D)) || (rc = B.need(2, "b", N, D, !need_b)) ||
          (rc = B.need(3, "c", N, D, !need_c)) || (rc = B.need(4, "d", N, D, !need_d))) return rc;
      break;
    }
    case KNPEMI_LINALG_BICG_UPDATE:
      if ((rc = B.need(0, "sc", 16, D))) return rc;
      for (int s = 1; s <= 6; ++s) if ((rc = B.need(s, "x, r, p, s, sres or t", N, D))) return rc;
      if ((rc = B.need(7, "dinv", N, D, true))) return rc;
      break;
    case KNPEMI_LINALG_BICG_INIT:
      if ((rc = B.need(0, "p", N, D)) || (rc = B.need(1, "v", N, D)) || (rc = B.need(2, "sc", 16, D))) return rc;
      break;
    case KNPEMI_LINALG_MASK:
      if ((rc = B.need(0, "owned", N, 1)) || (rc = B.need(1, "a", N, D))) return rc;
      break;
    case KNPEMI_LINALG_GHOST_IDENTITY:
      if ((rc = B.need(3, "vals", 0, D)) || (rc = B.check_rowptr(0, "rowptr", n, 3, D)) ||
          (rc = B.need(1, "colind", (size_t)B.hi(0)[n], sizeof(int))) || (rc = B.need(2, "owned", N, 1))) return rc;
      break;
    case KNPEMI_LINALG_DIAG_INV:
      if ((rc = debug_check_csr(B, n, n)) || (rc = B.need(3, "dinv", N, D))) return rc;
      break;
    case KNPEMI_LINALG_SCATTER_SHIFT:
      if (ip[0] < 1) return B.bad("stride (ip[0]) must be positive");
      if ((rc = B.need(0, "src", N, D)) || (rc = B.need(1, "dst", N * ip[0], D)) || (rc = B.need(2, "sc", 16, D))) return rc;
      break;
    case KNPEMI_LINALG_EXTRAPOLATE:
      if (ip[0] < 1) return B.bad("stride (ip[0]) must be positive");
      if ((rc = B.need(0, "cur", N * ip[0], D)) || (rc = B.need(1, "old", N, D)) || (rc = B.need(2, "old2", N, D, true))) return rc;
      break;
    case KNPEMI_LINALG_KNP_ORDER: {
      const int ks = ip[0], n_sub = ip[1];
      if (ks < 1 || ks > 8) return B.bad("ks (ip[0]) must be 1 .. 8");
      if (n_sub < 1 || n_sub > KN_MAXSUB) return B.bad("n_sub (ip[1]) must be 1 .. 8");
      if (ip[3] != 0 || ip[3 + n_sub] != n) return B.bad("voff (ip[3 ..]) must run from 0 to n");
      for (int s = 0; s < n_sub; ++s) if (ip[3 + s + 1] < ip[3 + s]) return B.bad("voff (ip[3 ..]) decreases");
      consts.n_sub = n_sub; consts.K = ks + 1;
      for (int s = 0; s <= n_sub; ++s) consts.voff[s] = ip[3 + s];
      if ((rc = B.need(0, "x", N * ks, D)) || (rc = B.need(1, "csol", N * ks, D))) return rc;
      break;
    }
    case KNPEMI_LINALG_COARSE_RESTRICT: {
      const int nl = ip[0], rank = ip[1], world = ip[2];
      if (nl < 1 || world < 1 || rank < 0 || rank >= world || world * nl > KN_COARSE_MAX)
        return B.bad("nl, rank, world (ip[0..2]): 0 <= rank < world, 1 <= world nl <= 64");
      if ((rc = B.need(0, "r", N, D)) || (rc = B.need(3, "agg_wt", 0, D)) || (rc = B.check_rowptr(1, "agg_ptr", nl, 3, D)) ||
          (rc = B.check_range(2, "agg_idx", (size_t)B.hi(1)[nl], 0, n)) ||
          (rc = B.need(4, "red", (size_t)KN_COARSE_OFF + world * nl, D))) return rc;
      break;
    }
    case KNPEMI_LINALG_COARSE_SOLVE: {
      const int rank = ip[0], nc = ip[1];
      if (n > KN_COARSE_MAX || rank < 0 || nc > KN_COARSE_MAX || (rank + 1) * n > nc) return B.bad("nl (n), rank, nc (ip[0..1]): (rank + 1) nl <= nc <= 64");
      if ((rc = B.need(0, "inv", (size_t)nc * nc, D)) || (rc = B.need(1, "red", (size_t)KN_COARSE_OFF + nc, D)) ||
          (rc = B.need(2, "zc", N, D))) return rc;
      break;
    }
    case KNPEMI_LINALG_COARSE_PROLONG: {
      const int mode = ip[0], nz = ip[2];
      if (mode != 0 && mode != 1) return B.bad("mode (ip[0]) must be 0 or 1");
      if ((rc = B.need(1, "agg_w", N, D)) || (rc = B.need(3, "z", N, D))) return rc;
      if (mode == 0) {
        if (nz < 1) return B.bad("length of zc (ip[2]) must be positive");
        if ((rc = B.need(2, "zc", nz, D)) || (rc = B.check_range(0, "agg_of", N, -1, nz))) return rc;
        const double* w = static_cast<const double*>(A.buf[1]);
        for (int i = 0; i < n; ++i)
          if (B.hi(0)[i] >= 0 && w[i] > 0.0 && B.hi(0)[i] + 1 >= nz) return B.bad("agg_of: the upper node of an unknown lies past zc");
      } else if ((rc = B.need(0, "agg_of", N, sizeof(int)))) return rc;
      break;
    }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return kn_fail(KNPEMI_EHIP, "knpemi_debug_linalg: no HIP device visible (the hot path has no CPU fallback)");
  if ((rc = B.upload())) return rc;
  hipStream_t st = nullptr;
  switch (op) {
    case KNPEMI_LINALG_SPMV:
      spmv_launch(st, n, ip[0], B.p<int>(0), B.p<int>(1), B.p<double>(2), B.p<double>(3), B.p<double>(4), B.p<double>(7),
                  B.p<double>(5), B.p<uint8_t>(6), B.p<double>(8));
      break;
    case KNPEMI_LINALG_BLOCK_SPMV: {
      KnBlockCols bc;
      bc.bcol = B.p<int>(1); bc.nv = ip[0]; bc.nbmax = ip[1]; bc.n = ip[2];
      if (ip[3] < 0) launch_block_spmv<double>(st, bc, n, B.p<int>(0), B.p<double>(2), B.p<double>(3), B.p<double>(4), B.p<double>(6), B.p<uint8_t>(5));
      else launch_block_spmv<double>(st, bc, n, B.p<int>(0), B.p<double>(2), B.p<double>(3), B.p<double>(4), B.p<double>(6), B.p<uint8_t>(5), ip[3] == 1);
      break;
    }
    case KNPEMI_LINALG_DOTS: {
      double* partial = nullptr;
      if ((rc = debug_partial(&partial))) return rc;
      double* red = ip[5] ? B.p<double>(7) : nullptr;
      dots_launch(st, n, ip[0], B.p<double>(0), B.p<double>(1), B.p<double>(2), B.p<double>(3), B.p<double>(4), B.p<double>(5), partial,
                  B.p<double>(6), ip[1], ip[2], ip[3], ip[4], A.dp[0], red);
      if (red) dots_apply_launch(st, B.p<double>(6), red, ip[1], ip[0], ip[2], ip[3], ip[4], A.dp[0]);
      break;
    }
    case KNPEMI_LINALG_VEC:
      vec_launch(st, n, ip[0], B.p<double>(0), B.p<double>(1), B.p<double>(2), B.p<double>(3), B.p<double>(4));
      break;
    case KNPEMI_LINALG_BICG_UPDATE:
      bicg_update_launch(st, n, B.p<double>(0), B.p<double>(1), B.p<double>(2), B.p<double>(3), B.p<double>(4), B.p<double>(5),
                         B.p<double>(6), B.p<double>(7));
      break;
    case KNPEMI_LINALG_BICG_INIT: bicg_init_launch(st, n, B.p<double>(0), B.p<double>(1), B.p<double>(2)); break;
    case KNPEMI_LINALG_MASK: mask_launch(st, n, B.p<uint8_t>(0), B.p<double>(1), ip[0]); break;
    case KNPEMI_LINALG_GHOST_IDENTITY: ghost_identity_launch(st, n, B.p<int>(0), B.p<int>(1), B.p<uint8_t>(2), B.p<double>(3)); break;
    case KNPEMI_LINALG_DIAG_INV: diag_inv_launch(st, n, B.p<int>(0), B.p<int>(1), B.p<double>(2), B.p<double>(3)); break;
    case KNPEMI_LINALG_SCATTER_SHIFT: scatter_shift_launch(st, B.p<double>(0), B.p<double>(1), n, ip[0], B.p<double>(2)); break;
    case KNPEMI_LINALG_EXTRAPOLATE: extrapolate_launch(st, n, B.p<double>(0), ip[0], B.p<double>(1), B.p<double>(2), ip[1]); break;
    case KNPEMI_LINALG_KNP_ORDER: {
      KnConsts* dc = nullptr;
      KN_HIP(hipMalloc(reinterpret_cast<void**>(&dc), sizeof(KnConsts)));
      if (hipMemcpy(dc, &consts, sizeof(KnConsts), hipMemcpyHostToDevice) == hipSuccess) {
        knp_order_launch(st, n, ip[0], ip[1], dc, B.p<double>(0), B.p<double>(1), ip[2]);
        (void)hipDeviceSynchronize();
      }
      (void)hipFree(dc);
      break;
    }
    case KNPEMI_LINALG_COARSE_RESTRICT:
      coarse_restrict_launch(st, B.p<double>(0), B.p<int>(1), B.p<int>(2), B.p<double>(3), ip[0], ip[1], ip[2], B.p<double>(4));
      break;
    case KNPEMI_LINALG_COARSE_SOLVE: coarse_solve_launch(st, B.p<double>(0), B.p<double>(1), n, ip[0], ip[1], B.p<double>(2)); break;
    case KNPEMI_LINALG_COARSE_PROLONG:
      coarse_prolong_launch(st, n, B.p<int>(0), B.p<double>(1), B.p<double>(2), B.p<double>(3), ip[0], ip[1]);
      break;
  }
  if ((rc = kn_launch_check(std::string("knpemi_debug_linalg(") + B.opname + ")"))) return rc;
  return B.download();
}
