// Fixed-step membrane integrators beside LSODA: forward Euler, classical RK4, first-order Rush-Larsen.
//
// The reference's drivers still carry the knob of its former splitting solver, `n_steps_ODE = 25` sub-steps per PDE
// step (examples/idealized_geometries/run_2D.py:176,205), which nothing reads since it moved to LSODA.  These are the
// schemes that knob belongs to: every dof and every step cost the same, there is no step-size control and so nothing
// that diverges within a wavefront.
//
// One dof over [t0, t0 + dt] in n equal sub-steps h = dt / n, sub-step j at t_j = t0 + j * h (a product, not a running
// sum, so that host and device see the same times):
//   euler        y <- y + h f(t_j, y)
//   rk4          k1 = f(t_j, y), k2 = f(t_j + h/2, y + h/2 k1), k3 = f(t_j + h/2, y + h/2 k2), k4 = f(t_j + h, y + h k3),
//                y <- y + h/6 ((k1 + 2 k2) + (2 k3 + k4))
//   rush_larsen  a component the model declares as a gate (bit i of M::GATES: dy_i/dt = a_i (1 - y_i) - b_i y_i with
//                a_i, b_i independent of y_i, handed out by M::rates) takes the exact solution of its equation with
//                the rates frozen at (t_j, y):  y_i <- y_i + (a_i / s_i - y_i) (-expm1(-s_i h)),  s_i = a_i + b_i,
//                i.e. y_inf + (y_i - y_inf) exp(-s_i h) written so that s_i h -> 0 tends to the Euler update (s_i = 0
//                exactly: the Euler update itself).  A convex combination of y_i and y_inf in [0, 1]: a gate cannot
//                leave [0, 1] whatever h.  Every other component takes the Euler update from the same y.
//                A model without gates (GATES == 0) runs the Euler code: the two agree bit for bit.
// Every update is one explicit fma, so the rounding does not depend on what the compiler chooses to contract.
//
// Currents.  LSODA hands the PDEs the currents of whichever right-hand-side evaluation came last, at a time beyond
// t0 + dt (kernels_ode.hip).  Here the right-hand side is evaluated once more after the last sub-step, at
// (t0 + dt, y_end), and `finish(p)` stores THOSE currents: I_ch belongs to the state that is written back, and a host
// build reproduces it.
//
// Failure.  There is no error estimate to fail; a dof whose state is not finite after the interval is reported as
// failed (return value 1) and counted like an LSODA failure.  `nfe` counts right-hand-side evaluations (the final one
// included; a Rush-Larsen sub-step counts as one), `nst` sub-steps.
//
// Like ode_kernel.h this header is compiled by hipcc into the library, by hipRTC for plug-in models and by the host
// compiler for the CPU tests: it includes nothing but ode_kernel.h (and through it lsoda_core.h).
#pragma once

#include "ode_kernel.h"

// The single-step and the multi-step kernel promise the same bits, and the host build the same arithmetic order: no
// multiply-add of this header may be contracted here and left alone there (the compiler decides by context).  The
// updates are explicit fma calls; everything else is compiled as written.  (kernels_ode_fixed.hip is built with
// -ffp-contract=off for the same reason: that covers the models' right-hand sides in that translation unit.)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define KN_FS_EULER 1         // == KNPEMI_ODE_EULER
#define KN_FS_RK4 2           // == KNPEMI_ODE_RK4
#define KN_FS_RUSH_LARSEN 3   // == KNPEMI_ODE_RUSH_LARSEN

// finite: neither NaN nor infinite (no <cmath> here)
KN_HD bool kn_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

template <class M, int METHOD>
struct FixedStep {
  static constexpr int NS = M::NS;
  M f;
  int nfe, nst;

  KN_HD void euler_step(double t, double h, double* y) {
    double dy[NS];
    f.rhs(t, y, dy);
#pragma unroll
    for (int i = 0; i < NS; ++i) y[i] = fma(h, dy[i], y[i]);
    nfe += 1;
  }

  KN_HD void rk4_step(double t, double h, double* y) {
    const double hh = 0.5 * h, h6 = h / 6.0;
    double k1[NS], k2[NS], k3[NS], k4[NS], w[NS];
    f.rhs(t, y, k1);
#pragma unroll
    for (int i = 0; i < NS; ++i) w[i] = fma(hh, k1[i], y[i]);
    f.rhs(t + hh, w, k2);
#pragma unroll
    for (int i = 0; i < NS; ++i) w[i] = fma(hh, k2[i], y[i]);
    f.rhs(t + hh, w, k3);
#pragma unroll
    for (int i = 0; i < NS; ++i) w[i] = fma(h, k3[i], y[i]);
    f.rhs(t + h, w, k4);
#pragma unroll
    for (int i = 0; i < NS; ++i) y[i] = fma(h6, (k1[i] + 2.0 * k2[i]) + (2.0 * k3[i] + k4[i]), y[i]);
    nfe += 4;
  }

  KN_HD void rush_larsen_step(double t, double h, double* y) {
    if constexpr (M::GATES == 0u) {
      euler_step(t, h, y);
    } else {
      double dy[NS], a[NS], b[NS];
      f.rhs(t, y, dy);
      f.rates(t, y, a, b);
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        if ((M::GATES >> i) & 1u) {
          const double s = a[i] + b[i];
          y[i] = s > 0.0 ? fma(a[i] / s - y[i], -expm1(-s * h), y[i]) : fma(h, dy[i], y[i]);
        } else {
          y[i] = fma(h, dy[i], y[i]);
        }
      }
      nfe += 1;
    }
  }

  // the caller has run f.prepare(p); afterwards f.finish(p) stores the currents at (t0 + dt, y).  Returns 0, or 1 when
  // the state is not finite.
  KN_HD int integrate(double* y, double t0, double dt, int n) {
    const double h = dt / n;
    nfe = 0;
    nst = 0;
    for (int j = 0; j < n; ++j) {
      const double t = t0 + j * h;
      if constexpr (METHOD == KN_FS_EULER) euler_step(t, h, y);
      else if constexpr (METHOD == KN_FS_RK4) rk4_step(t, h, y);
      else rush_larsen_step(t, h, y);
    }
    nst = n;
    double dy[NS];
    f.rhs(t0 + dt, y, dy);
    nfe += 1;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < NS; ++i) ok = ok && kn_finite(y[i]);
    return ok ? 0 : 1;
  }
};

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
// One thread per membrane dof, every model: the sub-steps are straight-line code, identical for all dofs, so a wave
// has nothing to diverge on and needs no lanes to share a dof's work through LDS or cross-lane moves.  Head and tail
// are those of ode_step_body (ode_kernel.h) with one lane per dof: traces -> parameter columns, V <- phi_M, stimulus
// under the mask, prepare, integrate, state / phi_M / I_ch write-back, counters per workgroup without atomics.
template <class M, int METHOD>
__device__ __forceinline__ void ode_fixed_step_body(const OdeDev& D, const OdeArgs& a, int n_sub) {
  constexpr int NS = M::NS;
  const int qw = blockIdx.x * ODE_BLOCK + threadIdx.x;
  // the lanes past the last dof repeat the last dof and drop their results: the wave-level sums see all 64 lanes
  const bool live = qw < a.nq;
  const int q = live ? qw : a.nq - 1;
  const int qg = a.q0 + q;
  const StridedRow<0> p{a.params + q, (size_t)a.nq};
  double y[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) y[j] = a.states[(size_t)j * a.nq + q];
  if (a.flags & KN_ODE_SET_TRACES) {
    const double* re = D.VR + (size_t)D.q2e[qg] * KN_ODE_REC;
    const double* ri = D.VR + (size_t)D.q2i[qg] * KN_ODE_REC;
    for (int k = 0; k < a.n_ions; ++k) {
      p[a.ion_param[3 * k]] = re[KN_ODE_CSLOT(k)];
      p[a.ion_param[3 * k + 1]] = ri[KN_ODE_CSLOT(k)];
    }
  }
  if (a.flags & KN_ODE_SET_V) {
    const double v = D.phiM[qg];
#pragma unroll
    for (int j = 0; j < NS; ++j) y[j] = (j == a.v_index) ? v : y[j];
  }
  if (a.n_stim > 0 && (!a.mask || a.mask[q]))
    for (int i = 0; i < a.n_stim; ++i) p[a.stim_idx[i]] = a.stim_val[i];
  FixedStep<M, METHOD> s;
  s.f.prepare(p);
  const int rc = s.integrate(y, a.t0, a.dt, n_sub);
  if (live) {
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      a.states[(size_t)j * a.nq + q] = y[j];
      if (j == a.v_index) D.phiM[qg] = y[j];
    }
    s.f.finish(p);
    for (int k = 0; k < a.n_ions; ++k)
      D.Ich[((size_t)a.model_slot * KN_ODE_MAXK + k) * a.NQtot + qg] = p[a.ion_param[3 * k + 2]];
  }
  unsigned n_rhs = live ? (unsigned)s.nfe : 0u, n_st = live ? (unsigned)s.nst : 0u, n_bad = (live && rc != 0) ? 1u : 0u;
#pragma unroll
  for (int msk = 32; msk >= 1; msk >>= 1) {
    n_rhs += __shfl_xor(n_rhs, msk);
    n_st += __shfl_xor(n_st, msk);
    n_bad += __shfl_xor(n_bad, msk);
  }
  if (threadIdx.x == 0) {
    unsigned long long* st = a.stats + 3 * (size_t)blockIdx.x;
    st[0] += n_rhs;
    st[1] += n_st;
    st[2] += n_bad;
  }
}

// n_steps consecutive intervals [t, t + dt], t <- t + dt, in one launch: the counterpart of ode_advance_body with the
// same records, steady-state freeze and failed_step, and bit for bit n_steps launches of ode_fixed_step_body with
// flags = 0 (every interval: stimulus into the row, prepare, integrate, finish).  A dof whose state is not finite
// after an interval is frozen with its last good state.
template <class M, int METHOD>
__device__ __forceinline__ void ode_fixed_advance_body(const OdeArgs& a, const OdeAdvArgs& v, int n_sub) {
  constexpr int NS = M::NS;
  const int qw = blockIdx.x * ODE_BLOCK + threadIdx.x;
  const bool live = qw < a.nq;
  const int q = live ? qw : a.nq - 1;
  const StridedRow<0> p{a.params + q, (size_t)a.nq};
  double y[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) y[j] = a.states[(size_t)j * a.nq + q];
  const bool stim = a.n_stim > 0 && (!a.mask || a.mask[q]);
  bool frozen = v.failed_step[q] >= 0 || (v.window > 0 && v.steps_taken[q] >= 0);
  int still = v.window > 0 ? v.still[q] : 0;
  unsigned long long n_rhs = 0, n_st = 0, n_bad = 0;
  double t = a.t0;
  int s = 0;
  for (; s < v.n_steps; ++s) {
    if (!KN_ANY(!frozen)) break;
    const int sg = v.s0 + s;
    if (!frozen) {
      // (lanes past the last dof repeat its row: they store what its own lane stores)
      if (stim)
        for (int i = 0; i < a.n_stim; ++i) p[a.stim_idx[i]] = a.stim_val[i];
      double y0[NS];
#pragma unroll
      for (int j = 0; j < NS; ++j) y0[j] = y[j];
      FixedStep<M, METHOD> in;
      in.f.prepare(p);
      const int rc = in.integrate(y, t, a.dt, n_sub);
      if (live) {
        in.f.finish(p);
        n_rhs += (unsigned)in.nfe;
        n_st += (unsigned)in.nst;
        n_bad += rc != 0 ? 1u : 0u;
      }
      if (rc != 0) {
#pragma unroll
        for (int j = 0; j < NS; ++j) y[j] = y0[j];
        frozen = true;
        if (live) v.failed_step[q] = sg;
      } else if (v.window > 0) {
        bool moved = false;
#pragma unroll
        for (int j = 0; j < NS; ++j) moved = moved || !(fabs(y[j] - y0[j]) <= v.ss_atol + v.ss_rtol * fabs(y[j]));
        still = moved ? 0 : still + 1;
        if (still >= v.window) {
          frozen = true;
          if (live) v.steps_taken[q] = sg + 1;
        }
      }
    }
    if (v.hist && (sg + 1) % v.every == 0 && live) {
      double* row = v.hist + (size_t)((sg + 1) / v.every - 1) * v.n_rec * a.nq + q;
      for (int i = 0; i < v.n_rec; ++i)
#pragma unroll
        for (int j = 0; j < NS; ++j)
          if (j == v.rec_idx[i]) row[(size_t)i * a.nq] = y[j];
    }
    t = t + a.dt;
  }
  // the wave is done early: its dofs' later records repeat their frozen states
  if (v.hist && live)
    for (; s < v.n_steps; ++s) {
      const int sg = v.s0 + s;
      if ((sg + 1) % v.every) continue;
      double* row = v.hist + (size_t)((sg + 1) / v.every - 1) * v.n_rec * a.nq + q;
      for (int i = 0; i < v.n_rec; ++i)
#pragma unroll
        for (int j = 0; j < NS; ++j)
          if (j == v.rec_idx[i]) row[(size_t)i * a.nq] = y[j];
    }
  if (live) {
#pragma unroll
    for (int j = 0; j < NS; ++j) a.states[(size_t)j * a.nq + q] = y[j];
    if (v.window > 0) v.still[q] = still;
  }
#pragma unroll
  for (int msk = 32; msk >= 1; msk >>= 1) {
    n_rhs += __shfl_xor(n_rhs, msk);
    n_st += __shfl_xor(n_st, msk);
    n_bad += __shfl_xor(n_bad, msk);
  }
  if (threadIdx.x == 0) {
    unsigned long long* st = a.stats + 3 * (size_t)blockIdx.x;
    st[0] += n_rhs;
    st[1] += n_st;
    st[2] += n_bad;
  }
}

template <class M, int METHOD>
__global__ __launch_bounds__(ODE_BLOCK) void ode_fixed_step_kernel(OdeDev D, OdeArgs a, int n_sub) {
  ode_fixed_step_body<M, METHOD>(D, a, n_sub);
}

template <class M, int METHOD>
__global__ __launch_bounds__(ODE_BLOCK) void ode_fixed_advance_kernel(OdeArgs a, OdeAdvArgs v, int n_sub) {
  ode_fixed_advance_body<M, METHOD>(a, v, n_sub);
}
#endif

#if defined(__clang__)
#pragma clang fp contract(fast)   // back to the HIP default for what follows the include
#endif
