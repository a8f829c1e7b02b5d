// The membrane ODE sweep kernel (see kernels_ode.hip for what it fuses).  This header is compiled twice: by hipcc into
// libknpemi_hip.so for the membrane models that ship with the library (membrane_models.h), and at run time by hipRTC
// for a plug-in that brings its own right-hand side as HIP source (knpemi_ode_bind_source): it therefore includes
// nothing but lsoda_core.h and uses plain types only.
#pragma once

#include "lsoda_core.h"

#define KN_ODE_MAXK 4     // == KNPEMI_MAX_IONS
#define KN_ODE_REC 8      // == KN_REC: doubles per vertex record, ion k in slot KN_ODE_CSLOT(k)
#define KN_ODE_CSLOT(k) ((k) < 3 ? 4 + (k) : 3)

// the slice of the device problem the sweep touches
struct OdeDev {
  const double* VR;      // [Ntot][8] vertex records
  const int* q2e;        // [NQtot] ECS / cell vertex of every membrane dof
  const int* q2i;
  double* phiM;          // [NQtot]
  double* Ich;           // [model slot][ion][NQtot]
};

struct OdeArgs {
  int nq, q0, n_stim, flags, v_index, model_slot, NQtot, n_ions;
  int dpw;               // membrane dofs per wavefront (<= 64 / LANES; 0 = all of them), see ode_step_body
  int ion_param[3 * KN_ODE_MAXK];
  int stim_idx[8];
  double stim_val[8];
  double t0, dt, rtol, atol;
  double* states;
  double* params;
  const unsigned char* mask;
  unsigned long long* stats;
  unsigned long long* stamps;   // diagnostic build: [workgroup][24] phase cycle sums and counts
};

// the extra arguments of the multi-step launch (ode_advance_body); the steps run with flags = 0
struct OdeAdvArgs {
  int n_steps;           // steps of this launch
  int s0;                // index of its first step within the whole run (records, steps_taken, failed_step)
  int n_rec, every;      // record states rec_idx[0..n_rec) after every `every`-th step of the run
  int rec_idx[8];
  double* hist;          // [run step / every][n_rec][nq], or NULL
  int window;            // steady-state mode: a dof is steady after `window` consecutive still steps (0: plain run)
  double ss_rtol, ss_atol;
  int* still;            // [nq] still steps in a row so far (carried from launch to launch)
  int* steps_taken;      // [nq] -1, or the number of steps after which the dof was declared steady
  int* failed_step;      // [nq] -1, or the step on which LSODA failed
};

#define KN_ODE_SET_V 1        // == KNPEMI_ODE_SET_V
#define KN_ODE_SET_TRACES 2   // == KNPEMI_ODE_SET_TRACES

constexpr int ODE_BLOCK = 64;

// a model may fix per-lane constants of its component-wise right-hand side once per sweep (membrane_models.h)
template <class M>
KN_HD auto kn_model_set_lane(M& m, int c, int) -> decltype(m.set_lane(c), void()) { m.set_lane(c); }
template <class M>
KN_HD void kn_model_set_lane(M&, int, long) {}

template <int S>
struct StridedRow {   // p[j] of dof q in a [column][dof] table: base + j * S
  double* b;
  size_t stride;
  KN_HD double& operator[](int j) const { return b[(size_t)j * stride]; }
};

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
// The parameter row of a dof as the sweep sees it: the row in the global table plus the wave's copy of it in LDS.
// A store goes to both; a load comes from the copy.  The sweep stores the traces and the stimulus into the row and
// `prepare` then reads the whole row, `finish` stores the currents and the write-back reads them again -- through
// runtime column indices, so the compiler cannot forward the values, and in global memory each of the two is a store,
// a wait for it and a dependent load: a memory round trip at the head and one at the tail of a sweep whose length is
// the latency of one wave.  In LDS the same pair costs a hundred cycles.  The models keep indexing `p[j]`.
// All lanes that work on a dof (its components, the lanes that mirror it, the lanes past the last dof that repeat it)
// share ONE column of the copy, as they share the row in the table: what the owner's `finish` stores is what the other
// lanes of the dof read next (ode_advance_body), exactly as through memory.  A dof belongs to one wave, a workgroup is
// one wave, and a wave's LDS accesses complete in order: no barrier is needed between such a store and load.
template <int COLS>
struct StagedRow {
  double* g;        // this dof's row in the transposed table: entry j at g[j * stride]
  size_t stride;
  double* l;        // its column of the LDS copy: entry j at l[j * COLS]
  struct Ref {
    double* g;
    double* l;
    __device__ __forceinline__ operator double() const { return *l; }
    __device__ __forceinline__ void operator=(double v) const { *g = v; *l = v; }
    __device__ __forceinline__ void operator=(const Ref& o) const { *this = (double)o; }
  };
  __device__ __forceinline__ Ref operator[](int j) const { return Ref{g + (size_t)j * stride, l + j * COLS}; }
  // entry j of the copy alone (staging: the value was just loaded from the table)
  __device__ __forceinline__ void stage(int j, double v) const { l[j * COLS] = v; }
};

// The copy takes NP columns-of-dofs doubles of LDS; a plug-in with a long parameter row at one thread per dof (up to 128
// x 64 doubles) works on the table itself, as every sweep did before.
template <class M, int LANES>
struct OdeRowKind {
  static constexpr int COLS = ODE_BLOCK / LANES;                         // dofs of a full wave
  static constexpr bool STAGED = M::NP * COLS * 8 <= 12 * 1024;         // shipped models: 2.8 kB (HH), 11.5 kB (glial)
  static constexpr int LDS_DOUBLES = STAGED ? M::NP * COLS : 1;
};
template <bool STAGED, int COLS>
struct OdeRow : StagedRow<COLS> {
  __device__ __forceinline__ OdeRow(double* g_, size_t stride_, double* lds, int col) : StagedRow<COLS>{g_, stride_, lds + col} {}
  // issue the loads of the whole row (they travel with the sweep's other first loads) ...
  template <int NP>
  __device__ __forceinline__ void load(double (&r)[NP]) const {
#pragma unroll
    for (int j = 0; j < NP; ++j) r[j] = this->g[(size_t)j * this->stride];
  }
  // ... and put them into the copy
  template <int NP>
  __device__ __forceinline__ void stage_all(const double (&r)[NP]) const {
#pragma unroll
    for (int j = 0; j < NP; ++j) this->stage(j, r[j]);
  }
};
template <int COLS>
struct OdeRow<false, COLS> : StridedRow<0> {
  __device__ __forceinline__ OdeRow(double* g_, size_t stride_, double*, int) : StridedRow<0>{g_, stride_} {}
  template <int NP>
  __device__ __forceinline__ void load(double (&)[NP]) const {}
  template <int NP>
  __device__ __forceinline__ void stage_all(const double (&)[NP]) const {}
};

// the workgroup's copy of LSODA's coefficient tables: loads first (beside the sweep's other first loads), LDS stores
// later; the caller's barrier makes the copy visible
constexpr int KN_COEF_DOUBLES = (int)(sizeof(LsodaCoef) / sizeof(double));
constexpr int KN_COEF_PER_LANE = (KN_COEF_DOUBLES + ODE_BLOCK - 1) / ODE_BLOCK;
__device__ __forceinline__ void kn_coef_load(const LsodaCoef* __restrict__ cf, double (&c)[KN_COEF_PER_LANE]) {
  const double* src = reinterpret_cast<const double*>(cf);
#pragma unroll
  for (int i = 0; i < KN_COEF_PER_LANE; ++i) {
    const int k = i * ODE_BLOCK + (int)threadIdx.x;
    c[i] = ((i + 1) * ODE_BLOCK <= KN_COEF_DOUBLES || k < KN_COEF_DOUBLES) ? src[k] : 0.0;
  }
}
__device__ __forceinline__ void kn_coef_store(LsodaCoef* scf, const double (&c)[KN_COEF_PER_LANE]) {
  double* dst = reinterpret_cast<double*>(scf);
#pragma unroll
  for (int i = 0; i < KN_COEF_PER_LANE; ++i) {
    const int k = i * ODE_BLOCK + (int)threadIdx.x;
    if ((i + 1) * ODE_BLOCK <= KN_COEF_DOUBLES || k < KN_COEF_DOUBLES) dst[k] = c[i];
  }
}

// LANES = M::NS: lane c of every group of NS adjacent lanes integrates component c of one membrane dof
// (lsoda_core.h); LANES = 1: one thread per dof (one-state models).
// WAVES = 2 caps the register budget at 256 per lane so that two waves share a SIMD.  It pays once there are more
// waves than SIMDs (large membranes); small sweeps run one wave per SIMD with the full register file.
// LONE_WAVE: the wave that runs the body is the only one of its workgroup that does (the fused launch of
// kernels_sweep_emi.hip: 256-thread workgroups whose other waves have returned).  What the workgroup shares in LDS is then
// written and read by this wave alone, whose LDS accesses complete in order: the barrier below becomes an ordering of the
// wave's own accesses, not a hardware barrier that siblings which have left would have to reach.
template <class M, int LANES, int WAVES, bool STAMPS, bool LONE_WAVE = false>
__device__ __forceinline__ void ode_step_body(const OdeDev& D, const OdeArgs& a, const LsodaCoef* __restrict__ cf) {
  using Integrator = Lsoda<M::NS, M, LANES, STAMPS, ODE_BLOCK>;
  constexpr int NI = Integrator::NI;
  // factorised iteration matrix + pivots of the BDF method, one column per lane (touched by stiff dofs only)
  __shared__ double work[Integrator::WORK * ODE_BLOCK];
  // LSODA's coefficient tables (5 kB) are consulted with a per-lane order index whenever an order changes: keep the
  // workgroup's copy in LDS.  Everything else the non-stiff integrator touches lives in registers.
  __shared__ LsodaCoef scf;
  using Kind = OdeRowKind<M, LANES>;
  __shared__ double rowbuf[Kind::LDS_DOUBLES];   // the wave's copy of its dofs' parameter rows (StagedRow)
  // Dofs per wavefront.  A wave runs the UNION of the trips of its dofs' phase machines, and an instruction costs the same
  // whatever the exec mask: with 64 / LANES dofs per wave ~10 % of the stream is other dofs' trips.  While the sweep has fewer
  // waves than the chip has SIMDs (config 2: 185 on 1 024) the idle SIMDs buy that back: `dpw` dofs per wave, the other
  // lanes MIRROR them (lane l integrates what lane l mod (dpw LANES) integrates and drops the result: identical control
  // flow, no divergence added, every lane active for the wave-level sums).
  constexpr int FULL = ODE_BLOCK / LANES;
  const int dpw = (a.dpw > 0 && a.dpw < FULL) ? a.dpw : FULL;
  const int lane_in = threadIdx.x % (dpw * LANES);
  const bool primary = threadIdx.x < dpw * LANES;
  const int qw = blockIdx.x * dpw + lane_in / LANES;
  // the lanes past the last dof repeat the last dof and drop their results: every lane of the wave stays active,
  // so the wave-level sums below see all 64 lanes
  const bool live = primary && qw < a.nq;
  const int q = qw < a.nq ? qw : a.nq - 1, comp = threadIdx.x % LANES;
  const int qg = a.q0 + q;
  const int col = q - (int)blockIdx.x * dpw;   // the dof's place in its wave, 0 <= col < dpw
  // this dof's parameter row in the transposed table, and its column of the wave's copy
  const OdeRow<Kind::STAGED, FULL> p(a.params + q, (size_t)a.nq, rowbuf, col > 0 ? col : 0);
  // Everything the head reads that depends on nothing but the arguments is requested at once -- coefficient tables,
  // state, the whole parameter row, the vertex numbers, V, the mask: ONE memory latency -- then the two vertex records
  // (a second one).  Before, the coefficient copy and its barrier came first, and the row was read back from memory after
  // the stores of step 1 and 2 had landed: five latencies in a row at the head of every wave.
  const bool traces = a.flags & KN_ODE_SET_TRACES, set_v = a.flags & KN_ODE_SET_V;
  double coef[KN_COEF_PER_LANE], row[M::NP];
  kn_coef_load(cf, coef);
  double y[NI];
#pragma unroll
  for (int j = 0; j < NI; ++j) y[j] = a.states[(size_t)(comp + j) * a.nq + q];
  p.load(row);
  int ve = 0, vi = 0;
  if (traces) { ve = D.q2e[qg]; vi = D.q2i[qg]; }
  double v = 0.0;
  if (set_v) v = D.phiM[qg];
  int in_mask = 1;
  if (a.n_stim > 0 && a.mask) in_mask = a.mask[q];
  double ce[KN_ODE_MAXK] = {0.0, 0.0, 0.0, 0.0}, ci[KN_ODE_MAXK] = {0.0, 0.0, 0.0, 0.0};
  if (traces) {
    const double* re = D.VR + (size_t)ve * KN_ODE_REC;
    const double* ri = D.VR + (size_t)vi * KN_ODE_REC;
#pragma unroll
    for (int k = 0; k < KN_ODE_MAXK; ++k)
      if (k < a.n_ions) { ce[k] = re[KN_ODE_CSLOT(k)]; ci[k] = ri[KN_ODE_CSLOT(k)]; }
  }
  // (the mask byte is first looked at here, behind the loads of the records: tested where it is loaded, it is waited for
  // there, a memory latency of its own)
  asm volatile("" : "+v"(in_mask));
  const bool stim = a.n_stim > 0 && in_mask;
  kn_coef_store(&scf, coef);
  p.stage_all(row);
  // 1. concentration traces (record components 4..6 hold c_0, c_1, c_eliminated) -> parameter columns.
  //    With several lanes per dof every lane writes the same values.
  if (traces) {
#pragma unroll
    for (int k = 0; k < KN_ODE_MAXK; ++k)
      if (k < a.n_ions) {
        p[a.ion_param[3 * k]] = ce[k];
        p[a.ion_param[3 * k + 1]] = ci[k];
      }
  }
  if (set_v) {
#pragma unroll
    for (int j = 0; j < NI; ++j) y[j] = (comp + j == a.v_index) ? v : y[j];
  }
  // 2. stimulus + LSODA (the parameter row is read once by prepare(); only the currents change)
  if (stim)
    for (int i = 0; i < a.n_stim; ++i) p[a.stim_idx[i]] = a.stim_val[i];
  if constexpr (LONE_WAVE) {   // the coefficient tables are in place: this wave's own stores, ordered before its loads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __syncthreads();   // the coefficient tables are in place
  }
  Integrator s;
  if constexpr (STAMPS) s.st_last = __builtin_amdgcn_s_memtime();
  s.f.prepare(p);
  if constexpr (LANES > 1) kn_model_set_lane(s.f, comp, 0);
  const int rc = s.integrate(&scf, work + threadIdx.x, y, a.t0, a.t0 + a.dt, a.rtol, a.atol, 10000, comp);
  // 3. write back: state row, phi_M_prev <- V; the lane that owns V stores the currents (the reference's
  //    RHS side effect) into the parameter row and the I_ch_k fields (read from the row's copy, not from memory)
  const bool owner = live && (LANES == 1 || comp == M::CURRENT_LANE);
  if (live) {
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      a.states[(size_t)(comp + j) * a.nq + q] = y[j];
      if (comp + j == a.v_index) D.phiM[qg] = y[j];
    }
  }
  if (owner) {
    s.f.finish(p);
    for (int k = 0; k < a.n_ions; ++k)
      D.Ich[((size_t)a.model_slot * KN_ODE_MAXK + k) * a.NQtot + qg] = p[a.ion_param[3 * k + 2]];
  }
  // counters: summed over the wave, then added to this workgroup's own slot (thousands of atomic adds to ONE word
  // serialise at ~90 per microsecond: the tail of the sweep); knpemi_ode_stats() adds the slots up
  unsigned n_rhs = owner ? (unsigned)s.nfe : 0u, n_st = owner ? (unsigned)s.nst : 0u, n_bad = (owner && rc != 0) ? 1u : 0u;
#pragma unroll
  for (int msk = 32; msk >= 1; msk >>= 1) {
    n_rhs += __shfl_xor(n_rhs, msk);
    n_st += __shfl_xor(n_st, msk);
    n_bad += __shfl_xor(n_bad, msk);
  }
  if constexpr (STAMPS) {
    if (threadIdx.x == 0 && a.stamps)
      for (int i = 0; i < 12; ++i) {
        a.stamps[24 * (size_t)blockIdx.x + i] = s.st_acc[i];
        a.stamps[24 * (size_t)blockIdx.x + 12 + i] = s.st_cnt[i];
      }
  }
  if (threadIdx.x == 0) {
    // adds without a return value: the wave ends without waiting for the slot's old contents (a load, a memory latency at
    // the very end of the sweep); no other workgroup touches this slot, so nothing serialises
    unsigned long long* st = a.stats + 3 * (size_t)blockIdx.x;
    atomicAdd(st + 0, (unsigned long long)n_rhs);
    atomicAdd(st + 1, (unsigned long long)n_st);
    atomicAdd(st + 2, (unsigned long long)n_bad);
  }
}


// n_steps consecutive knpemi_ode_step intervals [t, t + dt], t <- t + dt (the caller's time arithmetic), in one launch.
// Every interval is a fresh LSODA integration in the order of ode_step_body with flags = 0 (stimulus into the parameter
// row, prepare, integrate, finish) and with its lane layout, so the result is bit for bit that of n_steps sweeps; only
// the state stays in registers from one step to the next.  This is a separate body, not a loop around ode_step_body: the
// production sweep's code generation stays exactly as it is.
// A dof is frozen -- no longer integrated, its state kept -- once it is steady (window > 0) or after an LSODA failure
// (its last good state is kept); a wave ends its launch when all its dofs are frozen.
template <class M, int LANES, int WAVES>
__device__ __forceinline__ void ode_advance_body(const OdeArgs& a, const OdeAdvArgs& v, const LsodaCoef* __restrict__ cf) {
  using Integrator = Lsoda<M::NS, M, LANES, false, ODE_BLOCK>;
  constexpr int NI = Integrator::NI;
  __shared__ double work[Integrator::WORK * ODE_BLOCK];
  __shared__ LsodaCoef scf;
  using Kind = OdeRowKind<M, LANES>;
  __shared__ double rowbuf[Kind::LDS_DOUBLES];
  // lane layout of ode_step_body: `dpw` dofs per wave, the other lanes mirror them; lanes past the last dof repeat it
  constexpr int FULL = ODE_BLOCK / LANES;
  const int dpw = (a.dpw > 0 && a.dpw < FULL) ? a.dpw : FULL;
  const int lane_in = threadIdx.x % (dpw * LANES);
  const bool primary = threadIdx.x < dpw * LANES;
  const int qw = blockIdx.x * dpw + lane_in / LANES;
  const bool live = primary && qw < a.nq;
  const int q = qw < a.nq ? qw : a.nq - 1, comp = threadIdx.x % LANES;
  const bool owner = live && (LANES == 1 || comp == M::CURRENT_LANE);
  // the row and the wave's copy of it, as in ode_step_body: staged once, every step's stimulus and currents go to both
  const int col = q - (int)blockIdx.x * dpw;
  const OdeRow<Kind::STAGED, FULL> p(a.params + q, (size_t)a.nq, rowbuf, col > 0 ? col : 0);
  double coef[KN_COEF_PER_LANE], row[M::NP];
  kn_coef_load(cf, coef);
  double y[NI];
#pragma unroll
  for (int j = 0; j < NI; ++j) y[j] = a.states[(size_t)(comp + j) * a.nq + q];
  p.load(row);
  const bool stim = a.n_stim > 0 && (!a.mask || a.mask[q]);
  // frozen dofs stay frozen across launches
  bool frozen = v.failed_step[q] >= 0 || (v.window > 0 && v.steps_taken[q] >= 0);
  int still = v.window > 0 ? v.still[q] : 0;
  kn_coef_store(&scf, coef);
  p.stage_all(row);
  __syncthreads();
  unsigned long long n_rhs = 0, n_st = 0, n_bad = 0;
  double t = a.t0;
  int s = 0;
  for (; s < v.n_steps; ++s) {
    if (!KN_ANY(!frozen)) break;
    const int sg = v.s0 + s;
    if (!frozen) {
      if (stim)
        for (int i = 0; i < a.n_stim; ++i) p[a.stim_idx[i]] = a.stim_val[i];
      double y0[NI];
#pragma unroll
      for (int j = 0; j < NI; ++j) y0[j] = y[j];
      Integrator in;
      in.f.prepare(p);
      if constexpr (LANES > 1) kn_model_set_lane(in.f, comp, 0);
      const int rc = in.integrate(&scf, work + threadIdx.x, y, t, t + a.dt, a.rtol, a.atol, 10000, comp);
      if (owner) {
        in.f.finish(p);
        n_rhs += (unsigned)in.nfe;
        n_st += (unsigned)in.nst;
        n_bad += rc != 0 ? 1u : 0u;
      }
      // the lanes of a dof take one decision: the failure / stillness of the dof is the OR / AND over them
      const double failed = kn_group_max<LANES>(rc != 0 ? 1.0 : 0.0);
      if (failed != 0.0) {
#pragma unroll
        for (int j = 0; j < NI; ++j) y[j] = y0[j];
        frozen = true;
        if (live && comp == 0) v.failed_step[q] = sg;
      } else if (v.window > 0) {
        double moved = 0.0;
#pragma unroll
        for (int j = 0; j < NI; ++j)
          moved = fabs(y[j] - y0[j]) <= v.ss_atol + v.ss_rtol * fabs(y[j]) ? moved : 1.0;
        still = kn_group_max<LANES>(moved) == 0.0 ? still + 1 : 0;
        if (still >= v.window) {
          frozen = true;
          if (live && comp == 0) v.steps_taken[q] = sg + 1;
        }
      }
    }
    if (v.hist && (sg + 1) % v.every == 0 && live) {
      double* row = v.hist + (size_t)((sg + 1) / v.every - 1) * v.n_rec * a.nq + q;
      for (int i = 0; i < v.n_rec; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
          if (comp + j == v.rec_idx[i]) row[(size_t)i * a.nq] = y[j];
    }
    t = t + a.dt;
    // the next step's prepare() reads what this step's finish() stored in the row (its copy in LDS, or the table for a
    // row too long to stage), from other lanes of the wave
    __syncthreads();
  }
  // the wave is done early: its dofs' later records repeat their frozen states
  if (v.hist && live)
    for (; s < v.n_steps; ++s) {
      const int sg = v.s0 + s;
      if ((sg + 1) % v.every) continue;
      double* row = v.hist + (size_t)((sg + 1) / v.every - 1) * v.n_rec * a.nq + q;
      for (int i = 0; i < v.n_rec; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
          if (comp + j == v.rec_idx[i]) row[(size_t)i * a.nq] = y[j];
    }
  // only the tables are written: phi_M / I_ch of a PDE problem are formed from them by the next sweep with flags
  if (live) {
#pragma unroll
    for (int j = 0; j < NI; ++j) a.states[(size_t)(comp + j) * a.nq + q] = y[j];
    if (v.window > 0 && comp == 0) v.still[q] = still;
  }
#pragma unroll
  for (int msk = 32; msk >= 1; msk >>= 1) {
    n_rhs += __shfl_xor(n_rhs, msk);
    n_st += __shfl_xor(n_st, msk);
    n_bad += __shfl_xor(n_bad, msk);
  }
  if (threadIdx.x == 0) {
    // adds without a return value: the wave ends without waiting for the slot's old contents (a load, a memory latency at
    // the very end of the sweep); no other workgroup touches this slot, so nothing serialises
    unsigned long long* st = a.stats + 3 * (size_t)blockIdx.x;
    atomicAdd(st + 0, (unsigned long long)n_rhs);
    atomicAdd(st + 1, (unsigned long long)n_st);
    atomicAdd(st + 2, (unsigned long long)n_bad);
  }
}

template <class M, int LANES, int WAVES>
__global__ __launch_bounds__(ODE_BLOCK, WAVES) void ode_advance_kernel(OdeArgs a, OdeAdvArgs v, const LsodaCoef* __restrict__ cf) {
  ode_advance_body<M, LANES, WAVES>(a, v, cf);
}

template <class M, int LANES, int WAVES = 1, bool STAMPS = false>
__global__ __launch_bounds__(ODE_BLOCK, WAVES) void ode_step_kernel(OdeDev D, OdeArgs a, const LsodaCoef* __restrict__ cf) {
  ode_step_body<M, LANES, WAVES, STAMPS>(D, a, cf);
}
#endif
