// Membrane models supplied by the user as HIP source, compiled at bind time with hipRTC.
//
// The reference accepts any module that exposes `rhs_numba.address`, a numba cfunc with numbalsoda's signature
// `rhs(t, states, values, parameters)` (src/knpemi/odeSolver.py:96; e.g. examples/benchmark/mm_glial.py:127-215, which
// has another parameter order and other constants than the glial model of the astrocyte example).  A GPU cannot call
// a host function pointer; the MI355X-native counterpart is a plug-in that brings the same function as a
// `__device__` function in HIP source (module attribute RHS_HIP).  It is pasted under the sweep kernel
// (ode_kernel.h: the very code of the shipped models) and compiled for gfx950 when the model is bound; the result is
// launched through the module API.  Parameters are an in/out row, exactly as for the cfunc: whatever the last
// right-hand-side call stored there (the currents I_ch_*) is what the PDEs receive.
//
// This file compiles, caches and binds (kn_rtc_bind fills KnOdeModel::rtc_kernel[method][shape]) and has the one
// module launch, kn_rtc_launch.  Which entry point runs, with which grid and parameters, is decided with every other
// sweep in kernels_ode.hip (launch_sweep).
#include <hip/hiprtc.h>

#include <cstring>
#include <map>
#include <mutex>

#include "ode_host.h"

namespace {

// the three headers the generated translation unit includes, embedded at build time (csrc/Makefile)
const char* const SRC_LSODA_CORE =
#include "rtc_lsoda_core.inc"
    ;
const char* const SRC_ODE_KERNEL =
#include "rtc_ode_kernel.inc"
    ;
const char* const SRC_FIXED_STEP =
#include "rtc_fixed_step.inc"
    ;
// ... and the three more the monitor program of a plug-in includes (monitor_kernel.h: the record kernel's body)
const char* const SRC_MONITOR_TABLE =
#include "rtc_monitor_table.inc"
    ;
const char* const SRC_RECORD_TAIL =
#include "rtc_record_tail.inc"
    ;
const char* const SRC_MONITOR_KERNEL =
#include "rtc_monitor_kernel.inc"
    ;

std::string wrapper_source(int ns, int np, int lanes, const std::string& user) {
  std::string s;
  s += "#include \"fixed_step.h\"\n";
  s += "// ---- plug-in source -------------------------------------------------------------\n";
  s += user;
  // the model functor the integrators expect, around the plug-in's `rhs` in namespace `scope`
  auto adapter = [&](const std::string& scope) {
    std::string s;
    s += "\n// ---- adapter: the model functor the integrator expects ---------------------------\n";
    s += "struct ModelUser {\n";
    s += "  static constexpr int NS = " + std::to_string(ns) + ", NP = " + std::to_string(np) + ", CURRENT_LANE = 0;\n";
    s += "  double par[NP];\n";
    s += "  template <class Row> __device__ void prepare(const Row& p) {\n";
    s += "    _Pragma(\"unroll\") for (int j = 0; j < NP; ++j) par[j] = p[j];\n  }\n";
    s += "  __device__ void rhs(double t, const double* y, double* dy) { " + scope + "::rhs(t, y, dy, par); }\n";
    s += "  // every lane of a system evaluates the whole right-hand side and keeps its own component\n";
    s += "  __device__ double rhs_lane(int c, double t, const double* y) {\n";
    s += "    double dy[NS];\n    " + scope + "::rhs(t, y, dy, par);\n    double out = dy[0];\n";
    s += "    _Pragma(\"unroll\") for (int k = 1; k < NS; ++k) out = (k == c) ? dy[k] : out;\n    return out;\n  }\n";
    s += "  template <class Row> __device__ void finish(const Row& p) const {\n";
    s += "    _Pragma(\"unroll\") for (int j = 0; j < NP; ++j) p[j] = par[j];\n  }\n};\n";
    return s;
  };
  s += adapter("");
  s += "extern \"C\" __global__ __launch_bounds__(ODE_BLOCK, 1) void ode_user_kernel(OdeDev D, OdeArgs a, const LsodaCoef* cf) {\n";
  s += "  ode_step_body<ModelUser, " + std::to_string(lanes) + ", 1, false>(D, a, cf);\n}\n";
  s += "extern \"C\" __global__ __launch_bounds__(ODE_BLOCK, 1) void ode_user_advance_kernel(OdeArgs a, OdeAdvArgs v, "
       "const LsodaCoef* cf) {\n";
  s += "  ode_advance_body<ModelUser, " + std::to_string(lanes) + ", 1>(a, v, cf);\n}\n";
  // the fixed-step sweeps (fixed_step.h): a plug-in has a right-hand side but no gate rates, so Euler and RK4 only
  // They promise bit-identical results from the single-step and the multi-step kernel, which holds only if no
  // multiply-add is contracted in one and not in the other (the compiler decides by context): a second copy of the
  // plug-in source with contraction off, in a namespace of its own; the LSODA kernels keep the first copy as it was.
  s += "namespace kn_fs {\n#pragma clang fp contract(off)\n";
  s += user;
  s += "\n";
  s += adapter("kn_fs");
  s += "}  // namespace kn_fs\n";
  const char* fs_name[2] = {"euler", "rk4"};
  const char* fs_id[2] = {"KN_FS_EULER", "KN_FS_RK4"};
  for (int k = 0; k < 2; ++k) {
    s += std::string("extern \"C\" __global__ __launch_bounds__(ODE_BLOCK) void ode_user_fixed_") + fs_name[k] +
         "_kernel(OdeDev D, OdeArgs a, int n_sub) {\n  ode_fixed_step_body<kn_fs::ModelUser, " + fs_id[k] + ">(D, a, n_sub);\n}\n";
    s += std::string("extern \"C\" __global__ __launch_bounds__(ODE_BLOCK) void ode_user_fixed_") + fs_name[k] +
         "_advance_kernel(OdeArgs a, OdeAdvArgs v, int n_sub) {\n  ode_fixed_advance_body<kn_fs::ModelUser, " + fs_id[k] +
         ">(a, v, n_sub);\n}\n";
  }
  return s;
}

int lanes_for(int ns) { return (ns == 1 || ns == 2 || ns == 4 || ns == 8) ? ns : 1; }

// compile for gfx950; `code` receives the code object, `log` the compiler's messages
int compile(int ns, int np, const std::string& user, std::vector<char>* code, std::string* log) {
  const std::string src = wrapper_source(ns, np, lanes_for(ns), user);
  const char* headers[3] = {SRC_LSODA_CORE, SRC_ODE_KERNEL, SRC_FIXED_STEP};
  const char* names[3] = {"lsoda_core.h", "ode_kernel.h", "fixed_step.h"};
  hiprtcProgram prog = nullptr;
  if (hiprtcCreateProgram(&prog, src.c_str(), "knpemi_user_model.hip", 3, headers, names) != HIPRTC_SUCCESS) {
    *log = "hiprtcCreateProgram failed";
    return KNPEMI_EHIP;
  }
  // the integrator keeps its state in registers: same flag as csrc/Makefile uses for kernels_ode.hip
  // (the same code generation options as kernels_ode.o, Makefile: no common-code sinking, instruction scheduling for ILP)
  const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-simplifycfg-sink-common=false",
                        "-mllvm", "-amdgpu-sched-strategy=max-ilp"};
  const hiprtcResult res = hiprtcCompileProgram(prog, 7, opts);
  size_t n = 0;
  if (hiprtcGetProgramLogSize(prog, &n) == HIPRTC_SUCCESS && n > 1) {
    log->assign(n, '\0');
    (void)hiprtcGetProgramLog(prog, &(*log)[0]);
  }
  if (res != HIPRTC_SUCCESS) {
    *log = std::string("hipRTC: ") + hiprtcGetErrorString(res) + "\n" + *log;
    (void)hiprtcDestroyProgram(&prog);
    return KNPEMI_EINVAL;
  }
  if (code) {
    size_t sz = 0;
    if (hiprtcGetCodeSize(prog, &sz) != HIPRTC_SUCCESS) { (void)hiprtcDestroyProgram(&prog); *log = "hiprtcGetCodeSize failed"; return KNPEMI_EHIP; }
    code->resize(sz);
    if (hiprtcGetCode(prog, code->data()) != HIPRTC_SUCCESS) { (void)hiprtcDestroyProgram(&prog); *log = "hiprtcGetCode failed"; return KNPEMI_EHIP; }
  }
  (void)hiprtcDestroyProgram(&prog);
  return KNPEMI_OK;
}

std::mutex g_cache_mutex;
std::map<std::string, std::vector<char>> g_code_cache;    // (ns, np, source) -> code object, per process

}  // namespace

// Compile only (no device needed): the CPU test suite checks plug-in sources with this, and a driver can validate a
// model before the first launch.  log_len bytes of the compiler's messages go to `log` (may be NULL).
extern "C" int knpemi_ode_compile_source(int n_states, int n_params, const char* rhs_source, char* log, size_t log_len) {
  if (!rhs_source || n_states < 1 || n_states > 16 || n_params < 1 || n_params > 128) {
    kn_set_error("knpemi_ode_compile_source: bad argument (1..16 states, 1..128 parameters)");
    return KNPEMI_EINVAL;
  }
  std::string msg;
  std::vector<char> code;
  const int rc = compile(n_states, n_params, rhs_source, &code, &msg);
  if (log && log_len) {
    const size_t n = std::min(log_len - 1, msg.size());
    std::memcpy(log, msg.data(), n);
    log[n] = '\0';
  }
  if (rc) { kn_set_error("membrane model source did not compile:\n" + msg); return rc; }
  std::lock_guard<std::mutex> lock(g_cache_mutex);
  g_code_cache[std::to_string(n_states) + "/" + std::to_string(n_params) + "/" + rhs_source] = std::move(code);
  return KNPEMI_OK;
}

int kn_rtc_bind(KnSweeps& sw, KnOdeModel& m, int n_states, int n_params, const char* rhs_source) {
  const std::string key = std::to_string(n_states) + "/" + std::to_string(n_params) + "/" + rhs_source;
  std::vector<char> code;
  {
    std::lock_guard<std::mutex> lock(g_cache_mutex);
    auto it = g_code_cache.find(key);
    if (it != g_code_cache.end()) code = it->second;
  }
  if (code.empty()) {
    std::string msg;
    const int rc = compile(n_states, n_params, rhs_source, &code, &msg);
    if (rc) { kn_set_error("membrane model source did not compile:\n" + msg); return rc; }
    std::lock_guard<std::mutex> lock(g_cache_mutex);
    g_code_cache[key] = code;
  }
  hipModule_t mod = nullptr;
  KN_HIP(hipModuleLoadData(&mod, code.data()));
  // the entry points wrapper_source() generates, [method][step, advance]; a plug-in has no gate rates: no Rush-Larsen
  const char* const names[4][2] = {{"ode_user_kernel", "ode_user_advance_kernel"},
                                   {"ode_user_fixed_euler_kernel", "ode_user_fixed_euler_advance_kernel"},
                                   {"ode_user_fixed_rk4_kernel", "ode_user_fixed_rk4_advance_kernel"},
                                   {nullptr, nullptr}};
  for (int k = 0; k < 4; ++k)
    for (int j = 0; j < 2; ++j) {
      m.rtc_kernel[k][j] = nullptr;
      if (names[k][j] && hipModuleGetFunction(&m.rtc_kernel[k][j], mod, names[k][j]) != hipSuccess) {
        (void)hipModuleUnload(mod);
        kn_set_error(std::string("hipModuleGetFunction(") + names[k][j] + ") failed");
        return KNPEMI_EHIP;
      }
    }
  m.rtc_module = mod;
  m.rtc_lanes = lanes_for(n_states);
  sw.rtc_modules.push_back(mod);
  return KNPEMI_OK;
}

int kn_rtc_launch(hipStream_t st, hipFunction_t fn, unsigned grid, void* params, size_t bytes) {
  void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, params, HIP_LAUNCH_PARAM_BUFFER_SIZE, &bytes, HIP_LAUNCH_PARAM_END};
  KN_HIP(hipModuleLaunchKernel(fn, grid, 1, 1, ODE_BLOCK, 1, 1, 0, st, nullptr, config));
  return KNPEMI_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The monitor of a plug-in: `__device__ void monitor(double t, const double* states, const double* parameters, double*
// monitored)` as HIP source (module attribute MONITOR_HIP, or translated from a Gotran-style Python `monitor` by
// knpemi.rhs_codegen), the counterpart of the Gotran modules' `monitor` the reference's figure scripts restate by hand
// (make_figures.py:169-195).  It is pasted under the record kernel's body (monitor_kernel.h: the very code of the shipped
// models' monitors) and compiled as a program of its own -- the sweeps' program is compiled from the same text as before.
namespace {

std::string monitor_wrapper_source(int ns, int np, int nm, const std::string& user) {
  std::string s;
  s += "#include \"monitor_kernel.h\"\n";
  s += "#pragma clang fp contract(off)\n";
  s += "// ---- plug-in source -------------------------------------------------------------\n";
  s += user;
  s += "\n// ---- adapter: what the record kernel's body evaluates per dof -----------------------\n";
  s += "struct MonUser {\n";
  s += "  static constexpr int NS = " + std::to_string(ns) + ", NP = " + std::to_string(np) + ", NM = " + std::to_string(nm) + ";\n";
  s += "  __device__ __forceinline__ static void eval(const OdeDev& D, const KnMonWatch& W, int q, double t, double (&out)[KN_MON_MAX]) {\n";
  s += "    double y[NS], row[NP], m[NM];\n";
  s += "    mon_load<NS, NP>(D, W, q, y, row);\n";
  s += "    _Pragma(\"unroll\") for (int i = 0; i < NM; ++i) m[i] = 0.0;\n";
  s += "    monitor(t, y, row, m);\n";
  s += "    _Pragma(\"unroll\") for (int i = 0; i < NM; ++i) out[i] = m[i];\n  }\n};\n";
  s += "extern \"C\" __global__ __launch_bounds__(MON_THREADS) void monitor_user_kernel(OdeDev D, KnMonArgs A) {\n";
  s += "  monitor_body<MonUser, false>(D, A);\n}\n";
  s += "extern \"C\" __global__ __launch_bounds__(MON_THREADS) void monitor_user_fields_kernel(OdeDev D, KnMonArgs A) {\n";
  s += "  monitor_body<MonUser, true>(D, A);\n}\n";
  return s;
}

int compile_monitor(int ns, int np, int nm, const std::string& user, std::vector<char>* code, std::string* log) {
  const std::string src = monitor_wrapper_source(ns, np, nm, user);
  const char* headers[5] = {SRC_LSODA_CORE, SRC_ODE_KERNEL, SRC_MONITOR_TABLE, SRC_RECORD_TAIL, SRC_MONITOR_KERNEL};
  const char* names[5] = {"lsoda_core.h", "ode_kernel.h", "monitor_table.h", "record_tail.h", "monitor_kernel.h"};
  hiprtcProgram prog = nullptr;
  if (hiprtcCreateProgram(&prog, src.c_str(), "knpemi_user_monitor.hip", 5, headers, names) != HIPRTC_SUCCESS) {
    *log = "hiprtcCreateProgram failed";
    return KNPEMI_EHIP;
  }
  // as kernels_monitor.o (Makefile): no multiply-add contracted
  const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off"};
  const hiprtcResult res = hiprtcCompileProgram(prog, 4, opts);
  size_t n = 0;
  if (hiprtcGetProgramLogSize(prog, &n) == HIPRTC_SUCCESS && n > 1) {
    log->assign(n, '\0');
    (void)hiprtcGetProgramLog(prog, &(*log)[0]);
  }
  if (res != HIPRTC_SUCCESS) {
    *log = std::string("hipRTC: ") + hiprtcGetErrorString(res) + "\n" + *log;
    (void)hiprtcDestroyProgram(&prog);
    return KNPEMI_EINVAL;
  }
  size_t sz = 0;
  if (hiprtcGetCodeSize(prog, &sz) != HIPRTC_SUCCESS) { (void)hiprtcDestroyProgram(&prog); *log = "hiprtcGetCodeSize failed"; return KNPEMI_EHIP; }
  code->resize(sz);
  if (hiprtcGetCode(prog, code->data()) != HIPRTC_SUCCESS) { (void)hiprtcDestroyProgram(&prog); *log = "hiprtcGetCode failed"; return KNPEMI_EHIP; }
  (void)hiprtcDestroyProgram(&prog);
  return KNPEMI_OK;
}

std::string monitor_key(int ns, int np, int nm, const char* src) {
  return "monitor/" + std::to_string(ns) + "/" + std::to_string(np) + "/" + std::to_string(nm) + "/" + src;
}
bool monitor_sizes_ok(int ns, int np, int nm) { return ns >= 1 && ns <= 16 && np >= 1 && np <= 128 && nm >= 1 && nm <= KN_MON_MAX; }

}  // namespace

// Compile only (no device needed), like knpemi_ode_compile_source.
extern "C" int knpemi_monitor_compile_source(int n_states, int n_params, int n_monitored, const char* monitor_source, char* log,
                                             size_t log_len) {
  if (!monitor_source || !monitor_sizes_ok(n_states, n_params, n_monitored)) {
    kn_set_error("knpemi_monitor_compile_source: bad argument (1..16 states, 1..128 parameters, 1..KNPEMI_MON_MAX quantities)");
    return KNPEMI_EINVAL;
  }
  std::string msg;
  std::vector<char> code;
  const int rc = compile_monitor(n_states, n_params, n_monitored, monitor_source, &code, &msg);
  if (log && log_len) {
    const size_t n = std::min(log_len - 1, msg.size());
    std::memcpy(log, msg.data(), n);
    log[n] = '\0';
  }
  if (rc) { kn_set_error("membrane monitor source did not compile:\n" + msg); return rc; }
  std::lock_guard<std::mutex> lock(g_cache_mutex);
  g_code_cache[monitor_key(n_states, n_params, n_monitored, monitor_source)] = std::move(code);
  return KNPEMI_OK;
}

int kn_rtc_monitor_bind(KnSweeps& sw, KnOdeModel& m, int n_monitored, const char* monitor_source) {
  if (!monitor_sizes_ok(m.n_states, m.n_params, n_monitored))
    return kn_fail(KNPEMI_EINVAL, "knpemi_monitor_bind_source: 1..KNPEMI_MON_MAX monitored quantities");
  const std::string key = monitor_key(m.n_states, m.n_params, n_monitored, monitor_source);
  std::vector<char> code;
  {
    std::lock_guard<std::mutex> lock(g_cache_mutex);
    auto it = g_code_cache.find(key);
    if (it != g_code_cache.end()) code = it->second;
  }
  if (code.empty()) {
    std::string msg;
    const int rc = compile_monitor(m.n_states, m.n_params, n_monitored, monitor_source, &code, &msg);
    if (rc) { kn_set_error("membrane monitor source did not compile:\n" + msg); return rc; }
    std::lock_guard<std::mutex> lock(g_cache_mutex);
    g_code_cache[key] = code;
  }
  hipModule_t mod = nullptr;
  KN_HIP(hipModuleLoadData(&mod, code.data()));
  hipFunction_t fn[2] = {nullptr, nullptr};
  const char* const names[2] = {"monitor_user_kernel", "monitor_user_fields_kernel"};
  for (int j = 0; j < 2; ++j)
    if (hipModuleGetFunction(&fn[j], mod, names[j]) != hipSuccess) {
      (void)hipModuleUnload(mod);
      return kn_fail(KNPEMI_EHIP, std::string("hipModuleGetFunction(") + names[j] + ") failed");
    }
  m.mon_kernel[0] = fn[0]; m.mon_kernel[1] = fn[1];
  m.n_monitored = n_monitored;
  sw.rtc_modules.push_back(mod);
  return KNPEMI_OK;
}

int kn_rtc_launch_monitor(hipStream_t st, hipFunction_t fn, unsigned grid, unsigned block, const OdeDev& dv, const KnMonArgs& a) {
  struct { OdeDev d; KnMonArgs a; } p{dv, a};
  size_t bytes = sizeof(p);
  void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &p, HIP_LAUNCH_PARAM_BUFFER_SIZE, &bytes, HIP_LAUNCH_PARAM_END};
  KN_HIP(hipModuleLaunchKernel(fn, grid, 1, 1, block, 1, 1, 0, st, nullptr, config));
  return KNPEMI_OK;
}
