// Monitored quantities of the shipped membrane models: the named intermediates of their right-hand sides.
//
// The reference's figure scripts re-derive these numbers by hand from checkpoints of every step
// (examples/local_astrocyte_depolarization/make_figures.py:169-195, 279-327: E_K, E_Na, E_Cl, i_kir, i_pump;
// examples/idealized_geometries/make_figures.py:146-149: E_Na, E_K; calibrate_initial_conditions/run_calibration.py:
// 148-212: the Kir and pump currents at rest).  The models of membrane_models.h compute every one of them inside
// `prepare` / `rhs` / `rates`; KnMonitor<Model>::eval hands them out, evaluated after the model's own prepare(row):
//
//   M f; f.prepare(row); double out[KnMonitor<M>::N]; KnMonitor<M>::eval(f, t, y, out);
//
// The expressions are those of `prepare` / `rhs` / `rates`, written in their order: true divisions, the library's exp / log
// where the model calls them, the model's own kn_* calls where `rhs` uses them (glial).  The totals I_Na, I_K, I_Cl are
// formed exactly as `rhs` forms them, pump terms included: on the host build they equal its side-effect currents bit for
// bit.  Units are the model's own.  At most KN_MON_MAX quantities per model, so a selection is a 32-bit mask.
//
// Like fixed_step.h this header compiles for the device (kernels_monitor.hip) and for the host (tests/native): it includes
// nothing but membrane_models.h, and no multiply-add of it may be contracted on one side and not on the other
// (kernels_monitor.hip is built with -ffp-contract=off as well).
#pragma once

#include "membrane_models.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define KN_MON_MAX 32

template <class M>
struct KnMonitor;

// hh_si and hh_mv share names, order and expressions; what differs are the constants of the stimulus and the units of u
#define KN_MON_HH_NAMES                                                                                              \
  "E_Na", "E_K", "i_pump", "g_Na", "g_K", "g_stim", "i_Na_leak", "i_Na_gated", "i_stim", "i_K_leak", "i_K_gated", "I_Na", \
      "I_K", "m_inf", "h_inf", "n_inf", "tau_m", "tau_h", "tau_n"

template <class M>
struct KnMonitorHH {
  static constexpr int N = 19;
  // period, decay time and end of the stimulus: the constants of the model's `rhs`
  template <class F>
  KN_HD static void eval_hh(const F& f, double t, const double* y, double period, double tau, double t_end, double* out) {
    const double m = y[0], h = y[1], n = y[2], V = y[3];
    const double g_Na = f.gNa * h * (m * m * m);
    const double n2 = n * n;
    const double g_K = f.gK * (n2 * n2);
    const double g_stim = f.stim * exp(-kn_fmod_period(t, period) / tau) * (t < t_end ? 1.0 : 0.0);
    out[0] = f.E_Na;
    out[1] = f.E_K;
    out[2] = f.i_pump;
    out[3] = g_Na;
    out[4] = g_K;
    out[5] = g_stim;
    out[6] = f.glNa * (V - f.E_Na);
    out[7] = g_Na * (V - f.E_Na);
    out[8] = g_stim * (V - f.E_Na);
    out[9] = f.glK * (V - f.E_K);
    out[10] = g_K * (V - f.E_K);
    out[11] = (f.glNa + g_Na + g_stim) * (V - f.E_Na) + 3 * f.i_pump;
    out[12] = (f.glK + g_K) * (V - f.E_K) - 2 * f.i_pump;
    double a[4], b[4];
    f.rates(t, y, a, b);
    out[13] = a[0] / (a[0] + b[0]);
    out[14] = a[1] / (a[1] + b[1]);
    out[15] = a[2] / (a[2] + b[2]);
    out[16] = 1.0 / (a[0] + b[0]);
    out[17] = 1.0 / (a[1] + b[1]);
    out[18] = 1.0 / (a[2] + b[2]);
  }
};

template <>
struct KnMonitor<ModelHHSI> : KnMonitorHH<ModelHHSI> {
  KN_HD static void eval(const ModelHHSI& f, double t, const double* y, double* out) {
    eval_hh(f, t, y, 0.03, 0.002, 125e-3, out);
  }
};
template <>
struct KnMonitor<ModelHHMV> : KnMonitorHH<ModelHHMV> {
  KN_HD static void eval(const ModelHHMV& f, double t, const double* y, double* out) {
    eval_hh(f, t, y, 30.0, 2.0, 125, out);
  }
};

#define KN_MON_GLIAL_NAMES "E_Na", "E_K", "E_Cl", "i_pump", "g_Kir", "i_Kir", "i_Na_leak", "i_Cl_leak", "I_Na", "I_K", "I_Cl"

template <>
struct KnMonitor<ModelGlial> {
  static constexpr int N = 11;
  KN_HD static void eval(const ModelGlial& f, double t, const double* y, double* out) {
    (void)t;
    const double V = y[0];
    const double dphi = V - f.E_K;
    const double C = 1 + kn_exp(kn_div(dphi + 18.5, 42.4));
    const double D = 1 + kn_exp(kn_div(-(118.6 + V), 44.1));
    const double g_Kir = kn_div(f.gfac, C * D);
    const double i_Kir = f.glK * g_Kir * (V - f.E_K);
    out[0] = f.E_Na;
    out[1] = f.E_K;
    out[2] = f.E_Cl;
    out[3] = f.i_pump;
    out[4] = g_Kir;
    out[5] = i_Kir;
    out[6] = f.glNa * (V - f.E_Na);
    out[7] = f.glCl * (V - f.E_Cl);
    out[8] = f.glNa * (V - f.E_Na) + 3 * f.i_pump;
    out[9] = i_Kir - 2 * f.i_pump;
    out[10] = f.glCl * (V - f.E_Cl);
  }
};

// the catalogue: number of quantities and names of shipped model `model_id` (KNPEMI_MODEL_*); 0 / NULL otherwise
inline int kn_monitor_count(int model_id) {
  return model_id == 0 || model_id == 1 ? KnMonitor<ModelHHSI>::N : (model_id == 2 ? KnMonitor<ModelGlial>::N : 0);
}
inline const char* kn_monitor_name(int model_id, int i) {
  static const char* const hh[] = {KN_MON_HH_NAMES};
  static const char* const glial[] = {KN_MON_GLIAL_NAMES};
  if (i < 0 || i >= kn_monitor_count(model_id)) return nullptr;
  return model_id == 2 ? glial[i] : hh[i];
}

// (contraction stays off for whatever follows the include: the one device translation unit that includes this header,
// kernels_monitor.hip, is compiled without it from its first line to its last)
