// Test-only host build of the PRODUCT membrane monitors (csrc/membrane_monitors.h + membrane_models.h) so that
// `pytest -m "not gpu"` can check them against a numpy restatement and against the models' own right-hand sides on the
// CPU, and the GPU tests can compare the device kernel with it.  Not shipped, not a fallback: the product's monitors only
// exist as the HIP kernel of csrc/kernels_monitor.hip.
#include "../../knp-emi-fenics-x_amd/csrc/membrane_monitors.h"

template <class M>
static int eval(double t, const double* y, const double* p, double* out) {
  M f;
  f.prepare(p);
  KnMonitor<M>::eval(f, t, y, out);
  return KnMonitor<M>::N;
}

// the side-effect currents of Model::rhs at (t, y) with the parameter row p: cur = {I_Na, I_K, I_Cl}
template <class M>
static void currents(double t, const double* y, const double* p, double* cur, int i_na, int i_k, int i_cl) {
  double copy[M::NP], dy[M::NS];
  for (int j = 0; j < M::NP; ++j) copy[j] = p[j];
  double* row = copy;
  M f;
  f.prepare(row);
  f.rhs(t, y, dy);
  f.finish(row);
  cur[0] = row[i_na]; cur[1] = row[i_k]; cur[2] = row[i_cl];
}

extern "C" int monitor_host_count(int model) { return kn_monitor_count(model); }
extern "C" const char* monitor_host_name(int model, int i) { return kn_monitor_name(model, i); }

// the quantities of model `model` at (t, y) with the parameter row p into out[count]; returns the count, 0: unknown model
extern "C" int monitor_host(int model, double t, const double* y, const double* p, double* out) {
  if (model == 0) return eval<ModelHHSI>(t, y, p, out);
  if (model == 1) return eval<ModelHHMV>(t, y, p, out);
  if (model == 2) return eval<ModelGlial>(t, y, p, out);
  return 0;
}

extern "C" int monitor_host_currents(int model, double t, const double* y, const double* p, double* cur) {
  if (model == 0) currents<ModelHHSI>(t, y, p, cur, 15, 16, 17);
  else if (model == 1) currents<ModelHHMV>(t, y, p, cur, 15, 16, 17);
  else if (model == 2) currents<ModelGlial>(t, y, p, cur, 5, 6, 7);
  else return -1;
  return 0;
}
