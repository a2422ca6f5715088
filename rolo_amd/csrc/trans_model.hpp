// The translation stage's trial cost as a quadratic in the translation, from the 30 sums of the stage's own linearisation (lm_step.hpp trans_step).
//
// Within the stage the correspondences, the Mahalanobis matrices M and the weights w are constant (those of the last rotation linearisation), the residual
// e = mean - (q + t) is linear in t, and the continuous-time term's vector dv - last / dt_{n-1} = -(g + t) / dt_n - last / dt_{n-1} is the same for every point (up to the
// rounding of (q - g) - (q + t)). With kappa = lam_over_n * inv_dtn^2 and the linearisation at t0 (trans_pass_compute / lmp_trans_body: H's translation block is
// sum w (1 + kappa) M, b's is -sum w (M e + lam_over_n inv_dtn M ctB), y0 is sum w (e^T M e + lam_over_n ctB^T M ctB)):
//   A = sum w M         = H[3:6, 3:6] / (1 + kappa)
//   v = sum w M e(t0)   = -b[3:6] - lam_over_n inv_dtn A ctB(t0)
//   c = sum w e^T M e   = y0 - lam_over_n ctB(t0)^T A ctB(t0)
//   cost(t0 + d)        = c - 2 d^T v + d^T A d + lam_over_n ctA(t0 + d)^T A ctA(t0 + d)
// ctA / ctB are the vector above with the `last` term of compute_t_error / of t3_linearize (they differ as written, LmState::lastA_q / lastB_q).
//
// Pure C++: device code (lm_step.hpp) and a host test program (tests/cpp/trans_model_test.cpp) compile the same two functions, each one fixed order of operations
// (no contraction into fused multiply-adds: the host compiler has none to offer by default, the device compiler is told so below).
#pragma once
#include <cmath>

#ifndef ROLO_TM_FN
#if defined(__HIPCC__)
#define ROLO_TM_FN __host__ __device__ inline
#else
#define ROLO_TM_FN inline
#endif
#endif

namespace rolo {

struct TransModelConsts {   // the stage's constants (lm_step.hpp trans_start / trans_consts)
  double lam_over_n, inv_dtn;
  double g[3], lastA_q[3], lastB_q[3];
};
struct TransModel {
  double A[6];   // xx xy xz yy yz zz
  double v[3], c;
  double t0[3];  // the linearisation point
  int valid;     // 0: an input was not finite — trans_model_cost answers NaN, never a number
};

ROLO_TM_FN bool tm_finite(double x) { return x - x == 0.0; }   // false for NaN and +-inf (isfinite without a header's host / device overload sets)
ROLO_TM_FN void tm_sym_mulv(const double* A, const double* x, double* y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  y[0] = (A[0] * x[0] + A[1] * x[1]) + A[2] * x[2];
  y[1] = (A[1] * x[0] + A[3] * x[1]) + A[4] * x[2];
  y[2] = (A[2] * x[0] + A[4] * x[1]) + A[5] * x[2];
}
ROLO_TM_FN double tm_dot(const double* a, const double* b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}
// -(g + t) / dt_n - last / dt_{n-1}: what every point's dv - last_q is in exact arithmetic
ROLO_TM_FN void tm_ct(const TransModelConsts& K, const double* t, const double* last_q, double* ct) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int i = 0; i < 3; i++) ct[i] = -(K.g[i] + t[i]) * K.inv_dtn - last_q[i];
}

// the model of the linearisation (H: 6 x 6 row-major, b: 6, y0) taken at t0
ROLO_TM_FN void trans_model_build(TransModel& m, const double* H, const double* b, double y0, const TransModelConsts& K, const double* t0) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  bool ok = tm_finite(y0) && tm_finite(K.lam_over_n) && tm_finite(K.inv_dtn);
  for (int i = 0; i < 36; i++) ok = ok && tm_finite(H[i]);
  for (int i = 0; i < 6; i++) ok = ok && tm_finite(b[i]);
  for (int i = 0; i < 3; i++) ok = ok && tm_finite(t0[i]) && tm_finite(K.g[i]) && tm_finite(K.lastA_q[i]) && tm_finite(K.lastB_q[i]);
  const double k1 = 1.0 + K.lam_over_n * K.inv_dtn * K.inv_dtn;
  m.A[0] = H[3 * 6 + 3] / k1; m.A[1] = H[3 * 6 + 4] / k1; m.A[2] = H[3 * 6 + 5] / k1;
  m.A[3] = H[4 * 6 + 4] / k1; m.A[4] = H[4 * 6 + 5] / k1; m.A[5] = H[5 * 6 + 5] / k1;
  double ctB[3], AcB[3];
  tm_ct(K, t0, K.lastB_q, ctB);
  tm_sym_mulv(m.A, ctB, AcB);
  const double s1 = K.lam_over_n * K.inv_dtn;
  for (int i = 0; i < 3; i++) { m.v[i] = -b[3 + i] - s1 * AcB[i]; m.t0[i] = t0[i]; }
  m.c = y0 - K.lam_over_n * tm_dot(ctB, AcB);
  for (int i = 0; i < 6; i++) ok = ok && tm_finite(m.A[i]);
  for (int i = 0; i < 3; i++) ok = ok && tm_finite(m.v[i]);
  m.valid = ok && tm_finite(m.c) ? 1 : 0;
}

// the cost compute_t_error would return at tt — NaN where the model is not valid, tt is not finite or the value is not
ROLO_TM_FN double trans_model_cost(const TransModel& m, const TransModelConsts& K, const double* tt) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double nan = __builtin_nan("");
  if (!m.valid || !tm_finite(tt[0]) || !tm_finite(tt[1]) || !tm_finite(tt[2])) return nan;
  double d[3], Ad[3], ctA[3], AcA[3];
  for (int i = 0; i < 3; i++) d[i] = tt[i] - m.t0[i];
  tm_sym_mulv(m.A, d, Ad);
  tm_ct(K, tt, K.lastA_q, ctA);
  tm_sym_mulv(m.A, ctA, AcA);
  const double y = ((m.c - 2.0 * tm_dot(d, m.v)) + tm_dot(d, Ad)) + K.lam_over_n * tm_dot(ctA, AcA);
  return tm_finite(y) ? y : nan;
}

}  // namespace rolo
