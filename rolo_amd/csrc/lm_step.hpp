// The scalar LM step — one lane, on the state in LDS — of every launch form of the LM iteration (passes.hip, lm_persist.hip): the LDLT solve, the exponentials, the
// trace, the rotation / 6-dof and the translation stage's step functions with their exits, and how the kernels stage the state through LDS.
#pragma once
#include "rolo_internal.hpp"
#include "lm_begin.hpp"
#include "trans_model.hpp"
#include "dev_math.hpp"

namespace rolo {
namespace {

// ---- scalar LM logic (one thread) -----------------------------------------------------------------------
template <int N>
ROLO_DEV void ldlt_solve(const double* Hfull /* 6x6 storage, row stride 6 */, double lambda, const double* b, double* x) {
  // Solves (H + lambda I) x = -b by an LDL^T factorisation of the lower triangle. The reference uses Eigen::LDLT
  // (diagonal pivoting); H + lambda I is symmetric positive definite here, for which the unpivoted factorisation is
  // backward stable as well, so the two agree to rounding (checked against the oracle's pivoted solve by the parity
  // tests). No pivoting means no dynamic indexing: every loop unrolls and the whole solve lives in registers
  // instead of scratch memory (the pivoted version cost ~800 scratch round trips per controller launch).
  double L[N][N];
  double D[N];
#pragma unroll
  for (int j = 0; j < N; j++) {
    double d = Hfull[j * 6 + j] + lambda;
#pragma unroll
    for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k] * D[k];
    D[j] = d;
    const double inv = (d != 0.0) ? 1.0 / d : 0.0;
#pragma unroll
    for (int i = j + 1; i < N; i++) {
      double v = Hfull[i * 6 + j];
#pragma unroll
      for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k] * D[k];
      L[i][j] = v * inv;
    }
  }
  double y[N];
#pragma unroll
  for (int i = 0; i < N; i++) {
    double v = -b[i];
#pragma unroll
    for (int k = 0; k < i; k++) v -= L[i][k] * y[k];
    y[i] = v;
  }
#pragma unroll
  for (int i = 0; i < N; i++) y[i] = (D[i] != 0.0) ? y[i] / D[i] : 0.0;
#pragma unroll
  for (int i = N - 1; i >= 0; i--) {
    double v = y[i];
#pragma unroll
    for (int k = i + 1; k < N; k++) v -= L[k][i] * y[k];
    y[i] = v;
  }
#pragma unroll
  for (int i = 0; i < N; i++) x[i] = y[i];
}

// sin / cos of a small angle by their Taylor series (|x| <= 0.5: the 10th term is below 2e-23 relative) — the half angle of an LM step is
// a few 1e-2 at most; the library sincos() is ~150 instructions of range reduction on the controller's one serial lane. Agrees with libm
// to the last ulp or two, far inside what the LM decisions can see (the oracle comparison of the traces is the test).
ROLO_DEV void sincos_small(double x, double* s, double* c) {
  if (fabs(x) > 0.5) { sincos(x, s, c); return; }
  const double z = x * x;
  double ps = -1.0 / 121645100408832000.0;            // -1/19!
  ps = fma(ps, z, 1.0 / 355687428096000.0);           //  1/17!
  ps = fma(ps, z, -1.0 / 1307674368000.0);            // -1/15!
  ps = fma(ps, z, 1.0 / 6227020800.0);                //  1/13!
  ps = fma(ps, z, -1.0 / 39916800.0);                 // -1/11!
  ps = fma(ps, z, 1.0 / 362880.0);                    //  1/9!
  ps = fma(ps, z, -1.0 / 5040.0);                     // -1/7!
  ps = fma(ps, z, 1.0 / 120.0);                       //  1/5!
  ps = fma(ps, z, -1.0 / 6.0);                        // -1/3!
  *s = fma(x * z, ps, x);
  double pc = 1.0 / 6402373705728000.0;               //  1/18!
  pc = fma(pc, z, -1.0 / 20922789888000.0);           // -1/16!
  pc = fma(pc, z, 1.0 / 87178291200.0);               //  1/14!
  pc = fma(pc, z, -1.0 / 479001600.0);                // -1/12!
  pc = fma(pc, z, 1.0 / 3628800.0);                   //  1/10!
  pc = fma(pc, z, -1.0 / 40320.0);                    // -1/8!
  pc = fma(pc, z, 1.0 / 720.0);                       //  1/6!
  pc = fma(pc, z, -1.0 / 24.0);                       // -1/4!
  pc = fma(pc, z, 0.5);                               //  1/2!
  *c = fma(-z, pc, 1.0);
}

ROLO_DEV void so3_exp_R(const double* w, double* R) {  // so3.hpp:59-77 + Quaterniond::toRotationMatrix
  const double theta_sq = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double imag, real;
  if (theta_sq < 1e-10) {
    const double q4 = theta_sq * theta_sq;
    imag = 0.5 - 1.0 / 48.0 * theta_sq + 1.0 / 3840.0 * q4;
    real = 1.0 - 1.0 / 8.0 * theta_sq + 1.0 / 384.0 * q4;
  } else {
    const double theta = sqrt(theta_sq), half = 0.5 * theta;
    double sh, ch;
    sincos_small(half, &sh, &ch);
    imag = sh / theta;
    real = ch;
  }
  const double qw = real, qx = imag * w[0], qy = imag * w[1], qz = imag * w[2];
  const double tx = 2 * qx, ty = 2 * qy, tz = 2 * qz;
  const double twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
  R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

ROLO_DEV void se3_exp_Rt(const double* a, double* R, double* t) {  // so3.hpp:80-103
  const double wx = a[0], wy = a[1], wz = a[2];
  const double theta = sqrt(wx * wx + wy * wy + wz * wz);
  so3_exp_R(a, R);
  double V[9];
  if (theta < 1e-10) {
    for (int i = 0; i < 9; i++) V[i] = R[i];
  } else {
    const double O[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
    double O2[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) O2[i * 3 + j] = O[i * 3] * O[j] + O[i * 3 + 1] * O[3 + j] + O[i * 3 + 2] * O[6 + j];
    const double th2 = theta * theta;
    const double c1 = (1.0 - cos(theta)) / th2, c2 = (theta - sin(theta)) / (th2 * theta);
    for (int i = 0; i < 9; i++) V[i] = ((i % 4 == 0) ? 1.0 : 0.0) + c1 * O[i] + c2 * O2[i];
  }
  for (int i = 0; i < 3; i++) t[i] = V[i * 3] * a[3] + V[i * 3 + 1] * a[4] + V[i * 3 + 2] * a[5];
}

// (everything the controller runs is templated on the degrees of freedom: with a run-time count the loops below stay loops of dependent
// LDS accesses on ONE lane, and that lane's latency is the controller's whole duration)
template <int DOF>
ROLO_DEV void unpack_hb(LmState* __restrict__ st, const double* __restrict__ S) {
  int t = 0;
#pragma unroll
  for (int i = 0; i < DOF; i++) {
#pragma unroll
    for (int j = 0; j <= i; j++) { const double v = S[V_H + t]; st->H[i * 6 + j] = v; st->H[j * 6 + i] = v; t++; }
  }
#pragma unroll
  for (int i = 0; i < DOF; i++) st->b[i] = S[V_B + i];
  st->y0 = S[V_Y];
  st->n_corr = (int)(S[V_N] + 0.5);
}

// ONE: `trace` is a single record (the resident kernel's LDS slot: a wavefront other than the stepping one copies it to the buffer, lm_persist_kernel)
template <int DOF, bool ONE = false>
ROLO_DEV void trace_push(LmState* __restrict__ st, rolo_trace_rec* __restrict__ trace, int stage, int accepted, double yi, double rho) {
  if (!trace || st->trace_count >= TRACE_CAP) { st->trace_count++; return; }
  rolo_trace_rec& r = trace[ONE ? 0 : st->trace_count];
  st->trace_count++;
  r.stage = stage; r.outer = st->outer; r.trial = st->trial; r.accepted = accepted;
  r.y0 = st->y0; r.yi = yi; r.rho = rho; r.lambda = st->lambda;
  double dn = 0;
#pragma unroll
  for (int i = 0; i < DOF; i++) dn += st->d[i] * st->d[i];
  r.dnorm = sqrt(dn);
}
// the record of a converged-but-rejected rotation trial once more, for the repeat of that trial the step answers from its kept cost (rot_step_t): the state's outer / trial
// apart, the record pushed last. ONE: the slot keeps that first record and only the count advances — lmp_trace_flush writes the repeats from it.
template <int DOF, bool ONE>
ROLO_DEV void trace_push_repeat(LmState* __restrict__ st, rolo_trace_rec* __restrict__ trace, double yi, double rho) {
  if (ONE) { st->trace_count++; return; }
  trace_push<DOF, false>(st, trace, 0, 2, yi, rho);
}

// The damping update lambda * max(1/3, 1 - pow(2 rho - 1, 3)) (lsq_registration_impl.hpp:129, 262, 318): std::pow(double, int) is glibc's pow, whose result is the
// correctly rounded cube but for arguments within ~0.02 ulp of a rounding tie; q * q * q rounds twice and lands one ulp off for about a quarter of all q. The cube here
// carries the rounding errors of both products along (two-product through fma) and rounds once: lambda — and with it every later step of the stage — follows the CPU's bits.
ROLO_DEV double cube_rn(double q) {
  const double p = q * q, ep = fma(q, q, -p);        // q^2 = p + ep exactly
  const double r = p * q, er = fma(p, q, -r);        // p q = r + er exactly
  return r + (er + ep * q);
}
ROLO_DEV double lm_lambda_after_accept(double lambda, double rho) { return lambda * fmax(1.0 / 3.0, 1 - cube_rn(2 * rho - 1)); }

// ---- rotation / 6-dof stage -------------------------------------------------------------------------------
ROLO_DEV bool delta_converged(const LmState* __restrict__ st, bool rot_only) {  // lsq_registration_impl.hpp:182-191 / :328-335
  const double ir = st->inv_rot_eps;   // (1.0 / eps) * |.| as the reference writes it; the quotient is formed once per frame (rot_begin_dev)
  double rmax = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) rmax = fmax(rmax, ir * fabs(st->delta_R[i] - ((i % 4 == 0) ? 1.0 : 0.0)));
  if (rot_only) return rmax < 1;
  const double it = st->inv_trans_eps;
  double tmax = 0;
#pragma unroll
  for (int i = 0; i < 3; i++) tmax = fmax(tmax, it * fabs(st->delta_t[i]));
  return fmax(rmax, tmax) < 1;
}

template <int DOF>
ROLO_DEV void rot_compute_step(LmState* __restrict__ st) {
  if constexpr (DOF == 3) {
    ldlt_solve<3>(st->H, st->lambda, st->b, st->d);
    st->d[3] = st->d[4] = st->d[5] = 0;
    so3_exp_R(st->d, st->delta_R);
    st->delta_t[0] = st->delta_t[1] = st->delta_t[2] = 0;
  } else {
    ldlt_solve<6>(st->H, st->lambda, st->b, st->d);
    se3_exp_Rt(st->d, st->delta_R, st->delta_t);
  }
  // xi = delta * x0
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) st->xt_R[i * 3 + j] = st->delta_R[i * 3] * st->x0_R[j] + st->delta_R[i * 3 + 1] * st->x0_R[3 + j] + st->delta_R[i * 3 + 2] * st->x0_R[6 + j];
    st->xt_t[i] = st->delta_R[i * 3] * st->x0_t[0] + st->delta_R[i * 3 + 1] * st->x0_t[1] + st->delta_R[i * 3 + 2] * st->x0_t[2] + st->delta_t[i];
  }
  lm_set_rrt(st->xt_S, st->xt_R);
}

template <int DOF>
ROLO_DEV void rot_begin_outer(LmState* __restrict__ st) {
  if (st->optimizer == ROLO_OPT_GN) st->lambda = 0.0;
  else if (st->lambda < 0.0) {
    double m = 0;
#pragma unroll
    for (int i = 0; i < DOF; i++) m = fmax(m, fabs(st->H[i * 7]));
    st->lambda = st->lm_init * m;
  }
  st->nu = 2.0; st->trial = 0;
  rot_compute_step<DOF>(st);
}

ROLO_DEV void trans_compute_step(LmState* st) {
  ldlt_solve<6>(st->H, st->lambda, st->b, st->d);
  double Rd[9];
  se3_exp_Rt(st->d, Rd, st->delta_t);
  for (int i = 0; i < 3; i++) st->tt[i] = st->delta_t[i] + st->t0[i];
}
ROLO_DEV void trans_begin_outer(LmState* st) {
  if (st->lambda < 0.0) { double m = 0; for (int i = 0; i < 6; i++) m = fmax(m, fabs(st->H[i * 7])); st->lambda = st->lm_init * m; }
  st->nu = 2.0; st->trial = 0;
  trans_compute_step(st);
}
// the per-stage constants of the translation passes (same IEEE quotients every lane used to form for itself)
ROLO_DEV void trans_consts(LmState* st) {
  double lastA[3] = {1.0, 0.0, 0.0}, lastB[3] = {0.0, 0.0, 0.0};
  if (st->q2_intended) for (int i = 0; i < 3; i++) { lastA[i] = st->l[i]; lastB[i] = st->l[i]; }
  for (int i = 0; i < 3; i++) { st->lastA_q[i] = lastA[i] / st->dtn1; st->lastB_q[i] = lastB[i] / st->dtn1; }
  st->inv_dtn = 1.0 / st->dtn;
}
ROLO_DEV void trans_start(LmState* st) {  // lsq_registration_impl.hpp:55-61
  trans_consts(st);
  st->stage = 2; st->phase = 0; st->lin_skip = 0; st->outer = 0; st->trial = 0; st->lambda = -1.0;
  st->trans_done = 0; st->trans_failed = 0; st->trans_outer = 0; st->trans_passes = 0; st->trans_cost_only = 0; st->trans_modelled = 0; st->trans_lin_extra = 0; st->tm_free_lin = 0;
  for (int i = 0; i < 3; i++) st->tt[i] = st->t0[i];
  // lambda_/pt_size: float / size_t -> float (rot_vgicp.hpp:124, rot_vgicp_impl.hpp:557)
  st->lam_over_n = (double)(st->ct_lambda / (float)st->tr_n_corr);
  if (st->tr_n_corr <= 0) { st->error = ROLO_ENOCORR; st->trans_failed = 1; st->trans_done = 1; st->stage = 0; }
}

ROLO_DEV void rot_finish(LmState* st, bool converged, bool failed) {
  st->rot_done = 1; st->rot_converged = converged ? 1 : 0; st->rot_failed = failed ? 1 : 0;
  // outer iterations STARTED = nr_iterations_ + 1 (lsq_registration_impl.hpp:163): `outer` counts the completed ones, and a step that returns false ("lm not converged!!",
  // :166-169) leaves the loop inside an iteration it never completes
  st->rot_outer = st->outer + (failed && !st->error ? 1 : 0); st->rot_ncorr = st->tr_n_corr;
  if (st->run_trans && !st->error) trans_start(st);
  else st->stage = 0;
}

template <int DOF, bool ONE = false>
ROLO_DEV void rot_step_t(LmState* __restrict__ st, const double* __restrict__ S, rolo_trace_rec* __restrict__ trace) {
  constexpr int dof = DOF;
  st->rot_passes++;
  if (st->phase == 1 && st->lin_skip) st->rot_cost_only++;
  if (st->phase == 0) {
    // max_iterations <= 0: the loop of computeTransformation (:161) never runs — no linearisation, no correspondences, the guess comes back (this first pass was evaluated for nothing)
    if (st->outer == 0 && st->fixed_iterations <= 0 && st->max_iterations <= 0) { st->tr_n_corr = 0; st->n_corr = 0; rot_finish(st, false, false); return; }
    for (int i = 0; i < 9; i++) st->x0_R[i] = st->xt_R[i];
    for (int i = 0; i < 6; i++) st->x0_S[i] = st->xt_S[i];
    for (int i = 0; i < 3; i++) st->x0_t[i] = st->xt_t[i];
    unpack_hb<DOF>(st, S);
    st->tr_cur = st->cur; st->tr_n_corr = st->n_corr;
    for (int i = 0; i < 9; i++) st->tr_R[i] = st->x0_R[i];
    for (int i = 0; i < 6; i++) st->tr_S[i] = st->x0_S[i];
    if (st->n_corr <= 0) { st->error = ROLO_ENOCORR; rot_finish(st, false, true); return; }
    st->phase = 1; st->lin_skip = 0;
    rot_begin_outer<DOF>(st);
    // lm_max_iterations <= 0: the trial loop (:233, :287) has no iteration — the step returns false right after its linearisation (Gauss-Newton has no such loop)
    if (st->optimizer != ROLO_OPT_GN && st->lm_max <= 0) rot_finish(st, false, true);
    return;
  }
  const double yi = S[V_YI];
  double den = 0;
#pragma unroll
  for (int i = 0; i < dof; i++) den += st->d[i] * (st->lambda * st->d[i] - st->b[i]);
  const double rho = (st->y0 - yi) / den;
  const bool gn = st->optimizer == ROLO_OPT_GN;
  if (!gn && rho < 0) {
    if (delta_converged(st, dof == 3)) {  // returns true without moving x0
      trace_push<DOF, ONE>(st, trace, 0, 2, yi, rho);
      st->outer++;
      bool done = st->fixed_iterations > 0 ? (st->outer >= st->fixed_iterations) : true;
      if (done) { rot_finish(st, true, false); return; }
      // the reference re-linearises at the same x0: identical H, b, y0, correspondences — and, lambda staying what this trial's step was solved with, the identical
      // step: d, delta and xt are already what rot_begin_outer's LDLT + exponential would write again, bit for bit (the scalar step is a third of this launch)
      st->nu = 2.0; st->trial = 0;
      st->lin_skip = st->spec_lin;   // a rejected trial: the next pass evaluates its trial's cost alone (LmState::lin_skip)
      if (!st->keep_cost) return;    // ROLO_LM_KEEP_COST=0 (the A/B): the repeats below are passes of their own
      // ... one step further: the pass that would follow evaluates the cost of THIS xt against the correspondences of THIS buffer `cur` with the Mahalanobis matrices of
      // THIS x0 (the cache is M(x0) again whenever a pass reads it; the passes without one invert at x0 themselves), every point's term formed and the rows summed in the
      // same fixed order by the same launch form: the yi it returns is the one above, bit for bit. y0, lambda, d and b are untouched, so rho is the one above, negative
      // again, and delta has not moved, so delta_converged holds again: the step would stand exactly here with outer one higher and trial = 0 — until the forced
      // iterations are used up (only fixed_iterations > 0 comes here). DOF 3 and 6 alike: nothing above depends on it. With spec_lin = 0 that pass would also run its (B)
      // half at xt; it writes corr[cur ^ 1], which is not current and is written again before anything reads it (it becomes current only through an accepted trial's own
      // (B) half or a phase-0 pass), and the resident kernel's cache, which is refilled on demand: neither is observable. So every remaining iteration is taken here: its
      // trace record, its counts (rot_passes / rot_cost_only stay the solve's trials; rot_kept says how many of them cost no pass) and the bookkeeping of the exit above.
      while (!done) {
        st->rot_passes++; st->rot_kept++;
        if (st->lin_skip) st->rot_cost_only++;
        trace_push_repeat<DOF, ONE>(st, trace, yi, rho);
        st->outer++;
        done = st->outer >= st->fixed_iterations;
      }
      rot_finish(st, true, false);
      return;
    }
    trace_push<DOF, ONE>(st, trace, 0, 0, yi, rho);
    st->lambda = st->nu * st->lambda; st->nu = 2 * st->nu;
    st->trial++;
    if (st->trial >= st->lm_max) { rot_finish(st, false, true); return; }  // "lm not converged!!"
    rot_compute_step<DOF>(st);
    st->lin_skip = st->spec_lin;
    return;
  }
  trace_push<DOF, ONE>(st, trace, 0, 1, gn ? NAN : yi, gn ? NAN : rho);
  for (int i = 0; i < 9; i++) st->x0_R[i] = st->xt_R[i];
  for (int i = 0; i < 6; i++) st->x0_S[i] = st->xt_S[i];
  for (int i = 0; i < 3; i++) st->x0_t[i] = st->xt_t[i];
  if (!gn) st->lambda = lm_lambda_after_accept(st->lambda, rho);
  if (dof == 6) for (int i = 0; i < 36; i++) st->final_H[i] = st->H[i];  // final_hessian_ = H
  st->outer++;
  const bool conv = delta_converged(st, false);
  const bool done = st->fixed_iterations > 0 ? (st->outer >= st->fixed_iterations) : (conv || st->outer >= st->max_iterations);
  if (done) { rot_finish(st, conv, false); return; }
  if (st->lin_skip) {   // the accepted trial's pass carried no linearisation (the bet after a rejection was "rejected again"): the next pass is so3_linearize(x0_new) alone —
    st->cur ^= 1; st->phase = 0; st->lin_skip = 0;   // phase 0 = "linearise at xt (= x0 now) into corr[cur], then begin the outer iteration": the state after it is the one below
    return;
  }
  // next outer iteration: the (B) half of this pass IS so3_linearize(x0_new)
  unpack_hb<DOF>(st, S);
  st->cur ^= 1;
  st->tr_cur = st->cur; st->tr_n_corr = st->n_corr;
  for (int i = 0; i < 9; i++) st->tr_R[i] = st->x0_R[i];
  for (int i = 0; i < 6; i++) st->tr_S[i] = st->x0_S[i];
  if (st->n_corr <= 0) { st->error = ROLO_ENOCORR; rot_finish(st, false, true); return; }
  rot_begin_outer<DOF>(st);
}

ROLO_DEV void rot_step(LmState* __restrict__ st, const double* __restrict__ S, rolo_trace_rec* __restrict__ trace) {
  if (st->optimizer == ROLO_OPT_SO3_LM) rot_step_t<3>(st, S, trace);
  else rot_step_t<6>(st, S, trace);
}

ROLO_DEV bool t_converged(const LmState* __restrict__ st) {  // :142-148
  const double it = st->inv_trans_eps;
  double m = 0;
#pragma unroll
  for (int i = 0; i < 3; i++) m = fmax(m, it * fabs(st->delta_t[i]));
  return m < 1;
}
ROLO_DEV void trans_finish(LmState* st, bool failed) {
  st->trans_done = 1; st->trans_failed = failed ? 1 : 0; st->trans_outer = st->outer + (failed ? 1 : 0) /* iterations started: rot_finish */; st->stage = 0;
}

// One call of the translation stage's scalar step: the sums of the pass that just ran, then — LmState::trans_model — every trial the step can answer itself.
// Within the stage a trial's cost is a quadratic in the translation whose coefficients are in the sums of the stage's linearisation (trans_model.hpp). So once a
// linearisation has been unpacked here (a linearise-only pass, or the (B) half of an accepted trial's full pass), the trials that follow need no pass: each turn of the
// loop below is one trial of lsq_registration_impl.hpp:98-141 — the same rho, the same accept / reject / converged / lm_max / max_iterations exits, the same damping —
// whose yi is the pass's (`real`: the first turn of a call that found a trial pending) or the model's. A modelled trial leaves its trace record and is counted in
// trans_passes / trans_cost_only as if its pass had run (lin_skip says, as for a real one, whether that pass would have been a cost-only one) and in trans_modelled.
// The call ends when the stage ends, when a trial needs a pass (no valid model: the switch is off, the scripted hook, sums that are not finite, a cost that is not), or
// when an accepted trial needs the linearisation at the new t0: a linearise-only pass (phase = 0) — the exit for a trial accepted on a cost-only pass. Where a modelled
// trial's pass would have been a full one, its (B) half WAS that linearisation (the same sums, bit for bit: nothing of (B) depends on the phase) and the solve counts no
// further pass: tm_free_lin, and the step that consumes the pass counts it in trans_lin_extra.
// ONE (the resident kernel): `trace` is the LDS slot, which takes the first record of a call (another wavefront copies it to the buffer: lmp_trace_flush); every further
// record goes straight to the buffer `trace_g`, written by the stepping lane. Beyond TRACE_CAP only the count advances, as everywhere.
// (One loop with the step computed in two places — opening an outer iteration, after a rejection: as a function of its own behind the parent's step, with four inlined
// copies of the LDLT and the exponential, the resident kernel's step call needed 256 registers and 524 bytes of stack, and the kernel's scratch went from 272 to 924 bytes
// per lane, and the headline fell although the kernel alone was shorter: profiles/DEAD_ENDS.md round 18.)
template <bool ONE = false>
ROLO_DEV void trans_step(LmState* __restrict__ st, const double* __restrict__ S, rolo_trace_rec* __restrict__ trace, rolo_trace_rec* __restrict__ trace_g = nullptr) {
  const int tc_in = st->trace_count;
  if (st->phase == 0 && st->tm_free_lin) { st->tm_free_lin = 0; st->trans_lin_extra++; }
  else st->trans_passes++;
  if (st->phase == 1 && st->lin_skip) st->trans_cost_only++;
  if (st->phase == 0 && st->outer == 0 && st->max_iterations <= 0) { trans_finish(st, false); return; }   // the loop of computeTranslation (:63) never runs: the start value comes back
  // (the constants are read from the state where they are used, and the model lives there: nothing of it is held in registers across the next step's LDLT)
  auto consts = [&]() {
    TransModelConsts K;
    K.lam_over_n = st->lam_over_n; K.inv_dtn = st->inv_dtn;
#pragma unroll
    for (int i = 0; i < 3; i++) { K.g[i] = st->g[i]; K.lastA_q[i] = st->lastA_q[i]; K.lastB_q[i] = st->lastB_q[i]; }
    return K;
  };
  auto push = [&](int accepted, double yi, double rho) {
    if (ONE && st->trace_count != tc_in) trace_push<6, false>(st, trace ? trace_g : nullptr, 1, accepted, yi, rho);
    else trace_push<6, ONE>(st, trace, 1, accepted, yi, rho);
  };
  bool unpack = st->phase == 0;   // the sums hold a linearisation to open an outer iteration with
  bool real = !unpack;            // the sums hold the cost of the trial that is pending
  bool model = false;             // st->tm is the model of the linearisation in H, b, y0
  while (true) {
    // (a turn of the loop starts from the state in memory: nothing that stays the same from trial to trial — H, b, the model, the stage's constants — is to be carried
    // in registers across the turns; the resident kernel pays for every register this call clobbers with spills around it)
    asm volatile("" ::: "memory");
    if (unpack) {
      const bool first = st->phase == 0;
      const int keep = st->n_corr;
      unpack_hb<6>(st, S);
      st->n_corr = keep;
      st->phase = 1; st->lin_skip = 0;
      trans_begin_outer(st);
      if (first && st->lm_max <= 0) { trans_finish(st, true); return; }   // no trial at all (:98): "lm not converged!!" right after the linearisation
      unpack = false; real = false;
      if (st->trans_model && st->tr_n_corr > 0) { trans_model_build(st->tm, st->H, st->b, st->y0, consts(), st->t0); model = st->tm.valid != 0; }
    }
    double yi;
    if (real) yi = S[V_YI];
    else {
      if (!model) return;            // the pass the state asks for runs
      yi = trans_model_cost(st->tm, consts(), st->tt);
      if (!(yi == yi)) return;       // not a cost: likewise
      st->trans_passes++; st->trans_modelled++;
      if (st->lin_skip) st->trans_cost_only++;
    }
    double den = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) den += st->d[i] * (st->lambda * st->d[i] - st->b[i]);
    const double rho = (st->y0 - yi) / den;
    if (rho < 0) {
      if (t_converged(st)) { push(2, yi, rho); st->outer++; trans_finish(st, false); return; }
      push(0, yi, rho);
      st->lambda = st->nu * st->lambda; st->nu = 2 * st->nu;
      st->trial++;
      if (st->trial >= st->lm_max) { trans_finish(st, true); return; }
      trans_compute_step(st);
      st->lin_skip = st->spec_lin;   // a rejected trial: the next pass evaluates its trial's cost alone
      real = false;
      continue;
    }
    push(1, yi, rho);
    for (int i = 0; i < 3; i++) st->t0[i] = st->tt[i];
    st->lambda = lm_lambda_after_accept(st->lambda, rho);
    st->outer++;
    const bool conv = t_converged(st);
    if (conv || st->outer >= st->max_iterations) { trans_finish(st, false); return; }
    if (st->lin_skip || !real) {   // accepted on a cost-only pass, or from the model: the next pass is t3_linearize at tt (= t0 now) alone
      if (!st->lin_skip) st->tm_free_lin = 1;
      st->phase = 0; st->lin_skip = 0;
      return;
    }
    unpack = true;   // the (B) half of this pass is that linearisation
  }
}

// a peer or a row never answered: both stages end with ROLO_ECOMM instead of waiting forever
ROLO_DEV void lm_fail_comm(LmState* st) { st->error = ROLO_ECOMM; st->stage = 0; st->rot_done = 1; st->rot_failed = 1; st->trans_done = 1; st->trans_failed = 1; }

// ---- the LM state through LDS ---------------------------------------------------------------------------------------------------------------------------------
// the scalar LM step touches ~150 fields: the kernels stage the whole state through LDS (one coalesced read, one write) instead of paying a global-memory round trip
// per field from a single lane. The read has an issue half and a landing half: what else a kernel fetches goes between them, so the launch pays one round trip.
static_assert(sizeof(LmState) % sizeof(int) == 0, "LmState must be int-copyable");
constexpr int LM_STATE_WORDS = sizeof(LmState) / sizeof(int);
template <int THREADS>
struct StateFetch {
  int w[(LM_STATE_WORDS + THREADS - 1) / THREADS];
  ROLO_DEV void issue(const LmState* st) {
    const int* g = reinterpret_cast<const int*>(st);
#pragma unroll
    for (int k = 0; k < (LM_STATE_WORDS + THREADS - 1) / THREADS; k++) { const int i = threadIdx.x + THREADS * k; w[k] = i < LM_STATE_WORDS ? g[i] : 0; }
  }
  ROLO_DEV void land(LmState* lds) const {
    int* l = reinterpret_cast<int*>(lds);
#pragma unroll
    for (int k = 0; k < (LM_STATE_WORDS + THREADS - 1) / THREADS; k++) { const int i = threadIdx.x + THREADS * k; if (i < LM_STATE_WORDS) l[i] = w[k]; }
  }
};
// the whole state from one memory to another by the workgroup's THREADS threads (LDS -> the device's copy, LDS -> the pinned host copy, the device's copy -> LDS)
template <int THREADS>
ROLO_DEV void state_copy(LmState* dst, const LmState* src) {
  int* d = reinterpret_cast<int*>(dst);
  const int* s = reinterpret_cast<const int*>(src);
  for (int w = threadIdx.x; w < LM_STATE_WORDS; w += THREADS) d[w] = s[w];
}

}  // namespace
}  // namespace rolo
