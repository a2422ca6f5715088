// Pose-graph optimisation on gfx950: the back end's saveKeyFramesAndFactor / addOdomFactor / addLoopFactor / addPriorFactor / correctPoses (reference
// src/backMapping.cpp:1094-1320) as a BATCH minimiser of the same objective, built from the same factors and noise models. The reference hands the graph to iSAM2,
// which is not in its tree: the contract is the statement in include/rolo_hip.h, which tests/pgo_twin.py restates in numpy; parity with GTSAM is unpinned.
//
// MI355X design, everything in fp64 and every sum in a fixed order (no atomics: the same bits on every run):
//   pgo_linearize_kernel     one factor per thread: error, whitened Jacobians, the factor's five blocks and its cost term into the factor's own slot; a between
//                            factor under a Cauchy loss (performSCLoopClosure's Robust noise, :2464-2470) scales all three by sqrt(w) first and its cost term is rho
//   pgo_assemble_kernel      36 lanes per pose gather the slots of its incident factors in factor order (CSR incidence list kept by the host, the changed tail
//                            uploaded): diagonal block, chain block H[k, k+1], gradient; pgo_chord_kernel packs the off-chain blocks
//   pgo_solve_kernel         ONE workgroup of 1024 threads, __syncthreads only: block cyclic reduction of the block-tridiagonal part T of H + lambda I (6 x 6 blocks,
//                            padded with identity blocks to a power of two, every level's inverses and couplings kept), then the whole conjugate-gradient loop
//                            preconditioned with T^-1 (depth O(log N) per application), its dot products included: no host read-back inside a solve
//   pgo_retract_cost_kernel  trial poses X Exp(delta) and the trial cost; per-workgroup sums, added in a fixed order by pgo_sum_kernel
//   pgo_factor_error_kernel  one factor per thread: r^2 = |e / sigma|^2 and the loss's weight at the current poses, for rolo_pgo_get_factor_errors
// The Levenberg-Marquardt controller runs on the host in double with one small read-back per trial (cost, PCG iterations, residual) through pinned memory.
// Every loop is bounded: PCG by its cap, the trials by PGO_MAX_TRIALS and the lambda bound. A graph works on a stream of its own; its device store only grows.
#include "ctx_access.hpp"
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

namespace rolo {
namespace {

constexpr int PGO_SLOT = 121;        // gi 6, gj 6, Hii 36, Hjj 36, Hij 36, cost 1
constexpr int PGO_SOLVE_THREADS = 1024;   // the one workgroup of the solve
constexpr int PGO_SUM_THREADS = 1024;
constexpr int PGO_FACTOR_THREADS = 128;  // one factor per thread: the Jacobians fill a thread's registers
constexpr int PGO_MAX_TRIALS = 10000;
constexpr double PGO_SMALL = 1e-2;   // below this angle the coefficient series (their next terms are below 1e-18 there)

struct PgoFactor { int i, j; double Zi[12]; double isig[6]; double k2; };   // j < 0: a prior; Zi = Z^-1 (R row-major, t); isig = 1 / sigma; k2 = k^2 of the Cauchy loss, 0: no loss
struct Pose { double R[9], t[3]; };

#define PGO_DEV __device__ __forceinline__

PGO_DEV void pose_mul(const Pose& a, const Pose& b, Pose& o) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) o.R[3 * r + c] = a.R[3 * r] * b.R[c] + a.R[3 * r + 1] * b.R[3 + c] + a.R[3 * r + 2] * b.R[6 + c];
    o.t[r] = a.R[3 * r] * b.t[0] + a.R[3 * r + 1] * b.t[1] + a.R[3 * r + 2] * b.t[2] + a.t[r];
  }
}
PGO_DEV void pose_inv(const Pose& a, Pose& o) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) o.R[3 * r + c] = a.R[3 * c + r];
    o.t[r] = -(a.R[r] * a.t[0] + a.R[3 + r] * a.t[1] + a.R[6 + r] * a.t[2]);
  }
}
// A = sin th / th, B = (1 - cos th) / th^2, C = (th - sin th) / th^3, D = (1 - (th / 2) cot(th / 2)) / th^2
PGO_DEV void so3_coeffs(double th, double& A, double& B, double& C, double& D) {
  const double t2 = th * th;
  if (th < PGO_SMALL) {
    A = 1.0 - t2 / 6.0 * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0));
    B = 0.5 - t2 / 24.0 * (1.0 - t2 / 30.0 * (1.0 - t2 / 56.0));
    C = 1.0 / 6.0 - t2 / 120.0 * (1.0 - t2 / 42.0 * (1.0 - t2 / 72.0));
    D = 1.0 / 12.0 + t2 / 720.0 * (1.0 + t2 / 42.0 * (1.0 + t2 / 40.0));
    return;
  }
  const double s = sin(th), sh = sin(0.5 * th), ch = cos(0.5 * th);
  A = s / th; B = 2.0 * sh * sh / t2; C = (th - s) / (t2 * th); D = (1.0 - 0.5 * th * ch / sh) / t2;
}
PGO_DEV void hat(const double* w, double* W) { W[0] = 0; W[1] = -w[2]; W[2] = w[1]; W[3] = w[2]; W[4] = 0; W[5] = -w[0]; W[6] = -w[1]; W[7] = w[0]; W[8] = 0; }
PGO_DEV void mul3(const double* a, const double* b, double* o) {
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) o[3 * r + c] = a[3 * r] * b[c] + a[3 * r + 1] * b[3 + c] + a[3 * r + 2] * b[6 + c];
}
PGO_DEV void exp_se3(const double* xi, Pose& o) {
  const double th = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
  double A, B, C, D, W[9], W2[9];
  so3_coeffs(th, A, B, C, D);
  hat(xi, W); mul3(W, W, W2);
  double V[9];
#pragma unroll
  for (int k = 0; k < 9; k++) { const double I = (k % 4 == 0) ? 1.0 : 0.0; o.R[k] = I + A * W[k] + B * W2[k]; V[k] = I + B * W[k] + C * W2[k]; }
#pragma unroll
  for (int r = 0; r < 3; r++) o.t[r] = V[3 * r] * xi[3] + V[3 * r + 1] * xi[4] + V[3 * r + 2] * xi[5];
}
PGO_DEV void log_se3(const Pose& X, double* e) {
  double w[3] = {0.5 * (X.R[7] - X.R[5]), 0.5 * (X.R[2] - X.R[6]), 0.5 * (X.R[3] - X.R[1])};
  const double s = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), c = 0.5 * (X.R[0] + X.R[4] + X.R[8] - 1.0);
  const double f = (s < 1e-6 && c > 0.0) ? 1.0 + s * s / 6.0 : atan2(s, c) / s;   // (an angle within 1e-6 of pi is outside the statement)
#pragma unroll
  for (int k = 0; k < 3; k++) { w[k] *= f; e[k] = w[k]; }
  const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  double A, B, C, D, W[9], W2[9];
  so3_coeffs(th, A, B, C, D);
  hat(w, W); mul3(W, W, W2);
#pragma unroll
  for (int r = 0; r < 3; r++) {
    double v = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) v += (((r == k) ? 1.0 : 0.0) - 0.5 * W[3 * r + k] + D * W2[3 * r + k]) * X.t[k];
    e[3 + r] = v;
  }
}
PGO_DEV void mul6(const double* a, const double* b, double* o) {
  for (int r = 0; r < 6; r++)
    for (int c = 0; c < 6; c++) {
      double s = 0;
#pragma unroll
      for (int k = 0; k < 6; k++) s += a[6 * r + k] * b[6 * k + c];
      o[6 * r + c] = s;
    }
}
// the blocks [[Rw, 0], [Rv, Rw]] of ad(xi) (Rw = hat(omega), Rv = hat(v)) and of Ad(X) (Rw = R, Rv = hat(t) R)
PGO_DEV void blocks6(const double* Rw, const double* Rv, double* M) {
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) { M[6 * r + c] = Rw[3 * r + c]; M[6 * r + 3 + c] = 0.0; M[6 * (r + 3) + c] = Rv[3 * r + c]; M[6 * (r + 3) + 3 + c] = Rw[3 * r + c]; }
}
// Jr^-1 by its series I + ad / 2 + ad^2 / 12 - ad^4 / 720
PGO_DEV void jr_inv(const double* e, double* J) {
  double Ww[9], Wv[9], a[36], a2[36], a4[36];
  hat(e, Ww); hat(e + 3, Wv);
  blocks6(Ww, Wv, a);
  mul6(a, a, a2); mul6(a2, a2, a4);
  for (int k = 0; k < 36; k++) J[k] = ((k % 7 == 0) ? 1.0 : 0.0) + 0.5 * a[k] + a2[k] / 12.0 - a4[k] / 720.0;
}

// whitened error of one factor at the poses Xi, Xj; with J: the whitened Jacobians too
PGO_DEV void factor_error(const PgoFactor& F, const Pose& Xi, const Pose& Xj, double* ew, double* Ji, double* Jj) {
  Pose Z, D, P;
#pragma unroll
  for (int k = 0; k < 9; k++) Z.R[k] = F.Zi[k];
#pragma unroll
  for (int k = 0; k < 3; k++) Z.t[k] = F.Zi[9 + k];
  double e[6];
  if (F.j < 0) {
    pose_mul(Z, Xi, P);
    log_se3(P, e);
    if (Ji) { jr_inv(e, Ji); for (int k = 0; k < 36; k++) Ji[k] *= F.isig[k / 6]; }
  } else {
    Pose Xinv;
    pose_inv(Xi, Xinv);
    pose_mul(Xinv, Xj, D);
    pose_mul(Z, D, P);
    log_se3(P, e);
    if (Ji) {
      double A[36], tR[9], th[9];
      jr_inv(e, Jj);
      pose_inv(D, Xinv);
      hat(Xinv.t, th); mul3(th, Xinv.R, tR);
      blocks6(Xinv.R, tR, A);
      mul6(Jj, A, Ji);
      for (int k = 0; k < 36; k++) { Ji[k] = -Ji[k] * F.isig[k / 6]; Jj[k] *= F.isig[k / 6]; }
    }
  }
#pragma unroll
  for (int k = 0; k < 6; k++) ew[k] = e[k] * F.isig[k];
}

// mEstimator::Cauchy at distance r: weight k^2 / (k^2 + r^2) and loss k^2 / 2 log1p(r^2 / k^2)
PGO_DEV double cauchy_weight(double k2, double r2) { return k2 / (k2 + r2); }
PGO_DEV double cauchy_rho(double k2, double r2) { return 0.5 * k2 * log1p(r2 / k2); }

PGO_DEV void load_pose(const double* p, Pose& X) {
#pragma unroll
  for (int k = 0; k < 9; k++) X.R[k] = p[k];
#pragma unroll
  for (int k = 0; k < 3; k++) X.t[k] = p[9 + k];
}

// o (6 x 6) = a^T b
PGO_DEV void atb6(const double* a, const double* b, double* o) {
  for (int r = 0; r < 6; r++)
    for (int c = 0; c < 6; c++) {
      double s = 0;
#pragma unroll
      for (int k = 0; k < 6; k++) s += a[6 * k + r] * b[6 * k + c];
      o[6 * r + c] = s;
    }
}
PGO_DEV void atv6(const double* a, const double* v, double* o) {
  for (int r = 0; r < 6; r++) {
    double s = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) s += a[6 * k + r] * v[k];
    o[r] = s;
  }
}

// a between factor under a loss, as noiseModel::Robust::WhitenSystem leaves it: error and Jacobians by sqrt(w), so the blocks are w J^T J and the gradient
// w J^T e_w, that of rho. Kept out of line: inlined next to the path of a factor without loss it moved that path's Jacobians out of the registers (its scratch
// accesses tripled and linearise + assemble of a graph without any loss took 1.6 x the time), and as a call that path compiles as it did. It loads the factor
// and the poses itself, so that the caller keeps nothing in memory for it
__device__ __noinline__ void linearize_robust(const PgoFactor* __restrict__ factors, int f, const double* __restrict__ poses, double* __restrict__ s) {
  const PgoFactor Fa = factors[f];
  Pose Xi, Xj;
  load_pose(poses + 12 * (size_t)Fa.i, Xi);
  load_pose(poses + 12 * (size_t)Fa.j, Xj);
  double ew[6], Ji[36], Jj[36], r2 = 0;
  factor_error(Fa, Xi, Xj, ew, Ji, Jj);
#pragma unroll
  for (int k = 0; k < 6; k++) r2 += ew[k] * ew[k];
  const double sw = sqrt(cauchy_weight(Fa.k2, r2));
#pragma unroll
  for (int k = 0; k < 6; k++) ew[k] *= sw;
  for (int k = 0; k < 36; k++) { Ji[k] *= sw; Jj[k] *= sw; }
  atv6(Ji, ew, s); atb6(Ji, Ji, s + 12);
  atv6(Jj, ew, s + 6); atb6(Jj, Jj, s + 48); atb6(Ji, Jj, s + 84);   // (a loss is on a between factor only)
  s[120] = cauchy_rho(Fa.k2, r2);
}

__global__ __launch_bounds__(PGO_FACTOR_THREADS) void pgo_linearize_kernel(const PgoFactor* __restrict__ factors, int F, const double* __restrict__ poses, double* __restrict__ slots) {
  const int f = blockIdx.x * PGO_FACTOR_THREADS + threadIdx.x;
  if (f >= F) return;
  double* s = slots + (size_t)PGO_SLOT * f;
  if (factors[f].k2 > 0.0) { linearize_robust(factors, f, poses, s); return; }
  const PgoFactor Fa = factors[f];
  Pose Xi, Xj;
  load_pose(poses + 12 * (size_t)Fa.i, Xi);
  load_pose(poses + 12 * (size_t)(Fa.j < 0 ? Fa.i : Fa.j), Xj);
  double ew[6], Ji[36], Jj[36];
  factor_error(Fa, Xi, Xj, ew, Ji, Jj);
  atv6(Ji, ew, s);
  atb6(Ji, Ji, s + 12);
  if (Fa.j >= 0) { atv6(Jj, ew, s + 6); atb6(Jj, Jj, s + 48); atb6(Ji, Jj, s + 84); }
  double c = 0;
#pragma unroll
  for (int k = 0; k < 6; k++) c += ew[k] * ew[k];
  s[120] = 0.5 * c;
}

// entries of pose k: factor << 2 | 2 (the factor's other end is pose k + 1) | 1 (pose k is the factor's j)
constexpr int PGO_ASM_POSES = 7;
__global__ __launch_bounds__(256) void pgo_assemble_kernel(const double* __restrict__ slots, const int* __restrict__ rowptr, const int* __restrict__ entries, int N,
                                                           double* __restrict__ diag, double* __restrict__ chain, double* __restrict__ grad) {
  const int k = blockIdx.x * PGO_ASM_POSES + threadIdx.x / 36, e = threadIdx.x % 36;
  if (threadIdx.x >= 36 * PGO_ASM_POSES || k >= N) return;
  const int r = e / 6, c = e % 6;
  double d = 0, ch = 0, g = 0;
  for (int q = rowptr[k]; q < rowptr[k + 1]; q++) {
    const int ent = entries[q];
    const double* s = slots + (size_t)PGO_SLOT * (ent >> 2);
    const bool is_j = ent & 1;
    d += s[(is_j ? 48 : 12) + e];
    if (e < 6) g += s[(is_j ? 6 : 0) + e];
    if (ent & 2) ch += is_j ? s[84 + 6 * c + r] : s[84 + e];
  }
  diag[36 * (size_t)k + e] = d;
  chain[36 * (size_t)k + e] = ch;
  if (e < 6) grad[6 * (size_t)k + e] = g;
}

__global__ __launch_bounds__(256) void pgo_chord_kernel(const double* __restrict__ slots, const int* __restrict__ chord_factor, int n_chords, double* __restrict__ chordH) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= 36 * n_chords) return;
  chordH[q] = slots[(size_t)PGO_SLOT * chord_factor[q / 36] + 84 + q % 36];
}

// out[0] = sum of src[offset + stride i], i < n, in a fixed order: strided sums, then a tree
__global__ __launch_bounds__(PGO_SUM_THREADS) void pgo_sum_kernel(const double* __restrict__ src, int stride, int offset, int n, double* __restrict__ out) {
  __shared__ double red[PGO_SUM_THREADS];
  double s = 0;
  for (int i = threadIdx.x; i < n; i += PGO_SUM_THREADS) s += src[(size_t)stride * i + offset];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = PGO_SUM_THREADS / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}

__global__ __launch_bounds__(PGO_FACTOR_THREADS) void pgo_retract_cost_kernel(const PgoFactor* __restrict__ factors, int F, const double* __restrict__ poses, int N,
                                                               const double* __restrict__ delta, double* __restrict__ trial, double* __restrict__ partials) {
  __shared__ double red[(PGO_FACTOR_THREADS + 63) / 64];
  const int q = blockIdx.x * PGO_FACTOR_THREADS + threadIdx.x;
  if (q < N) {
    Pose X, E, O;
    load_pose(poses + 12 * (size_t)q, X);
    exp_se3(delta + 6 * (size_t)q, E);
    pose_mul(X, E, O);
    double* o = trial + 12 * (size_t)q;
    for (int k = 0; k < 9; k++) o[k] = O.R[k];
    for (int k = 0; k < 3; k++) o[9 + k] = O.t[k];
  }
  double term = 0;
  if (q < F) {   // the factor's own two trial poses, formed again here: no workgroup waits for another
    const PgoFactor Fa = factors[q];
    const int j = Fa.j < 0 ? Fa.i : Fa.j;
    Pose X, E, Xi, Xj;
    load_pose(poses + 12 * (size_t)Fa.i, X); exp_se3(delta + 6 * (size_t)Fa.i, E); pose_mul(X, E, Xi);
    load_pose(poses + 12 * (size_t)j, X); exp_se3(delta + 6 * (size_t)j, E); pose_mul(X, E, Xj);
    double ew[6];
    factor_error(Fa, Xi, Xj, ew, nullptr, nullptr);
    for (int k = 0; k < 6; k++) term += ew[k] * ew[k];
    term = Fa.k2 > 0.0 ? cauchy_rho(Fa.k2, term) : 0.5 * term;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) term += __shfl_xor(term, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = term;
  __syncthreads();
  if (threadIdx.x == 0) { double t = 0; for (int w = 0; w < (PGO_FACTOR_THREADS + 63) / 64; w++) t += red[w]; partials[blockIdx.x] = t; }
}

// r^2 and the weight of every factor at the poses: error only, plain stores
__global__ __launch_bounds__(PGO_FACTOR_THREADS) void pgo_factor_error_kernel(const PgoFactor* __restrict__ factors, int F, const double* __restrict__ poses,
                                                                              double* __restrict__ r2_out, double* __restrict__ w_out) {
  const int f = blockIdx.x * PGO_FACTOR_THREADS + threadIdx.x;
  if (f >= F) return;
  const PgoFactor Fa = factors[f];
  Pose Xi, Xj;
  load_pose(poses + 12 * (size_t)Fa.i, Xi);
  load_pose(poses + 12 * (size_t)(Fa.j < 0 ? Fa.i : Fa.j), Xj);
  double ew[6], r2 = 0;
  factor_error(Fa, Xi, Xj, ew, nullptr, nullptr);
#pragma unroll
  for (int k = 0; k < 6; k++) r2 += ew[k] * ew[k];
  r2_out[f] = r2;
  w_out[f] = Fa.k2 > 0.0 ? cauchy_weight(Fa.k2, r2) : 1.0;
}

// ---- the solve -------------------------------------------------------------------------------------------------------------------------------
struct SolveArgs {
  int N, M, L, n_chords, n_touched, pcg_cap;
  double lambda, tol;
  const double *diag, *chain, *grad, *chordH;
  const int *chord_ij, *touched, *touched_ptr, *touched_ent;   // the poses chords end at, ascending; their (chord << 1 | side) entries in chord order
  double *LD, *LU, *LW;   // the levels' blocks, (2M) x 36: level l starts at block 2M - (2M >> l)
  double *B, *X;          // the levels' right-hand sides and solutions, (2M) x 6
  double *x, *r, *z, *p, *q, *cscr;
  double* delta;
  double* info;           // pinned: PCG iterations, sqrt(r z) / sqrt(r0 z0), 1 = a block was not positive definite, wall-clock ticks of the factorisation and of PCG
  // the grid form only: PCG's scalars (PGO_ST_*) and the lane sums of a dot product in device memory; a pinned word that is 1 once the loop has left
  double *st, *lanes, *done;
};

// W = A^-1 of a symmetric positive definite 6 x 6 block through its Cholesky factor (the lower triangle of A is read); false: a pivot was not positive
PGO_DEV bool inv6(const double* __restrict__ A, double* __restrict__ W) {
  double L[21], Li[21];
#define LT(i, j) ((i) * ((i) + 1) / 2 + (j))
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = 0; j <= i; j++) {
      double s = A[6 * i + j];
#pragma unroll
      for (int k = 0; k < j; k++) s -= L[LT(i, k)] * L[LT(j, k)];
      if (i == j) { if (!(s > 0.0)) { ok = false; s = 1.0; } L[LT(i, i)] = sqrt(s); }
      else L[LT(i, j)] = s / L[LT(j, j)];
    }
#pragma unroll
  for (int j = 0; j < 6; j++) {
    Li[LT(j, j)] = 1.0 / L[LT(j, j)];
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      double s = 0;
#pragma unroll
      for (int k = j; k < i; k++) s += L[LT(i, k)] * Li[LT(k, j)];
      Li[LT(i, j)] = -s / L[LT(i, i)];
    }
  }
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int c = 0; c <= r; c++) {
      double s = 0;
#pragma unroll
      for (int k = r; k < 6; k++) s += Li[LT(k, r)] * Li[LT(k, c)];
      W[6 * r + c] = ok ? s : 0.0; W[6 * c + r] = ok ? s : 0.0;
    }
#undef LT
  return ok;
}

// The solve has two forms that compute the same bits: pgo_solve_kernel, one workgroup that runs everything, and the pgo_grid_* kernels, the same arithmetic cut
// into launches at every seam where one level, sweep or product needs all of the one before. Every element of every level, sweep, matrix-vector row and vector
// update is ONE of the bodies below, evaluated by one thread; both forms call the same text. Only the dot product depends on the thread layout, and both forms
// keep that layout: PGO_SOLVE_THREADS lane sums, lane t adding elements t, t + 1024, ... in order, then one halving tree over the lanes.

// lane `lane` of the PGO_SOLVE_THREADS lane sums of a . b
PGO_DEV double pgo_dot_lane(const double* a, const double* b, int n, int lane) {
  double s = 0;
  for (int i = lane; i < n; i += PGO_SOLVE_THREADS) s += a[i] * b[i];
  return s;
}

// the halving tree over red[0 .. PGO_SOLVE_THREADS), which the caller's PGO_SOLVE_THREADS threads have filled (one lane each, not yet synchronised)
PGO_DEV double pgo_dot_tree(double* red) {
  __syncthreads();
  for (int h = PGO_SOLVE_THREADS / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  const double v = red[0];
  __syncthreads();
  return v;
}

PGO_DEV double pgo_dot(const double* a, const double* b, int n, double* red) {
  red[threadIdx.x] = pgo_dot_lane(a, b, n, threadIdx.x);
  return pgo_dot_tree(red);
}

// level 0, element q of M x 36: the damped diagonal and the chain; identity blocks beyond N
PGO_DEV void pgo_fill_elem(const SolveArgs& S, int q) {
  const int k = q / 36, e = q % 36;
  const double I = (e % 7 == 0) ? 1.0 : 0.0;
  S.LD[q] = k < S.N ? S.diag[q] + S.lambda * I : I;
  S.LU[q] = k + 1 < S.N ? S.chain[q] : 0.0;
}

// the right-hand side of level 0, element q of M x 6: src, zero beyond N
PGO_DEV void pgo_rhs_elem(const SolveArgs& S, const double* src, int q) { S.B[q] = q < 6 * S.N ? src[q] : 0.0; }

// the down sweep, element q of the nn x 6 of the level above `off`: the odd unknowns of this level leave
PGO_DEV void pgo_down_elem(const SolveArgs& S, int off, int noff, int q) {
  const int m = q / 6, r = q % 6;
  double acc = S.B[6 * (size_t)(off + 2 * m) + r];
  {
    const double* U = S.LU + 36 * (size_t)(off + 2 * m);
    const double* W = S.LW + 36 * (size_t)(off + 2 * m + 1);
    const double* b = S.B + 6 * (size_t)(off + 2 * m + 1);
#pragma unroll
    for (int c = 0; c < 6; c++) {
      double y = 0;
#pragma unroll
      for (int d = 0; d < 6; d++) y += W[6 * c + d] * b[d];
      acc -= U[6 * r + c] * y;
    }
  }
  if (m > 0) {
    const double* U = S.LU + 36 * (size_t)(off + 2 * m - 1);
    const double* W = S.LW + 36 * (size_t)(off + 2 * m - 1);
    const double* b = S.B + 6 * (size_t)(off + 2 * m - 1);
#pragma unroll
    for (int c = 0; c < 6; c++) {
      double y = 0;
#pragma unroll
      for (int d = 0; d < 6; d++) y += W[6 * c + d] * b[d];
      acc -= U[6 * c + r] * y;
    }
  }
  S.B[6 * (size_t)(noff + m) + r] = acc;
}

// the top level's one block at `off`, row r
PGO_DEV void pgo_top_elem(const SolveArgs& S, int off, int r) {
  const double* W = S.LW + 36 * (size_t)off;
  double s = 0;
#pragma unroll
  for (int c = 0; c < 6; c++) s += W[6 * r + c] * S.B[6 * (size_t)off + c];
  S.X[6 * (size_t)off + r] = s;
}

// the up sweep, element q of the level's n x 6: the even unknowns come from the level above, the odd ones from their two neighbours
PGO_DEV void pgo_up_elem(const SolveArgs& S, int off, int noff, int nn, int q) {
  const int k = q / 6, r = q % 6;
  double out;
  if ((k & 1) == 0) out = S.X[6 * (size_t)(noff + (k >> 1)) + r];
  else {
    const int m = k >> 1;
    const double* Um = S.LU + 36 * (size_t)(off + k - 1);
    const double* Uk = S.LU + 36 * (size_t)(off + k);
    const double* W = S.LW + 36 * (size_t)(off + k);
    const double* xl = S.X + 6 * (size_t)(noff + m);
    const double* xr = S.X + 6 * (size_t)(noff + m + 1);
    const bool have_r = m + 1 < nn;
    out = 0;
#pragma unroll
    for (int c = 0; c < 6; c++) {
      double t = S.B[6 * (size_t)(off + k) + c];
#pragma unroll
      for (int a = 0; a < 6; a++) t -= Um[6 * a + c] * xl[a];
      if (have_r) {
#pragma unroll
        for (int a = 0; a < 6; a++) t -= Uk[6 * c + a] * xr[a];
      }
      out += W[6 * r + c] * t;
    }
  }
  S.X[6 * (size_t)(off + k) + r] = out;
}

// where level l starts among the (2M) stored blocks; it has M >> l blocks, and level l + 1 starts right behind it
PGO_DEV int pgo_level_off(const SolveArgs& S, int l) { return 2 * S.M - ((2 * S.M) >> l); }

// dst = T^-1 src through the stored levels; every thread of the workgroup calls it
PGO_DEV void pgo_apply(const SolveArgs& S, const double* src, double* dst) {
  const int tid = threadIdx.x, n6 = 6 * S.N;
  for (int q = tid; q < 6 * S.M; q += PGO_SOLVE_THREADS) pgo_rhs_elem(S, src, q);
  __syncthreads();
  for (int l = 0; l < S.L; l++) {
    const int off = pgo_level_off(S, l), n = S.M >> l, noff = off + n, nn = n >> 1;
    for (int q = tid; q < 6 * nn; q += PGO_SOLVE_THREADS) pgo_down_elem(S, off, noff, q);
    __syncthreads();
  }
  for (int r = tid; r < 6; r += PGO_SOLVE_THREADS) pgo_top_elem(S, pgo_level_off(S, S.L), r);
  __syncthreads();
  for (int l = S.L - 1; l >= 0; l--) {
    const int off = pgo_level_off(S, l), n = S.M >> l, noff = off + n, nn = n >> 1;
    for (int q = tid; q < 6 * n; q += PGO_SOLVE_THREADS) pgo_up_elem(S, off, noff, nn, q);
    __syncthreads();
  }
  for (int q = tid; q < n6; q += PGO_SOLVE_THREADS) dst[q] = S.X[q];
  __syncthreads();
}

// q = (H + lambda I) p in three bodies: a row of the block-tridiagonal part from level 0, a chord's row into its scratch, the gather per pose in chord order
PGO_DEV void pgo_mv_tri_elem(const SolveArgs& S, const double* p, double* q, int u) {
  const int k = u / 6, r = u % 6;
  const double* D = S.LD + 36 * (size_t)k;
  double s = 0;
#pragma unroll
  for (int c = 0; c < 6; c++) s += D[6 * r + c] * p[6 * (size_t)k + c];
  if (k + 1 < S.N) {
    const double* U = S.LU + 36 * (size_t)k;
#pragma unroll
    for (int c = 0; c < 6; c++) s += U[6 * r + c] * p[6 * (size_t)(k + 1) + c];
  }
  if (k > 0) {
    const double* U = S.LU + 36 * (size_t)(k - 1);
#pragma unroll
    for (int c = 0; c < 6; c++) s += U[6 * c + r] * p[6 * (size_t)(k - 1) + c];
  }
  q[u] = s;
}

PGO_DEV void pgo_mv_chord_elem(const SolveArgs& S, const double* p, int u) {
  const int ch = u / 12, side = (u % 12) / 6, r = u % 6;
  const double* H = S.chordH + 36 * (size_t)ch;
  const int i = S.chord_ij[2 * ch], j = S.chord_ij[2 * ch + 1];
  double s = 0;
  if (side == 0) {   // row i: H p_j
#pragma unroll
    for (int a = 0; a < 6; a++) s += H[6 * r + a] * p[6 * (size_t)j + a];
  } else {           // row j: H^T p_i
#pragma unroll
    for (int a = 0; a < 6; a++) s += H[6 * a + r] * p[6 * (size_t)i + a];
  }
  S.cscr[u] = s;
}

PGO_DEV void pgo_mv_gather_elem(const SolveArgs& S, double* q, int u) {
  const int t = u / 6, r = u % 6;
  double s = q[6 * (size_t)S.touched[t] + r];
  for (int e = S.touched_ptr[t]; e < S.touched_ptr[t + 1]; e++) { const int ent = S.touched_ent[e]; s += S.cscr[12 * (size_t)(ent >> 1) + 6 * (ent & 1) + r]; }
  q[6 * (size_t)S.touched[t] + r] = s;
}

PGO_DEV void pgo_matvec(const SolveArgs& S, const double* p, double* q) {
  const int tid = threadIdx.x;
  for (int u = tid; u < 6 * S.N; u += PGO_SOLVE_THREADS) pgo_mv_tri_elem(S, p, q, u);
  for (int u = tid; u < 12 * S.n_chords; u += PGO_SOLVE_THREADS) pgo_mv_chord_elem(S, p, u);
  __syncthreads();
  for (int u = tid; u < 6 * S.n_touched; u += PGO_SOLVE_THREADS) pgo_mv_gather_elem(S, q, u);
  __syncthreads();
}

// the factorisation's step from level `off` to the next, element q of nn x 36: LD and LU of the level above through W = inv6 of this level's odd blocks
PGO_DEV void pgo_reduce_elem(const SolveArgs& S, int off, int noff, int q) {
  const int m = q / 36, e = q % 36, r = e / 6, c = e % 6;
  const double* U = S.LU + 36 * (size_t)(off + 2 * m);
  const double* W = S.LW + 36 * (size_t)(off + 2 * m + 1);
  const double* U2 = S.LU + 36 * (size_t)(off + 2 * m + 1);
  double d = S.LD[36 * (size_t)(off + 2 * m) + e], u = 0;
#pragma unroll
  for (int a = 0; a < 6; a++) {
    double wd = 0, wu = 0;
#pragma unroll
    for (int b = 0; b < 6; b++) { wd += W[6 * a + b] * U[6 * c + b]; wu += W[6 * a + b] * U2[6 * b + c]; }
    d -= U[6 * r + a] * wd;   // - U W U^T
    u -= U[6 * r + a] * wu;   // - U W U'
  }
  if (m > 0) {
    const double* Um = S.LU + 36 * (size_t)(off + 2 * m - 1);
    const double* Wm = S.LW + 36 * (size_t)(off + 2 * m - 1);
#pragma unroll
    for (int a = 0; a < 6; a++) {
      double wd = 0;
#pragma unroll
      for (int b = 0; b < 6; b++) wd += Wm[6 * a + b] * Um[6 * b + c];
      d -= Um[6 * a + r] * wd;   // - U^T W U of the block before
    }
  }
  S.LD[36 * (size_t)(noff + m) + e] = d;
  S.LU[36 * (size_t)(noff + m) + e] = u;
}

// W of odd block m of the level at `off`; false: not positive definite
PGO_DEV bool pgo_inv_elem(const SolveArgs& S, int off, int m) { return inv6(S.LD + 36 * (size_t)(off + 2 * m + 1), S.LW + 36 * (size_t)(off + 2 * m + 1)); }

// the vector updates of PCG, element q of 6N
PGO_DEV void pgo_start_elem(const SolveArgs& S, int q) { S.x[q] = 0.0; S.r[q] = -S.grad[q]; }
PGO_DEV void pgo_step_elem(const SolveArgs& S, double a, int q) { S.x[q] += a * S.p[q]; S.r[q] -= a * S.q[q]; }
PGO_DEV void pgo_dir_elem(const SolveArgs& S, double beta, int q) { S.p[q] = S.z[q] + beta * S.p[q]; }

__global__ __launch_bounds__(PGO_SOLVE_THREADS) void pgo_solve_kernel(SolveArgs S) {
  __shared__ double red[PGO_SOLVE_THREADS];
  __shared__ int bad;
  const int tid = threadIdx.x, n6 = 6 * S.N;
  const long long t0 = wall_clock64();
  if (tid == 0) bad = 0;
  for (int q = tid; q < 36 * S.M; q += PGO_SOLVE_THREADS) pgo_fill_elem(S, q);
  __syncthreads();
  for (int l = 0; l < S.L; l++) {
    const int off = pgo_level_off(S, l), n = S.M >> l, noff = off + n, nn = n >> 1;
    for (int m = tid; m < nn; m += PGO_SOLVE_THREADS)
      if (!pgo_inv_elem(S, off, m)) bad = 1;
    __syncthreads();
    for (int q = tid; q < 36 * nn; q += PGO_SOLVE_THREADS) pgo_reduce_elem(S, off, noff, q);
    __syncthreads();
  }
  if (tid == 0) { const int off = pgo_level_off(S, S.L); if (!inv6(S.LD + 36 * (size_t)off, S.LW + 36 * (size_t)off)) bad = 1; }
  __syncthreads();
  const long long t1 = wall_clock64();
  int iters = 0;
  double residual = 0.0;
  for (int q = tid; q < n6; q += PGO_SOLVE_THREADS) pgo_start_elem(S, q);
  __syncthreads();
  if (!bad) {
    pgo_apply(S, S.r, S.z);
    double rz = pgo_dot(S.r, S.z, n6, red);
    const double rz0 = rz;
    if (rz0 > 0.0) {   // (a zero gradient: delta = 0 at once, nothing divided)
      for (int q = tid; q < n6; q += PGO_SOLVE_THREADS) S.p[q] = S.z[q];
      __syncthreads();
      for (int it = 1; it <= S.pcg_cap; it++) {
        pgo_matvec(S, S.p, S.q);
        const double pq = pgo_dot(S.p, S.q, n6, red);
        if (!(pq > 0.0)) break;
        iters = it;
        const double a = rz / pq;
        for (int q = tid; q < n6; q += PGO_SOLVE_THREADS) pgo_step_elem(S, a, q);
        __syncthreads();
        pgo_apply(S, S.r, S.z);
        const double rzn = pgo_dot(S.r, S.z, n6, red);
        if (!(rzn > 0.0)) { rz = 0.0; break; }
        const bool done = sqrt(rzn) <= S.tol * sqrt(rz0);
        const double beta = rzn / rz;
        for (int q = tid; q < n6; q += PGO_SOLVE_THREADS) pgo_dir_elem(S, beta, q);
        __syncthreads();
        rz = rzn;
        if (done) break;
      }
      residual = sqrt(rz) / sqrt(rz0);
    }
  }
  for (int q = tid; q < n6; q += PGO_SOLVE_THREADS) S.delta[q] = S.x[q];
  if (tid == 0) {
    S.info[0] = (double)iters; S.info[1] = residual; S.info[2] = bad ? 1.0 : 0.0;
    S.info[3] = (double)(t1 - t0); S.info[4] = (double)(wall_clock64() - t1);
  }
}

// ---- the grid form: the same bodies, one launch per seam ---------------------------------------------------------------------------------------
// A seam is where every element of a stage may read what any thread of the stage before wrote: between two levels of the reduction, between a sweep and a dot
// product, between a dot product and the update that uses it. Each seam is the end of a launch: no workgroup ever waits for another, so nothing here can hang.
// A level of at most PGO_GRID_TOP blocks is finished, together with every level above it, by ONE workgroup (the loop of pgo_solve_kernel on the top of the
// tree). PCG's scalars live in S.st; every launch of the loop returns at once when PGO_ST_DONE is set, so iterations enqueued past the exit change nothing.
constexpr int PGO_GRID_THREADS = 256;
constexpr int PGO_GRID_TOP = 256;      // blocks: at 1 024 threads the fused top has at most one element of the down sweep and two of the up sweep per thread and level
constexpr int PGO_GRID_TILE = 32;      // blocks of the NEXT level that one workgroup of a level's launch makes, from 64 blocks of its own
constexpr int PGO_GRID_LANE_WG = 64;   // the 1 024 lane sums of a dot product go over 16 workgroups
constexpr int PGO_GRID_BATCH = 4;      // PCG iterations enqueued between two looks at the pinned done word
// rolo_pgo's AUTO: the grid form from this many poses on. The smallest size of profiles/r14/posegraph_grid.json from which the grid form beat the one-workgroup
// form at 1, 10 and 100 loops and in the per-key-frame call by more than the spread of the repeats (slower up to 256 poses, faster from 512 on)
constexpr int PGO_GRID_FROM = 512;
enum { PGO_ST_RZ, PGO_ST_RZ0, PGO_ST_PQ, PGO_ST_ALPHA, PGO_ST_BETA, PGO_ST_ITERS, PGO_ST_BAD, PGO_ST_DONE, PGO_ST_WORDS };
enum { PGO_DOT_RZ0, PGO_DOT_PQ, PGO_DOT_RZ };

PGO_DEV bool pgo_grid_stop(const SolveArgs& S) { return S.st[PGO_ST_DONE] != 0.0; }

__global__ __launch_bounds__(PGO_GRID_THREADS) void pgo_grid_fill_kernel(SolveArgs S) {
  const int q = blockIdx.x * PGO_GRID_THREADS + threadIdx.x;
  if (q < PGO_ST_WORDS) S.st[q] = 0.0;
  if (q == 0) S.done[0] = 0.0;
  if (q < 36 * S.M) pgo_fill_elem(S, q);
}

__global__ __launch_bounds__(64) void pgo_grid_inv_kernel(SolveArgs S, int l) {
  const int off = pgo_level_off(S, l), nn = S.M >> (l + 1), m = blockIdx.x * 64 + threadIdx.x;
  if (m < nn && !pgo_inv_elem(S, off, m)) S.st[PGO_ST_BAD] = 1.0;
}

__global__ __launch_bounds__(PGO_GRID_THREADS) void pgo_grid_reduce_kernel(SolveArgs S, int l) {
  const int off = pgo_level_off(S, l), n = S.M >> l, noff = off + n, nn = n >> 1;
  for (int e = threadIdx.x; e < 36 * PGO_GRID_TILE; e += PGO_GRID_THREADS) {
    const int q = blockIdx.x * 36 * PGO_GRID_TILE + e;
    if (q < 36 * nn) pgo_reduce_elem(S, off, noff, q);
  }
}

// levels l0 .. L of the factorisation: pgo_solve_kernel's loop from l0 on
__global__ __launch_bounds__(PGO_SOLVE_THREADS) void pgo_grid_top_factor_kernel(SolveArgs S, int l0) {
  const int tid = threadIdx.x;
  for (int l = l0; l < S.L; l++) {
    const int off = pgo_level_off(S, l), n = S.M >> l, noff = off + n, nn = n >> 1;
    for (int m = tid; m < nn; m += PGO_SOLVE_THREADS)
      if (!pgo_inv_elem(S, off, m)) S.st[PGO_ST_BAD] = 1.0;
    __syncthreads();
    for (int q = tid; q < 36 * nn; q += PGO_SOLVE_THREADS) pgo_reduce_elem(S, off, noff, q);
    __syncthreads();
  }
  if (tid == 0) { const int off = pgo_level_off(S, S.L); if (!inv6(S.LD + 36 * (size_t)off, S.LW + 36 * (size_t)off)) S.st[PGO_ST_BAD] = 1.0; }
}

// x = 0, r = -g and the first right-hand side; a factorisation that was not positive definite ends the loop before it starts
__global__ __launch_bounds__(PGO_GRID_THREADS) void pgo_grid_start_kernel(SolveArgs S) {
  const int q = blockIdx.x * PGO_GRID_THREADS + threadIdx.x;
  if (q == 0 && S.st[PGO_ST_BAD] != 0.0) { S.st[PGO_ST_DONE] = 1.0; S.done[0] = 1.0; }
  if (q < 6 * S.N) pgo_start_elem(S, q);
  if (q < 6 * S.M) pgo_rhs_elem(S, S.r, q);
}

__global__ __launch_bounds__(PGO_GRID_THREADS) void pgo_grid_down_kernel(SolveArgs S, int l) {
  if (pgo_grid_stop(S)) return;
  const int off = pgo_level_off(S, l), n = S.M >> l, noff = off + n, nn = n >> 1;
  for (int e = threadIdx.x; e < 6 * PGO_GRID_TILE; e += PGO_GRID_THREADS) {
    const int q = blockIdx.x * 6 * PGO_GRID_TILE + e;
    if (q < 6 * nn) pgo_down_elem(S, off, noff, q);
  }
}

// levels l0 .. L down, the top block, levels L - 1 .. l0 up: pgo_apply's loops from l0 on. dst is written where level 0 is among them
__global__ __launch_bounds__(PGO_SOLVE_THREADS) void pgo_grid_top_apply_kernel(SolveArgs S, int l0, double* dst) {
  if (pgo_grid_stop(S)) return;
  const int tid = threadIdx.x;
  for (int l = l0; l < S.L; l++) {
    const int off = pgo_level_off(S, l), n = S.M >> l, noff = off + n, nn = n >> 1;
    for (int q = tid; q < 6 * nn; q += PGO_SOLVE_THREADS) pgo_down_elem(S, off, noff, q);
    __syncthreads();
  }
  for (int r = tid; r < 6; r += PGO_SOLVE_THREADS) pgo_top_elem(S, pgo_level_off(S, S.L), r);
  __syncthreads();
  for (int l = S.L - 1; l >= l0; l--) {
    const int off = pgo_level_off(S, l), n = S.M >> l, noff = off + n, nn = n >> 1;
    for (int q = tid; q < 6 * n; q += PGO_SOLVE_THREADS) pgo_up_elem(S, off, noff, nn, q);
    __syncthreads();
  }
  if (l0 == 0)
    for (int q = tid; q < 6 * S.N; q += PGO_SOLVE_THREADS) dst[q] = S.X[q];
}

// one level of the up sweep; level 0 also hands the solution to dst (level 0 starts at block 0: X's index there is q)
__global__ __launch_bounds__(PGO_GRID_THREADS) void pgo_grid_up_kernel(SolveArgs S, int l, double* dst) {
  if (pgo_grid_stop(S)) return;
  const int off = pgo_level_off(S, l), n = S.M >> l, noff = off + n, nn = n >> 1;
  for (int e = threadIdx.x; e < 12 * PGO_GRID_TILE; e += PGO_GRID_THREADS) {
    const int q = blockIdx.x * 12 * PGO_GRID_TILE + e;
    if (q < 6 * n) {
      pgo_up_elem(S, off, noff, nn, q);
      if (l == 0 && q < 6 * S.N) dst[q] = S.X[q];
    }
  }
}

__global__ __launch_bounds__(PGO_GRID_THREADS) void pgo_grid_mv_kernel(SolveArgs S) {
  if (pgo_grid_stop(S)) return;
  const int u = blockIdx.x * PGO_GRID_THREADS + threadIdx.x;
  if (u < 6 * S.N) pgo_mv_tri_elem(S, S.p, S.q, u);
  if (u < 12 * S.n_chords) pgo_mv_chord_elem(S, S.p, u);
}

__global__ __launch_bounds__(PGO_GRID_THREADS) void pgo_grid_gather_kernel(SolveArgs S) {
  if (pgo_grid_stop(S)) return;
  const int u = blockIdx.x * PGO_GRID_THREADS + threadIdx.x;
  if (u < 6 * S.n_touched) pgo_mv_gather_elem(S, S.q, u);
}

// the PGO_SOLVE_THREADS lane sums of a . b, PGO_GRID_LANE_WG lanes per workgroup: each lane adds what its thread of pgo_solve_kernel adds, in that order
__global__ __launch_bounds__(PGO_GRID_LANE_WG) void pgo_grid_lanes_kernel(SolveArgs S, const double* a, const double* b) {
  if (pgo_grid_stop(S)) return;
  const int lane = blockIdx.x * PGO_GRID_LANE_WG + threadIdx.x;
  S.lanes[lane] = pgo_dot_lane(a, b, 6 * S.N, lane);
}

// the tree over the lane sums, and what pgo_solve_kernel does with the value: which = PGO_DOT_RZ0 (r0 z0), PGO_DOT_PQ (p q), PGO_DOT_RZ (r z of an iteration)
__global__ __launch_bounds__(PGO_SOLVE_THREADS) void pgo_grid_scalar_kernel(SolveArgs S, int which) {
  __shared__ double red[PGO_SOLVE_THREADS];
  if (pgo_grid_stop(S)) return;
  red[threadIdx.x] = S.lanes[threadIdx.x];
  const double v = pgo_dot_tree(red);
  if (threadIdx.x != 0) return;
  bool done = false;
  if (which == PGO_DOT_RZ0) {
    S.st[PGO_ST_RZ] = v; S.st[PGO_ST_RZ0] = v;
    done = !(v > 0.0);
  } else if (which == PGO_DOT_PQ) {
    S.st[PGO_ST_PQ] = v;
    if (!(v > 0.0)) done = true;
    else { S.st[PGO_ST_ITERS] += 1.0; S.st[PGO_ST_ALPHA] = S.st[PGO_ST_RZ] / v; }
  } else {
    if (!(v > 0.0)) { S.st[PGO_ST_RZ] = 0.0; done = true; }
    else {
      done = sqrt(v) <= S.tol * sqrt(S.st[PGO_ST_RZ0]);
      S.st[PGO_ST_BETA] = v / S.st[PGO_ST_RZ];
      S.st[PGO_ST_RZ] = v;
    }
  }
  if (done) { S.st[PGO_ST_DONE] = 1.0; S.done[0] = 1.0; }
}

__global__ __launch_bounds__(PGO_GRID_THREADS) void pgo_grid_step_kernel(SolveArgs S) {
  if (pgo_grid_stop(S)) return;
  const int q = blockIdx.x * PGO_GRID_THREADS + threadIdx.x;
  if (q < 6 * S.N) { pgo_step_elem(S, S.st[PGO_ST_ALPHA], q); pgo_rhs_elem(S, S.r, q); }
}

// first: p = z; later: p = z + beta p (after the exit of the loop p is read by nobody, so the launch may return with the others)
__global__ __launch_bounds__(PGO_GRID_THREADS) void pgo_grid_dir_kernel(SolveArgs S, int first) {
  if (pgo_grid_stop(S)) return;
  const int q = blockIdx.x * PGO_GRID_THREADS + threadIdx.x;
  if (q >= 6 * S.N) return;
  if (first) S.p[q] = S.z[q];
  else pgo_dir_elem(S, S.st[PGO_ST_BETA], q);
}

__global__ __launch_bounds__(PGO_GRID_THREADS) void pgo_grid_finish_kernel(SolveArgs S) {
  const int q = blockIdx.x * PGO_GRID_THREADS + threadIdx.x;
  if (q < 6 * S.N) S.delta[q] = S.x[q];
  if (q == 0) {
    const double rz0 = S.st[PGO_ST_RZ0];
    S.info[0] = S.st[PGO_ST_ITERS]; S.info[1] = rz0 > 0.0 ? sqrt(S.st[PGO_ST_RZ]) / sqrt(rz0) : 0.0; S.info[2] = S.st[PGO_ST_BAD] != 0.0 ? 1.0 : 0.0;
  }
}

}  // namespace
}  // namespace rolo

using namespace rolo;

struct rolo_pgo {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  double wall_khz = 100000.0;
  // the graph on the host: factors, the incidence lists, the chords; poses added since the last upload
  int N = 0;
  std::vector<PgoFactor> factors;
  std::vector<std::vector<int>> inc;
  std::vector<int> chord_factor, chord_ij;
  std::vector<double> pending;             // 12 doubles per pose not yet on the device
  std::vector<int> h_rowptr, h_entries;
  int up_poses = 0, up_factors = 0, dirty_from = 0;
  bool chords_dirty = false, linearized = false;
  int n_touched = 0;
  // device store: only grows; outgrown buffers are kept until rolo_pgo_destroy
  double *poses = nullptr, *trial = nullptr; size_t poses_cap = 0, trial_cap = 0;
  PgoFactor* d_factors = nullptr; size_t factors_cap = 0;
  double* slots = nullptr; size_t slots_cap = 0;
  int *rowptr = nullptr, *entries = nullptr; size_t rowptr_cap = 0, entries_cap = 0;
  double *diag = nullptr, *chain = nullptr, *grad = nullptr; size_t diag_cap = 0, chain_cap = 0, grad_cap = 0;
  double* chordH = nullptr; size_t chordH_cap = 0;
  int *d_chord_factor = nullptr, *d_chord_ij = nullptr, *touched = nullptr, *touched_ptr = nullptr, *touched_ent = nullptr;
  size_t d_chord_factor_cap = 0, d_chord_ij_cap = 0, touched_cap = 0, touched_ptr_cap = 0, touched_ent_cap = 0;
  double *LD = nullptr, *LU = nullptr, *LW = nullptr, *B = nullptr, *X = nullptr; size_t LD_cap = 0, LU_cap = 0, LW_cap = 0, B_cap = 0, X_cap = 0;
  double* vec[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; size_t vec_cap[5] = {0, 0, 0, 0, 0};
  double *cscr = nullptr, *delta = nullptr, *partials = nullptr; size_t cscr_cap = 0, delta_cap = 0, partials_cap = 0;
  double* ferr = nullptr; size_t ferr_cap = 0;   // rolo_pgo_get_factor_errors: F x r^2, then F x w
  double* gst = nullptr; size_t gst_cap = 0;   // the grid form's PGO_ST_WORDS scalars, then its PGO_SOLVE_THREADS lane sums
  int solve_form = ROLO_PGO_SOLVE_AUTO, last_form = 0;
  hipEvent_t gev[3] = {nullptr, nullptr, nullptr};   // the grid form: before the factorisation, between it and PCG, after PCG
  double* h_info = nullptr;                // pinned: [0] cost, [1..5] the solve's info, [6] the grid form's done word
  DevStore store;                          // grows the device store on the graph's stream
  float ms[4] = {0.f, 0.f, 0.f, 0.f};
  std::vector<rolo_pgo_trace_rec> trace;
};

namespace {

bool finite_n(const double* v, int n) { for (int i = 0; i < n; i++) if (!std::isfinite(v[i])) return false; return true; }

// what the host has added since the last call goes to the device: new poses, new factors, the changed tail of the incidence list, the chord tables
int pgo_sync_graph(rolo_pgo* g) {
  HIPCHK(hipSetDevice(g->device));
  hipStream_t s = g->stream;
  int rc;
  const int N = g->N, F = (int)g->factors.size();
  if (g->up_poses < N) {
    if ((rc = g->store.grow(g->poses, g->poses_cap, 12 * (size_t)N, 12 * (size_t)g->up_poses))) return rc;
    HIPCHK(hipMemcpyAsync(g->poses + 12 * (size_t)g->up_poses, g->pending.data(), sizeof(double) * g->pending.size(), hipMemcpyHostToDevice, s));
  }
  if ((rc = g->store.grow(g->trial, g->trial_cap, 12 * (size_t)N))) return rc;
  if (g->up_factors < F) {
    const size_t cap0 = g->factors_cap;
    if ((rc = g->store.grow(g->d_factors, g->factors_cap, (size_t)F))) return rc;
    const int from = g->factors_cap != cap0 ? 0 : g->up_factors;
    HIPCHK(hipMemcpyAsync(g->d_factors + from, g->factors.data() + from, sizeof(PgoFactor) * (size_t)(F - from), hipMemcpyHostToDevice, s));
  }
  if ((rc = g->store.grow(g->slots, g->slots_cap, (size_t)PGO_SLOT * std::max(F, 1)))) return rc;
  if (g->dirty_from < N || (int)g->h_rowptr.size() != N + 1) {
    const size_t c0 = g->rowptr_cap, c1 = g->entries_cap;
    if ((rc = g->store.grow(g->rowptr, g->rowptr_cap, (size_t)N + 1))) return rc;
    if ((rc = g->store.grow(g->entries, g->entries_cap, 2 * (size_t)std::max(F, 1)))) return rc;
    int from = std::min(g->dirty_from, std::max((int)g->h_rowptr.size() - 1, 0));
    if (g->rowptr_cap != c0 || g->entries_cap != c1) from = 0;
    g->h_rowptr.resize((size_t)N + 1);
    const int e0 = from > 0 ? g->h_rowptr[from] : 0;
    g->h_entries.resize((size_t)e0);
    for (int k = from; k < N; k++) { g->h_rowptr[k] = (int)g->h_entries.size(); g->h_entries.insert(g->h_entries.end(), g->inc[k].begin(), g->inc[k].end()); }
    g->h_rowptr[N] = (int)g->h_entries.size();
    HIPCHK(hipMemcpyAsync(g->rowptr + from, g->h_rowptr.data() + from, sizeof(int) * (size_t)(N + 1 - from), hipMemcpyHostToDevice, s));
    if ((int)g->h_entries.size() > e0)
      HIPCHK(hipMemcpyAsync(g->entries + e0, g->h_entries.data() + e0, sizeof(int) * (g->h_entries.size() - (size_t)e0), hipMemcpyHostToDevice, s));
  }
  const int nc = (int)g->chord_factor.size();
  std::vector<int> touched, tptr, tent;
  if (g->chords_dirty && nc) {
    std::vector<std::pair<int, int>> ends;   // (pose, chord << 1 | side), sorted: per pose in chord order
    for (int c = 0; c < nc; c++) { ends.push_back({g->chord_ij[2 * c], 2 * c}); ends.push_back({g->chord_ij[2 * c + 1], 2 * c + 1}); }
    std::sort(ends.begin(), ends.end());
    for (size_t e = 0; e < ends.size(); e++) {
      if (e == 0 || ends[e].first != ends[e - 1].first) { touched.push_back(ends[e].first); tptr.push_back((int)e); }
      tent.push_back(ends[e].second);
    }
    tptr.push_back((int)ends.size());
    g->n_touched = (int)touched.size();
    if ((rc = g->store.grow(g->d_chord_factor, g->d_chord_factor_cap, (size_t)nc))) return rc;
    if ((rc = g->store.grow(g->d_chord_ij, g->d_chord_ij_cap, 2 * (size_t)nc))) return rc;
    if ((rc = g->store.grow(g->touched, g->touched_cap, touched.size()))) return rc;
    if ((rc = g->store.grow(g->touched_ptr, g->touched_ptr_cap, tptr.size()))) return rc;
    if ((rc = g->store.grow(g->touched_ent, g->touched_ent_cap, tent.size()))) return rc;
    HIPCHK(hipMemcpyAsync(g->d_chord_factor, g->chord_factor.data(), sizeof(int) * (size_t)nc, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(g->d_chord_ij, g->chord_ij.data(), sizeof(int) * 2 * (size_t)nc, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(g->touched, touched.data(), sizeof(int) * touched.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(g->touched_ptr, tptr.data(), sizeof(int) * tptr.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(g->touched_ent, tent.data(), sizeof(int) * tent.size(), hipMemcpyHostToDevice, s));
  }
  if ((rc = g->store.grow(g->chordH, g->chordH_cap, 36 * (size_t)std::max(nc, 1)))) return rc;
  if ((rc = g->store.grow(g->cscr, g->cscr_cap, 12 * (size_t)std::max(nc, 1)))) return rc;
  if ((rc = g->store.grow(g->diag, g->diag_cap, 36 * (size_t)N))) return rc;
  if ((rc = g->store.grow(g->chain, g->chain_cap, 36 * (size_t)N))) return rc;
  if ((rc = g->store.grow(g->grad, g->grad_cap, 6 * (size_t)N))) return rc;
  if ((rc = g->store.grow(g->delta, g->delta_cap, 6 * (size_t)N))) return rc;
  for (int v = 0; v < 5; v++) if ((rc = g->store.grow(g->vec[v], g->vec_cap[v], 6 * (size_t)N))) return rc;
  int M = 1;
  while (M < N) M <<= 1;
  if ((rc = g->store.grow(g->LD, g->LD_cap, 72 * (size_t)M))) return rc;
  if ((rc = g->store.grow(g->LU, g->LU_cap, 72 * (size_t)M))) return rc;
  if ((rc = g->store.grow(g->LW, g->LW_cap, 72 * (size_t)M))) return rc;
  if ((rc = g->store.grow(g->B, g->B_cap, 12 * (size_t)M))) return rc;
  if ((rc = g->store.grow(g->X, g->X_cap, 12 * (size_t)M))) return rc;
  if ((rc = g->store.grow(g->gst, g->gst_cap, (size_t)PGO_ST_WORDS + PGO_SOLVE_THREADS))) return rc;
  if ((rc = g->store.grow(g->partials, g->partials_cap, (size_t)(std::max(N, F) + PGO_FACTOR_THREADS - 1) / PGO_FACTOR_THREADS + 1))) return rc;
  HIPCHK(hipStreamSynchronize(s));   // the host vectors are free again
  g->pending.clear();
  g->up_poses = N; g->up_factors = F; g->dirty_from = N; g->chords_dirty = false;
  return ROLO_OK;
}

// every buffer pgo_sync_graph would grow for a graph larger by these counts, grown now: what the device holds is carried over (poses, factors, the incidence list,
// the chord tables), the rest is scratch of one linearisation or one solve
int pgo_reserve_impl(rolo_pgo* g, int more_poses, int more_factors, int more_chords) {
  HIPCHK(hipSetDevice(g->device));
  const size_t N = (size_t)g->N + (size_t)more_poses, F = g->factors.size() + (size_t)more_factors, nc0 = g->chord_factor.size(), nc = nc0 + (size_t)more_chords;
  const size_t F1 = std::max<size_t>(F, 1), nc1 = std::max<size_t>(nc, 1), have_chords = g->d_chord_factor ? nc0 : 0, have_touched = g->touched ? (size_t)g->n_touched : 0;
  int rc;
  g->linearized = false;
  if ((rc = g->store.grow(g->poses, g->poses_cap, 12 * N, 12 * (size_t)g->up_poses))) return rc;
  if ((rc = g->store.grow(g->trial, g->trial_cap, 12 * N))) return rc;
  if ((rc = g->store.grow(g->d_factors, g->factors_cap, F1, (size_t)g->up_factors))) return rc;
  if ((rc = g->store.grow(g->slots, g->slots_cap, (size_t)PGO_SLOT * F1))) return rc;
  if ((rc = g->store.grow(g->rowptr, g->rowptr_cap, N + 1, g->rowptr ? g->h_rowptr.size() : 0))) return rc;
  if ((rc = g->store.grow(g->entries, g->entries_cap, 2 * F1, g->entries ? g->h_entries.size() : 0))) return rc;
  if (nc) {
    if ((rc = g->store.grow(g->d_chord_factor, g->d_chord_factor_cap, nc, have_chords))) return rc;
    if ((rc = g->store.grow(g->d_chord_ij, g->d_chord_ij_cap, 2 * nc, 2 * have_chords))) return rc;
    if ((rc = g->store.grow(g->touched, g->touched_cap, 2 * nc, have_touched))) return rc;
    if ((rc = g->store.grow(g->touched_ptr, g->touched_ptr_cap, 2 * nc + 1, have_touched ? have_touched + 1 : 0))) return rc;
    if ((rc = g->store.grow(g->touched_ent, g->touched_ent_cap, 2 * nc, 2 * have_chords))) return rc;
  }
  if ((rc = g->store.grow(g->chordH, g->chordH_cap, 36 * nc1))) return rc;
  if ((rc = g->store.grow(g->cscr, g->cscr_cap, 12 * nc1))) return rc;
  if ((rc = g->store.grow(g->diag, g->diag_cap, 36 * N))) return rc;
  if ((rc = g->store.grow(g->chain, g->chain_cap, 36 * N))) return rc;
  if ((rc = g->store.grow(g->grad, g->grad_cap, 6 * N))) return rc;
  if ((rc = g->store.grow(g->delta, g->delta_cap, 6 * N))) return rc;
  for (int v = 0; v < 5; v++) if ((rc = g->store.grow(g->vec[v], g->vec_cap[v], 6 * N))) return rc;
  size_t M = 1;
  while (M < N) M <<= 1;
  if ((rc = g->store.grow(g->LD, g->LD_cap, 72 * M))) return rc;
  if ((rc = g->store.grow(g->LU, g->LU_cap, 72 * M))) return rc;
  if ((rc = g->store.grow(g->LW, g->LW_cap, 72 * M))) return rc;
  if ((rc = g->store.grow(g->B, g->B_cap, 12 * M))) return rc;
  if ((rc = g->store.grow(g->X, g->X_cap, 12 * M))) return rc;
  if ((rc = g->store.grow(g->gst, g->gst_cap, (size_t)PGO_ST_WORDS + PGO_SOLVE_THREADS))) return rc;
  return g->store.grow(g->partials, g->partials_cap, (std::max(N, F) + PGO_FACTOR_THREADS - 1) / PGO_FACTOR_THREADS + 1);
}

// linearise at g->poses: slots, the assembled blocks, the cost into h_info[0] (valid after the stream has been waited for)
int pgo_enqueue_linearize(rolo_pgo* g) {
  hipStream_t s = g->stream;
  const int N = g->N, F = (int)g->factors.size(), nc = (int)g->chord_factor.size();
  pgo_linearize_kernel<<<(F + PGO_FACTOR_THREADS - 1) / PGO_FACTOR_THREADS, PGO_FACTOR_THREADS, 0, s>>>(g->d_factors, F, g->poses, g->slots);
  HIPCHK(hipGetLastError());
  pgo_assemble_kernel<<<(N + PGO_ASM_POSES - 1) / PGO_ASM_POSES, 256, 0, s>>>(g->slots, g->rowptr, g->entries, N, g->diag, g->chain, g->grad);
  HIPCHK(hipGetLastError());
  if (nc) { pgo_chord_kernel<<<(36 * nc + 255) / 256, 256, 0, s>>>(g->slots, g->d_chord_factor, nc, g->chordH); HIPCHK(hipGetLastError()); }
  pgo_sum_kernel<<<1, PGO_SUM_THREADS, 0, s>>>(g->slots, PGO_SLOT, 120, F, g->h_info);
  HIPCHK(hipGetLastError());
  return ROLO_OK;
}

int pgo_cap(int n_chords, int pcg_max) {
  if (pcg_max > 0) return pcg_max;
  return n_chords ? std::min(12 * n_chords + 2, 1000) : 1;   // without chords the preconditioner is the matrix: one application is the solve
}

// the grid form of the solve on the graph's stream. The host enqueues PCG iterations PGO_GRID_BATCH at a time and reads the pinned done word once after each
// batch; the iterations of a batch that follow the exit are empty launches. Never more than pcg_cap iterations are enqueued: the cap is the host's count
int pgo_enqueue_solve_grid(rolo_pgo* g, const SolveArgs& S) {
  hipStream_t s = g->stream;
  const int T = PGO_GRID_THREADS;
  const auto blocks = [](int n, int per) { return (n + per - 1) / per; };
  int l0 = 0;   // the first level that the fused top takes
  while ((S.M >> l0) > PGO_GRID_TOP) l0++;
  const auto apply = [&](double* dst) -> int {   // dst = T^-1 (the right-hand side in B)
    for (int l = 0; l < l0; l++) { pgo_grid_down_kernel<<<blocks(S.M >> (l + 1), PGO_GRID_TILE), T, 0, s>>>(S, l); HIPCHK(hipGetLastError()); }
    pgo_grid_top_apply_kernel<<<1, PGO_SOLVE_THREADS, 0, s>>>(S, l0, dst);
    HIPCHK(hipGetLastError());
    for (int l = l0 - 1; l >= 0; l--) { pgo_grid_up_kernel<<<blocks(S.M >> (l + 1), PGO_GRID_TILE), T, 0, s>>>(S, l, dst); HIPCHK(hipGetLastError()); }
    return ROLO_OK;
  };
  const auto dot = [&](const double* a, const double* b, int which) -> int {
    pgo_grid_lanes_kernel<<<PGO_SOLVE_THREADS / PGO_GRID_LANE_WG, PGO_GRID_LANE_WG, 0, s>>>(S, a, b);
    HIPCHK(hipGetLastError());
    pgo_grid_scalar_kernel<<<1, PGO_SOLVE_THREADS, 0, s>>>(S, which);
    HIPCHK(hipGetLastError());
    return ROLO_OK;
  };
  int rc;
  HIPCHK(hipEventRecord(g->gev[0], s));
  pgo_grid_fill_kernel<<<blocks(36 * S.M, T), T, 0, s>>>(S);
  HIPCHK(hipGetLastError());
  for (int l = 0; l < l0; l++) {
    const int nn = S.M >> (l + 1);
    pgo_grid_inv_kernel<<<blocks(nn, 64), 64, 0, s>>>(S, l);
    HIPCHK(hipGetLastError());
    pgo_grid_reduce_kernel<<<blocks(nn, PGO_GRID_TILE), T, 0, s>>>(S, l);
    HIPCHK(hipGetLastError());
  }
  pgo_grid_top_factor_kernel<<<1, PGO_SOLVE_THREADS, 0, s>>>(S, l0);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(g->gev[1], s));
  pgo_grid_start_kernel<<<blocks(6 * S.M, T), T, 0, s>>>(S);
  HIPCHK(hipGetLastError());
  if ((rc = apply(S.z))) return rc;
  if ((rc = dot(S.r, S.z, PGO_DOT_RZ0))) return rc;
  pgo_grid_dir_kernel<<<blocks(6 * S.N, T), T, 0, s>>>(S, 1);
  HIPCHK(hipGetLastError());
  for (int it = 0; it < S.pcg_cap;) {
    const int batch = std::min(PGO_GRID_BATCH, S.pcg_cap - it);
    for (int k = 0; k < batch; k++) {
      pgo_grid_mv_kernel<<<blocks(std::max(6 * S.N, 12 * S.n_chords), T), T, 0, s>>>(S);
      HIPCHK(hipGetLastError());
      if (S.n_touched) { pgo_grid_gather_kernel<<<blocks(6 * S.n_touched, T), T, 0, s>>>(S); HIPCHK(hipGetLastError()); }
      if ((rc = dot(S.p, S.q, PGO_DOT_PQ))) return rc;
      pgo_grid_step_kernel<<<blocks(6 * S.N, T), T, 0, s>>>(S);
      HIPCHK(hipGetLastError());
      if ((rc = apply(S.z))) return rc;
      if ((rc = dot(S.r, S.z, PGO_DOT_RZ))) return rc;
      pgo_grid_dir_kernel<<<blocks(6 * S.N, T), T, 0, s>>>(S, 0);
      HIPCHK(hipGetLastError());
    }
    it += batch;
    if (it < S.pcg_cap) {
      HIPCHK(hipStreamSynchronize(s));
      if (*(volatile double*)S.done != 0.0) break;
    }
  }
  pgo_grid_finish_kernel<<<blocks(6 * S.N, T), T, 0, s>>>(S);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(g->gev[2], s));
  return ROLO_OK;
}

int pgo_enqueue_solve(rolo_pgo* g, double lambda, double tol, int pcg_max) {
  SolveArgs S{};
  S.N = g->N; S.M = 1; S.L = 0;
  while (S.M < S.N) { S.M <<= 1; S.L++; }
  S.n_chords = (int)g->chord_factor.size(); S.n_touched = S.n_chords ? g->n_touched : 0; S.pcg_cap = pgo_cap(S.n_chords, pcg_max);
  S.lambda = lambda; S.tol = tol;
  S.diag = g->diag; S.chain = g->chain; S.grad = g->grad; S.chordH = g->chordH;
  S.chord_ij = g->d_chord_ij; S.touched = g->touched; S.touched_ptr = g->touched_ptr; S.touched_ent = g->touched_ent;
  S.LD = g->LD; S.LU = g->LU; S.LW = g->LW; S.B = g->B; S.X = g->X;
  S.x = g->vec[0]; S.r = g->vec[1]; S.z = g->vec[2]; S.p = g->vec[3]; S.q = g->vec[4]; S.cscr = g->cscr;
  S.delta = g->delta; S.info = g->h_info + 1;
  S.st = g->gst; S.lanes = g->gst + PGO_ST_WORDS; S.done = g->h_info + 6;
  const int form = g->solve_form != ROLO_PGO_SOLVE_AUTO ? g->solve_form : S.N >= PGO_GRID_FROM ? ROLO_PGO_SOLVE_GRID : ROLO_PGO_SOLVE_ONE_WG;
  g->last_form = form;
  if (form == ROLO_PGO_SOLVE_GRID) return pgo_enqueue_solve_grid(g, S);
  pgo_solve_kernel<<<1, PGO_SOLVE_THREADS, 0, g->stream>>>(S);
  HIPCHK(hipGetLastError());
  return ROLO_OK;
}

// device milliseconds of the last solve once the stream has been waited for: k = 0 the factorisation, 1 PCG. Between HIP events in the grid form; by the
// device's wall clock inside the one launch of the one-workgroup form
double pgo_solve_ms(rolo_pgo* g, int k) {
  if (g->last_form != ROLO_PGO_SOLVE_GRID) return g->h_info[4 + k] / g->wall_khz;
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, g->gev[k], g->gev[k + 1]);
  return (double)ms;
}

void pose6_of(const double* P, float* o) {   // pcl::getTranslationAndEulerAngles, transformTobeMapped order
  o[0] = (float)std::atan2(P[7], P[8]);
  o[1] = (float)std::asin(std::min(1.0, std::max(-1.0, -P[6])));
  o[2] = (float)std::atan2(P[3], P[0]);
  o[3] = (float)P[9]; o[4] = (float)P[10]; o[5] = (float)P[11];
}

int pgo_check_var(const double* var6) {
  for (int k = 0; k < 6; k++) if (!std::isfinite(var6[k]) || !(var6[k] > 0.0)) { ctx_set_error("pose graph: a variance must be finite and positive"); return ROLO_EINVAL; }
  return ROLO_OK;
}

void pgo_fill_factor(PgoFactor& f, int i, int j, const double* T, const double* var6) {
  f.i = i; f.j = j;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) f.Zi[3 * r + c] = T[4 * c + r];
    f.Zi[9 + r] = -(T[r] * T[3] + T[4 + r] * T[7] + T[8 + r] * T[11]);
  }
  for (int k = 0; k < 6; k++) f.isig[k] = 1.0 / std::sqrt(var6[k]);
}

bool pgo_finite_T(const double* T) { for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) if (!std::isfinite(T[4 * r + c])) return false; return true; }

}  // namespace

namespace rolo {
int pgo_reserve(rolo_pgo* g, int more_poses, int more_factors, int more_chords) {
  if (!g || more_poses < 0 || more_factors < 0 || more_chords < 0) return ROLO_EINVAL;
  if (g->N + more_poses > ROLO_PGO_MAX_POSES) { ctx_set_error("pose graph: more than ROLO_PGO_MAX_POSES poses"); return ROLO_EINVAL; }
  return pgo_reserve_impl(g, more_poses, more_factors, more_chords);
}
}  // namespace rolo

extern "C" {

int rolo_pgo_create(int device, rolo_pgo** out) {
  if (!out) return ROLO_EINVAL;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { ctx_set_error("no HIP device"); return ROLO_EHIP; }
  if (device < 0 || device >= count) return ROLO_EINVAL;
  HIPCHK(hipSetDevice(device));
  rolo_pgo* g = new rolo_pgo();
  g->device = device;
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0) g->wall_khz = (double)khz;
  if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&g->ev[0]) != hipSuccess || hipEventCreate(&g->ev[1]) != hipSuccess ||
      hipEventCreate(&g->gev[0]) != hipSuccess || hipEventCreate(&g->gev[1]) != hipSuccess || hipEventCreate(&g->gev[2]) != hipSuccess) {
    ctx_set_error("rolo_pgo_create: stream or events");
    rolo_pgo_destroy(g);
    return ROLO_EHIP;
  }
  g->store.stream = g->stream; g->store.who = "pose graph"; g->store.slack = 64;
  if (const int rc = g->store.alloc_pinned(g->h_info, 8)) { rolo_pgo_destroy(g); return rc; }
  *out = g;
  return ROLO_OK;
}

void rolo_pgo_destroy(rolo_pgo* g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  if (g->stream) (void)hipStreamSynchronize(g->stream);
  g->store.release();
  for (hipEvent_t e : g->ev) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : g->gev) if (e) (void)hipEventDestroy(e);
  if (g->stream) (void)hipStreamDestroy(g->stream);
  delete g;
}

void rolo_pgo_default_params(rolo_pgo_params* p) {
  if (!p) return;
  p->max_iterations = 100;
  p->absolute_error_tol = 1e-5;
  p->relative_error_tol = 1e-5;
  p->lambda_initial = 1e-5;
  p->lambda_factor = 10.0;
  p->lambda_upper = 1e5;
  p->pcg_tol = 1e-10;
  p->pcg_max_iterations = 0;
}

int rolo_pgo_add_pose(rolo_pgo* g, const double* T16) {
  if (!g || !T16) return ROLO_EINVAL;
  if (g->N >= ROLO_PGO_MAX_POSES) { ctx_set_error("rolo_pgo_add_pose: more than ROLO_PGO_MAX_POSES poses"); return ROLO_EINVAL; }
  if (!pgo_finite_T(T16)) { ctx_set_error("rolo_pgo_add_pose: a non-finite pose"); return ROLO_EINVAL; }
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) g->pending.push_back(T16[4 * r + c]);
  for (int r = 0; r < 3; r++) g->pending.push_back(T16[4 * r + 3]);
  g->inc.emplace_back();
  g->linearized = false;
  return g->N++;
}

int rolo_pgo_add_prior(rolo_pgo* g, int i, const double* T16, const double* var6) {
  if (!g || !T16 || !var6 || i < 0 || i >= g->N) return ROLO_EINVAL;
  if (!pgo_finite_T(T16)) { ctx_set_error("rolo_pgo_add_prior: a non-finite pose"); return ROLO_EINVAL; }
  if (pgo_check_var(var6)) return ROLO_EINVAL;
  if (g->factors.size() >= (size_t)(1 << 28)) return ROLO_EINVAL;
  PgoFactor f{};
  pgo_fill_factor(f, i, -1, T16, var6);
  const int id = (int)g->factors.size();
  g->factors.push_back(f);
  g->inc[i].push_back(id << 2);
  g->dirty_from = std::min(g->dirty_from, i);
  g->linearized = false;
  return ROLO_OK;
}

// k2: k^2 of the Cauchy loss, 0 for none
static int pgo_add_between(rolo_pgo* g, int i, int j, const double* T16, const double* var6, double k2) {
  if (!g || !T16 || !var6 || i < 0 || i >= g->N || j < 0 || j >= g->N || i == j) return ROLO_EINVAL;
  if (!pgo_finite_T(T16)) { ctx_set_error("rolo_pgo_add_between: a non-finite pose"); return ROLO_EINVAL; }
  if (pgo_check_var(var6)) return ROLO_EINVAL;
  if (g->factors.size() >= (size_t)(1 << 28)) return ROLO_EINVAL;
  PgoFactor f{};
  pgo_fill_factor(f, i, j, T16, var6);
  f.k2 = k2;
  const int id = (int)g->factors.size();
  g->factors.push_back(f);
  g->inc[i].push_back((id << 2) | (j == i + 1 ? 2 : 0));
  g->inc[j].push_back((id << 2) | (i == j + 1 ? 2 : 0) | 1);
  if (j != i + 1 && i != j + 1) { g->chord_factor.push_back(id); g->chord_ij.push_back(i); g->chord_ij.push_back(j); g->chords_dirty = true; }
  g->dirty_from = std::min(g->dirty_from, std::min(i, j));
  g->linearized = false;
  return ROLO_OK;
}

int rolo_pgo_add_between(rolo_pgo* g, int i, int j, const double* T16, const double* var6) { return pgo_add_between(g, i, j, T16, var6, 0.0); }

int rolo_pgo_add_between_robust(rolo_pgo* g, int i, int j, const double* T16, const double* var6, int loss, double k) {
  if (!g) return ROLO_EINVAL;
  if (loss != ROLO_PGO_LOSS_CAUCHY) { ctx_set_error("rolo_pgo_add_between_robust: only ROLO_PGO_LOSS_CAUCHY (the reference configures no other)"); return ROLO_EUNSUPPORTED; }
  if (!std::isfinite(k) || !(k > 0.0) || !std::isfinite(k * k) || !(k * k > 0.0)) { ctx_set_error("rolo_pgo_add_between_robust: k must be finite and positive"); return ROLO_EINVAL; }
  return pgo_add_between(g, i, j, T16, var6, k * k);
}

int rolo_pgo_size(rolo_pgo* g, int* n_poses, int* n_factors, int* n_chords) {
  if (!g) return ROLO_EINVAL;
  if (n_poses) *n_poses = g->N;
  if (n_factors) *n_factors = (int)g->factors.size();
  if (n_chords) *n_chords = (int)g->chord_factor.size();
  return ROLO_OK;
}

int rolo_pgo_linearize(rolo_pgo* g, double* cost, double* grad, double* diag, double* chain, double* chord, int32_t* chord_ij) {
  if (!g) return ROLO_EINVAL;
  if (g->N == 0 || g->factors.empty()) { ctx_set_error("rolo_pgo_linearize: the graph has no pose or no factor"); return ROLO_ESTATE; }
  int rc;
  if ((rc = pgo_sync_graph(g))) return rc;
  if ((rc = pgo_enqueue_linearize(g))) return rc;
  hipStream_t s = g->stream;
  const size_t N = (size_t)g->N, nc = g->chord_factor.size();
  if (grad) HIPCHK(hipMemcpyAsync(grad, g->grad, sizeof(double) * 6 * N, hipMemcpyDeviceToHost, s));
  if (diag) HIPCHK(hipMemcpyAsync(diag, g->diag, sizeof(double) * 36 * N, hipMemcpyDeviceToHost, s));
  if (chain && N > 1) HIPCHK(hipMemcpyAsync(chain, g->chain, sizeof(double) * 36 * (N - 1), hipMemcpyDeviceToHost, s));
  if (chord && nc) HIPCHK(hipMemcpyAsync(chord, g->chordH, sizeof(double) * 36 * nc, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (chord_ij) for (size_t k = 0; k < 2 * nc; k++) chord_ij[k] = g->chord_ij[k];
  if (cost) *cost = g->h_info[0];
  g->linearized = true;
  return ROLO_OK;
}

int rolo_pgo_solve_linear(rolo_pgo* g, double lambda, double pcg_tol, int pcg_max, double* delta, int* pcg_iterations, double* residual) {
  if (!g || !(lambda >= 0.0) || !(pcg_tol >= 0.0) || pcg_max < 0) return ROLO_EINVAL;
  if (!g->linearized) { ctx_set_error("rolo_pgo_solve_linear: call rolo_pgo_linearize first (the graph has changed since, or was never linearised)"); return ROLO_ESTATE; }
  HIPCHK(hipSetDevice(g->device));
  int rc;
  if ((rc = pgo_enqueue_solve(g, lambda, pcg_tol, pcg_max))) return rc;
  if (delta) HIPCHK(hipMemcpyAsync(delta, g->delta, sizeof(double) * 6 * (size_t)g->N, hipMemcpyDeviceToHost, g->stream));
  HIPCHK(hipStreamSynchronize(g->stream));
  if (g->h_info[3] != 0.0) { ctx_set_error("rolo_pgo_solve_linear: H + lambda I is not positive definite (lambda = 0 on a graph without a prior?)"); return ROLO_EINVAL; }
  if (pcg_iterations) *pcg_iterations = (int)g->h_info[1];
  if (residual) *residual = g->h_info[2];
  return ROLO_OK;
}

int rolo_pgo_optimize(rolo_pgo* g, const rolo_pgo_params* P, rolo_pgo_result* out) {
  if (!g || !P || !out) return ROLO_EINVAL;
  if (!(P->lambda_factor > 1.0) || !(P->lambda_initial >= 0.0) || !(P->pcg_tol >= 0.0) || P->pcg_max_iterations < 0 || !(P->absolute_error_tol >= 0.0) ||
      !(P->relative_error_tol >= 0.0)) { ctx_set_error("rolo_pgo_optimize: bad parameters"); return ROLO_EINVAL; }
  if (g->N == 0 || g->factors.empty()) { ctx_set_error("rolo_pgo_optimize: the graph has no pose or no factor"); return ROLO_ESTATE; }
  int rc;
  if ((rc = pgo_sync_graph(g))) return rc;
  hipStream_t s = g->stream;
  const int N = g->N, F = (int)g->factors.size(), grid = (std::max(N, F) + PGO_FACTOR_THREADS - 1) / PGO_FACTOR_THREADS;
  g->trace.clear();
  g->linearized = false;
  double acc_ms[4] = {0, 0, 0, 0};
  float ms = 0.f;
  auto linearize = [&]() -> int {
    HIPCHK(hipEventRecord(g->ev[0], s));
    int r = pgo_enqueue_linearize(g);
    if (r) return r;
    HIPCHK(hipEventRecord(g->ev[1], s));
    HIPCHK(hipEventSynchronize(g->ev[1]));
    (void)hipEventElapsedTime(&ms, g->ev[0], g->ev[1]);
    acc_ms[0] += ms;
    return ROLO_OK;
  };
  if ((rc = linearize())) return rc;
  double cost = g->h_info[0], lambda = P->lambda_initial;
  rolo_pgo_result res{};
  res.initial_cost = cost;
  while (true) {
    if (res.iterations >= P->max_iterations || res.trials >= PGO_MAX_TRIALS) { res.state = ROLO_PGO_ITERATIONS; break; }
    if (lambda > P->lambda_upper) { res.state = ROLO_PGO_LAMBDA; break; }
    if ((rc = pgo_enqueue_solve(g, lambda, P->pcg_tol, P->pcg_max_iterations))) return rc;
    HIPCHK(hipEventRecord(g->ev[0], s));
    pgo_retract_cost_kernel<<<grid, PGO_FACTOR_THREADS, 0, s>>>(g->d_factors, F, g->poses, N, g->delta, g->trial, g->partials);
    HIPCHK(hipGetLastError());
    pgo_sum_kernel<<<1, PGO_SUM_THREADS, 0, s>>>(g->partials, 1, 0, grid, g->h_info);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(g->ev[1], s));
    HIPCHK(hipEventSynchronize(g->ev[1]));
    (void)hipEventElapsedTime(&ms, g->ev[0], g->ev[1]);
    acc_ms[3] += ms; acc_ms[1] += pgo_solve_ms(g, 0); acc_ms[2] += pgo_solve_ms(g, 1);
    const bool bad = g->h_info[3] != 0.0;
    const double trial_cost = bad ? INFINITY : g->h_info[0];
    const int its = (int)g->h_info[1];
    res.trials++; res.pcg_iterations += its;
    const double change = cost - trial_cost;
    rolo_pgo_trace_rec tr{};
    tr.lambda = lambda; tr.cost = trial_cost; tr.accepted = change > 0.0; tr.pcg_iterations = its; tr.residual = g->h_info[2];
    g->trace.push_back(tr);
    if (change > 0.0) {
      std::swap(g->poses, g->trial); std::swap(g->poses_cap, g->trial_cap);
      lambda /= P->lambda_factor;
      res.iterations++;
      const double old = cost;
      cost = trial_cost;
      if (change <= P->absolute_error_tol || change <= P->relative_error_tol * old) { res.state = ROLO_PGO_CONVERGED; break; }
      if ((rc = linearize())) return rc;
    } else if (-change < P->absolute_error_tol) {   // not lowered, and not raised by a resolvable amount: nothing left to gain (a zero gradient ends here)
      res.state = ROLO_PGO_CONVERGED; break;
    } else {
      lambda *= P->lambda_factor;
    }
  }
  HIPCHK(hipStreamSynchronize(s));
  res.final_cost = cost; res.lambda = lambda;
  for (int k = 0; k < 4; k++) g->ms[k] = (float)acc_ms[k];
  *out = res;
  return ROLO_OK;
}

int rolo_pgo_get_poses(rolo_pgo* g, double* T16_out, float* pose6_out, int cap) {
  if (!g || cap < 0) return ROLO_EINVAL;
  const int n = std::min(g->N, cap);
  if (n == 0 || (!T16_out && !pose6_out)) return g->N;
  int rc;
  if ((rc = pgo_sync_graph(g))) return rc;
  std::vector<double> P(12 * (size_t)n);
  HIPCHK(hipMemcpyAsync(P.data(), g->poses, sizeof(double) * P.size(), hipMemcpyDeviceToHost, g->stream));
  HIPCHK(hipStreamSynchronize(g->stream));
  for (int k = 0; k < n; k++) {
    const double* p = P.data() + 12 * (size_t)k;
    if (T16_out) {
      double* T = T16_out + 16 * (size_t)k;
      for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) T[4 * r + c] = p[3 * r + c]; T[4 * r + 3] = p[9 + r]; }
      T[12] = T[13] = T[14] = 0.0; T[15] = 1.0;
    }
    if (pose6_out) pose6_of(p, pose6_out + 6 * (size_t)k);
  }
  return g->N;
}

int rolo_pgo_get_factor_errors(rolo_pgo* g, double* r2, double* weight, int cap) {
  if (!g || cap < 0) return ROLO_EINVAL;
  if (g->N == 0 || g->factors.empty()) { ctx_set_error("rolo_pgo_get_factor_errors: the graph has no pose or no factor"); return ROLO_ESTATE; }
  const int F = (int)g->factors.size(), n = std::min(F, cap);
  if (n == 0 || (!r2 && !weight)) return F;
  int rc;
  if ((rc = pgo_sync_graph(g))) return rc;
  if ((rc = g->store.grow(g->ferr, g->ferr_cap, 2 * (size_t)F))) return rc;
  pgo_factor_error_kernel<<<(F + PGO_FACTOR_THREADS - 1) / PGO_FACTOR_THREADS, PGO_FACTOR_THREADS, 0, g->stream>>>(g->d_factors, F, g->poses, g->ferr, g->ferr + F);
  HIPCHK(hipGetLastError());
  if (r2) HIPCHK(hipMemcpyAsync(r2, g->ferr, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, g->stream));
  if (weight) HIPCHK(hipMemcpyAsync(weight, g->ferr + F, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, g->stream));
  HIPCHK(hipStreamSynchronize(g->stream));
  return F;
}

int rolo_pgo_get_trace(rolo_pgo* g, rolo_pgo_trace_rec* out, int cap) {
  if (!g || cap < 0 || (cap && !out)) return ROLO_EINVAL;
  const int m = (int)g->trace.size();
  for (int i = 0; i < std::min(m, cap); i++) out[i] = g->trace[i];
  return m;
}

int rolo_pgo_set_solve_form(rolo_pgo* g, int form) {
  if (!g) return ROLO_EINVAL;
  if (form != ROLO_PGO_SOLVE_AUTO && form != ROLO_PGO_SOLVE_ONE_WG && form != ROLO_PGO_SOLVE_GRID) {
    ctx_set_error("rolo_pgo_set_solve_form: the form is ROLO_PGO_SOLVE_AUTO, ROLO_PGO_SOLVE_ONE_WG or ROLO_PGO_SOLVE_GRID");
    return ROLO_EINVAL;
  }
  g->solve_form = form;
  return ROLO_OK;
}

int rolo_pgo_get_solve_form(rolo_pgo* g, int* requested, int* last_used) {
  if (!g) return ROLO_EINVAL;
  if (requested) *requested = g->solve_form;
  if (last_used) *last_used = g->last_form;
  return ROLO_OK;
}

int rolo_pgo_last_ms(rolo_pgo* g, float* ms4) {
  if (!g || !ms4) return ROLO_EINVAL;
  for (int k = 0; k < 4; k++) ms4[k] = g->ms[k];
  return ROLO_OK;
}

}  // extern "C"
