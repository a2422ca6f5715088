// What an LM pass does to a point, for every launch form of the LM iteration (passes.hip: pass + controller launches and one launch per trial; lm_persist.hip: the
// resident kernel): the point and voxel-record loads, the per-correspondence terms of both stages, accumulate_hb, the wavefront / workgroup reduction with its DPP
// moves, the row layout and the XCD mapping of the point blocks. The forms give the same bits because they add these terms, in this operation order.
#pragma once
#include "rolo_internal.hpp"
#include "dev_math.hpp"
#include "voxel_dev.hpp"

namespace rolo {
namespace {   // (internal linkage in every unit that includes this: c_offsets, and the kernels built from these functions)

// neighbor_offsets (vmp_voxel.hpp:13-47): [0] DIRECT1, [1..8) DIRECT7, [8..35) DIRECT27
__constant__ int c_offsets[35][3] = {
    {0, 0, 0},
    {0, 0, 0}, {1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1},
    {-1, -1, -1}, {-1, -1, 0}, {-1, -1, 1}, {-1, 0, -1}, {-1, 0, 0}, {-1, 0, 1}, {-1, 1, -1}, {-1, 1, 0}, {-1, 1, 1},
    {0, -1, -1},  {0, -1, 0},  {0, -1, 1},  {0, 0, -1},  {0, 0, 0},  {0, 0, 1},  {0, 1, -1},  {0, 1, 0},  {0, 1, 1},
    {1, -1, -1},  {1, -1, 0},  {1, -1, 1},  {1, 0, -1},  {1, 0, 0},  {1, 0, 1},  {1, 1, -1},  {1, 1, 0},  {1, 1, 1}};

ROLO_DEV int offset_base(int n_off) { return n_off == 1 ? 0 : (n_off == 7 ? 1 : 8); }

struct Rec { Vec3 mean; Sym3 cov; double w; };
ROLO_DEV Rec load_rec(const double* __restrict__ rec, int id) {
  const double* r = rec + (size_t)id * REC_DOUBLES;
  Rec o;
  o.mean = Vec3{r[0], r[1], r[2]};
  o.cov = Sym3{r[3], r[4], r[5], r[6], r[7], r[8]};
  o.w = r[9];
  return o;
}

// DPP lane moves of a double (two 32-bit halves): pure VALU, no LDS crossbar. Lanes a row_mask leaves out receive 0.0.
template <int CTRL, int ROW_MASK = 0xf>
ROLO_DEV double dpp_mov_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, false);
  return __hiloint2double(hi, lo);
}
// Sum over the wavefront, result valid in lane 63: pairs, quads (quad_perm), 8 (row_half_mirror), 16 (row_mirror),
// 32 (row_bcast:15 into rows 1 and 3), 64 (row_bcast:31 into rows 2 and 3). ds_bpermute exchanges cost ~40 cycles each
// here (the LDS crossbar is shared by the CU's wavefronts): 144 of them were a third of the SO(3) pass.
ROLO_DEV double wave_sum_dpp63(double v) {
  v += dpp_mov_f64<0xB1>(v);          // quad_perm [1,0,3,2]
  v += dpp_mov_f64<0x4E>(v);          // quad_perm [2,3,0,1]
  v += dpp_mov_f64<0x141>(v);         // row_half_mirror
  v += dpp_mov_f64<0x140>(v);         // row_mirror
  v += dpp_mov_f64<0x142, 0xa>(v);    // row_bcast:15
  v += dpp_mov_f64<0x143, 0xc>(v);    // row_bcast:31
  return v;
}

// Sum NV per-lane values over the 64 lanes of the wavefront as a reduce-scatter WITHOUT selects (round 5). At every halving step the
// values are taken in pairs (k, k + half): the lanes whose step bit is 0 will own value k, the others value k + half, and each hands the
// value it does not own to its partner and adds what it receives. gfx950's v_permlane32_swap / v_permlane16_swap do the hand-over of a
// whole pair in place — swap(X, Y) leaves [X.lo | Y.lo] in X and [X.hi | Y.hi] in Y, so X + Y IS the step (2 swaps + 1 add per pair of
// doubles, no v_cndmask); inside a row of 16 the same step is three DPP moves under a bank mask (keep = X with Y's banks patched in,
// received = row_ror:8 / row_shl:4 + row_shr:4 of the other value) and the last two distances are plain butterflies on what is left.
// 12 values (SO(3) pass): 63 VALU instructions against 216 for one DPP butterfly per value; 30 values (translation / 6-dof passes): 126
// against ~400 for round 2's reduce-scatter, whose generic lane-xor moves paid four v_cndmask per exchanged double (half of that
// kernel's instructions). Afterwards lane l holds the complete sums of the NP / 16 values j + (NP / 16) * (b2 + 2 b3 + 4 b4 + 8 b5),
// b_i = bit i of l — identical in the four lanes of a quad; the order of the additions is fixed (deterministic).
ROLO_DEV void rs_swap32(double& x, double& y) {
  const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
  x = __hiloint2double((int)hi[0], (int)lo[0]); y = __hiloint2double((int)hi[1], (int)lo[1]);
}
ROLO_DEV void rs_swap16(double& x, double& y) {
  const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
  x = __hiloint2double((int)hi[0], (int)lo[0]); y = __hiloint2double((int)hi[1], (int)lo[1]);
}
// one reduce-scatter step inside a row of 16 lanes: OFF = 8 (banks 0,1 own x, banks 2,3 own y) or 4 (banks 0,2 own x, banks 1,3 own y)
template <int OFF>
ROLO_DEV double rs_row_step(double x, double y) {
  constexpr int YB = OFF == 8 ? 0xc : 0xa, XB = OFF == 8 ? 0x3 : 0x5;   // bank masks of the lanes that own y / x
  constexpr int UP = OFF == 8 ? 0x128 : 0x104, DN = OFF == 8 ? 0x128 : 0x114;   // lane <- lane + OFF (row_ror:8 / row_shl:4), lane <- lane - OFF (row_ror:8 / row_shr:4)
  const int xl = __double2loint(x), xh = __double2hiint(x), yl = __double2loint(y), yh = __double2hiint(y);
  const int kl = __builtin_amdgcn_update_dpp(xl, yl, 0xE4, 0xf, YB, false), kh = __builtin_amdgcn_update_dpp(xh, yh, 0xE4, 0xf, YB, false);   // keep: x, y where y is owned
  int rl = __builtin_amdgcn_update_dpp(0, xl, UP, 0xf, XB, false), rh = __builtin_amdgcn_update_dpp(0, xh, UP, 0xf, XB, false);               // received: the partner's x ...
  rl = __builtin_amdgcn_update_dpp(rl, yl, DN, 0xf, YB, false); rh = __builtin_amdgcn_update_dpp(rh, yh, DN, 0xf, YB, false);                 // ... or the partner's y
  return __hiloint2double(kh, kl) + __hiloint2double(rh, rl);
}
template <int NV>
ROLO_DEV void wave_reduce_scatter(const double (&acc)[NV], double* __restrict__ red_row /* LDS, NV_MAX */) {
  constexpr int NP = NV <= 16 ? 16 : 32;
  constexpr int NL = NP / 16;   // values left per lane after the four scatter steps
  static_assert(NV <= 32, "at most 32 values");
  const int lane = threadIdx.x & 63;
  double v[NP];
#pragma unroll
  for (int k = 0; k < NP; k++) v[k] = k < NV ? acc[k] : 0.0;
#pragma unroll
  for (int k = 0; k < NP / 2; k++) { rs_swap32(v[k], v[k + NP / 2]); v[k] += v[k + NP / 2]; }
#pragma unroll
  for (int k = 0; k < NP / 4; k++) { rs_swap16(v[k], v[k + NP / 4]); v[k] += v[k + NP / 4]; }
#pragma unroll
  for (int k = 0; k < NP / 8; k++) v[k] = rs_row_step<8>(v[k], v[k + NP / 8]);
#pragma unroll
  for (int k = 0; k < NL; k++) v[k] = rs_row_step<4>(v[k], v[k + NL]);
#pragma unroll
  for (int k = 0; k < NL; k++) { v[k] += lane_xor_f64<2>(v[k]); v[k] += lane_xor_f64<1>(v[k]); }
  if ((lane & 3) == 0) {
    const int base = NL * (((lane >> 2) & 1) + 2 * ((lane >> 3) & 1) + 4 * ((lane >> 4) & 1) + 8 * ((lane >> 5) & 1));
#pragma unroll
    for (int k = 0; k < NL; k++) if (base + k < NV) red_row[base + k] = v[k];
  }
}

// A pass's accumulators are compact — [0] = yi, [1] = y, [2] = n, [3 .. 3 + nh) H's lower triangle, then b — and so are the rows the fat workgroups exchange; the
// scalar step reads the V_* slots (rolo_internal.hpp): entry t of a compact row with nh entries of H belongs in slot row_slot(t, nh)
ROLO_DEV constexpr int row_slot(int t, int nh) { return t < 3 ? t : (t < 3 + nh ? V_H + (t - 3) : V_B + (t - 3 - nh)); }

// only_first (wave-uniform): a pass that evaluated the trial cost alone (LmState::lin_skip) has ONE value to sum — acc[0] — and writes zeros to the other slots
// The wavefronts' sums are added in groups of PASS_THREADS / 64, the groups after one another: the row of a fat workgroup (the one-launch-per-trial form, the resident
// kernel) is the sum, in order, of the rows that the pass kernel's workgroups write for the same points, so a cloud that is ONE row there (up to 512 points at one point
// per thread) ends at the same bits in all three launch forms. (Until then the 8 wavefronts of a 512-thread workgroup were added in one run: the forms differed in
// the last bit of H and b, tests/test_gpu_voxel_cases.py.) With THREADS == PASS_THREADS this is the one run it always was.
template <int ROWS>
ROLO_DEV double sum_wave_rows(const double (*red)[NV_MAX], int col) {
  constexpr int G = PASS_THREADS / 64;
  static_assert(ROWS % G == 0, "a workgroup is whole groups of the pass kernel's wavefronts");
  double s = 0;
#pragma unroll
  for (int g0 = 0; g0 < ROWS; g0 += G) {
    double sg = 0;
#pragma unroll
    for (int w = 0; w < G; w++) sg += red[g0 + w][col];
    s += sg;
  }
  return s;
}
template <int NV, int THREADS = PASS_THREADS>
ROLO_DEV void block_reduce_store(double (&acc)[NV], const int (&slot)[NV], double* __restrict__ out_row, bool only_first = false) {
  __shared__ double red[THREADS / 64][NV_MAX];
  const int wv = threadIdx.x >> 6;
  if (only_first) {
    // the additions value 0 goes through in wave_reduce_scatter, in the same order (lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1: lane 0 ends up with the same bits), so a
    // trial's cost does not depend on whether its pass carried the linearisation half
    double t = acc[0];
    t += lane_xor_f64<32>(t); t += lane_xor_f64<16>(t); t += lane_xor_f64<8>(t); t += lane_xor_f64<4>(t); t += lane_xor_f64<2>(t); t += lane_xor_f64<1>(t);
    if ((threadIdx.x & 63) == 0) red[wv][0] = t;
    __syncthreads();
    if (threadIdx.x < NV) {
      double s0 = 0;
      if (threadIdx.x == 0) s0 = sum_wave_rows<THREADS / 64>(red, 0);
      int sl = 0;
#pragma unroll
      for (int v = 0; v < NV; v++) if (threadIdx.x == v) sl = slot[v];
      out_row[sl] = s0;
    }
    return;
  }
  wave_reduce_scatter<NV>(acc, red[wv]);
  __syncthreads();
  if (threadIdx.x < NV) {
    const double s = sum_wave_rows<THREADS / 64>(red, threadIdx.x);
    // slot[] is a compile-time table; pick by thread index
    int sl = 0;
#pragma unroll
    for (int v = 0; v < NV; v++) if (threadIdx.x == v) sl = slot[v];
    out_row[sl] = s;
  }
}

// H += wh * J^T M J, b += J^T Mv_b for J = [skew(a) | -I]  (rot_vgicp_impl.hpp:264-266, 353, 576-578). The columns u_i of J are
// u_0 = (0, a.z, -a.y), u_1 = (-a.z, 0, a.x), u_2 = (a.y, -a.x, 0), u_3.. = -e_x, -e_y, -e_z. Round 5: the structure is written out — the
// zero components are dropped (0 * x + y IS y for the finite values a pass sees) and the -I columns are read off M: -M's columns, H's
// translation block wh * M, the mixed block -wh * (M u_j) — instead of the generic dot3(u_i, M u_j) with its multiplications by 0.0 and
// -1.0, which the compiler must keep. Same operation order for what remains, so H and b keep their bits (up to the sign of a zero);
// 42 fp64 instructions against 60 (SO(3)), 60 against 156 (6 dof).
// acc layout inside the kernels: [0]=yi [1]=y [2]=n [3 .. 3+NH) H lower triangle, then b
template <int DOF>
ROLO_DEV void accumulate_hb(const Sym3& M, const Vec3& a, double wh, double wb_unused, const Vec3& Mv_b, double* Hacc, double* bacc) {
  (void)wb_unused;
  // (p2: the generic expression's own order once its zero term is gone — the first product rounded, the second fused into the sum)
  auto p2 = [](double x1, double y1, double x2, double y2) { return fma(x2, y2, x1 * y1); };
  // M u_j for the three skew columns: two products per component
  const Vec3 Mu0{p2(M.xy, a.z, M.xz, -a.y), p2(M.yy, a.z, M.yz, -a.y), p2(M.yz, a.z, M.zz, -a.y)};
  const Vec3 Mu1{p2(M.xx, -a.z, M.xz, a.x), p2(M.xy, -a.z, M.yz, a.x), p2(M.xz, -a.z, M.zz, a.x)};
  const Vec3 Mu2{p2(M.xx, a.y, M.xy, -a.x), p2(M.xy, a.y, M.yy, -a.x), p2(M.xz, a.y, M.yz, -a.x)};
  // rotation block, lower triangle row-major: (0,0) (1,0) (1,1) (2,0) (2,1) (2,2); u_i . v with the zero component left out
  auto d0 = [&](const Vec3& v) { return p2(a.z, v.y, -a.y, v.z); };
  auto d1 = [&](const Vec3& v) { return p2(-a.z, v.x, a.x, v.z); };
  auto d2 = [&](const Vec3& v) { return p2(a.y, v.x, -a.x, v.y); };
  if constexpr (DOF == 3) {
    Hacc[0] += wh * d0(Mu0);
    Hacc[1] += wh * d1(Mu0); Hacc[2] += wh * d1(Mu1);
    Hacc[3] += wh * d2(Mu0); Hacc[4] += wh * d2(Mu1); Hacc[5] += wh * d2(Mu2);
    bacc[0] += d0(Mv_b); bacc[1] += d1(Mv_b); bacc[2] += d2(Mv_b);
  } else {
    static_assert(DOF == 6, "3 or 6 degrees of freedom");
    // row-major lower triangle of the 6 x 6: rows 0..2 as above, row 3+c = [ -(M u_0).c  -(M u_1).c  -(M u_2).c | M(c, 0..c) ]
    Hacc[0] += wh * d0(Mu0);
    Hacc[1] += wh * d1(Mu0); Hacc[2] += wh * d1(Mu1);
    Hacc[3] += wh * d2(Mu0); Hacc[4] += wh * d2(Mu1); Hacc[5] += wh * d2(Mu2);
    Hacc[6] += wh * (-Mu0.x); Hacc[7] += wh * (-Mu1.x); Hacc[8] += wh * (-Mu2.x); Hacc[9] += wh * M.xx;
    Hacc[10] += wh * (-Mu0.y); Hacc[11] += wh * (-Mu1.y); Hacc[12] += wh * (-Mu2.y); Hacc[13] += wh * M.xy; Hacc[14] += wh * M.yy;
    Hacc[15] += wh * (-Mu0.z); Hacc[16] += wh * (-Mu1.z); Hacc[17] += wh * (-Mu2.z); Hacc[18] += wh * M.xz; Hacc[19] += wh * M.yz; Hacc[20] += wh * M.zz;
    bacc[0] += d0(Mv_b); bacc[1] += d1(Mv_b); bacc[2] += d2(Mv_b);
    bacc[3] -= Mv_b.x; bacc[4] -= Mv_b.y; bacc[5] -= Mv_b.z;
  }
}

// wave-uniform values that come out of LDS (the fused launches keep the state there) belong in scalar registers
ROLO_DEV double uni(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
ROLO_DEV int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// what a pass needs of one source point: loaded before anything that depends on the LM state
// CA: the six-entry covariance; or, when the PLANE covariances were computed by the library (a.nrm), m with C_A = I - m m^T: 24 bytes per point and pass
// instead of 48, and the rotation R C_A R^T = R R^T - (R m)(R m)^T is 27 multiply-adds instead of 45 (rotated_cov)
struct PtIn { float4 pf; Sym3 CA; Vec3 m; };
ROLO_DEV PtIn load_pt(const PassArgs& a, int i) {
  PtIn o{};
  o.pf = a.src[i];
  const size_t pitch = (size_t)a.n_total;
  if (a.nrm) {
    o.m = Vec3{a.nrm[i], a.nrm[pitch + i], a.nrm[2 * pitch + i]};
    if (o.m.x == o.m.x) return o;   // (NaN: a rank <= 1 neighbourhood whose covariance is not of the plane form — knn_covariance_finish — takes its six entries)
  }
  o.CA = Sym3{a.cov[i], a.cov[pitch + i], a.cov[2 * pitch + i], a.cov[3 * pitch + i], a.cov[4 * pitch + i], a.cov[5 * pitch + i]};
  return o;
}
// R (I - m m^T) R^T = R R^T - (R m)(R m)^T. R R^T is NOT taken as the identity: a caller's guess arrives as a float matrix, orthonormal to 1e-7 only, and the
// reference rotates the covariance with exactly that matrix (rot_vgicp_impl.hpp:204-222) — the first version of this path assumed I and was 2e-6 off in the cost of a
// solve started from a float guess. The product comes from the LM state, where the controller keeps it next to each rotation (lm_set_rrt): 9 + 6 multiply-adds per
// lane are left of the rotation's 45.
ROLO_DEV Sym3 rotated_plane_cov(const double* R, const double* __restrict__ S6 /* R R^T from the LM state (lm_set_rrt) */, const Vec3& m) {
  const Sym3 S{uni(S6[0]), uni(S6[1]), uni(S6[2]), uni(S6[3]), uni(S6[4]), uni(S6[5])};
  const Vec3 q = mat3_mulv(R, m);
  return Sym3{S.xx - q.x * q.x, S.xy - q.x * q.y, S.xz - q.x * q.z, S.yy - q.y * q.y, S.yz - q.y * q.z, S.zz - q.z * q.z};
}
ROLO_DEV Sym3 rotated_cov(const PassArgs& a, const double* R, const double* __restrict__ S6, const PtIn& in) {
  if (a.nrm && in.m.x == in.m.x) return rotated_plane_cov(R, S6, in.m);
  return sym3_rotate(R, in.CA);
}

// ---- the per-correspondence terms: every launch form adds these, in this operation order ------------------------------------------------------------------
// rotation / 6-dof stage, (A): compute_error's term on a cached correspondence, M = the Mahalanobis matrix of the linearisation pose
ROLO_DEV void rot_cost_term(double* acc, const Vec3& mean, double w, const Sym3& M, const Vec3& tp) {
  const Vec3 e{mean.x - tp.x, mean.y - tp.y, mean.z - tp.z};
  acc[0] += w * dot3(e, sym3_mulv(M, e));
}
// rotation / 6-dof stage, (B): so3_linearize / linearize's term on a correspondence found at the trial pose
template <int DOF>
ROLO_DEV void rot_lin_term(double* acc, const Vec3& mean, double w, const Sym3& M, const Vec3& tp) {
  constexpr int NH = DOF * (DOF + 1) / 2;
  const Vec3 e{mean.x - tp.x, mean.y - tp.y, mean.z - tp.z};
  const Vec3 Me = sym3_mulv(M, e);
  acc[1] += w * dot3(e, Me);
  acc[2] += 1.0;
  const Vec3 wMe{w * Me.x, w * Me.y, w * Me.z};
  accumulate_hb<DOF>(M, tp, w, 0.0, wMe, &acc[3], &acc[3 + NH]);
}
// what a rotation / 6-dof pass reads of the LM state (wave-uniform: scalar registers)
struct RotUni {
  int phase, cur; bool skip_lin; double R0[9], R1[9], t1[3];
  ROLO_DEV explicit RotUni(const LmState* __restrict__ st) {
    phase = uni(st->phase); cur = uni(st->cur);
    skip_lin = phase == 1 && uni(st->lin_skip) != 0;   // (A) only: the trial before this one was rejected (LmState::lin_skip)
#pragma unroll
    for (int k = 0; k < 9; k++) { R0[k] = uni(st->x0_R[k]); R1[k] = uni(st->xt_R[k]); }
#pragma unroll
    for (int k = 0; k < 3; k++) t1[k] = uni(st->xt_t[k]);
  }
  ROLO_DEV Vec3 at_trial(const Vec3& p) const { Vec3 tp = mat3_mulv(R1, p); tp.x += t1[0]; tp.y += t1[1]; tp.z += t1[2]; return tp; }
};
// what a translation pass reads of the LM state, and its term on one correspondence: t3_linearize (B) + compute_t_error (A), Mahalanobis from st->tr_R
struct TransUni {
  int phase, tr_cur; bool skip_lin; double R[9]; Vec3 tt, g, lAq, lBq; double lam_n, inv_dtn;
  ROLO_DEV explicit TransUni(const LmState* __restrict__ st) {
    phase = uni(st->phase);
    skip_lin = phase == 1 && uni(st->lin_skip) != 0;
    tr_cur = uni(st->tr_cur);
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = uni(st->tr_R[k]);
    tt = Vec3{uni(st->tt[0]), uni(st->tt[1]), uni(st->tt[2])};
    g = Vec3{uni(st->g[0]), uni(st->g[1]), uni(st->g[2])};
    lam_n = uni(st->lam_over_n);
    // last_transform keeps its initial value — Zero in t3_linearize (:539), (1,0,0,0) in compute_t_error (:637). The quotients
    // last / dt_{n-1} and 1 / dt_n are the same for every point: formed once when the stage starts (trans_consts), not by every lane of every pass
    // (seven fp64 divisions = ~100 of the pass's ~700 instructions).
    lAq = Vec3{uni(st->lastA_q[0]), uni(st->lastA_q[1]), uni(st->lastA_q[2])}; lBq = Vec3{uni(st->lastB_q[0]), uni(st->lastB_q[1]), uni(st->lastB_q[2])};
    inv_dtn = uni(st->inv_dtn);
  }
};
// the point's own part of a translation term: the same for every correspondence of the point
struct TransPt {
  Vec3 tp, ctA, ctB;
  ROLO_DEV TransPt(const TransUni& u, const Vec3& p) {
    tp = Vec3{p.x + u.tt.x, p.y + u.tt.y, p.z + u.tt.z};
    const Vec3 ba{p.x - u.g.x, p.y - u.g.y, p.z - u.g.z};
    // (times 1 / dt_n instead of the reference's division: one rounding of a uniform factor, far below the rounding noise ba - tp already carries — the
    // difference is -(g + t) for every point in exact arithmetic — and three fp64 divisions = 45 instructions per lane and pass less)
    const Vec3 dv{(ba.x - tp.x) * u.inv_dtn, (ba.y - tp.y) * u.inv_dtn, (ba.z - tp.z) * u.inv_dtn};
    ctA = Vec3{dv.x - u.lAq.x, dv.y - u.lAq.y, dv.z - u.lAq.z};
    ctB = Vec3{dv.x - u.lBq.x, dv.y - u.lBq.y, dv.z - u.lBq.z};
  }
};
ROLO_DEV void trans_term(double* acc, const TransUni& u, const TransPt& q, const Vec3& mean, double w, const Sym3& M) {
  constexpr int NH = 21;
  const Vec3 e{mean.x - q.tp.x, mean.y - q.tp.y, mean.z - q.tp.z};
  const Vec3 Me = sym3_mulv(M, e);
  const double eMe = dot3(e, Me);
  if (u.phase == 1) acc[0] += w * (eMe + u.lam_n * dot3(q.ctA, sym3_mulv(M, q.ctA)));
  if (u.skip_lin) return;   // the trial before this one was rejected: the cost alone (LmState::lin_skip)
  const Vec3 McB = sym3_mulv(M, q.ctB);
  acc[1] += w * (eMe + u.lam_n * dot3(q.ctB, McB));
  acc[2] += 1.0;
  const double s1 = u.lam_n * u.inv_dtn;
  const Vec3 vb{w * (Me.x + s1 * McB.x), w * (Me.y + s1 * McB.y), w * (Me.z + s1 * McB.z)};
  accumulate_hb<6>(M, q.tp, w * (1.0 + u.lam_n * u.inv_dtn * u.inv_dtn), 0.0, vb, &acc[3], &acc[3 + NH]);
}

template <int DOF>
ROLO_DEV void rot_pass_compute(const PassArgs& a, const LmState* __restrict__ st, const int i, const bool valid, const PtIn& in,
                               double (&acc)[3 + DOF * (DOF + 1) / 2 + DOF]) {
  const RotUni u(st);
  const int* __restrict__ corr_old = a.corr[u.cur];
  int* __restrict__ corr_new = a.corr[u.phase == 0 ? u.cur : (u.cur ^ 1)];
  if (valid) {
    const float4 pf = in.pf;
    const Vec3 tp = u.at_trial(Vec3{(double)pf.x, (double)pf.y, (double)pf.z});
    const int n_off = a.n_off;
    // (A) compute_error(xi): cached correspondences, Mahalanobis of the linearisation pose x0
    // (round 5 measured the reference's per-correspondence Mahalanobis cache here — six fp64 of M(x0) per point, written by the (B) half, read by the next
    // trial's (A) half, rot_vgicp_impl.hpp:204-222 — and it LOST: 96 B per point and pass of extra traffic cost more than the ~100 instructions saved,
    // 2694 against 2875 scans/s; profiles/DEAD_ENDS.md. Neither stage of these PASS kernels caches M: the translation stage's cache, whose M is constant, measured neutral and is not kept either. The resident kernel does — in LDS, where it costs no traffic: lmp_rot_body.)
    if (u.phase == 1) {
      const Sym3 RCA0 = rotated_cov(a, u.R0, st->x0_S, in);
      for (int o = 0; o < n_off; o++) {
        const int vid = corr_old[(size_t)i * n_off + o];
        if (vid >= 0) {
          const Rec r = load_rec(a.tab.rec, vid);
          rot_cost_term(acc, r.mean, r.w, sym3_inverse(sym3_add(r.cov, RCA0)), tp);
        }
      }
    }
    // (B) so3_linearize / linearize at xi, with update_correspondences(xi) fused in
    if (u.skip_lin) return;
    int kx, ky, kz;
    voxel_coord_dev(a.tab, tp.x, tp.y, tp.z, kx, ky, kz);
    const Sym3 RCA1 = rotated_cov(a, u.R1, st->xt_S, in);
    const int ob = offset_base(n_off);
    for (int o = 0; o < n_off; o++) {
      const int vid = voxel_lookup(a.tab, kx + c_offsets[ob + o][0], ky + c_offsets[ob + o][1], kz + c_offsets[ob + o][2]);
      corr_new[(size_t)i * n_off + o] = vid;
      if (vid >= 0) {
        const Rec r = load_rec(a.tab.rec, vid);
        rot_lin_term<DOF>(acc, r.mean, r.w, sym3_inverse(sym3_add(r.cov, RCA1)), tp);
      }
    }
  }
}

// the translation stage's pass over one point, on the correspondences of the last rotation linearisation
ROLO_DEV void trans_pass_compute(const PassArgs& a, const LmState* __restrict__ st, const int i, const bool valid, const PtIn& in, double (&acc)[30]) {
  const TransUni u(st);
  const int* __restrict__ corr = a.corr[u.tr_cur];
  // (the stage's Mahalanobis matrices are those of the LAST rotation linearisation — constant over all its passes. Caching the six fp64 per point
  // after the first pass instead of rotating / inverting again was measured in round 5 and is not kept: 2957 against 2958 scans/s, profiles/DEAD_ENDS.md)
  if (valid) {
    const float4 pf = in.pf;
    const TransPt q(u, Vec3{(double)pf.x, (double)pf.y, (double)pf.z});
    const int n_off = a.n_off;
    const Sym3 RCA = rotated_cov(a, u.R, st->tr_S, in);
    for (int o = 0; o < n_off; o++) {
      const int vid = corr[(size_t)i * n_off + o];
      if (vid < 0) continue;
      const double* __restrict__ rr = a.tab.rec + (size_t)vid * REC_DOUBLES;
      const Vec3 mean{rr[0], rr[1], rr[2]};
      const double w = rr[9];
      trans_term(acc, u, q, mean, w, sym3_inverse(sym3_add(Sym3{rr[3], rr[4], rr[5], rr[6], rr[7], rr[8]}, RCA)));
    }
  }
}
// STAGE 1: the rotation / 6-dof stage's pass (DOF 3 or 6); STAGE 2: the translation stage's (DOF 6)
template <int STAGE, int DOF>
ROLO_DEV void pass_compute(const PassArgs& a, const LmState* __restrict__ st, const int i, const bool valid, const PtIn& in, double (&acc)[3 + DOF * (DOF + 1) / 2 + DOF]) {
  if constexpr (STAGE == 1) rot_pass_compute<DOF>(a, st, i, valid, in, acc);
  else trans_pass_compute(a, st, i, valid, in, acc);
}
// the ppt slabs of a fat workgroup's points, one point after the other (the resident kernel's generic body)
template <int STAGE, int DOF, int THREADS>
ROLO_DEV void pass_slabs(const PassArgs& a, const LmState* __restrict__ st, const int i0, const int ppt, double (&acc)[3 + DOF * (DOF + 1) / 2 + DOF]) {
  for (int p = 0; p < ppt; p++) {   // (twins: lm_kernel's two loops, whose first point is in flight before the prologue)
    const int i = i0 + p * THREADS;
    const bool valid = i < a.end;
    PtIn in{};
    if (valid) in = load_pt(a, i);
    pass_compute<STAGE, DOF>(a, st, i, valid, in, acc);
  }
}

// Workgroup b of a launch runs on XCD b mod 8, and every XCD has its own L2, emptied at every kernel boundary: with the points dealt round-robin each
// XCD fetches (nearly) ALL voxel records and hash slots again in every pass — 8 x the map from the Infinity Cache per launch. A LiDAR cloud arrives in
// firing order (column-major: consecutive points sweep the azimuth), so giving XCD x the x-th EIGHTH of the point blocks makes it a 45-degree sector
// whose voxels no other XCD needs (round 5; the permutation of knn_packet.hpp's small-launch case). Rows stay indexed by the logical block: the
// controller's summation order does not depend on the mapping.
ROLO_DEV int pass_xcd_block(const PassArgs& a, int b, int G) {
  if (!a.xcd_map) return b;
  const int x = b & 7, k = b >> 3, q = G >> 3, r = G & 7;   // XCD x owns G / 8 (+1 for x < G % 8) consecutive blocks
  return x * q + min(x, r) + k;
}
}  // namespace
}  // namespace rolo
