// The loop closure's ICP on gfx950: pcl::IterativeClosestPoint as performRSLoopClosure / performSCLoopClosure configure it (reference src/backMapping.cpp:2339-2354,
// :2430-2446: SVD estimation, no rejectors, no RANSAC) and getFitnessScore, on two clouds that are on the device already (the key map's loop clouds, submap.hip
// rolo_keymap_loop_cloud) or come from the host (rolo_loopicp_align). PCL is not in the reference tree: the contract is the statement in include/rolo_hip.h, which
// tests/icp_twin.py restates in numpy.
//
// MI355X design: the target gets the Hilbert-sorted implicit BVH of the neighbour search (knn_cov.hip, through ctx_build_map_trees) once per call, and the same build
// sorts the source, moved by the guess, along the same curve. A rigid motion keeps neighbours neighbours, so 64 consecutive source points stay one blob over all
// iterations: one wavefront walks the target's tree once for its 64 queries (ballot-driven descent, node boxes and leaves through wave-uniform fetches, as
// knn_packet.hpp's walk) with ONE best key per lane, (d2, index) packed so that an integer minimum is the nearest point with the smallest index. The search starts
// at the correspondence cap, so a source point beyond it leaves the tree at the root. The same kernel forms the 17 fp64 sums of the kept pairs and reduces them per
// workgroup; sum_rows_segmented (dev_rows.hpp) adds the workgroups' rows in a fixed order into pinned host memory (one 136-byte read-back per iteration, the precedent of scan2map.hip).
// The 3 x 3 SVD and the convergence tests run on the host in double; the float increment goes into a 56-byte control record in pinned host memory, which the next
// launch reads in place and applies to the resident source when it loads a point: no transform launch, no copy. The tree and the walk live in a registration context (its stream, its builder); the scratch
// hangs off that context, only grows and is freed with it.
//
// ONE loop serves one source and many (loop_align_batch; rolo_loopicp_align_batch is the ground prior's association, performPriorAssociation :1943-2158, one ICP
// per stored patch near the current key pose, all against the same ground patch): patch-sized clouds leave most of the device idle and would pay the
// per-iteration launches and the host exchange once per candidate and iteration. Every candidate owns whole workgroups of one `cur`, ONE launch of
// icp_assoc_batch_kernel per iteration serves all of them, sum_rows_segmented adds each candidate's rows, and the host waits once per iteration for the batch and
// runs loop_host_step per candidate. A candidate's bits depend on its own source, the target and the settings alone; the single entry points (loop_align:
// rolo_loopicp_align, rolo_keymap_loop_icp) are a batch of one, and rolo_loopicp_associate is one launch of it with the per-point outputs switched on.
#include "keymap.hpp"
#include "knn_packet.hpp"
#include "dev_rows.hpp"
#include <cfloat>
#include <climits>
#include <cstddef>
#include <cmath>
#include <cstring>
#include <vector>

namespace rolo {
namespace {

constexpr int ICP_THREADS = 256;
constexpr int ICP_NV = 17;   // n, sum d2, sum p (3), sum q (3), sum p q^T (9, row = p, column = q)

ROLO_DEV unsigned long long icp_key(float d2, int idx) { return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)idx; }

// one wavefront's walk of the target's tree for its 64 queries: the best key per lane, started at the cap
ROLO_DEV unsigned long long icp_walk(const float4* __restrict__ sorted, const float4* __restrict__ boxes, int P, int n_leaves, float4 q, bool active, float cap2, lds_int* stk) {
  // a real candidate's index is below INT_MAX: a pair at exactly the cap sorts below this key and is kept; an idle lane accepts nothing
  unsigned long long best = active ? icp_key(cap2, INT_MAX) : 0ull;
  float bd = active ? cap2 : -1.0f;
  int sp = 0, h = 1;
  while (true) {   // (no store ahead of or inside this loop: the node and leaf fetches stay scalar, knn_packet.hpp's clobber rule)
    h = __builtin_amdgcn_readfirstlane(h);
    if (h < P) {
      float4 llo, lhi, rlo, rhi;
      sload_node(boxes + 4 * (size_t)h, llo, lhi, rlo, rhi);
      const box_f2 bd2 = box_d2_pair(llo, lhi, rlo, rhi, q);
      const float bl = bd2[0], br = bd2[1];
      const bool okl = (bl <= bd) && (bl < INFINITY), okr = (br <= bd) && (br < INFINITY);   // "<=": an equal distance may hide a smaller index
      const unsigned long long ml = __ballot(okl), mr = __ballot(okr);
      if (ml != 0ull && mr != 0ull) {
        const unsigned long long pref = __ballot((okl || okr) && (bl <= br));
        const bool left_first = 2 * __popcll(pref) >= __popcll(ml | mr);
        if (sp < WALK_STACK) { stk[sp] = left_first ? 2 * h + 1 : 2 * h; sp++; }
        h = left_first ? 2 * h : 2 * h + 1;
        continue;
      }
      if (ml != 0ull) { h = 2 * h; continue; }
      if (mr != 0ull) { h = 2 * h + 1; continue; }
    } else if (h - P < n_leaves) {
      float4 pts[KNN_LEAF];
      sload_leaf(sorted + KNN_LEAF * (size_t)(h - P), pts);
#pragma unroll
      for (int u = 0; u < KNN_LEAF; u++) {
        const float4 c = pts[u];
        const float dx = q.x - c.x, dy = q.y - c.y, dz = q.z - c.z;
        const float cd = ((dx * dx) + (dy * dy)) + (dz * dz);   // (-ffp-contract=off)
        const unsigned long long ck = icp_key(cd, __float_as_int(c.w));   // (a padding point: +infinity, INT_MAX — never below the start key)
        best = ck < best ? ck : best;
      }
      bd = active ? __uint_as_float((unsigned)(best >> 32)) : -1.0f;
    }
    if (sp == 0) break;
    sp--;
    h = stk[sp];
  }
  return best;
}

// the 17 terms of one lane's pair (zeros when it kept none)
ROLO_DEV void icp_pair_terms(bool kept, float4 qs, float d2, int ti, const float4* __restrict__ txyz, double* acc) {
#pragma unroll
  for (int v = 0; v < ICP_NV; v++) acc[v] = 0.0;
  if (kept) {
    const float4 t = txyz[ti];
    const double p[3] = {(double)qs.x, (double)qs.y, (double)qs.z}, qq[3] = {(double)t.x, (double)t.y, (double)t.z};
    acc[0] = 1.0; acc[1] = (double)d2;
#pragma unroll
    for (int r = 0; r < 3; r++) {
      acc[2 + r] = p[r]; acc[5 + r] = qq[r];
#pragma unroll
      for (int c = 0; c < 3; c++) acc[8 + 3 * r + c] = p[r] * qq[c];
    }
  }
}

// workgroup sum, fixed order, into this workgroup's row
ROLO_DEV void icp_block_row(const double* acc, double (*red)[ICP_NV], int wv, int lane, double* __restrict__ row) {
#pragma unroll
  for (int v = 0; v < ICP_NV; v++) {
    double x = acc[v];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    if (lane == 0) red[wv][v] = x;
  }
  __syncthreads();
  if (threadIdx.x < ICP_NV) {
    double s = 0;
#pragma unroll
    for (int w = 0; w < ICP_THREADS / 64; w++) s += red[w][threadIdx.x];
    row[threadIdx.x] = s;
  }
}

// ---- B sources against one target, every candidate's association in ONE launch per iteration ---------------------------------------------------------
// Candidate b owns the workgroups [seg[b].x, seg[b].x + seg[b].y) of `cur` (its source, moved by its guess and sorted along the target's curve, padded to whole
// workgroups with INT_MAX slots); a workgroup reads its candidate's control record, which the host rewrites between launches.
constexpr int ICP_MODE_ITERATE = 0, ICP_MODE_FITNESS = 1, ICP_MODE_IDLE = 2;   // the kernel treats ITERATE and FITNESS alike: they differ in cap2 and on the host
constexpr int ICP_MODE_MOVE = 4;                                              // bit: apply `inc` on load (absent in a candidate's first launch: the points stay as they are, signed zeros too)
struct IcpCtl { float inc[12]; float cap2; int mode; };
constexpr int ICP_CTL_WORDS = (int)(sizeof(IcpCtl) / sizeof(int)), ICP_CTL_MODE_WORD = 13;
static_assert(sizeof(IcpCtl) == 56 && offsetof(IcpCtl, mode) == 4 * ICP_CTL_MODE_WORD, "control record layout");

struct IcpBatchArgs {
  float4* cur;             // all candidates' segments: x, y, z, bits(index in the caller's order); padding: index INT_MAX
  const int* blk_cand;     // workgroup -> candidate
  const IcpCtl* ctl;       // per candidate, in pinned host memory
  const float4* tsorted;
  const float4* tboxes;
  const float4* txyz;
  int P, n_leaves;
  double* partials;        // grid x ICP_NV
  int32_t* idx_out;        // rolo_loopicp_associate: per point of ONE candidate in the caller's order; nullptr otherwise
  float* d2_out;
};

__global__ __launch_bounds__(ICP_THREADS) void icp_assoc_batch_kernel(IcpBatchArgs A) {
  __shared__ int stk_[ICP_THREADS / 64][WALK_STACK];
  __shared__ double red[ICP_THREADS / 64][ICP_NV];
  const int b = A.blk_cand[blockIdx.x];
  const IcpCtl* __restrict__ ctl = A.ctl + b;
  const int mode = ctl->mode;
  if ((mode & 3) == ICP_MODE_IDLE) return;   // (workgroup-uniform)
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const size_t j = (size_t)blockIdx.x * ICP_THREADS + threadIdx.x;   // (segments are whole workgroups: always inside `cur`)
  float4 qs = A.cur[j];
  const int qidx = __float_as_int(qs.w);
  const bool active = qidx != INT_MAX;
  if (mode & ICP_MODE_MOVE) {   // the increment of the previous iteration
    float T[12];
#pragma unroll
    for (int i = 0; i < 12; i++) T[i] = ctl->inc[i];
    const float4 m = transform12(T, qs);
    if (active) qs = m;
  }
  const float4 q = make_float4(active ? qs.x : 0.f, active ? qs.y : 0.f, active ? qs.z : 0.f, 0.f);
  const unsigned long long best = icp_walk(A.tsorted, A.tboxes, A.P, A.n_leaves, q, active, ctl->cap2, (lds_int*)&stk_[wv][0]);
  if (active && (mode & ICP_MODE_MOVE)) A.cur[j] = qs;   // (after the walk: the clobber rule)
  const int ti = (int)(unsigned)(best & 0xffffffffull);
  const bool kept = active && ti != INT_MAX;
  const float d2 = __uint_as_float((unsigned)(best >> 32));
  double acc[ICP_NV];
  icp_pair_terms(kept, qs, d2, ti, A.txyz, acc);
  if (active && A.idx_out) { A.idx_out[qidx] = kept ? ti : -1; A.d2_out[qidx] = kept ? d2 : INFINITY; }
  icp_block_row(acc, red, wv, lane, A.partials + (size_t)blockIdx.x * ICP_NV);
}

// candidate b's sorted source into its segment of `cur`, one workgroup of this launch per workgroup of the segment; the slots behind the source become
// padding. The launch writes the candidate's entries of the two tables too: no table travels from the host.
__global__ __launch_bounds__(ICP_THREADS) void icp_segment_kernel(const float4* __restrict__ sorted, int n_sorted, float4* __restrict__ cur, int2 sg, int b,
                                                                  int* __restrict__ blk_cand, int2* __restrict__ seg) {
  const int i = blockIdx.x * ICP_THREADS + threadIdx.x;   // (gridDim.x = sg.y)
  cur[(size_t)sg.x * ICP_THREADS + i] = i < n_sorted ? sorted[i] : make_float4(0.f, 0.f, 0.f, __int_as_float(INT_MAX));
  if (threadIdx.x == 0) { blk_cand[sg.x + blockIdx.x] = b; if (blockIdx.x == 0) seg[b] = sg; }
}

struct Rows12 { float T[12]; };
// out = T * in (transform12): the guess, ahead of the sort
__global__ __launch_bounds__(256) void icp_transform_kernel(const float4* in, float4* out, int n, Rows12 R) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out[i] = transform12(R.T, in[i]);
}

// ---- host: Umeyama without scaling, in double ------------------------------------------------------------------------------------------------
inline double det3(const double* M) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// A = U diag(S) V^T of a 3 x 3 matrix (row-major), singular values descending, U and V orthogonal whatever A's rank: one-sided Jacobi on the columns of A; U's first
// column is the largest column normalised, the second the next one made orthogonal to it, the third their cross product with the sign of the third column
void svd3(const double* Ain, double* U, double* S, double* V) {
  double A[9], Vv[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  std::memcpy(A, Ain, sizeof(A));
  for (int sweep = 0; sweep < 60; sweep++) {
    bool rotated = false;
    for (int p = 0; p < 2; p++)
      for (int q = p + 1; q < 3; q++) {
        double a = 0, b = 0, g = 0;
        for (int r = 0; r < 3; r++) { a += A[3 * r + p] * A[3 * r + p]; b += A[3 * r + q] * A[3 * r + q]; g += A[3 * r + p] * A[3 * r + q]; }
        if (g == 0.0 || std::fabs(g) <= 1e-17 * std::sqrt(a * b)) continue;
        rotated = true;
        const double zeta = (b - a) / (2.0 * g);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
        for (int r = 0; r < 3; r++) {
          const double x = A[3 * r + p], y = A[3 * r + q];
          A[3 * r + p] = c * x - s * y; A[3 * r + q] = s * x + c * y;
          const double vx = Vv[3 * r + p], vy = Vv[3 * r + q];
          Vv[3 * r + p] = c * vx - s * vy; Vv[3 * r + q] = s * vx + c * vy;
        }
      }
    if (!rotated) break;
  }
  double nrm[3]; int ord[3] = {0, 1, 2};
  for (int k = 0; k < 3; k++) nrm[k] = std::sqrt(A[k] * A[k] + A[3 + k] * A[3 + k] + A[6 + k] * A[6 + k]);
  for (int a = 0; a < 2; a++) for (int b = a + 1; b < 3; b++) if (nrm[ord[b]] > nrm[ord[a]]) std::swap(ord[a], ord[b]);
  double col[3][3];
  for (int k = 0; k < 3; k++) { S[k] = nrm[ord[k]]; for (int r = 0; r < 3; r++) { col[k][r] = A[3 * r + ord[k]]; V[3 * r + k] = Vv[3 * r + ord[k]]; } }
  double u[3][3];
  auto unit_perp = [](const double* a, double* o) {   // a unit vector orthogonal to the unit vector a
    const int k = std::fabs(a[0]) <= std::fabs(a[1]) && std::fabs(a[0]) <= std::fabs(a[2]) ? 0 : (std::fabs(a[1]) <= std::fabs(a[2]) ? 1 : 2);
    double e[3] = {0, 0, 0}; e[k] = 1.0;
    const double d = a[k];
    double n = 0;
    for (int r = 0; r < 3; r++) { o[r] = e[r] - d * a[r]; n += o[r] * o[r]; }
    n = std::sqrt(n);
    for (int r = 0; r < 3; r++) o[r] /= n;
  };
  if (S[0] > 0) for (int r = 0; r < 3; r++) u[0][r] = col[0][r] / S[0]; else { u[0][0] = 1; u[0][1] = 0; u[0][2] = 0; }
  {
    double d = 0, w[3], n = 0;
    for (int r = 0; r < 3; r++) d += col[1][r] * u[0][r];
    for (int r = 0; r < 3; r++) { w[r] = col[1][r] - d * u[0][r]; n += w[r] * w[r]; }
    n = std::sqrt(n);
    if (n > 1e-14 * S[0] && n > 0) for (int r = 0; r < 3; r++) u[1][r] = w[r] / n; else unit_perp(u[0], u[1]);
  }
  u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1]; u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2]; u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
  if (u[2][0] * col[2][0] + u[2][1] * col[2][1] + u[2][2] * col[2][2] < 0) for (int r = 0; r < 3; r++) u[2][r] = -u[2][r];
  for (int k = 0; k < 3; k++) for (int r = 0; r < 3; r++) U[3 * r + k] = u[k][r];
}

// the 17 sums -> R (row-major) and t with q ~ R p + t
void umeyama(const double* h, double* R, double* t) {
  const double n = h[0];
  double mp[3], mq[3], Sg[9], U[9], S[3], V[9];
  for (int r = 0; r < 3; r++) { mp[r] = h[2 + r] / n; mq[r] = h[5 + r] / n; }
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Sg[3 * r + c] = h[8 + 3 * c + r] / n - mq[r] * mp[c];   // row = q, column = p
  svd3(Sg, U, S, V);
  const double s = det3(U) * det3(V) < 0 ? -1.0 : 1.0;
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) R[3 * r + c] = U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1] + s * U[3 * r + 2] * V[3 * c + 2];
  for (int r = 0; r < 3; r++) t[r] = mq[r] - (R[3 * r] * mp[0] + R[3 * r + 1] * mp[1] + R[3 * r + 2] * mp[2]);
}

inline float cap2_float(double max_dist) {   // the largest float f with (double)f <= max_dist^2: "(double)d2 <= max_dist^2" as a float comparison
  const double c2 = max_dist * max_dist;
  if (!(c2 < (double)FLT_MAX)) return INFINITY;
  float f = (float)c2;
  if ((double)f > c2) f = std::nextafterf(f, 0.f);
  return f;
}

struct LoopIcp {
  float4 *src = nullptr, *tgt = nullptr, *srcg = nullptr, *cur = nullptr; size_t src_cap = 0, tgt_cap = 0, srcg_cap = 0, cur_cap = 0;   // src: the (concatenated) sources in the caller's order
  double* part = nullptr; size_t part_cap = 0;
  int32_t* idx = nullptr; size_t idx_cap = 0;
  float* d2 = nullptr; size_t d2_cap = 0;
  int* blk_cand = nullptr; size_t blk_cand_cap = 0;
  int2* seg = nullptr; size_t seg_cap = 0;           // (an empty candidate's entry is never written, nor read: it is IDLE from the start)
  IcpCtl* h_ctl = nullptr; size_t h_ctl_cap = 0;   // pinned: the control table, which the kernels read where it lies (no copy per launch); the host rewrites it
                                                   // only between a wait for the stream and the next launch
  double* h_sum = nullptr; size_t h_sum_cap = 0;   // pinned: B x 17 sums, written by sum_rows_segmented
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // start, set-up done, the single form's fitness pass begins, end
  DevStore store{nullptr, "loop ICP"};   // every buffer above (nothing is kept across a growth: no stream); freed with the context
  // per call kind: the last single alignment's (or association's) times and records, the last batch call's
  float ms[4] = {0.f, 0.f, 0.f, 0.f}, bms[4] = {0.f, 0.f, 0.f, 0.f};
  std::vector<std::vector<rolo_loopicp_trace_rec>> trace, btrace;   // (trace: no or one candidate)
};

int loop_state(rolo_ctx* c, LoopIcp** out) {
  LoopIcp* W = static_cast<LoopIcp*>(*ctx_loop_slot(c));
  if (!W) {
    W = new LoopIcp();
    *ctx_loop_slot(c) = W;
    HIPCHK(hipSetDevice(ctx_device(c)));
    for (int i = 0; i < 4; i++) HIPCHK(hipEventCreate(&W->ev[i]));
  }
  *out = W;
  return ROLO_OK;
}

bool is_identity16(const float* T) {
  for (int i = 0; i < 16; i++) if (T[i] != ((i % 5 == 0) ? 1.f : 0.f)) return false;
  return true;
}

// the target's tree (pair->c[0]) and the source, moved by T16, sorted along the same curve (pair->c[1]); d_src / d_tgt: device clouds of float4
int loop_sorted(rolo_ctx* c, LoopIcp* W, const float4* d_src, int ns, const float4* d_tgt, int nt, const float* T16, KnnPair* pair) {
  hipStream_t s = ctx_stream(c);
  int rc;
  const float4* moved = d_src;
  if (T16 && !is_identity16(T16)) {
    if ((rc = W->store.grow(W->srcg, W->srcg_cap, (size_t)ns))) return rc;
    Rows12 R; std::memcpy(R.T, T16, sizeof(R.T));
    icp_transform_kernel<<<(ns + 255) / 256, 256, 0, s>>>(d_src, W->srcg, ns, R);
    HIPCHK(hipGetLastError());
    moved = W->srcg;
  }
  *pair = KnnPair{};
  return ctx_build_map_trees(c, reinterpret_cast<const float*>(d_tgt), nt, reinterpret_cast<const float*>(moved), ns, 4, pair, true);
}

void matmul4f(const float* a, const float* b, float* o) {   // o = a b, each entry a0 b0 + a1 b1 + a2 b2 + a3 b3 left to right
  float r[16];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      float x = a[4 * i] * b[j];
      for (int k = 1; k < 4; k++) x = x + a[4 * i + k] * b[4 * k + j];
      r[4 * i + j] = x;
    }
  std::memcpy(o, r, sizeof(r));
}

// The host's share of one iteration, from the 17 sums of its association: the trace record, the increment (have_inc: the source is to be moved by it), the pose
// and the exit tests in pcl's order. True when the alignment has ended (res.state says how).
bool loop_host_step(const double* h, const rolo_loopicp_params* P, double rot_thr, rolo_loopicp_result& res, double& prev, std::vector<rolo_loopicp_trace_rec>& trace,
                    float* inc /* 16 */, bool* have_inc) {
  *have_inc = false;
  rolo_loopicp_trace_rec tr{};
  const int n = (int)(h[0] + 0.5);
  tr.n = n; tr.mse = n > 0 ? h[1] / n : 0.0;
  std::memcpy(tr.sums, h, sizeof(tr.sums));
  res.n_last = n;
  if (n < P->min_correspondences || n < 1) { trace.push_back(tr); res.state = ROLO_ICP_NO_CORRESPONDENCES; res.converged = 0; return true; }
  double R[9], t[3];
  umeyama(h, R, t);
  const float incv[16] = {(float)R[0], (float)R[1], (float)R[2], (float)t[0], (float)R[3], (float)R[4], (float)R[5], (float)t[1],
                          (float)R[6], (float)R[7], (float)R[8], (float)t[2], 0.f, 0.f, 0.f, 1.f};
  std::memcpy(inc, incv, sizeof(incv));
  std::memcpy(tr.increment, inc, sizeof(incv));
  trace.push_back(tr);
  *have_inc = true;
  matmul4f(inc, res.T, res.T);
  res.iterations++;
  const double cosa = 0.5 * ((double)inc[0] + (double)inc[5] + (double)inc[10] - 1.0);
  const double tsq = (double)inc[3] * (double)inc[3] + (double)inc[7] * (double)inc[7] + (double)inc[11] * (double)inc[11];
  const double mse = tr.mse;
  if (res.iterations >= P->max_iterations) { res.state = ROLO_ICP_ITERATIONS; res.converged = 1; return true; }
  if (cosa >= rot_thr && tsq <= P->transformation_epsilon) { res.state = ROLO_ICP_TRANSFORM; res.converged = 1; return true; }
  if (mse < 1e-12) { res.state = ROLO_ICP_ABS_MSE; res.converged = 1; return true; }
  if (std::fabs(mse - prev) / prev < P->euclidean_fitness_epsilon) { res.state = ROLO_ICP_REL_MSE; res.converged = 1; return true; }
  prev = mse;
  return false;
}

// getFitnessScore() from the sums of the association without a cap
void loop_host_fitness(const double* h, rolo_loopicp_result& res, std::vector<rolo_loopicp_trace_rec>& trace) {
  rolo_loopicp_trace_rec tr{};
  tr.n = (int)(h[0] + 0.5); tr.mse = tr.n > 0 ? h[1] / tr.n : 0.0;
  std::memcpy(tr.sums, h, sizeof(tr.sums));
  trace.push_back(tr);
  res.fitness = tr.n > 0 ? tr.mse : DBL_MAX;
}

int loop_upload(rolo_ctx* c, LoopIcp* W, const float* src, long long ns, const float* tgt, int nt) {
  int rc;
  if ((rc = W->store.grow(W->src, W->src_cap, (size_t)std::max(ns, 1ll)))) return rc;
  if ((rc = W->store.grow(W->tgt, W->tgt_cap, (size_t)std::max(nt, 1)))) return rc;
  hipStream_t s = ctx_stream(c);
  if (ns > 0) HIPCHK(hipMemcpyAsync(W->src, src, sizeof(float4) * (size_t)ns, hipMemcpyHostToDevice, s));
  if (nt > 0) HIPCHK(hipMemcpyAsync(W->tgt, tgt, sizeof(float4) * (size_t)nt, hipMemcpyHostToDevice, s));
  return ROLO_OK;
}

// Set-up for B sources (concatenated at d_srcs, ns[b] points each) against one target: every live candidate's segment of W->cur (the builder's sort, once per
// candidate; the target's tree of the last build serves all, a tree's shape never changes an association's result), the tables, and the control records in
// ITERATE mode at cap2. *n_live = 0 (an empty target, or no source with a point): nothing was touched on the device.
int loop_segments(rolo_ctx* c, LoopIcp* W, const float4* d_srcs, const int* ns, int B, const float4* d_tgt, int nt, const float* guess16, float cap2, IcpBatchArgs* A,
                  int* total_blocks_out, int* n_live_out) {
  hipStream_t s = ctx_stream(c);
  int rc, total_blocks = 0, n_live = 0;
  std::vector<int2> seg((size_t)B);
  for (int b = 0; b < B; b++) {
    const bool live = ns[b] > 0 && nt > 0;
    const int n_sorted = live ? KNN_LEAF * ((ns[b] + KNN_LEAF - 1) / KNN_LEAF) : 0;   // (the builder's: KnnCloud::n_sorted)
    seg[b] = make_int2(total_blocks, (n_sorted + ICP_THREADS - 1) / ICP_THREADS);
    total_blocks += seg[b].y;
    n_live += live ? 1 : 0;
  }
  *total_blocks_out = total_blocks; *n_live_out = n_live;
  if (n_live == 0) return ROLO_OK;
  HIPCHK(hipEventRecord(W->ev[0], s));
  if ((rc = W->store.grow(W->cur, W->cur_cap, (size_t)total_blocks * ICP_THREADS))) return rc;
  if ((rc = W->store.grow(W->part, W->part_cap, (size_t)total_blocks * ICP_NV))) return rc;
  if ((rc = W->store.grow(W->blk_cand, W->blk_cand_cap, (size_t)total_blocks))) return rc;
  if ((rc = W->store.grow(W->seg, W->seg_cap, (size_t)B))) return rc;
  if ((rc = W->store.grow_pinned(W->h_ctl, W->h_ctl_cap, (size_t)B, 16))) return rc;
  if ((rc = W->store.grow_pinned(W->h_sum, W->h_sum_cap, (size_t)B * ICP_NV, 16 * ICP_NV))) return rc;
  *A = IcpBatchArgs{};
  size_t off = 0;
  for (int b = 0; b < B; b++) {
    if (seg[b].y > 0) {
      KnnPair pair{};
      if ((rc = loop_sorted(c, W, d_srcs + off, ns[b], d_tgt, nt, guess16 ? guess16 + 16 * (size_t)b : nullptr, &pair))) return rc;
      if (pair.c[1].n_sorted > seg[b].y * ICP_THREADS) { ctx_set_error("loop ICP: the builder's sorted size is not the expected one"); return ROLO_ESTATE; }
      icp_segment_kernel<<<seg[b].y, ICP_THREADS, 0, s>>>(pair.c[1].sorted, pair.c[1].n_sorted, W->cur, seg[b], b, W->blk_cand, W->seg);
      HIPCHK(hipGetLastError());
      A->tsorted = pair.c[0].sorted; A->tboxes = pair.c[0].boxes; A->txyz = pair.c[0].xyz; A->P = pair.c[0].P; A->n_leaves = pair.c[0].n_leaves;
    }
    off += (size_t)ns[b];
  }
  A->cur = W->cur; A->blk_cand = W->blk_cand; A->ctl = W->h_ctl; A->partials = W->part;
  for (int b = 0; b < B; b++) {
    IcpCtl& k = W->h_ctl[b];
    std::memset(&k, 0, sizeof(k));
    k.cap2 = cap2;
    k.mode = seg[b].y > 0 ? ICP_MODE_ITERATE : ICP_MODE_IDLE;
  }
  return ROLO_OK;
}

// one launch for all candidates as W->h_ctl stands, every live candidate's 17 sums in W->h_sum when this returns
int loop_associate(rolo_ctx* c, LoopIcp* W, const IcpBatchArgs& A, int total_blocks, int B) {
  hipStream_t s = ctx_stream(c);
  icp_assoc_batch_kernel<<<total_blocks, ICP_THREADS, 0, s>>>(A);
  HIPCHK(hipGetLastError());
  sum_rows_segmented<ICP_NV><<<B, 256, 0, s>>>(W->part, W->seg, reinterpret_cast<const int*>(A.ctl) + ICP_CTL_MODE_WORD, ICP_CTL_WORDS, ICP_MODE_IDLE, W->h_sum);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s));
  return ROLO_OK;
}

// The ICP of B sources against one target, with every candidate's association in one launch per iteration and one exchange with the host per iteration for all
// of them. Candidate b's results depend on nothing but its own source, the target, the settings and its guess: its sorted order and 256-point workgroups are its
// own, its rows are added in a fixed order, and the host step is per candidate. traces[b] takes candidate b's records; ms4: set-up, iterations, the fitness pass
// when split_fitness (B == 1: the host knows the launch at which the one candidate turns FITNESS) and 0 otherwise (then the iterations carry the fitness
// passes), the whole call.
int loop_align_batch(rolo_ctx* c, LoopIcp* W, const float4* d_srcs, const int* ns, int B, const float4* d_tgt, int nt, const rolo_loopicp_params* P, const float* guess16,
                     rolo_loopicp_result* out, std::vector<std::vector<rolo_loopicp_trace_rec>>& traces, float* ms4, bool split_fitness) {
  if (!(P->max_correspondence_distance >= 0.0) || P->max_iterations < 0) { ctx_set_error("loop ICP: bad parameters"); return ROLO_EINVAL; }
  int rc;
  HIPCHK(hipSetDevice(ctx_device(c)));
  hipStream_t s = ctx_stream(c);
  traces.assign((size_t)B, {});
  for (int i = 0; i < 4; i++) ms4[i] = 0.f;
  std::vector<double> prev((size_t)B, DBL_MAX);
  for (int b = 0; b < B; b++) {
    rolo_loopicp_result& res = out[b];
    res = rolo_loopicp_result{};
    for (int i = 0; i < 16; i++) res.T[i] = guess16 ? guess16[16 * (size_t)b + i] : ((i % 5 == 0) ? 1.f : 0.f);
    res.n_source = ns[b]; res.n_target = nt; res.fitness = DBL_MAX;
    res.state = ns[b] > 0 && nt > 0 ? ROLO_ICP_NOT_CONVERGED : ROLO_ICP_NO_CORRESPONDENCES;
  }
  IcpBatchArgs A{};
  int total_blocks = 0, n_live = 0;
  if ((rc = loop_segments(c, W, d_srcs, ns, B, d_tgt, nt, guess16, cap2_float(P->max_correspondence_distance), &A, &total_blocks, &n_live))) return rc;
  if (n_live == 0) return ROLO_OK;
  HIPCHK(hipEventRecord(W->ev[1], s));
  const double rot_thr = P->rotation_epsilon > 0 ? P->rotation_epsilon : 1.0 - P->transformation_epsilon;
  while (n_live > 0) {
    if ((rc = loop_associate(c, W, A, total_blocks, B))) return rc;
    for (int b = 0; b < B; b++) {
      IcpCtl& k = W->h_ctl[b];
      if (k.mode == ICP_MODE_IDLE) continue;
      const double* h = W->h_sum + (size_t)b * ICP_NV;
      if ((k.mode & 3) == ICP_MODE_FITNESS) {   // getFitnessScore(): the moved source as it stood, no cap
        loop_host_fitness(h, out[b], traces[b]);
        k.mode = ICP_MODE_IDLE;
        n_live--;
        continue;
      }
      float inc[16];
      bool have_inc = false;
      const bool done = loop_host_step(h, P, rot_thr, out[b], prev[b], traces[b], inc, &have_inc);
      if (have_inc) std::memcpy(k.inc, inc, sizeof(k.inc));
      k.mode = (done ? ICP_MODE_FITNESS : ICP_MODE_ITERATE) | (have_inc ? ICP_MODE_MOVE : 0);   // the next launch applies the increment on load
      if (done) k.cap2 = INFINITY;
      if (done && split_fitness) HIPCHK(hipEventRecord(W->ev[2], s));
    }
  }
  HIPCHK(hipEventRecord(W->ev[3], s));
  HIPCHK(hipEventSynchronize(W->ev[3]));
  (void)hipEventElapsedTime(&ms4[0], W->ev[0], W->ev[1]);
  (void)hipEventElapsedTime(&ms4[1], W->ev[1], split_fitness ? W->ev[2] : W->ev[3]);
  if (split_fitness) (void)hipEventElapsedTime(&ms4[2], W->ev[2], W->ev[3]);
  (void)hipEventElapsedTime(&ms4[3], W->ev[0], W->ev[3]);
  return ROLO_OK;
}

// one source: a batch of one, its records and times kept apart from the batch calls'
int loop_align(rolo_ctx* c, const float4* d_src, int ns, const float4* d_tgt, int nt, const rolo_loopicp_params* P, const float* guess16, rolo_loopicp_result* out) {
  LoopIcp* W = nullptr;
  int rc = loop_state(c, &W);
  if (rc) return rc;
  rolo_loopicp_result res{};
  if ((rc = loop_align_batch(c, W, d_src, &ns, 1, d_tgt, nt, P, guess16, &res, W->trace, W->ms, true))) return rc;
  *out = res;
  return ROLO_OK;
}

int copy_records(const std::vector<rolo_loopicp_trace_rec>& t, rolo_loopicp_trace_rec* out, int cap) {
  for (int i = 0; i < std::min((int)t.size(), cap); i++) out[i] = t[i];
  return (int)t.size();
}
int copy_trace(rolo_ctx* c, rolo_loopicp_trace_rec* out, int cap) {   // the last single alignment's or association's
  LoopIcp* W = static_cast<LoopIcp*>(*ctx_loop_slot(c));
  return !W || W->trace.empty() ? 0 : copy_records(W->trace[0], out, cap);
}

}  // namespace
}  // namespace rolo

using namespace rolo;

extern "C" {

void rolo_loopicp_destroy(rolo_ctx* c) {   // called by rolo_ctx_destroy
  LoopIcp* W = static_cast<LoopIcp*>(*ctx_loop_slot(c));
  if (!W) return;
  (void)hipSetDevice(ctx_device(c));
  (void)hipStreamSynchronize(ctx_stream(c));
  W->store.release();
  for (hipEvent_t e : W->ev) if (e) (void)hipEventDestroy(e);
  delete W;
  *ctx_loop_slot(c) = nullptr;
}

void rolo_loopicp_default_params(rolo_loopicp_params* p) {
  if (!p) return;
  p->max_iterations = 100;
  p->transformation_epsilon = 1e-6;
  p->euclidean_fitness_epsilon = 1e-6;
  p->rotation_epsilon = 0.0;
  p->max_correspondence_distance = INFINITY;
  p->min_correspondences = 3;
}

int rolo_loopicp_align(rolo_ctx* c, const float* source, int n_source, const float* target, int n_target, const rolo_loopicp_params* params, const float* guess16,
                       rolo_loopicp_result* out) {
  if (!c || !params || !out || n_source < 0 || n_target < 0 || (n_source && !source) || (n_target && !target) || n_source > ROLO_KEYMAP_MAX_POINTS ||
      n_target > ROLO_KEYMAP_MAX_POINTS)
    return ROLO_EINVAL;
  LoopIcp* W = nullptr;
  int rc = loop_state(c, &W);
  if (rc) return rc;
  HIPCHK(hipSetDevice(ctx_device(c)));
  if ((rc = loop_upload(c, W, source, n_source, target, n_target))) return rc;
  rc = loop_align(c, W->src, n_source, W->tgt, n_target, params, guess16, out);
  if (rc) (void)hipStreamSynchronize(ctx_stream(c));   // the caller's arrays are free again, whatever happened
  return rc;
}

int rolo_keymap_loop_icp(rolo_keymap* km, const rolo_loopicp_params* params, const float* guess16, rolo_loopicp_result* out) {
  if (!km || !params || !out) return ROLO_EINVAL;
  if (!km->have_loop[0] || !km->have_loop[1]) { ctx_set_error("rolo_keymap_loop_icp: build both loop clouds first (rolo_keymap_loop_cloud, slots 0 and 1)"); return ROLO_ESTATE; }
  if (!km->loop_ctx) { const int rc = rolo_ctx_acquire(km->device, &km->loop_ctx); if (rc) return rc; }
  // (rolo_keymap_loop_cloud waited for the key map's stream before it returned: the clouds are complete, and this call waits for the context's stream before it returns)
  return loop_align(km->loop_ctx, km->loop[0], km->m_loop[0], km->loop[1], km->m_loop[1], params, guess16, out);
}

int rolo_loopicp_get_trace(rolo_ctx* c, rolo_loopicp_trace_rec* out, int cap) {
  if (!c || cap < 0 || (cap && !out)) return ROLO_EINVAL;
  return copy_trace(c, out, cap);
}

int rolo_loopicp_align_batch(rolo_ctx* c, const float* sources, const int* n_source, int B, const float* target, int n_target, const rolo_loopicp_params* params,
                             const float* guess16, rolo_loopicp_result* out) {
  if (!c || !params || B < 0 || B > ROLO_LOOPICP_MAX_BATCH || n_target < 0 || (n_target && !target) || n_target > ROLO_KEYMAP_MAX_POINTS) return ROLO_EINVAL;
  if (B == 0) return ROLO_OK;
  if (!n_source || !out) return ROLO_EINVAL;
  long long total = 0;
  for (int b = 0; b < B; b++) {
    if (n_source[b] < 0) return ROLO_EINVAL;
    total += n_source[b];
  }
  if (total > ROLO_KEYMAP_MAX_POINTS || (total && !sources)) return ROLO_EINVAL;
  LoopIcp* W = nullptr;
  int rc = loop_state(c, &W);
  if (rc) return rc;
  HIPCHK(hipSetDevice(ctx_device(c)));
  if ((rc = loop_upload(c, W, sources, total, target, n_target))) return rc;
  rc = loop_align_batch(c, W, W->src, n_source, B, W->tgt, n_target, params, guess16, out, W->btrace, W->bms, false);
  if (rc) (void)hipStreamSynchronize(ctx_stream(c));   // the caller's arrays are free again, whatever happened
  return rc;
}

int rolo_loopicp_get_trace_batch(rolo_ctx* c, int b, rolo_loopicp_trace_rec* out, int cap) {
  if (!c || b < 0 || cap < 0 || (cap && !out)) return ROLO_EINVAL;
  LoopIcp* W = static_cast<LoopIcp*>(*ctx_loop_slot(c));
  if (!W || b >= (int)W->btrace.size()) return ROLO_EINVAL;
  return copy_records(W->btrace[b], out, cap);
}

int rolo_loopicp_batch_last_ms(rolo_ctx* c, float* ms4) {
  if (!c || !ms4) return ROLO_EINVAL;
  LoopIcp* W = static_cast<LoopIcp*>(*ctx_loop_slot(c));
  for (int i = 0; i < 4; i++) ms4[i] = W ? W->bms[i] : 0.f;
  return ROLO_OK;
}

int rolo_keymap_loop_trace(rolo_keymap* km, rolo_loopicp_trace_rec* out, int cap) {
  if (!km || cap < 0 || (cap && !out)) return ROLO_EINVAL;
  return km->loop_ctx ? copy_trace(km->loop_ctx, out, cap) : 0;
}

int rolo_loopicp_associate(rolo_ctx* c, const float* source, int n_source, const float* target, int n_target, const float* T16, double max_correspondence_distance,
                           int32_t* index_out, float* d2_out) {
  if (!c || n_source <= 0 || n_target <= 0 || !source || !target || !index_out || !d2_out || !(max_correspondence_distance >= 0.0) ||
      n_source > ROLO_KEYMAP_MAX_POINTS || n_target > ROLO_KEYMAP_MAX_POINTS)
    return ROLO_EINVAL;
  LoopIcp* W = nullptr;
  int rc = loop_state(c, &W);
  if (rc) return rc;
  HIPCHK(hipSetDevice(ctx_device(c)));
  hipStream_t s = ctx_stream(c);
  if ((rc = loop_upload(c, W, source, n_source, target, n_target))) return rc;
  if ((rc = W->store.grow(W->idx, W->idx_cap, (size_t)n_source))) return rc;
  if ((rc = W->store.grow(W->d2, W->d2_cap, (size_t)n_source))) return rc;
  IcpBatchArgs A{};
  int total_blocks = 0, n_live = 0;
  W->trace.assign(1, {});
  rc = loop_segments(c, W, W->src, &n_source, 1, W->tgt, n_target, T16, cap2_float(max_correspondence_distance), &A, &total_blocks, &n_live);
  if (rc) { (void)hipStreamSynchronize(s); return rc; }
  A.idx_out = W->idx; A.d2_out = W->d2;
  if ((rc = loop_associate(c, W, A, total_blocks, 1))) return rc;
  rolo_loopicp_result unused{};
  loop_host_fitness(W->h_sum, unused, W->trace[0]);
  HIPCHK(hipMemcpyAsync(index_out, W->idx, sizeof(int32_t) * (size_t)n_source, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(d2_out, W->d2, sizeof(float) * (size_t)n_source, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return ROLO_OK;
}

int rolo_loopicp_last_ms(rolo_ctx* c, float* ms4) {
  if (!c || !ms4) return ROLO_EINVAL;
  LoopIcp* W = static_cast<LoopIcp*>(*ctx_loop_slot(c));
  for (int i = 0; i < 4; i++) ms4[i] = W ? W->ms[i] : 0.f;
  return ROLO_OK;
}

int rolo_keymap_loop_last_ms(rolo_keymap* km, float* ms6) {
  if (!km || !ms6) return ROLO_EINVAL;
  for (int i = 0; i < 4; i++) ms6[i] = 0.f;
  if (km->loop_ctx) rolo_loopicp_last_ms(km->loop_ctx, ms6);
  ms6[4] = km->loop_ms[0]; ms6[5] = km->loop_ms[1];
  return ROLO_OK;
}

}  // extern "C"
