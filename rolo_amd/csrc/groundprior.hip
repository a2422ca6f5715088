// The ground prior on gfx950: a resident ground cloud with nearest / radius queries in the x-y plane and the square patch cut (rolo_ground_*), and the batched
// terrain pose solver over it (rolo_priorpose_*). Replaces (reference) ground_factor::GroundModel and PoseSolver::Solve of src/prior_pose/pose_solver.cpp and what
// PriorPoseNode::HandlePose (prior_pose_node.cpp:164-233) makes of the result. include/rolo_hip.h states the arithmetic; tests/prior_twin.py restates it in numpy.
//
// The grid: points binned by (row, column) of a uniform x-y grid with the stable sort of (cell, point index) that the voxel filter uses (sort_dev.hpp), cells
// row-major, so the cells [c0, c1] of one row are ONE run of the sorted points. A query never trusts the grid for its answer: gp_cell is monotone in its
// argument, so every point whose float distance can pass the test lies in the cells between those of the padded interval's ends (gp_window).
//   gp_key_kernel / sort_* / gp_cell_start_kernel / gp_sorted_points_kernel     the build
//   gp_patch_kernel<0>, scan_excl_kernel, <1>                                   ExtractPatch: flags per workgroup, their scan, the ordered copy (+ transform)
//   gp_nearest_kernel, gp_radius_kernel, gp_fit_kernel                          the debug entry points, one workgroup per query, the solver's own device functions
//   gp_solve_kernel                                                             PoseSolver::Solve, one workgroup per pose
// A workgroup works through one query at a time: its lanes scan the window, hits go to LDS as packed (d2 bits, index) keys and are sorted there (by rank up to
// GP_THREADS keys, a bitonic network above), the neighbours' points are gathered in that order, and thread 0 runs the ordered fp64 sums while the others wait at
// the barrier. The solver's state lives in LDS and belongs to thread 0; every decision that bends the control flow goes through LDS and a barrier, so all lanes
// take every barrier. No workgroup waits for another; every loop is bounded by max_iters, the wheel count, the list size or the grid's side.
#include "ctx_access.hpp"
#include "dev_rows.hpp"
#include "sort_dev.hpp"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

struct rolo_ground {
  int device = 0;
  hipStream_t stream = nullptr;
  rolo::DevStore store;
  // the next build's grid settings
  float cell0 = 0.6f;
  int max_cells = ROLO_GROUND_MAX_CELLS;
  // the cloud
  bool have_cloud = false;
  int n = 0, stride = 0, nx = 0, ny = 0, doubled = 0;
  float minx = 0.f, miny = 0.f, cell = 0.f;
  float* rec = nullptr; size_t rec_cap = 0;          // the caller's records
  float4* pts = nullptr; size_t pts_cap = 0;         // x y z 0 in the caller's order
  float4* spts = nullptr; size_t spts_cap = 0;       // x y z (index bits), sorted by cell
  int* cell_start = nullptr; size_t cell_start_cap = 0;   // [cells + 1]
  rolo::SortScratch sort;                            // the sort of (cell, point index)
  float* box_part = nullptr; size_t box_part_cap = 0;
  unsigned* bcnt = nullptr; size_t bcnt_cap = 0;     // the patch's kept points per workgroup, then their scan
  float* patch = nullptr; size_t patch_cap = 0;
  float* h_box = nullptr;                            // pinned [8]
  int* h_m = nullptr; int* d_m = nullptr;            // the patch's size
  // queries
  double* d_q = nullptr; size_t d_q_cap = 0;         // staged queries / poses
  unsigned char* d_out = nullptr; size_t d_out_cap = 0;
  hipEvent_t ev[2] = {nullptr, nullptr};
  float ms[3] = {0.f, 0.f, 0.f};
};

namespace rolo {
namespace {

constexpr int GP_THREADS = 256;
constexpr int GP_CAP = ROLO_GROUND_MAX_NEIGHBOURS;
constexpr int GP_W = ROLO_PRIOR_MAX_WHEELS;
constexpr unsigned long long GP_NONE = ~0ull;

struct GpGrid { float minx, miny, inv; int nx, ny, n; const int* cell_start; const float4* spts; const float4* pts; };

// the solver's constants in the form the kernel reads them
struct GpParams {
  int n_wheels, max_iters, avg_min_nb, fit_min_pts;
  double wheel[GP_W][2], com_z, bl_t[3], bl_R[9];
  double k_spring, g, lambda0, tol_cost, tol_step;
  double avg_radius, avg_pad; float avg_r2;          // the search's (float)(r r) and the padded radius of its window
  double fit_pad, fit_thr; float fit_r2;
  double z_min, z_max, roll_max, pitch_max, dist_max;
};

struct GpWindow { int x0, x1, y0, y1; };

// ---- the grid -----------------------------------------------------------------------------------------------------------------------------------------------
// monotone (non-decreasing) in v for a fixed grid: float subtraction, a positive factor, floor and the clamp all are. A NaN lands in cell 0
ROLO_DEV int gp_cell(float v, float mn, float inv, int cells) { return (int)fminf(fmaxf(floorf((v - mn) * inv), 0.f), (float)(cells - 1)); }
ROLO_DEV float gp_down(double v) { float f = (float)v; if ((double)f > v) f = nextafterf(f, -INFINITY); return f; }
ROLO_DEV float gp_up(double v) { float f = (float)v; if ((double)f < v) f = nextafterf(f, INFINITY); return f; }
// the cells that can hold a point whose float d2 to (qx, qy) is at most the float square of a radius whose padded value (r (1 + 1e-5) + 1e-30) is pad: such a
// point's |x - qx| is below pad (three float roundings, each within 2^-24, lie between), so its x is inside [down(qx - pad), up(qx + pad)]
ROLO_DEV GpWindow gp_window(const GpGrid& G, float qx, float qy, double pad) {
  GpWindow w;
  w.x0 = gp_cell(gp_down((double)qx - pad), G.minx, G.inv, G.nx); w.x1 = gp_cell(gp_up((double)qx + pad), G.minx, G.inv, G.nx);
  w.y0 = gp_cell(gp_down((double)qy - pad), G.miny, G.inv, G.ny); w.y1 = gp_cell(gp_up((double)qy + pad), G.miny, G.inv, G.ny);
  return w;
}

__global__ __launch_bounds__(SM_THREADS) void gp_key_kernel(const float4* __restrict__ pts, int n, GpGrid G, unsigned* __restrict__ keys, int* __restrict__ vals) {
  const int i = blockIdx.x * SM_THREADS + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  keys[i] = (unsigned)gp_cell(p.y, G.miny, G.inv, G.ny) * (unsigned)G.nx + (unsigned)gp_cell(p.x, G.minx, G.inv, G.nx);
  vals[i] = i;
}
__global__ __launch_bounds__(SM_THREADS) void gp_cell_start_kernel(const unsigned* __restrict__ keys, int n, int cells, int* __restrict__ cell_start) {
  const int c = blockIdx.x * SM_THREADS + threadIdx.x;
  if (c <= cells) cell_start[c] = lower_bound_u32(keys, n, (unsigned)c);
}
__global__ __launch_bounds__(SM_THREADS) void gp_sorted_points_kernel(const float4* __restrict__ pts, const int* __restrict__ vals, int n, float4* __restrict__ spts) {
  const int j = blockIdx.x * SM_THREADS + threadIdx.x;
  if (j >= n) return;
  const int i = vals[j];
  const float4 p = pts[i];
  spts[j] = make_float4(p.x, p.y, p.z, __int_as_float(i));
}

// ---- ExtractPatch -------------------------------------------------------------------------------------------------------------------------------------------
struct GpPatch { float xlo, xhi, ylo, yhi; int has_T; float T[12]; };
// WRITE = 0: kept points per workgroup -> bcnt[block]; WRITE = 1 (bcnt scanned): the kept records to their places, in the caller's order
template <int WRITE>
__global__ __launch_bounds__(SM_THREADS) void gp_patch_kernel(const float* __restrict__ rec, int n, int stride, GpPatch P, unsigned* __restrict__ bcnt, float* __restrict__ out) {
  __shared__ unsigned wsum[SM_THREADS / 64];
  const int i = blockIdx.x * SM_THREADS + threadIdx.x;
  bool keep = false;
  float x = 0.f, y = 0.f, z = 0.f;
  if (i < n) {
    x = rec[(size_t)i * stride]; y = rec[(size_t)i * stride + 1]; z = rec[(size_t)i * stride + 2];
    keep = isfinite(x) && isfinite(y) && isfinite(z) && !(x < P.xlo || x > P.xhi) && !(y < P.ylo || y > P.yhi);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long b = __ballot(keep);
  if (lane == 0) wsum[wv] = (unsigned)__popcll(b);
  __syncthreads();
  unsigned before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < SM_THREADS / 64; w++) { const unsigned t = wsum[w]; if (w < wv) before += t; total += t; }
  if (!WRITE) { if (threadIdx.x == 0) bcnt[blockIdx.x] = total; return; }
  if (!keep) return;
  const size_t pos = (size_t)bcnt[blockIdx.x] + before + (unsigned)__popcll(b & ((1ull << lane) - 1ull));   // < the number kept, which the host has sized out for
  float* o = out + pos * stride;
  if (P.has_T) { const float4 t = transform12(P.T, make_float4(x, y, z, 0.f)); x = t.x; y = t.y; z = t.z; }
  o[0] = x; o[1] = y; o[2] = z;
  for (int k = 3; k < stride; k++) o[k] = rec[(size_t)i * stride + k];
}

// ---- one workgroup's query machinery ------------------------------------------------------------------------------------------------------------------------
struct GpLds {
  union {
    unsigned long long key[GP_CAP];    // packed (d2 bits, index)
    float2 xy[GP_CAP];                 // then, slot by slot, the neighbours' x y in list order (gp_radius's gather: a thread overwrites the key it has read)
  };
  float pz[GP_CAP];                    // and their z
  unsigned long long best;
  int cnt;
  int ctl;                             // thread 0's decision for all
};

ROLO_DEV unsigned long long gp_pack(float d2, int idx) { return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)idx; }
ROLO_DEV float gp_d2(float4 p, float qx, float qy) { const float dx = qx - p.x, dy = qy - p.y; return dx * dx + dy * dy; }   // no contraction (build.py)

ROLO_DEV unsigned long long gp_wave_min(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
  return v;
}

// the points of the cells [x0, x1] of row y against the running best
ROLO_DEV unsigned long long gp_scan_best(const GpGrid& G, int y, int x0, int x1, float qx, float qy, int first, int step, unsigned long long best) {
  const int s = G.cell_start[y * G.nx + x0], e = G.cell_start[y * G.nx + x1 + 1];
  for (int j = s + first; j < e; j += step) {
    const float4 p = G.spts[j];
    const unsigned long long k = gp_pack(gp_d2(p, qx, qy), __float_as_int(p.w));
    best = k < best ? k : best;
  }
  return best;
}
ROLO_DEV void gp_commit_best(GpLds& L, unsigned long long mine) {
  mine = gp_wave_min(mine);
  if ((threadIdx.x & 63) == 0 && mine != GP_NONE) atomicMin(&L.best, mine);
}

// nearest in x-y: rings of cells around the query's (clamped) cell until one holds a point, then ONE pass over the window of that point's distance proves the
// answer: every point at most that far away lies in the window (gp_window). All threads; returns the packed key (the grid holds at least one point)
ROLO_DEV unsigned long long gp_nearest(const GpGrid& G, GpLds& L, float qx, float qy) {
  const int tid = threadIdx.x;
  const int cx = gp_cell(qx, G.minx, G.inv, G.nx), cy = gp_cell(qy, G.miny, G.inv, G.ny);
  __syncthreads();
  if (tid == 0) L.best = GP_NONE;
  __syncthreads();
  const int kmax = max(G.nx, G.ny);
  unsigned long long found = GP_NONE;
  for (int k = 0; k <= kmax; k++) {
    unsigned long long mine = GP_NONE;
    const int x0 = max(cx - k, 0), x1 = min(cx + k, G.nx - 1);
    for (int side = 0; side < (k ? 2 : 1); side++) {   // the ring's bottom and top rows
      const int y = side ? cy + k : cy - k;
      if (y >= 0 && y < G.ny) mine = gp_scan_best(G, y, x0, x1, qx, qy, tid, GP_THREADS, mine);
    }
    for (int y = max(cy - k + 1, 0) + tid; y <= min(cy + k - 1, G.ny - 1); y += GP_THREADS) {   // its two columns, a row per thread
      if (cx - k >= 0) mine = gp_scan_best(G, y, cx - k, cx - k, qx, qy, 0, 1, mine);
      if (cx + k < G.nx) mine = gp_scan_best(G, y, cx + k, cx + k, qx, qy, 0, 1, mine);
    }
    gp_commit_best(L, mine);
    __syncthreads();
    found = L.best;
    __syncthreads();   // every thread has read it before the next ring or the window pass lowers it
    if (found != GP_NONE) break;
  }
  if (found == GP_NONE) return found;   // an empty grid: the host refuses it
  const float d2 = __uint_as_float((unsigned)(found >> 32));
  const double pad = sqrt((double)d2) * 1.00001 + 1e-30;
  const GpWindow w = gp_window(G, qx, qy, pad);
  unsigned long long mine = GP_NONE;
  for (int y = w.y0; y <= w.y1; y++) mine = gp_scan_best(G, y, w.x0, w.x1, qx, qy, tid, GP_THREADS, mine);
  gp_commit_best(L, mine);
  __syncthreads();
  return L.best;
}

// L.key[0 .. n) ascending. Keys are distinct (the index is part of them)
ROLO_DEV void gp_sort(GpLds& L, int n) {
  const int tid = threadIdx.x;
  if (n <= GP_THREADS) {   // by rank: one key per thread
    const unsigned long long k = tid < n ? L.key[tid] : 0ull;
    int rank = 0;
    if (tid < n) for (int j = 0; j < n; j++) rank += L.key[j] < k ? 1 : 0;
    __syncthreads();
    if (tid < n) L.key[rank] = k;
    __syncthreads();
    return;
  }
  int P = 2 * GP_THREADS;
  while (P < n) P <<= 1;   // <= GP_CAP: a power of two itself
  for (int i = n + tid; i < P; i += GP_THREADS) L.key[i] = GP_NONE;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += GP_THREADS) {
        const int o = i ^ j;
        if (o > i) {
          const unsigned long long a = L.key[i], b = L.key[o];
          if ((a > b) == ((i & k) == 0)) { L.key[i] = b; L.key[o] = a; }
        }
      }
      __syncthreads();
    }
  }
}

// the sorted radius search around (qx, qy): the number of hits; the list (sorted keys; with gather the points in its order INSTEAD) only when it fits. All threads
ROLO_DEV int gp_radius(const GpGrid& G, GpLds& L, float qx, float qy, float r2, double pad, bool gather) {
  const int tid = threadIdx.x;
  __syncthreads();
  if (tid == 0) L.cnt = 0;
  __syncthreads();
  if (r2 > 0.f) {   // a strict test against 0 (or a NaN) passes nothing
    const GpWindow w = gp_window(G, qx, qy, pad);
    for (int y = w.y0; y <= w.y1; y++) {
      const int s = G.cell_start[y * G.nx + w.x0], e = G.cell_start[y * G.nx + w.x1 + 1];
      for (int j = s + tid; j < e; j += GP_THREADS) {
        const float4 p = G.spts[j];
        const float d2 = gp_d2(p, qx, qy);
        if (d2 < r2) {
          const int slot = atomicAdd(&L.cnt, 1);
          if (slot < GP_CAP) L.key[slot] = gp_pack(d2, __float_as_int(p.w));
        }
      }
    }
  }
  __syncthreads();
  const int total = L.cnt;
  if (total > GP_CAP || total == 0) return total;
  gp_sort(L, total);
  if (gather) {
    for (int t = tid; t < total; t += GP_THREADS) {
      const float4 p = G.pts[(unsigned)L.key[t]];   // an index below n: it came from spts
      L.xy[t] = make_float2(p.x, p.y); L.pz[t] = p.z;
    }
    __syncthreads();
  }
  return total;
}

// ---- thread 0's arithmetic ----------------------------------------------------------------------------------------------------------------------------------
// one rotation of the cyclic Jacobi on a symmetric 3 x 3 (a: the full matrix, v: the vectors in columns), P < Q, R the third index
template <int P, int Q, int R>
ROLO_DEV void gp_jacobi_rot(double (&a)[9], double (&v)[9]) {
  const double apq = a[3 * P + Q];
  if (apq == 0.0) return;
  const double app = a[3 * P + P], aqq = a[3 * Q + Q], g = fabs(apq);
  if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) { a[3 * P + Q] = 0.0; a[3 * Q + P] = 0.0; return; }
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  a[3 * P + P] = app - t * apq; a[3 * Q + Q] = aqq + t * apq; a[3 * P + Q] = 0.0; a[3 * Q + P] = 0.0;
  const double arp = a[3 * R + P], arq = a[3 * R + Q];
  a[3 * R + P] = c * arp - s * arq; a[3 * P + R] = a[3 * R + P];
  a[3 * R + Q] = s * arp + c * arq; a[3 * Q + R] = a[3 * R + Q];
#pragma unroll
  for (int r = 0; r < 3; r++) { const double vp = v[3 * r + P], vq = v[3 * r + Q]; v[3 * r + P] = c * vp - s * vq; v[3 * r + Q] = s * vp + c * vq; }
}
// the eigenvector of the smallest eigenvalue (the first of equal ones) of the symmetric matrix xx xy xz yy yz zz
ROLO_DEV void gp_smallest_eigenvector(const double (&m)[6], double (&nrm)[3]) {
  double a[9] = {m[0], m[1], m[2], m[1], m[3], m[4], m[2], m[4], m[5]};
  double v[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  for (int sweep = 0; sweep < 30; sweep++) {
    if (a[1] == 0.0 && a[2] == 0.0 && a[5] == 0.0) break;
    gp_jacobi_rot<0, 1, 2>(a, v);
    gp_jacobi_rot<0, 2, 1>(a, v);
    gp_jacobi_rot<1, 2, 0>(a, v);
  }
  const bool c1 = a[4] < a[0];
  const double lo01 = c1 ? a[4] : a[0];
  const bool c2 = a[8] < lo01;
#pragma unroll
  for (int r = 0; r < 3; r++) nrm[r] = c2 ? v[3 * r + 2] : (c1 ? v[3 * r + 1] : v[3 * r]);
}

struct GpFit { int hits, inliers, fallback; double z; };

// FitLocalSurface after its search: the list of n >= 1 points is in L.xy / pz. Thread 0
ROLO_DEV void gp_fit_thread0(const GpLds& L, int n, double qx, double qy, double thr, int min_pts, GpFit& f) {
  f.inliers = 0; f.z = 0.0;
  double s = 0.0;
  for (int i = 0; i < n; i++) s += (double)L.pz[i];
  const double mean = s / (double)n;
  double ss = 0.0;
  for (int i = 0; i < n; i++) ss += ((double)L.pz[i] - mean) * ((double)L.pz[i] - mean);
  const double sd = sqrt(ss / (double)n);
  const double lo = mean - thr * sd, hi = mean + thr * sd;
  int m = 0;
  double cx = 0.0, cy = 0.0, cz = 0.0;
  for (int i = 0; i < n; i++) {
    const double z = (double)L.pz[i];
    if (z >= lo && z <= hi) { m++; cx += (double)L.xy[i].x; cy += (double)L.xy[i].y; cz += z; }
  }
  f.inliers = m;
  if (m < min_pts) { f.fallback = ROLO_PRIOR_FIT_FEW_INLIERS; return; }
  if (m < 3) { f.fallback = ROLO_PRIOR_FIT_NO_PLANE; return; }
  cx /= (double)m; cy /= (double)m; cz /= (double)m;
  double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < n; i++) {
    const double z = (double)L.pz[i];
    if (z >= lo && z <= hi) {
      const double dx = (double)L.xy[i].x - cx, dy = (double)L.xy[i].y - cy, dz = z - cz;
      c[0] += dx * dx; c[1] += dx * dy; c[2] += dx * dz; c[3] += dy * dy; c[4] += dy * dz; c[5] += dz * dz;
    }
  }
  double nrm[3];
  gp_smallest_eigenvector(c, nrm);
  const double d = -((nrm[0] * cx + nrm[1] * cy) + nrm[2] * cz);
  if (fabs(nrm[2]) < 1e-6) { f.fallback = ROLO_PRIOR_FIT_VERTICAL; return; }
  f.z = -((nrm[0] * qx + nrm[1] * qy) + d) / nrm[2];
  f.fallback = ROLO_PRIOR_FIT_OK;
}

// the ground point under a double query as ComputeResidualAndJacobian takes it: the fit, else the nearest point. All threads; pn / rec are thread 0's to write.
// Returns the status bits it raises (uniform)
ROLO_DEV int gp_ground_point(const GpGrid& G, GpLds& L, const GpParams& P, double qx, double qy, double* pn, rolo_priorpose_fit* rec) {
  const int tid = threadIdx.x;
  const float fx = (float)qx, fy = (float)qy;
  const int hits = gp_radius(G, L, fx, fy, P.fit_r2, P.fit_pad, true);
  __syncthreads();   // thread 0 wrote L.ctl last in an earlier call: every thread has read it by now
  if (tid == 0) {
    GpFit f; f.hits = hits; f.inliers = 0; f.z = 0.0;
    if (hits > GP_CAP) f.fallback = ROLO_PRIOR_FIT_OVERFLOW;
    else if (hits < P.fit_min_pts) f.fallback = ROLO_PRIOR_FIT_FEW_HITS;
    else if (hits == 0) f.fallback = ROLO_PRIOR_FIT_NO_PLANE;   // fit_min_points = 0 and an empty disc: FitPlane's own refusal
    else gp_fit_thread0(L, hits, qx, qy, P.fit_thr, P.fit_min_pts, f);
    if (f.fallback == ROLO_PRIOR_FIT_OK) { pn[0] = qx; pn[1] = qy; pn[2] = f.z; }
    if (rec) { rec->hits = hits; rec->inliers = f.inliers; rec->fallback = f.fallback; rec->nearest = -1; }
    L.ctl = f.fallback;
  }
  __syncthreads();
  const int fb = L.ctl;
  if (fb == ROLO_PRIOR_FIT_OK) return 0;
  const unsigned long long k = gp_nearest(G, L, fx, fy);
  if (tid == 0) {
    const float4 p = G.pts[(unsigned)k];
    pn[0] = (double)p.x; pn[1] = (double)p.y; pn[2] = (double)p.z;
    if (rec) rec->nearest = (int)(unsigned)k;
  }
  return fb == ROLO_PRIOR_FIT_OVERFLOW ? ROLO_PRIOR_STATUS_OVERFLOW : 0;
}

// AverageHeightAt. All threads; *h is thread 0's to write. Returns the status bits it raises (uniform)
ROLO_DEV int gp_average_height(const GpGrid& G, GpLds& L, const GpParams& P, double qx, double qy, double* h) {
  const int tid = threadIdx.x;
  const unsigned long long k = gp_nearest(G, L, (float)qx, (float)qy);
  const float4 c = G.pts[(unsigned)k];
  if (!(P.avg_radius > 0.0)) { if (tid == 0) *h = (double)c.z; return 0; }
  const int hits = gp_radius(G, L, c.x, c.y, P.avg_r2, P.avg_pad, true);
  if (tid == 0) {
    if (hits <= 0 || hits < P.avg_min_nb || hits > GP_CAP) *h = (double)c.z;
    else {
      double s = 0.0;
      for (int i = 0; i < hits; i++) s += (double)L.pz[i];
      *h = s / (double)hits;
    }
  }
  return hits > GP_CAP ? ROLO_PRIOR_STATUS_OVERFLOW : 0;
}

// 3 x 3 products, each element (a0 b0 + a1 b1) + a2 b2
ROLO_DEV void gp_mul33(const double* a, const double* b, double* o) {
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) o[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}
ROLO_DEV void gp_rotx(double a, double* R) { const double c = cos(a), s = sin(a); R[0] = 1; R[1] = 0; R[2] = 0; R[3] = 0; R[4] = c; R[5] = -s; R[6] = 0; R[7] = s; R[8] = c; }
ROLO_DEV void gp_roty(double a, double* R) { const double c = cos(a), s = sin(a); R[0] = c; R[1] = 0; R[2] = s; R[3] = 0; R[4] = 1; R[5] = 0; R[6] = -s; R[7] = 0; R[8] = c; }
ROLO_DEV void gp_rotz(double a, double* R) { const double c = cos(a), s = sin(a); R[0] = c; R[1] = -s; R[2] = 0; R[3] = s; R[4] = c; R[5] = 0; R[6] = 0; R[7] = 0; R[8] = 1; }

// Eigen::FullPivLU<Matrix3d>(A).solve(b): false when A is not invertible by its rank rule. x may be LDS (it is indexed by the column permutation)
ROLO_DEV bool gp_lu3_solve(const double* A, const double* b, double* x) {
  double a[3][3] = {{A[0], A[1], A[2]}, {A[3], A[4], A[5]}, {A[6], A[7], A[8]}};
  double c[3] = {b[0], b[1], b[2]};
  int col[3] = {0, 1, 2};
  double maxpivot = 0.0;
  bool zero = false;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (zero) break;
    int pr = k, pc = k;
    double big = -1.0;
#pragma unroll
    for (int j = k; j < 3; j++) {   // Eigen's maxCoeff walks column by column and keeps the first of equals
#pragma unroll
      for (int i = k; i < 3; i++) { const double v = fabs(a[i][j]); if (v > big) { big = v; pr = i; pc = j; } }
    }
    if (big == 0.0 || !(big >= 0.0)) { zero = true; break; }
    if (big > maxpivot) maxpivot = big;
#pragma unroll
    for (int r = k + 1; r < 3; r++) if (pr == r) {
#pragma unroll
      for (int j = 0; j < 3; j++) { const double t = a[k][j]; a[k][j] = a[r][j]; a[r][j] = t; }
      const double t = c[k]; c[k] = c[r]; c[r] = t;
    }
#pragma unroll
    for (int q = k + 1; q < 3; q++) if (pc == q) {
#pragma unroll
      for (int i = 0; i < 3; i++) { const double t = a[i][k]; a[i][k] = a[i][q]; a[i][q] = t; }
      const int t = col[k]; col[k] = col[q]; col[q] = t;
    }
#pragma unroll
    for (int i = k + 1; i < 3; i++) {
      const double l = a[i][k] / a[k][k];
      a[i][k] = l;
#pragma unroll
      for (int j = k + 1; j < 3; j++) a[i][j] -= l * a[k][j];
      c[i] -= l * c[k];
    }
  }
  if (zero) return false;
  const double thr = 3.0 * DBL_EPSILON * maxpivot;
  if (!(fabs(a[0][0]) > thr && fabs(a[1][1]) > thr && fabs(a[2][2]) > thr)) return false;
  const double y2 = c[2] / a[2][2];
  const double y1 = (c[1] - a[1][2] * y2) / a[1][1];
  const double y0 = ((c[0] - a[0][1] * y1) - a[0][2] * y2) / a[0][0];
  x[col[0]] = y0; x[col[1]] = y1; x[col[2]] = y2;
  return true;
}

// the solver's state: thread 0's, in LDS so that its arrays are indexed freely
struct GpState {
  double x, y, yaw, z, R[9], best_z, best_R[9], best_cost, last_cost, lambda;
  double zt, Rt[9];              // the trial pose
  double pw[GP_W][3], pn[GP_W][3], h[GP_W];
  double res[3], J[9], delta[3], step, c0;
  double f[4][GP_W];             // per wheel: the contact force and its derivatives by z, roll, pitch
};

// the wheels' world points for (R, z) into S.pw. Thread 0; false when one is not finite
ROLO_DEV bool gp_wheel_points(GpState& S, const GpParams& P, const double* R, double z) {
  bool ok = true;
  for (int w = 0; w < P.n_wheels; w++) {
    const double b[3] = {P.wheel[w][0], P.wheel[w][1], -P.com_z};
    S.pw[w][0] = ((R[0] * b[0] + R[1] * b[1]) + R[2] * b[2]) + S.x;
    S.pw[w][1] = ((R[3] * b[0] + R[4] * b[1]) + R[5] * b[2]) + S.y;
    S.pw[w][2] = ((R[6] * b[0] + R[7] * b[1]) + R[8] * b[2]) + z;
    ok = ok && isfinite(S.pw[w][0]) && isfinite(S.pw[w][1]) && isfinite(S.pw[w][2]);
  }
  return ok;
}

// ComputeResidualAndJacobian once S.pw and S.pn are there. Thread 0
ROLO_DEV void gp_residual(GpState& S, const GpParams& P, const double* R, bool want_J) {
  const double nx = R[2], ny = R[5], nz = R[8];   // R ez
  double *f = S.f[0], *fz = S.f[1], *fr = S.f[2], *fp = S.f[3];
  for (int w = 0; w < P.n_wheels; w++) {
    const double a0 = S.pw[w][0] - S.pn[w][0], a1 = S.pw[w][1] - S.pn[w][1], a2 = S.pw[w][2] - S.pn[w][2];
    const double d = (a0 * nx + a1 * ny) + a2 * nz;
    const bool active = d < 0.0;
    f[w] = active ? P.k_spring * d : 0.0;
    const double b[3] = {P.wheel[w][0], P.wheel[w][1], -P.com_z};
    const double rp1 = (R[3] * b[0] + R[4] * b[1]) + R[5] * b[2], rp2 = (R[6] * b[0] + R[7] * b[1]) + R[8] * b[2], rp0 = (R[0] * b[0] + R[1] * b[1]) + R[2] * b[2];
    // Sx v = (0, -vz, vy), Sy v = (vz, 0, -vx)
    const double dd_dz = ((0.0 * nx + 0.0 * ny) + 1.0 * nz);
    const double dd_dr = ((0.0 * nx + (-rp2) * ny) + rp1 * nz) + ((a0 * 0.0 + a1 * (-nz)) + a2 * ny);
    const double dd_dp = ((rp2 * nx + 0.0 * ny) + (-rp0) * nz) + ((a0 * nz + a1 * 0.0) + a2 * (-nx));
    fz[w] = active ? P.k_spring * dd_dz : 0.0; fr[w] = active ? P.k_spring * dd_dr : 0.0; fp[w] = active ? P.k_spring * dd_dp : 0.0;
  }
  // wrench_map rows: 1, wy, -wx
  double r0 = 0.0, r1 = 0.0, r2 = 0.0;
  for (int w = 0; w < P.n_wheels; w++) { r0 += 1.0 * f[w]; r1 += P.wheel[w][1] * f[w]; r2 += (-P.wheel[w][0]) * f[w]; }
  S.res[0] = r0 + P.g * ((nx * 0.0 + ny * 0.0) + nz * 1.0); S.res[1] = r1 + P.g * 0.0; S.res[2] = r2 + P.g * 0.0;
  if (!want_J) return;
  for (int c = 0; c < 3; c++) {
    const double* v = c == 0 ? fz : (c == 1 ? fr : fp);
    double j0 = 0.0, j1 = 0.0, j2 = 0.0;
    for (int w = 0; w < P.n_wheels; w++) { j0 += 1.0 * v[w]; j1 += P.wheel[w][1] * v[w]; j2 += (-P.wheel[w][0]) * v[w]; }
    S.J[c] = j0; S.J[3 + c] = j1; S.J[6 + c] = j2;
  }
  S.J[1] += P.g * ny;      // ez . (Sx n) = ny
  S.J[2] += P.g * (-nx);   // ez . (Sy n) = -nx
}

// the ground under every wheel of S.pw into S.pn (fit, else nearest). All threads; returns the status bits (uniform)
ROLO_DEV int gp_ground_under_wheels(const GpGrid& G, GpLds& L, GpState& S, const GpParams& P) {
  int st = 0;
  for (int w = 0; w < P.n_wheels; w++) st |= gp_ground_point(G, L, P, S.pw[w][0], S.pw[w][1], S.pn[w], nullptr);
  __syncthreads();
  return st;
}

// tf2::Matrix3x3::getRPY (getEulerYPR, its first solution)
ROLO_DEV void gp_get_rpy(const double* m, double* rpy) {
  if (fabs(m[6]) >= 1.0) {
    const double delta = atan2(m[7], m[8]);
    rpy[2] = 0.0; rpy[0] = delta; rpy[1] = m[6] < 0.0 ? 1.5707963267948966 : -1.5707963267948966;
  } else {
    const double pitch = -asin(m[6]), cp = cos(pitch);
    rpy[1] = pitch; rpy[0] = atan2(m[7] / cp, m[8] / cp); rpy[2] = atan2(m[3] / cp, m[0] / cp);
  }
}

__global__ __launch_bounds__(GP_THREADS) void gp_solve_kernel(GpGrid G, GpParams P, const double* __restrict__ xyyaw, rolo_priorpose_result* __restrict__ out) {
  __shared__ GpLds L;
  __shared__ GpState S;
  const int tid = threadIdx.x;
  const int W = P.n_wheels;
  if (tid == 0) {
    S.x = xyyaw[3 * (size_t)blockIdx.x]; S.y = xyyaw[3 * (size_t)blockIdx.x + 1]; S.yaw = xyyaw[3 * (size_t)blockIdx.x + 2];
    gp_rotz(S.yaw, S.R);
    // InitialZ's queries: (x, y) + RotZ(yaw) vertex
    for (int w = 0; w < W; w++) {
      const double b[3] = {P.wheel[w][0], P.wheel[w][1], -P.com_z};
      S.pw[w][0] = S.x + ((S.R[0] * b[0] + S.R[1] * b[1]) + S.R[2] * b[2]);
      S.pw[w][1] = S.y + ((S.R[3] * b[0] + S.R[4] * b[1]) + S.R[5] * b[2]);
    }
  }
  __syncthreads();
  int status = 0;   // uniform
  for (int w = 0; w < W; w++) status |= gp_average_height(G, L, P, S.pw[w][0], S.pw[w][1], &S.h[w]);
  __syncthreads();
  if (tid == 0) {
    double min_h = INFINITY;
    for (int w = 0; w < W; w++) min_h = S.h[w] < min_h ? S.h[w] : min_h;   // std::min(min_h, h)
    S.z = isfinite(min_h) ? (min_h + P.com_z) - 1.0 : 0.0;
    S.last_cost = INFINITY; S.best_cost = INFINITY; S.best_z = S.z; S.lambda = P.lambda0;
    for (int k = 0; k < 9; k++) S.best_R[k] = S.R[k];
  }
  __syncthreads();
  // L.ctl codes of the loop
  enum { GO = 0, SINGULAR = 1, STOP_NONFINITE = 2, CONVERGED = 3 };
  int iterations = 0, end_reason = ROLO_PRIOR_END_MAX_ITERS;
  for (int it = 0; it < P.max_iters; it++) {
    iterations = it + 1;
    if (tid == 0) L.ctl = gp_wheel_points(S, P, S.R, S.z) ? GO : STOP_NONFINITE;
    __syncthreads();
    if (L.ctl == STOP_NONFINITE) { status |= ROLO_PRIOR_STATUS_NONFINITE; break; }
    status |= gp_ground_under_wheels(G, L, S, P);
    if (tid == 0) {
      gp_residual(S, P, S.R, true);
      const double c0 = (S.res[0] * S.res[0] + S.res[1] * S.res[1]) + S.res[2] * S.res[2];
      int ctl = GO;
      if (!isfinite(c0)) ctl = STOP_NONFINITE;
      else {
        if (c0 < S.best_cost) { S.best_cost = c0; S.best_z = S.z; for (int k = 0; k < 9; k++) S.best_R[k] = S.R[k]; }
        double A[9], b[3];
        for (int i = 0; i < 3; i++) {
          for (int j = 0; j < 3; j++) A[3 * i + j] = ((S.J[i] * S.J[j] + S.J[3 + i] * S.J[3 + j]) + S.J[6 + i] * S.J[6 + j]) + (i == j ? S.lambda : 0.0);
          b[i] = -((S.J[i] * S.res[0] + S.J[3 + i] * S.res[1]) + S.J[6 + i] * S.res[2]);
        }
        if (!gp_lu3_solve(A, b, S.delta)) { S.lambda *= 10.0; ctl = SINGULAR; }
        else {
          S.step = sqrt((S.delta[0] * S.delta[0] + S.delta[1] * S.delta[1]) + S.delta[2] * S.delta[2]);
          S.zt = S.z + S.delta[0];
          double Rx[9], Ry[9], Rxy[9], Rn[9], Rz[9], tilt[9];
          gp_rotx(S.delta[1], Rx); gp_roty(S.delta[2], Ry);
          gp_mul33(Rx, Ry, Rxy); gp_mul33(Rxy, S.R, Rn);
          gp_rotz(-atan2(Rn[3], Rn[0]), Rz); gp_mul33(Rz, Rn, tilt);   // EnforceFixedYaw
          gp_rotz(S.yaw, Rz); gp_mul33(Rz, tilt, S.Rt);
          if (!gp_wheel_points(S, P, S.Rt, S.zt)) ctl = STOP_NONFINITE;
        }
      }
      S.c0 = c0;
      L.ctl = ctl;
    }
    __syncthreads();
    const int ctl = L.ctl;
    if (ctl == STOP_NONFINITE) { status |= ROLO_PRIOR_STATUS_NONFINITE; break; }
    if (ctl == SINGULAR) { __syncthreads(); continue; }
    status |= gp_ground_under_wheels(G, L, S, P);
    if (tid == 0) {
      const double c0 = S.c0;
      gp_residual(S, P, S.Rt, false);
      const double c1 = (S.res[0] * S.res[0] + S.res[1] * S.res[1]) + S.res[2] * S.res[2];
      int c = GO;
      if (c1 < c0) {
        S.z = S.zt;
        for (int k = 0; k < 9; k++) S.R[k] = S.Rt[k];
        S.lambda = fmax(S.lambda / 2.0, 1e-8);
        if (fabs(S.last_cost - c1) < P.tol_cost && S.step < P.tol_step) c = CONVERGED;
        else S.last_cost = c1;
      } else {
        S.lambda *= 5.0;
        S.last_cost = c0;
      }
      L.ctl = c;
    }
    __syncthreads();
    const int c = L.ctl;
    __syncthreads();   // L.ctl is rewritten at the top of the next iteration
    if (c == CONVERGED) { end_reason = ROLO_PRIOR_END_CONVERGED; break; }
  }
  __syncthreads();
  // the wheels' signed distances to the nearest points, at the best pose
  if (tid == 0) L.ctl = gp_wheel_points(S, P, S.best_R, S.best_z) ? GO : STOP_NONFINITE;
  __syncthreads();
  const bool finite_end = L.ctl == GO;
  if (!finite_end) status |= ROLO_PRIOR_STATUS_NONFINITE;
  for (int w = 0; w < W; w++) {
    if (!finite_end) break;
    const unsigned long long k = gp_nearest(G, L, (float)S.pw[w][0], (float)S.pw[w][1]);
    if (tid == 0) { const float4 p = G.pts[(unsigned)k]; S.pn[w][0] = (double)p.x; S.pn[w][1] = (double)p.y; S.pn[w][2] = (double)p.z; }
  }
  __syncthreads();
  if (tid == 0) {
    rolo_priorpose_result& r = out[blockIdx.x];   // written in place: the wheel loop indexes it
    for (int w = W; w < GP_W; w++) r.wheel_distance[w] = 0.0;
    r.z = S.best_z; r.cost = S.best_cost;
    for (int k = 0; k < 9; k++) r.R[k] = S.best_R[k];
    double Rz[9], tilt[9];
    gp_rotz(-S.yaw, Rz); gp_mul33(Rz, S.best_R, tilt);   // ComputeRollPitchFromFixedYaw
    r.roll = atan2(tilt[7], tilt[8]); r.pitch = atan2(-tilt[6], tilt[0]);
    const double nx = S.best_R[2], ny = S.best_R[5], nz = S.best_R[8];
    bool ok = status == 0 && end_reason == ROLO_PRIOR_END_CONVERGED;
    for (int w = 0; w < W; w++) {
      const double d = finite_end ? ((S.pw[w][0] - S.pn[w][0]) * nx + (S.pw[w][1] - S.pn[w][1]) * ny) + (S.pw[w][2] - S.pn[w][2]) * nz : 0.0;
      r.wheel_distance[w] = d;
      if (fabs(d) > P.dist_max) ok = false;
    }
    if (r.z < P.z_min || r.z > P.z_max) ok = false;
    if (fabs(r.roll) > P.roll_max || fabs(r.pitch) > P.pitch_max) ok = false;
    // HandlePose: T_world_body (setRPY(roll, pitch, yaw), (x, y, z)) times body_to_lidar
    double Rx[9], Ry[9], Ryx[9], Rwb[9], Rwl[9];
    gp_rotx(r.roll, Rx); gp_roty(r.pitch, Ry); gp_rotz(S.yaw, Rz);
    gp_mul33(Ry, Rx, Ryx); gp_mul33(Rz, Ryx, Rwb); gp_mul33(Rwb, P.bl_R, Rwl);
    r.lidar_pose[0] = ((Rwb[0] * P.bl_t[0] + Rwb[1] * P.bl_t[1]) + Rwb[2] * P.bl_t[2]) + S.x;
    r.lidar_pose[1] = ((Rwb[3] * P.bl_t[0] + Rwb[4] * P.bl_t[1]) + Rwb[5] * P.bl_t[2]) + S.y;
    r.lidar_pose[2] = ((Rwb[6] * P.bl_t[0] + Rwb[7] * P.bl_t[1]) + Rwb[8] * P.bl_t[2]) + r.z;
    gp_get_rpy(Rwl, r.lidar_pose + 3);
    r.iterations = iterations; r.end_reason = end_reason; r.success = ok ? 1 : 0; r.status = status;
  }
}

// the debug entry points: one workgroup per query
__global__ __launch_bounds__(GP_THREADS) void gp_nearest_kernel(GpGrid G, const float* __restrict__ xy, int32_t* __restrict__ idx, float* __restrict__ d2) {
  __shared__ GpLds L;
  const unsigned long long k = gp_nearest(G, L, xy[2 * (size_t)blockIdx.x], xy[2 * (size_t)blockIdx.x + 1]);
  if (threadIdx.x == 0) { idx[blockIdx.x] = (int32_t)(unsigned)k; d2[blockIdx.x] = __uint_as_float((unsigned)(k >> 32)); }
}
__global__ __launch_bounds__(GP_THREADS) void gp_radius_kernel(GpGrid G, const float* __restrict__ xy, float r2, double pad, int cap, int32_t* __restrict__ count,
                                                               int32_t* __restrict__ idx, float* __restrict__ d2) {
  __shared__ GpLds L;
  const int total = gp_radius(G, L, xy[2 * (size_t)blockIdx.x], xy[2 * (size_t)blockIdx.x + 1], r2, pad, false);
  if (threadIdx.x == 0) count[blockIdx.x] = total;
  if (total > GP_CAP) return;
  for (int t = threadIdx.x; t < min(total, cap); t += GP_THREADS) {
    const unsigned long long k = L.key[t];
    idx[(size_t)blockIdx.x * cap + t] = (int32_t)(unsigned)k; d2[(size_t)blockIdx.x * cap + t] = __uint_as_float((unsigned)(k >> 32));
  }
}
__global__ __launch_bounds__(GP_THREADS) void gp_fit_kernel(GpGrid G, GpParams P, const double* __restrict__ xy, rolo_priorpose_fit* __restrict__ out) {
  __shared__ GpLds L;
  __shared__ double pn[3];
  __shared__ rolo_priorpose_fit rec;
  gp_ground_point(G, L, P, xy[2 * (size_t)blockIdx.x], xy[2 * (size_t)blockIdx.x + 1], pn, &rec);
  __syncthreads();
  if (threadIdx.x == 0) { rec.point[0] = pn[0]; rec.point[1] = pn[1]; rec.point[2] = pn[2]; out[blockIdx.x] = rec; }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------------
GpGrid grid_of(const rolo_ground* g) { return GpGrid{g->minx, g->miny, 1.0f / g->cell, g->nx, g->ny, g->n, g->cell_start, g->spts, g->pts}; }

bool all_finite(const double* v, int n) { for (int i = 0; i < n; i++) if (!std::isfinite(v[i])) return false; return true; }

// what the radius search passes down for a radius, and the padding of its window
void radius_terms(double r, float* r2, double* pad) { *r2 = (float)(r * r); *pad = std::fabs(r) * 1.00001 + 1e-30; }

int params_to_device(const rolo_priorpose_params* p, GpParams* P) {
  if (!p) return ROLO_EINVAL;
  if (p->n_wheels < 1 || p->n_wheels > ROLO_PRIOR_MAX_WHEELS) { ctx_set_error("rolo_priorpose: n_wheels outside 1 .. ROLO_PRIOR_MAX_WHEELS"); return ROLO_EINVAL; }
  if (p->max_iters < 0 || p->max_iters > ROLO_PRIOR_MAX_ITERS) { ctx_set_error("rolo_priorpose: max_iters outside 0 .. ROLO_PRIOR_MAX_ITERS"); return ROLO_EINVAL; }
  if (p->ground_min_neighbors < 0 || p->fit_min_points < 0) { ctx_set_error("rolo_priorpose: a negative neighbour count"); return ROLO_EINVAL; }
  const double scal[] = {p->vehicle_com_z, p->k_spring, p->g, p->lm_lambda, p->tol_cost, p->tol_step, p->ground_avg_radius, p->fit_radius, p->fit_outlier_factor,
                         p->z_min, p->z_max, p->roll_max, p->pitch_max, p->wheel_distance_max};
  if (!all_finite(scal, (int)(sizeof(scal) / sizeof(double))) || !all_finite(p->wheel_xy, 2 * p->n_wheels) || !all_finite(p->body_to_lidar_t, 3) ||
      !all_finite(p->body_to_lidar_R, 9)) { ctx_set_error("rolo_priorpose: a non-finite parameter"); return ROLO_ENONFINITE; }
  memset(P, 0, sizeof(*P));
  P->n_wheels = p->n_wheels; P->max_iters = p->max_iters; P->avg_min_nb = p->ground_min_neighbors; P->fit_min_pts = p->fit_min_points;
  for (int w = 0; w < p->n_wheels; w++) { P->wheel[w][0] = p->wheel_xy[2 * w]; P->wheel[w][1] = p->wheel_xy[2 * w + 1]; }
  P->com_z = p->vehicle_com_z;
  for (int k = 0; k < 3; k++) P->bl_t[k] = p->body_to_lidar_t[k];
  for (int k = 0; k < 9; k++) P->bl_R[k] = p->body_to_lidar_R[k];
  P->k_spring = p->k_spring; P->g = p->g; P->lambda0 = p->lm_lambda; P->tol_cost = p->tol_cost; P->tol_step = p->tol_step;
  P->avg_radius = p->ground_avg_radius; radius_terms(p->ground_avg_radius, &P->avg_r2, &P->avg_pad);
  P->fit_thr = p->fit_outlier_factor; radius_terms(p->fit_radius, &P->fit_r2, &P->fit_pad);
  P->z_min = p->z_min; P->z_max = p->z_max; P->roll_max = p->roll_max; P->pitch_max = p->pitch_max; P->dist_max = p->wheel_distance_max;
  return ROLO_OK;
}

int need_cloud(const rolo_ground* g, const char* who) {
  if (!g) return ROLO_EINVAL;
  if (!g->have_cloud) { ctx_set_error((std::string(who) + ": the ground model holds no cloud").c_str()); return ROLO_ESTATE; }
  return ROLO_OK;
}

int ensure_events(rolo_ground* g) {
  for (int k = 0; k < 2; k++) if (!g->ev[k]) HIPCHK(hipEventCreate(&g->ev[k]));
  return ROLO_OK;
}

// queries (bytes) up, one kernel's records (bytes) down: the staging every batched entry point shares
int stage_in(rolo_ground* g, const void* src, size_t bytes) {
  const int rc = g->store.grow(g->d_q, g->d_q_cap, (bytes + 7) / 8);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(g->d_q, src, bytes, hipMemcpyHostToDevice, g->stream));
  return ROLO_OK;
}

}  // namespace
}  // namespace rolo

using namespace rolo;

extern "C" {

int rolo_ground_create(int device, rolo_ground** out) {
  if (!out) return ROLO_EINVAL;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { ctx_set_error("no HIP device"); return ROLO_EHIP; }
  if (device < 0 || device >= ndev) return ROLO_EINVAL;
  HIPCHK(hipSetDevice(device));
  rolo_ground* g = new rolo_ground();
  g->device = device;
  const hipError_t e = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking);
  if (e != hipSuccess) { ctx_set_error((std::string("rolo_ground_create: ") + hipGetErrorString(e)).c_str()); rolo_ground_destroy(g); return ROLO_EHIP; }
  g->store.stream = g->stream; g->store.who = "ground";
  int rc = g->store.alloc_pinned(g->h_box, 8);
  if (!rc) rc = g->store.alloc_pinned(g->h_m, 2);
  if (!rc) rc = g->store.alloc(g->d_m, 2);
  if (rc) { rolo_ground_destroy(g); return rc; }
  *out = g;
  return ROLO_OK;
}

void rolo_ground_destroy(rolo_ground* g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  if (g->stream) (void)hipStreamSynchronize(g->stream);
  g->store.release();
  for (hipEvent_t e : g->ev) if (e) (void)hipEventDestroy(e);
  if (g->stream) (void)hipStreamDestroy(g->stream);
  delete g;
}

int rolo_ground_set_grid(rolo_ground* g, float cell_size, int max_cells) {
  if (!g) return ROLO_EINVAL;
  if (!(cell_size > 0.f) || !std::isfinite(cell_size) || max_cells < 1 || max_cells > ROLO_GROUND_MAX_CELLS) {
    ctx_set_error("rolo_ground_set_grid: the cell size must be positive and finite, the cell limit within 1 .. ROLO_GROUND_MAX_CELLS"); return ROLO_EINVAL;
  }
  g->cell0 = cell_size; g->max_cells = max_cells;
  return ROLO_OK;
}

int rolo_ground_set_cloud(rolo_ground* g, const float* pts, int n, int stride) {
  if (!g || n < 0 || n > ROLO_GROUND_MAX_POINTS || stride < 3 || stride > 8 || (n > 0 && !pts)) { ctx_set_error("rolo_ground_set_cloud: bad argument"); return ROLO_EINVAL; }
  std::vector<float> p4((size_t)n * 4);
  for (int i = 0; i < n; i++) {
    const float* r = pts + (size_t)i * stride;
    if (!(std::isfinite(r[0]) && std::isfinite(r[1]))) { ctx_set_error("rolo_ground_set_cloud: a non-finite x or y"); return ROLO_ENONFINITE; }
    p4[4 * (size_t)i] = r[0]; p4[4 * (size_t)i + 1] = r[1]; p4[4 * (size_t)i + 2] = r[2]; p4[4 * (size_t)i + 3] = 0.f;
  }
  g->have_cloud = false;
  g->n = 0;
  if (n == 0) return ROLO_OK;
  HIPCHK(hipSetDevice(g->device));
  hipStream_t s = g->stream;
  int rc;
  if ((rc = ensure_events(g))) return rc;
  if ((rc = g->store.grow(g->rec, g->rec_cap, (size_t)n * stride))) return rc;
  if ((rc = g->store.grow(g->pts, g->pts_cap, (size_t)n))) return rc;
  if ((rc = g->store.grow(g->spts, g->spts_cap, (size_t)n))) return rc;
  if ((rc = g->sort.reserve(g->store, (size_t)n))) return rc;
  if ((rc = g->store.grow(g->box_part, g->box_part_cap, 8 * (size_t)BOX_BLOCKS_MAX))) return rc;
  HIPCHK(hipMemcpyAsync(g->rec, pts, sizeof(float) * (size_t)n * stride, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(g->pts, p4.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, s));
  HIPCHK(hipEventRecord(g->ev[0], s));
  if ((rc = enqueue_box(s, g->pts, n, g->box_part, g->h_box))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  const float minx = g->h_box[0], miny = g->h_box[1], maxx = g->h_box[3], maxy = g->h_box[4];
  // the cell size: doubled until no side and not the whole grid is over its limit
  const long long limit = std::min<long long>(g->max_cells, 4ll * n + 1024);
  float cell = g->cell0;
  int doubled = 0, nx = 1, ny = 1;
  for (;; doubled++, cell *= 2.f) {
    if (!std::isfinite(cell)) { ctx_set_error("rolo_ground_set_cloud: the cloud's extent does not fit a grid"); return ROLO_EINVAL; }
    const float inv = 1.0f / cell;
    const double ex = std::floor((double)((maxx - minx) * inv)) + 1.0, ey = std::floor((double)((maxy - miny) * inv)) + 1.0;
    if (!(ex <= ROLO_GROUND_MAX_SIDE && ey <= ROLO_GROUND_MAX_SIDE && ex * ey <= (double)limit)) continue;
    nx = (int)ex; ny = (int)ey;
    break;
  }
  g->minx = minx; g->miny = miny; g->cell = cell; g->nx = nx; g->ny = ny; g->doubled = doubled; g->stride = stride;
  const int cells = nx * ny;
  if ((rc = g->store.grow(g->cell_start, g->cell_start_cap, (size_t)cells + 1))) return rc;
  g->n = n;
  const GpGrid G = grid_of(g);
  gp_key_kernel<<<(n + SM_THREADS - 1) / SM_THREADS, SM_THREADS, 0, s>>>(g->pts, n, G, g->sort.keys[0], g->sort.vals[0]);
  HIPCHK(hipGetLastError());
  int cur = 0;
  if ((rc = g->sort.sort_pairs(s, n, sort_bits_for_cells(cells), &cur))) return rc;
  gp_cell_start_kernel<<<(cells + 1 + SM_THREADS - 1) / SM_THREADS, SM_THREADS, 0, s>>>(g->sort.keys[cur], n, cells, g->cell_start);
  HIPCHK(hipGetLastError());
  gp_sorted_points_kernel<<<(n + SM_THREADS - 1) / SM_THREADS, SM_THREADS, 0, s>>>(g->pts, g->sort.vals[cur], n, g->spts);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(g->ev[1], s));
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipEventElapsedTime(&g->ms[0], g->ev[0], g->ev[1]));
  g->have_cloud = true;
  return ROLO_OK;
}

int rolo_ground_info(rolo_ground* g, long long* out, int cap) {
  if (!g || !out || cap < 0) return ROLO_EINVAL;
  const long long v[5] = {g->have_cloud ? g->n : 0, g->have_cloud ? g->nx : 0, g->have_cloud ? g->ny : 0, g->have_cloud ? g->doubled : 0, g->have_cloud ? g->stride : 0};
  for (int k = 0; k < std::min(cap, 5); k++) out[k] = v[k];
  return ROLO_OK;
}

int rolo_ground_nearest_xy(rolo_ground* g, const float* xy, int nq, int32_t* idx, float* d2) {
  int rc = need_cloud(g, "rolo_ground_nearest_xy");
  if (rc) return rc;
  if (!xy || !idx || !d2 || nq < 1 || nq > ROLO_GROUND_MAX_QUERIES) { ctx_set_error("rolo_ground_nearest_xy: bad argument"); return ROLO_EINVAL; }
  for (int i = 0; i < 2 * nq; i++) if (!std::isfinite(xy[i])) { ctx_set_error("rolo_ground_nearest_xy: a non-finite query"); return ROLO_ENONFINITE; }
  HIPCHK(hipSetDevice(g->device));
  if ((rc = stage_in(g, xy, sizeof(float) * 2 * (size_t)nq))) return rc;
  if ((rc = g->store.grow(g->d_out, g->d_out_cap, 8 * (size_t)nq))) return rc;
  int32_t* d_idx = reinterpret_cast<int32_t*>(g->d_out); float* d_d2 = reinterpret_cast<float*>(g->d_out) + nq;
  gp_nearest_kernel<<<nq, GP_THREADS, 0, g->stream>>>(grid_of(g), reinterpret_cast<const float*>(g->d_q), d_idx, d_d2);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(idx, d_idx, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, g->stream));
  HIPCHK(hipMemcpyAsync(d2, d_d2, sizeof(float) * (size_t)nq, hipMemcpyDeviceToHost, g->stream));
  HIPCHK(hipStreamSynchronize(g->stream));
  return ROLO_OK;
}

int rolo_ground_radius_xy(rolo_ground* g, const float* xy, int nq, double radius, int cap, int32_t* count, int32_t* idx, float* d2) {
  int rc = need_cloud(g, "rolo_ground_radius_xy");
  if (rc) return rc;
  if (!xy || !count || nq < 1 || nq > ROLO_GROUND_MAX_QUERIES || cap < 0 || cap > ROLO_GROUND_MAX_NEIGHBOURS || (cap > 0 && (!idx || !d2))) {
    ctx_set_error("rolo_ground_radius_xy: bad argument"); return ROLO_EINVAL;
  }
  if (!std::isfinite(radius)) { ctx_set_error("rolo_ground_radius_xy: a non-finite radius"); return ROLO_ENONFINITE; }
  for (int i = 0; i < 2 * nq; i++) if (!std::isfinite(xy[i])) { ctx_set_error("rolo_ground_radius_xy: a non-finite query"); return ROLO_ENONFINITE; }
  HIPCHK(hipSetDevice(g->device));
  if ((rc = stage_in(g, xy, sizeof(float) * 2 * (size_t)nq))) return rc;
  const size_t rows = (size_t)nq * (size_t)std::max(cap, 1);
  if ((rc = g->store.grow(g->d_out, g->d_out_cap, 4 * (size_t)nq + 8 * rows))) return rc;
  int32_t* d_cnt = reinterpret_cast<int32_t*>(g->d_out); int32_t* d_idx = d_cnt + nq; float* d_d2 = reinterpret_cast<float*>(d_idx + rows);
  float r2; double pad;
  radius_terms(radius, &r2, &pad);
  gp_radius_kernel<<<nq, GP_THREADS, 0, g->stream>>>(grid_of(g), reinterpret_cast<const float*>(g->d_q), r2, pad, cap, d_cnt, d_idx, d_d2);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(count, d_cnt, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, g->stream));
  if (cap > 0) {
    HIPCHK(hipMemcpyAsync(idx, d_idx, sizeof(int32_t) * rows, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipMemcpyAsync(d2, d_d2, sizeof(float) * rows, hipMemcpyDeviceToHost, g->stream));
  }
  HIPCHK(hipStreamSynchronize(g->stream));
  return ROLO_OK;
}

int rolo_ground_extract_patch(rolo_ground* g, double cx, double cy, double patch_size, const float* T16, float* out, int cap, int* m) {
  int rc = need_cloud(g, "rolo_ground_extract_patch");
  if (rc) return rc;
  if (!m || cap < 0 || (cap > 0 && !out)) { ctx_set_error("rolo_ground_extract_patch: bad argument"); return ROLO_EINVAL; }
  *m = 0;
  if (!(std::isfinite(cx) && std::isfinite(cy) && std::isfinite(patch_size))) { ctx_set_error("rolo_ground_extract_patch: a non-finite centre or size"); return ROLO_ENONFINITE; }
  HIPCHK(hipSetDevice(g->device));
  hipStream_t s = g->stream;
  const int n = g->n, stride = g->stride, nblk = (n + SM_THREADS - 1) / SM_THREADS;
  if ((rc = g->store.grow(g->bcnt, g->bcnt_cap, (size_t)nblk))) return rc;
  GpPatch P;
  const double half = patch_size * 0.5;
  P.xlo = (float)(cx - half); P.xhi = (float)(cx + half); P.ylo = (float)(cy - half); P.yhi = (float)(cy + half);
  P.has_T = T16 ? 1 : 0;
  for (int k = 0; k < 12; k++) P.T[k] = T16 ? T16[k] : 0.f;
  HIPCHK(hipEventRecord(g->ev[0], s));
  gp_patch_kernel<0><<<nblk, SM_THREADS, 0, s>>>(g->rec, n, stride, P, g->bcnt, nullptr);
  HIPCHK(hipGetLastError());
  scan_excl_kernel<<<1, 1024, 0, s>>>(g->bcnt, nblk, g->d_m, g->h_m);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s));
  const int kept = g->h_m[0];
  if (kept < 0 || kept > n) { ctx_set_error("rolo_ground_extract_patch: an inconsistent count"); return ROLO_ESTATE; }
  *m = kept;
  if (kept > cap) { ctx_set_error("rolo_ground_extract_patch: cap is smaller than the patch"); return ROLO_EINVAL; }
  if (kept > 0) {
    if ((rc = g->store.grow(g->patch, g->patch_cap, (size_t)kept * stride))) return rc;
    gp_patch_kernel<1><<<nblk, SM_THREADS, 0, s>>>(g->rec, n, stride, P, g->bcnt, g->patch);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(g->ev[1], s));
  if (kept > 0) HIPCHK(hipMemcpyAsync(out, g->patch, sizeof(float) * (size_t)kept * stride, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipEventElapsedTime(&g->ms[1], g->ev[0], g->ev[1]));
  return ROLO_OK;
}

int rolo_ground_last_ms(rolo_ground* g, float* ms3) {
  if (!g || !ms3) return ROLO_EINVAL;
  for (int k = 0; k < 3; k++) ms3[k] = g->ms[k];
  return ROLO_OK;
}

void rolo_priorpose_default_params(rolo_priorpose_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->n_wheels = 4;
  const double w[8] = {-3.0046, 0.7836, 0.8942, 0.7836, 0.8942, -0.7836, -3.0046, -0.7836};
  for (int k = 0; k < 8; k++) p->wheel_xy[k] = w[k];
  p->vehicle_com_z = 1.0;
  p->body_to_lidar_t[2] = 1.04;
  p->body_to_lidar_R[0] = p->body_to_lidar_R[4] = p->body_to_lidar_R[8] = 1.0;
  p->k_spring = 20.0; p->g = 1.0; p->max_iters = 50; p->lm_lambda = 0.01; p->tol_cost = 1.0e-12; p->tol_step = 1.0e-10;
  p->ground_avg_radius = 0.3; p->ground_min_neighbors = 5;
  p->fit_radius = 0.6; p->fit_outlier_factor = 3.0; p->fit_min_points = 15;
  p->z_min = -8.0; p->z_max = 8.0; p->roll_max = 0.5; p->pitch_max = 0.5; p->wheel_distance_max = 0.1;
}

int rolo_priorpose_solve(rolo_ground* g, const rolo_priorpose_params* params, const double* xyyaw, int B, rolo_priorpose_result* out) {
  int rc = need_cloud(g, "rolo_priorpose_solve");
  if (rc) return rc;
  if (!xyyaw || !out || B < 1 || B > ROLO_PRIOR_MAX_BATCH) { ctx_set_error("rolo_priorpose_solve: B outside 1 .. ROLO_PRIOR_MAX_BATCH, or a null array"); return ROLO_EINVAL; }
  GpParams P;
  if ((rc = params_to_device(params, &P))) return rc;
  if (!all_finite(xyyaw, 3 * B)) { ctx_set_error("rolo_priorpose_solve: a non-finite pose"); return ROLO_ENONFINITE; }
  HIPCHK(hipSetDevice(g->device));
  if ((rc = ensure_events(g))) return rc;
  if ((rc = stage_in(g, xyyaw, sizeof(double) * 3 * (size_t)B))) return rc;
  if ((rc = g->store.grow(g->d_out, g->d_out_cap, sizeof(rolo_priorpose_result) * (size_t)B))) return rc;
  HIPCHK(hipEventRecord(g->ev[0], g->stream));
  gp_solve_kernel<<<B, GP_THREADS, 0, g->stream>>>(grid_of(g), P, g->d_q, reinterpret_cast<rolo_priorpose_result*>(g->d_out));
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(g->ev[1], g->stream));
  HIPCHK(hipMemcpyAsync(out, g->d_out, sizeof(rolo_priorpose_result) * (size_t)B, hipMemcpyDeviceToHost, g->stream));
  HIPCHK(hipStreamSynchronize(g->stream));
  HIPCHK(hipEventElapsedTime(&g->ms[2], g->ev[0], g->ev[1]));
  return ROLO_OK;
}

int rolo_priorpose_fit_surface(rolo_ground* g, const rolo_priorpose_params* params, const double* xy, int nq, rolo_priorpose_fit* out) {
  int rc = need_cloud(g, "rolo_priorpose_fit_surface");
  if (rc) return rc;
  if (!xy || !out || nq < 1 || nq > ROLO_GROUND_MAX_QUERIES) { ctx_set_error("rolo_priorpose_fit_surface: bad argument"); return ROLO_EINVAL; }
  GpParams P;
  if ((rc = params_to_device(params, &P))) return rc;
  if (!all_finite(xy, 2 * nq)) { ctx_set_error("rolo_priorpose_fit_surface: a non-finite query"); return ROLO_ENONFINITE; }
  HIPCHK(hipSetDevice(g->device));
  if ((rc = stage_in(g, xy, sizeof(double) * 2 * (size_t)nq))) return rc;
  if ((rc = g->store.grow(g->d_out, g->d_out_cap, sizeof(rolo_priorpose_fit) * (size_t)nq))) return rc;
  gp_fit_kernel<<<nq, GP_THREADS, 0, g->stream>>>(grid_of(g), P, g->d_q, reinterpret_cast<rolo_priorpose_fit*>(g->d_out));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, g->d_out, sizeof(rolo_priorpose_fit) * (size_t)nq, hipMemcpyDeviceToHost, g->stream));
  HIPCHK(hipStreamSynchronize(g->stream));
  return ROLO_OK;
}

}  // extern "C"
