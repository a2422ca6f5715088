// Scan Context place recognition on gfx950 from the key map's resident key frames: the descriptor store (rolo_keymap_sc_add_*) and loop detection
// (rolo_keymap_sc_detect). Replaces (reference src/scancontext/Scancontext.cpp, include/scancontext/Scancontext.h) SCManager::makeScancontext :151-195 with
// xy2theta :23-36, makeRingkeyFromScancontext / makeSectorkeyFromScancontext :198-227, makeAndSaveScancontextAndKeys :236-250, and of detectLoopClosureID
// :253-344 the candidate search (:288-296, the vendored nanoflann L2 metric nanoflann.hpp:383-408), distanceBtnScanContext :116-148 with fastAlignUsingVkey
// :93-113 and distDirectSC :69-90, and the minimum over the candidates :302-317. Three kernels, and two single-workgroup launches that finish the second and the third:
//   sc_make_kernel       one workgroup per cloud: the bins in LDS as order-preserving unsigned encodings of the float z', reduced with an integer atomicMax (exact
//                        in any order); then, one lane per column / row, the column norms, the sector key and the ring key as SERIAL fp64 sums in index order
//   sc_ringkey_kernel    the float squared distance of the query's ring key to every searched key, accumulated in groups of four as nanoflann's metric writes it;
//                        each workgroup keeps its K smallest (distance, index) keys, sc_select_kernel (one workgroup) merges the partial lists
//   sc_distance_kernel   one workgroup per candidate, the query's matrix, column norms and sector key in LDS: the sector-key alignment over all shifts, then the
//                        column-wise cosine distance at every shift of the search window, parallel over (shift, column) — no sum is ever split
//   sc_best_kernel       the first strict minimum over the candidates, in candidate order
// Arithmetic per point (the reference's own expression types): z' = float(double(z) + LIDAR_HEIGHT); r = sqrtf(x * x + y * y) in float; dropped if double(r) >
// PC_MAX_RADIUS; ring = clamp(int(ceil(double(r) / PC_MAX_RADIUS * PC_NUM_RING)), 1, PC_NUM_RING); theta by xy2theta's four branches — the float quotient widened to
// double, atan in fp64, (180 / M_PI) * and the branch's 180 - / 180 + / 360 - in fp64, rounded once to float — and sector = clamp(int(ceil(double(theta) / 360.0 *
// PC_NUM_SECTOR)), 1, PC_NUM_SECTOR), a NaN angle (the origin) giving sector 1 as x86's int(NaN) = INT_MIN does after the clamp. atan is the correctly rounded
// ddx::atan2_cr(q, 1.0) of polar_exact.hpp wherever the float rounding of theta could depend on it (sc_theta), the device's own atan elsewhere. The float
// products, the sum, the root and the quotient are formed in fp64 and rounded to float: for these four operations that is the correctly rounded float result
// (53 >= 2 * 24 + 2 bits), whatever the device's float division does. (A product below the smallest normal float still passes through the narrowing's denormal
// handling; it can only move r within ring 1.)
// Parity unpinned: the order in which Eigen's norm(), mean() and dot() add (here: serial, index 0 upward); the order in which the kd-tree returns equal distances
// (here: lower index first); which atan overload the reference's build selects for the float quotient (here: double). The parity target of the tests is the numpy
// statement tests/sc_twin.py, written from the reference's text.
#pragma STDC FP_CONTRACT OFF
#include "keymap.hpp"
#include "polar_exact.hpp"
#include <algorithm>
#include <cmath>
#include <vector>

namespace rolo {
namespace {

typedef unsigned long long u64;

constexpr int SC_THREADS = 256;
constexpr int SC_MAKE_THREADS = 1024;                  // one workgroup per cloud: all the lanes a workgroup can have
constexpr int SC_MAX_BINS = ROLO_SC_MAX_BINS;         // num_ring * num_sector: the bins (16 KiB) share a workgroup's LDS with the distance kernel's columns
constexpr int SC_MAX_SECTORS = ROLO_SC_MAX_SECTORS;
constexpr int SC_MAX_CAND = ROLO_SC_MAX_CANDIDATES;
constexpr int SC_RK_BLOCKS = 64;                      // partial candidate lists
constexpr int SC_SIMS = 2048;                         // (shift, column) similarities one round of the distance kernel holds
constexpr double SC_FAR = 10000000.0;                 // "init with something large" :96, :134, :284

struct ScGeom { int R, S; double max_radius, lidar_height; };
struct ScBest { double min_dist; int nn_idx, nn_align, pos, pad; };

__device__ __forceinline__ unsigned sc_enc(float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }   // > 0 for every non-NaN float
__device__ __forceinline__ float sc_dec(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e ^ 0x80000000u) : ~e); }
__device__ __forceinline__ float sc_div_f(float a, float b) { return (float)((double)a / (double)b); }

// xy2theta :23-36. The branch's fp64 expression is evaluated on the device's atan first. That atan is a few ulp from the correctly rounded one, which moves
// the fp64 angle by less than 1e-12 degrees; if the angle -+ SC_THETA_GUARD rounds to one float, so does the correctly rounded angle (rounding is monotonic)
// and that float is the result. Otherwise (about one point in 10^4, and a NaN angle) the expression is evaluated again on ddx::atan2_cr(q, 1.0).
constexpr double SC_THETA_GUARD = 1e-10;
template <bool EXACT>
__device__ __forceinline__ double sc_theta_d(float x, float y) {
  const double K = 180.0 / M_PI;
  int branch; float q;
  if ((x >= 0.f) & (y >= 0.f)) { branch = 0; q = sc_div_f(y, x); }
  else if ((x < 0.f) & (y >= 0.f)) { branch = 1; q = sc_div_f(y, -x); }
  else if ((x < 0.f) & (y < 0.f)) { branch = 2; q = sc_div_f(y, x); }
  else { branch = 3; q = sc_div_f(-y, x); }
  const double a = EXACT ? ddx::atan2_cr((double)q, 1.0) : atan((double)q);
  const double ka = K * a;
  return branch == 0 ? ka : branch == 1 ? 180.0 - ka : branch == 2 ? 180.0 + ka : 360.0 - ka;
}
__device__ float sc_theta(float x, float y) {
  const double t = sc_theta_d<false>(x, y);
  const float lo = (float)(t - SC_THETA_GUARD), hi = (float)(t + SC_THETA_GUARD);
  if (lo == hi) return lo;
  return (float)sc_theta_d<true>(x, y);
}

__device__ __forceinline__ int sc_clamp_ceil(double v, int hi) {
  if (!(v == v)) return 1;
  const double c = ceil(v);
  if (c >= (double)hi) return hi;
  if (c <= 1.0) return 1;
  return (int)c;
}

// makeScancontext :151-195 and both keys :198-227 of one cloud; desc[s * R + r] (each sector's rings contiguous). *flag = 1 and nothing else written if a coordinate is not finite
__global__ __launch_bounds__(SC_MAKE_THREADS) void sc_make_kernel(const float4* __restrict__ pts, int n, ScGeom G, float* __restrict__ desc, double* __restrict__ colnorm,
                                                             double* __restrict__ seckey, float* __restrict__ ringkey, int* __restrict__ flag) {
  __shared__ unsigned bins[SC_MAX_BINS];
  __shared__ int bad;
  const int nb = G.R * G.S;   // <= SC_MAX_BINS (rolo_keymap_sc_set_params)
  for (int i = threadIdx.x; i < nb; i += SC_MAKE_THREADS) bins[i] = 0u;   // below every encoding: "no point"
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += SC_MAKE_THREADS) {
    const float4 p = pts[i];
    if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) { bad = 1; continue; }
    const float zf = (float)((double)p.z + G.lidar_height);                                   // :168
    const float xx = (float)((double)p.x * (double)p.x), yy = (float)((double)p.y * (double)p.y);
    const float r = (float)sqrt((double)(float)((double)xx + (double)yy));                     // :171
    const float th = sc_theta(p.x, p.y);                                                       // :172
    if ((double)r > G.max_radius) continue;                                                    // :175
    const int ring = sc_clamp_ceil(((double)r / G.max_radius) * (double)G.R, G.R);             // :178
    const int sector = sc_clamp_ceil(((double)th / 360.0) * (double)G.S, G.S);                 // :179
    atomicMax(&bins[(sector - 1) * G.R + (ring - 1)], sc_enc(zf));                             // :182-183
  }
  __syncthreads();
  if (bad) { if (threadIdx.x == 0) *flag = 1; return; }
  float* vals = reinterpret_cast<float*>(bins);
  for (int i = threadIdx.x; i < nb; i += SC_MAKE_THREADS) {   // NO_POINT :158-190: a bin keeps its maximum only if that exceeds -1000
    const unsigned e = bins[i];
    float v = 0.f;
    if (e) { const float z = sc_dec(e); if (z > -1000.f) v = z; }
    if (v == 0.f) v = 0.f;   // a zero maximum is +0.0
    vals[i] = v;
    desc[i] = v;
  }
  __syncthreads();
  for (int s = threadIdx.x; s < G.S; s += SC_MAKE_THREADS) {
    double ss = 0.0, sum = 0.0;
    for (int r = 0; r < G.R; r++) { const double v = (double)vals[s * G.R + r]; ss = ss + v * v; sum = sum + v; }
    colnorm[s] = sqrt(ss);
    seckey[s] = sum / (double)G.R;          // :222-223
  }
  for (int r = threadIdx.x; r < G.R; r += SC_MAKE_THREADS) {
    double sum = 0.0;
    for (int s = 0; s < G.S; s++) sum = sum + (double)vals[s * G.R + r];
    ringkey[r] = (float)(sum / (double)G.S);   // :206-207, eig2stdvec :62-66
  }
  if (threadIdx.x == 0) *flag = 0;
}

__device__ __forceinline__ u64 sc_shfl_xor_u64(u64 v, int off) {
  const unsigned lo = __shfl_xor((unsigned)(v & 0xffffffffull), off, 64), hi = __shfl_xor((unsigned)(v >> 32), off, 64);
  return ((u64)hi << 32) | lo;
}

// the K smallest of keys[start + threadIdx.x + j * stride] (< n), ascending, to out[0 .. K); ~0 where there are fewer. Keys are unique (the index is in them).
__device__ void sc_select_k(const u64* keys, int n, int start, int stride, int K, u64* out) {
  __shared__ u64 wmin[SC_THREADS / 64];
  u64 lo = 0;
  for (int k = 0; k < K; k++) {
    u64 best = ~0ull;
    for (long long i = (long long)start + threadIdx.x; i < n; i += stride) { const u64 key = keys[i]; if (key >= lo && key < best) best = key; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const u64 o = sc_shfl_xor_u64(best, off); if (o < best) best = o; }
    __syncthreads();   // wmin of the previous round has been read
    if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = best;
    __syncthreads();
    u64 m = wmin[0];
#pragma unroll
    for (int w = 1; w < SC_THREADS / 64; w++) if (wmin[w] < m) m = wmin[w];
    if (threadIdx.x == 0) out[k] = m;
    lo = m == ~0ull ? m : m + 1;
  }
}

// keys[i] = (bits of the float squared distance : 32 | i : 32) for i < n_search (a non-negative float's bits order as the float does); part[block * K + k]
__global__ __launch_bounds__(SC_THREADS) void sc_ringkey_kernel(const float* __restrict__ ringkeys, int R, int query, int n_search, int K, u64* __restrict__ keys,
                                                                u64* __restrict__ part) {
  __shared__ float q[SC_MAX_BINS];
  for (int d = threadIdx.x; d < R; d += SC_THREADS) q[d] = ringkeys[(size_t)query * R + d];
  __syncthreads();
  const int start = blockIdx.x * SC_THREADS, stride = gridDim.x * SC_THREADS;
  for (long long i = (long long)start + threadIdx.x; i < n_search; i += stride) {
    const float* b = ringkeys + (size_t)i * R;
    float result = 0.f;
    int d = 0;
    for (; d + 3 < R; d += 4) {   // nanoflann.hpp:391-397
      const float d0 = q[d] - b[d], d1 = q[d + 1] - b[d + 1], d2 = q[d + 2] - b[d + 2], d3 = q[d + 3] - b[d + 3];
      result += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    }
    for (; d < R; d++) { const float d0 = q[d] - b[d]; result += d0 * d0; }   // :403-406
    keys[i] = ((u64)__float_as_uint(result) << 32) | (u64)(unsigned)i;
  }
  // each thread re-reads only what it wrote itself
  sc_select_k(keys, n_search, start, stride, K, part + (size_t)blockIdx.x * K);
}

__global__ __launch_bounds__(SC_THREADS) void sc_select_kernel(const u64* __restrict__ part, int nparts, int K, u64* __restrict__ sel) {
  sc_select_k(part, nparts, 0, SC_THREADS, K, sel);
}

// distanceBtnScanContext(query, candidate) :116-148 -> out_dist[c], out_align[c]; candidate c is descriptor sel[c] (low word), or c itself without a list
__global__ __launch_bounds__(SC_THREADS) void sc_distance_kernel(const float* __restrict__ desc, const double* __restrict__ colnorm, const double* __restrict__ seckey, int R, int S,
                                                                 int query, const u64* __restrict__ sel, int radius, double* __restrict__ out_dist, int* __restrict__ out_align) {
  __shared__ float qm[SC_MAX_BINS];
  __shared__ double qn[SC_MAX_SECTORS], qk[SC_MAX_SECTORS];
  __shared__ double sims[SC_SIMS];
  __shared__ double cdist[SC_THREADS];
  __shared__ int wlist[SC_MAX_SECTORS];
  __shared__ unsigned char valid[SC_SIMS];
  __shared__ double s_min;
  __shared__ int s_align, s_nw;
  const int c = blockIdx.x, tid = threadIdx.x;
  const int cand = sel ? (int)(sel[c] & 0xffffffffull) : c;
  const float* cm = desc + (size_t)cand * R * S;
  const double* cn = colnorm + (size_t)cand * S;
  const double* ck = seckey + (size_t)cand * S;
  for (int i = tid; i < R * S; i += SC_THREADS) qm[i] = desc[(size_t)query * R * S + i];
  for (int j = tid; j < S; j += SC_THREADS) { qn[j] = colnorm[(size_t)query * S + j]; qk[j] = seckey[(size_t)query * S + j]; }
  __syncthreads();
  // fastAlignUsingVkey :93-113: circshift(vkey2, s)[j] = vkey2[(j - s) mod S] (:39-59)
  for (int s = tid; s < S; s += SC_THREADS) {
    double acc = 0.0;
    for (int j = 0; j < S; j++) { int jj = j - s; if (jj < 0) jj += S; const double d = qk[j] - ck[jj]; acc = acc + d * d; }
    sims[s] = sqrt(acc);
  }
  __syncthreads();
  if (tid == 0) {
    int a = 0; double mn = SC_FAR;
    for (int s = 0; s < S; s++) if (sims[s] < mn) { a = s; mn = sims[s]; }
    int nw = 0;   // :123-130: a and radius shifts either side, modulo S, ascending, each once
    for (int s = 0; s < S; s++) { int d1 = s - a; if (d1 < 0) d1 += S; const int d2 = S - d1; if ((d1 < d2 ? d1 : d2) <= radius) wlist[nw++] = s; }
    s_nw = nw; s_min = SC_FAR; s_align = 0;
  }
  __syncthreads();
  const int nw = s_nw;
  const int chunk = SC_SIMS / S < SC_THREADS ? SC_SIMS / S : SC_THREADS;   // >= 2: S <= SC_MAX_SECTORS
  for (int w0 = 0; w0 < nw; w0 += chunk) {
    const int cw = nw - w0 < chunk ? nw - w0 : chunk;
    for (int it = tid; it < cw * S; it += SC_THREADS) {   // distDirectSC :69-90, one (shift, column) each
      const int wi = it / S, j = it - wi * S;
      int jj = j - wlist[w0 + wi]; if (jj < 0) jj += S;
      const double n1 = qn[j], n2 = cn[jj];
      if ((n1 == 0.0) | (n2 == 0.0)) { valid[it] = 0; continue; }
      const float* a = qm + j * R;
      const float* b = cm + (size_t)jj * R;
      double dot = 0.0;
      for (int r = 0; r < R; r++) dot = dot + (double)a[r] * (double)b[r];
      sims[it] = dot / (n1 * n2);
      valid[it] = 1;
    }
    __syncthreads();
    if (tid < cw) {
      double sum = 0.0; int cnt = 0;
      for (int j = 0; j < S; j++) if (valid[tid * S + j]) { sum = sum + sims[tid * S + j]; cnt = cnt + 1; }
      cdist[tid] = 1.0 - sum / (double)cnt;   // no counted column: 0 / 0 = NaN, never below the minimum
    }
    __syncthreads();
    if (tid == 0) for (int wi = 0; wi < cw; wi++) if (cdist[wi] < s_min) { s_min = cdist[wi]; s_align = wlist[w0 + wi]; }
    __syncthreads();
  }
  if (tid == 0) { out_dist[c] = s_min; out_align[c] = s_align; }
}

// :302-317 over n candidates in candidate order with strict <: contiguous slices per thread, then the slices in order
__global__ __launch_bounds__(SC_THREADS) void sc_best_kernel(const double* __restrict__ dist, const int* __restrict__ align, const u64* __restrict__ sel, int n, ScBest* __restrict__ out) {
  __shared__ double bd[SC_THREADS];
  __shared__ int bi[SC_THREADS];
  const int per = (n + SC_THREADS - 1) / SC_THREADS;
  const long long lo = (long long)threadIdx.x * per;
  const int hi = (int)(lo + per < n ? lo + per : n);
  double d = SC_FAR; int b = -1;
  for (int i = (int)(lo < n ? lo : n); i < hi; i++) if (dist[i] < d) { d = dist[i]; b = i; }
  bd[threadIdx.x] = d; bi[threadIdx.x] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    double g = SC_FAR; int gi = -1;
    for (int t = 0; t < SC_THREADS; t++) if (bd[t] < g) { g = bd[t]; gi = bi[t]; }
    ScBest o;
    o.min_dist = g; o.pos = gi; o.pad = 0;
    o.nn_idx = gi < 0 ? 0 : (sel ? (int)(sel[gi] & 0xffffffffull) : gi);
    o.nn_align = gi < 0 ? 0 : align[gi];
    *out = o;
  }
}

}  // namespace

struct ScStore {
  rolo_sc_params P;
  int n = 0;
  size_t cap = 0;                    // descriptors the four arrays hold
  float* desc = nullptr; double* colnorm = nullptr; double* seckey = nullptr; float* ringkey = nullptr;
  u64* keys = nullptr; size_t keys_cap = 0;
  u64* part = nullptr; size_t part_cap = 0;      // [SC_RK_BLOCKS][K], then the merged list [K]
  double* cdist = nullptr; size_t cdist_cap = 0;
  int* calign = nullptr; size_t calign_cap = 0;
  int* h_flag = nullptr;             // pinned
  ScBest* h_best = nullptr;          // pinned
  hipEvent_t t0 = nullptr, t1 = nullptr;
  float last_ms = 0.f;
};

void sc_store_destroy(ScStore* sc) {   // (every buffer is the key map's store's)
  if (!sc) return;
  if (sc->t0) (void)hipEventDestroy(sc->t0);
  if (sc->t1) (void)hipEventDestroy(sc->t1);
  delete sc;
}

namespace {

void sc_defaults(rolo_sc_params* p) {   // Scancontext.h:80-95
  p->num_ring = 20; p->num_sector = 60; p->max_radius = 80.0; p->lidar_height = 2.0;
  p->num_exclude_recent = 30; p->num_candidates = 3; p->search_ratio = 0.1; p->dist_thres = 0.4;
}

int sc_store(rolo_keymap* km, ScStore** out) {
  if (!km->sc) {
    HIPCHK(hipSetDevice(km->device));
    ScStore* sc = new ScStore();
    sc_defaults(&sc->P);
    int rc = km->store.alloc_pinned(sc->h_flag, 1);
    if (!rc) rc = km->store.alloc_pinned(sc->h_best, 1);
    if (rc) { sc_store_destroy(sc); return rc; }
    hipError_t e = hipEventCreate(&sc->t0);
    if (e == hipSuccess) e = hipEventCreate(&sc->t1);
    if (e != hipSuccess) { ctx_set_error((std::string("rolo_keymap_sc: ") + hipGetErrorString(e)).c_str()); sc_store_destroy(sc); return ROLO_EHIP; }
    km->sc = sc;
  }
  *out = km->sc;
  return ROLO_OK;
}

// room for one more descriptor: four larger arrays (sc->cap counts descriptors, so the sizes are given outright), the stored descriptors copied on the key map's
// stream
int sc_reserve(rolo_keymap* km, ScStore* sc) {
  if ((size_t)sc->n < sc->cap) return ROLO_OK;
  const size_t want = sc->cap + sc->cap / 2 + 64;
  const size_t R = (size_t)sc->P.num_ring, S = (size_t)sc->P.num_sector, n = (size_t)sc->n;
  int rc;
  if ((rc = km->store.alloc(sc->desc, want * R * S, n * R * S))) return rc;
  if ((rc = km->store.alloc(sc->colnorm, want * S, n * S))) return rc;
  if ((rc = km->store.alloc(sc->seckey, want * S, n * S))) return rc;
  if ((rc = km->store.alloc(sc->ringkey, want * R, n * R))) return rc;
  sc->cap = want;
  return ROLO_OK;
}

// the descriptor of a device cloud into slot sc->n; counted only when every coordinate was finite
int sc_add_device(rolo_keymap* km, ScStore* sc, const float4* d_pts, int n) {
  int rc;
  if ((rc = sc_reserve(km, sc))) return rc;
  const size_t R = (size_t)sc->P.num_ring, S = (size_t)sc->P.num_sector, i = (size_t)sc->n;
  const ScGeom G{sc->P.num_ring, sc->P.num_sector, sc->P.max_radius, sc->P.lidar_height};
  sc_make_kernel<<<1, SC_MAKE_THREADS, 0, km->stream>>>(d_pts, n, G, sc->desc + i * R * S, sc->colnorm + i * S, sc->seckey + i * S, sc->ringkey + i * R, sc->h_flag);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(sc->t1, km->stream));
  HIPCHK(hipStreamSynchronize(km->stream));
  (void)hipEventElapsedTime(&sc->last_ms, sc->t0, sc->t1);
  if (*sc->h_flag != 0) { ctx_set_error("a non-finite coordinate reached the Scan Context descriptor"); return ROLO_ENONFINITE; }
  return sc->n++;
}

}  // namespace

// for mapper.hip: the reservation ahead of a key frame, and the descriptor of a cloud that is resident already (the scan's surface cloud, or the filtered raw cloud)
int keymap_sc_reserve(rolo_keymap* km) {
  ScStore* sc;
  if (const int rc = sc_store(km, &sc)) return rc;
  HIPCHK(hipSetDevice(km->device));
  return sc_reserve(km, sc);
}
int keymap_sc_add_resident(rolo_keymap* km, const float4* d_pts, int n) {
  if (n <= 0) { ctx_set_error("Scan Context: empty cloud"); return ROLO_EINVAL; }
  ScStore* sc;
  if (const int rc = sc_store(km, &sc)) return rc;
  HIPCHK(hipSetDevice(km->device));
  HIPCHK(hipEventRecord(sc->t0, km->stream));
  return sc_add_device(km, sc, d_pts, n);
}
}  // namespace rolo

using namespace rolo;

extern "C" {

void rolo_sc_default_params(rolo_sc_params* p) { if (p) sc_defaults(p); }

int rolo_keymap_sc_set_params(rolo_keymap* km, const rolo_sc_params* p) {
  if (!km || !p) return ROLO_EINVAL;
  if (p->num_ring < 1 || p->num_sector < 1 || p->num_sector > SC_MAX_SECTORS || (long long)p->num_ring * p->num_sector > SC_MAX_BINS) {
    ctx_set_error("rolo_keymap_sc_set_params: num_ring * num_sector above ROLO_SC_MAX_BINS or num_sector above ROLO_SC_MAX_SECTORS");
    return ROLO_EINVAL;
  }
  if (p->num_candidates < 0 || p->num_candidates > SC_MAX_CAND) { ctx_set_error("rolo_keymap_sc_set_params: num_candidates above ROLO_SC_MAX_CANDIDATES"); return ROLO_EINVAL; }
  if (!(p->max_radius > 0.0) || !std::isfinite(p->max_radius) || !std::isfinite(p->lidar_height) || !(p->search_ratio >= 0.0) || !std::isfinite(p->search_ratio) ||
      p->num_exclude_recent < 0 || p->dist_thres != p->dist_thres)
    return ROLO_EINVAL;
  ScStore* sc;
  int rc;
  if ((rc = sc_store(km, &sc))) return rc;
  if (sc->n > 0 && (p->num_ring != sc->P.num_ring || p->num_sector != sc->P.num_sector || p->max_radius != sc->P.max_radius || p->lidar_height != sc->P.lidar_height)) {
    ctx_set_error("rolo_keymap_sc_set_params: the descriptor geometry is fixed once a descriptor is stored");
    return ROLO_ESTATE;
  }
  if (sc->cap > 0 && (p->num_ring != sc->P.num_ring || p->num_sector != sc->P.num_sector)) {
    // no descriptor is stored, but an add that failed (a non-finite coordinate) has already sized the arrays for the old geometry: the next add allocates anew (the store frees these with the rest)
    sc->desc = nullptr; sc->colnorm = nullptr; sc->seckey = nullptr; sc->ringkey = nullptr;
    sc->cap = 0;
  }
  sc->P = *p;
  return ROLO_OK;
}

int rolo_keymap_sc_get_params(rolo_keymap* km, rolo_sc_params* out) {
  if (!km || !out) return ROLO_EINVAL;
  if (km->sc) *out = km->sc->P; else sc_defaults(out);
  return ROLO_OK;
}

int rolo_keymap_sc_add_surface(rolo_keymap* km, int keyframe) {
  if (!km || keyframe < 0 || keyframe >= (int)km->frames.size()) return ROLO_EINVAL;
  const rolo_keymap::Frame& f = km->frames[keyframe];
  if (f.n[1] <= 0) { ctx_set_error("rolo_keymap_sc_add_surface: the key frame's surface cloud is empty"); return ROLO_EINVAL; }
  ScStore* sc;
  int rc;
  if ((rc = sc_store(km, &sc))) return rc;
  HIPCHK(hipSetDevice(km->device));
  HIPCHK(hipEventRecord(sc->t0, km->stream));
  return sc_add_device(km, sc, f.pts[1], f.n[1]);
}

int rolo_keymap_sc_add_cloud(rolo_keymap* km, const float* pts, int n, float leaf) {
  if (!km || n < 0 || (n && !pts) || !(leaf >= 0.f) || n > ROLO_KEYMAP_MAX_POINTS) return ROLO_EINVAL;
  if (n == 0) { ctx_set_error("rolo_keymap_sc_add_cloud: empty cloud"); return ROLO_EINVAL; }
  ScStore* sc;
  int rc;
  if ((rc = sc_store(km, &sc))) return rc;
  HIPCHK(hipSetDevice(km->device));
  HIPCHK(hipEventRecord(sc->t0, km->stream));
  const float4* d = nullptr; int m = 0;
  if ((rc = keymap_stage_cloud(km, pts, n, leaf, &d, &m))) return rc;
  if (m <= 0) { ctx_set_error("rolo_keymap_sc_add_cloud: empty cloud"); return ROLO_EINVAL; }
  return sc_add_device(km, sc, d, m);
}

int rolo_keymap_sc_size(rolo_keymap* km) { return km ? (km->sc ? km->sc->n : 0) : ROLO_EINVAL; }

int rolo_keymap_sc_get(rolo_keymap* km, int index, double* desc, float* ringkey, double* sectorkey, double* colnorm) {
  if (!km || !km->sc || index < 0 || index >= km->sc->n) return ROLO_EINVAL;
  ScStore* sc = km->sc;
  const size_t R = (size_t)sc->P.num_ring, S = (size_t)sc->P.num_sector, i = (size_t)index;
  HIPCHK(hipSetDevice(km->device));
  std::vector<float> m(desc ? R * S : 0);
  if (desc) HIPCHK(hipMemcpyAsync(m.data(), sc->desc + i * R * S, sizeof(float) * R * S, hipMemcpyDeviceToHost, km->stream));
  if (ringkey) HIPCHK(hipMemcpyAsync(ringkey, sc->ringkey + i * R, sizeof(float) * R, hipMemcpyDeviceToHost, km->stream));
  if (sectorkey) HIPCHK(hipMemcpyAsync(sectorkey, sc->seckey + i * S, sizeof(double) * S, hipMemcpyDeviceToHost, km->stream));
  if (colnorm) HIPCHK(hipMemcpyAsync(colnorm, sc->colnorm + i * S, sizeof(double) * S, hipMemcpyDeviceToHost, km->stream));
  HIPCHK(hipStreamSynchronize(km->stream));
  if (desc) for (size_t r = 0; r < R; r++) for (size_t s = 0; s < S; s++) desc[r * S + s] = (double)m[s * R + r];
  return ROLO_OK;
}

float rolo_keymap_sc_last_ms(rolo_keymap* km) { return km && km->sc ? km->sc->last_ms : 0.f; }

int rolo_keymap_sc_detect(rolo_keymap* km, int query, int n_search, rolo_sc_result* out, int32_t* cand_idx, double* cand_dist, int32_t* cand_align, int cap) {
  if (!km || !out || !km->sc || query < 0 || query >= km->sc->n || n_search > km->sc->n || cap < 0) return ROLO_EINVAL;
  ScStore* sc = km->sc;
  out->loop_id = -1; out->yaw_diff_rad = 0.f; out->nn_idx = 0; out->nn_align = 0; out->min_dist = SC_FAR; out->n_candidates = 0;
  if (n_search <= 0) return ROLO_OK;   // :263-267
  HIPCHK(hipSetDevice(km->device));
  hipStream_t s = km->stream;
  const int R = sc->P.num_ring, S = sc->P.num_sector, K = sc->P.num_candidates;
  const int ncand = K > 0 ? std::min(K, n_search) : n_search;
  const int radius = (int)std::min<double>(std::round(0.5 * sc->P.search_ratio * (double)S), (double)S);   // :123
  int rc;
  if ((rc = km->store.grow(sc->cdist, sc->cdist_cap, (size_t)ncand))) return rc;
  if ((rc = km->store.grow(sc->calign, sc->calign_cap, (size_t)ncand))) return rc;
  HIPCHK(hipEventRecord(sc->t0, s));
  const u64* sel = nullptr;
  if (K > 0) {
    const int blocks = std::min((n_search + SC_THREADS - 1) / SC_THREADS, SC_RK_BLOCKS);
    if ((rc = km->store.grow(sc->keys, sc->keys_cap, (size_t)n_search))) return rc;
    if ((rc = km->store.grow(sc->part, sc->part_cap, (size_t)(SC_RK_BLOCKS + 1) * SC_MAX_CAND))) return rc;
    u64* merged = sc->part + (size_t)SC_RK_BLOCKS * SC_MAX_CAND;
    sc_ringkey_kernel<<<blocks, SC_THREADS, 0, s>>>(sc->ringkey, R, query, n_search, ncand, sc->keys, sc->part);
    HIPCHK(hipGetLastError());
    sc_select_kernel<<<1, SC_THREADS, 0, s>>>(sc->part, blocks * ncand, ncand, merged);
    HIPCHK(hipGetLastError());
    sel = merged;
  }
  sc_distance_kernel<<<ncand, SC_THREADS, 0, s>>>(sc->desc, sc->colnorm, sc->seckey, R, S, query, sel, radius, sc->cdist, sc->calign);
  HIPCHK(hipGetLastError());
  sc_best_kernel<<<1, SC_THREADS, 0, s>>>(sc->cdist, sc->calign, sel, ncand, sc->h_best);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(sc->t1, s));
  HIPCHK(hipStreamSynchronize(s));
  (void)hipEventElapsedTime(&sc->last_ms, sc->t0, sc->t1);
  const ScBest b = *sc->h_best;
  out->nn_idx = b.nn_idx; out->nn_align = b.nn_align; out->min_dist = b.min_dist; out->n_candidates = ncand;
  if (b.min_dist < sc->P.dist_thres) out->loop_id = b.nn_idx;   // :323-326
  // :339 deg2rad(nn_align * PC_UNIT_SECTORANGLE): the double product narrowed to deg2rad's float parameter, then degrees * M_PI / 180.0 in double, returned as float (:17-20)
  const float degrees = (float)((double)b.nn_align * (360.0 / (double)S));
  out->yaw_diff_rad = (float)((double)degrees * M_PI / 180.0);
  const int m = std::min(ncand, cap);
  if (m > 0) {
    if (cand_idx) {
      if (sel) {
        std::vector<u64> h((size_t)m);
        HIPCHK(hipMemcpy(h.data(), sel, sizeof(u64) * (size_t)m, hipMemcpyDeviceToHost));
        for (int i = 0; i < m; i++) cand_idx[i] = (int32_t)(h[(size_t)i] & 0xffffffffull);
      } else {
        for (int i = 0; i < m; i++) cand_idx[i] = i;
      }
    }
    if (cand_dist) HIPCHK(hipMemcpy(cand_dist, sc->cdist, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost));
    if (cand_align) HIPCHK(hipMemcpy(cand_align, sc->calign, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost));
  }
  return ROLO_OK;
}

}  // extern "C"
