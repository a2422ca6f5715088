// Device kernels shared by the units that bin points into grid cells: submap.hip (pcl::VoxelGrid's cells) and groundprior.hip (the ground model's x-y grid).
// The box of a cloud, the stable LSD radix sort of (cell, point index), the one-workgroup exclusive scan and the lower bound in a sorted array. Each unit that
// includes this gets its own copy (unnamed namespace); the units are built without contraction. Behind the kernels, the host's one rule for launching them:
// the sort's scratch and pass loop (SortScratch), the key width for a number of cells, the box pass.
#pragma once
#include "ctx_access.hpp"
#include "dev_math.hpp"
#include <algorithm>
#include <cfloat>

namespace rolo {
namespace {

constexpr int SM_THREADS = 256;
constexpr int SORT_ITEMS = 16;                         // keys per lane of a sort tile
constexpr int SORT_TILE = SM_THREADS * SORT_ITEMS;     // 4096 keys per workgroup, 1024 per wavefront
constexpr int BOX_BLOCKS_MAX = 1024;

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// min / max of x, y, z and "a coordinate is not finite", per workgroup: part[8 * block + (0..2 min, 3..5 max, 6 flag)]
__global__ __launch_bounds__(SM_THREADS) void vg_box_kernel(const float4* __restrict__ pts, int n, float* __restrict__ part) {
  __shared__ float red[SM_THREADS / 64][8];
  float v[7] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX, 0.f};
  for (int i = blockIdx.x * SM_THREADS + threadIdx.x; i < n; i += gridDim.x * SM_THREADS) {
    const float4 p = pts[i];
    if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) v[6] = 1.f;
    v[0] = fminf(v[0], p.x); v[1] = fminf(v[1], p.y); v[2] = fminf(v[2], p.z);
    v[3] = fmaxf(v[3], p.x); v[4] = fmaxf(v[4], p.y); v[5] = fmaxf(v[5], p.z);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 7; k++) { const float r = k < 3 ? wave_min(v[k]) : wave_max(v[k]); if (lane == 0) red[wv][k] = r; }
  __syncthreads();
  if (threadIdx.x < 7) {
    const int k = threadIdx.x;
    float r = red[0][k];
    for (int w = 1; w < SM_THREADS / 64; w++) r = k < 3 ? fminf(r, red[w][k]) : fmaxf(r, red[w][k]);
    part[8 * (size_t)blockIdx.x + k] = r;
  }
}
// the workgroups' rows -> out[0..6] (pinned host memory)
__global__ __launch_bounds__(SM_THREADS) void vg_box_final_kernel(const float* __restrict__ part, int nparts, float* __restrict__ out) {
  __shared__ float red[SM_THREADS / 64][8];
  float v[7] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX, 0.f};
  for (int b = threadIdx.x; b < nparts; b += SM_THREADS) {
#pragma unroll
    for (int k = 0; k < 7; k++) { const float x = part[8 * (size_t)b + k]; v[k] = k < 3 ? fminf(v[k], x) : fmaxf(v[k], x); }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 7; k++) { const float r = k < 3 ? wave_min(v[k]) : wave_max(v[k]); if (lane == 0) red[wv][k] = r; }
  __syncthreads();
  if (threadIdx.x < 7) {
    const int k = threadIdx.x;
    float r = red[0][k];
    for (int w = 1; w < SM_THREADS / 64; w++) r = k < 3 ? fminf(r, red[w][k]) : fmaxf(r, red[w][k]);
    out[k] = r;
  }
}

// ---- stable LSD radix sort of (cell, point index), 8 bits per pass ---------------------------------------------------------------------------------------
// digit counts of every tile: hist[digit * nblocks + block] (digit-major: its exclusive scan is where each tile's keys of each digit go)
__global__ __launch_bounds__(SM_THREADS) void sort_hist_kernel(const unsigned* __restrict__ keys, int n, int shift, unsigned* __restrict__ hist, int nblocks,
                                                               unsigned* __restrict__ dtot /* 256, zeroed: keys per digit */) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int base = blockIdx.x * SORT_TILE;
#pragma unroll
  for (int k = 0; k < SORT_ITEMS; k++) {
    const int i = base + k * SM_THREADS + threadIdx.x;
    if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);   // integer counts: exact in any order
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];
  if (h[threadIdx.x]) atomicAdd(&dtot[threadIdx.x], h[threadIdx.x]);
}

// exclusive scan of the digit-major table, one workgroup per digit: the keys of the digits below (dtot), then along the digit's row of tile counts
__global__ __launch_bounds__(SM_THREADS) void sort_scan_kernel(unsigned* __restrict__ hist, int nblocks, const unsigned* __restrict__ dtot) {
  __shared__ unsigned wsum[SM_THREADS / 64];
  const int d = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  auto block_incl = [&](unsigned x, unsigned& total) {   // inclusive scan over the workgroup
    unsigned incl = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const unsigned o = __shfl_up(incl, off, 64); if (lane >= off) incl += o; }
    __syncthreads();   // wsum of the previous use has been read
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    unsigned before = 0; total = 0;
#pragma unroll
    for (int w = 0; w < SM_THREADS / 64; w++) { const unsigned t = wsum[w]; if (w < wv) before += t; total += t; }
    return before + incl;
  };
  unsigned running;
  block_incl((int)threadIdx.x < d ? dtot[threadIdx.x] : 0u, running);
  unsigned* row = hist + (size_t)d * nblocks;
  for (int b0 = 0; b0 < nblocks; b0 += SM_THREADS) {
    const int i = b0 + threadIdx.x;
    const unsigned x = i < nblocks ? row[i] : 0u;
    unsigned total;
    const unsigned incl = block_incl(x, total);
    if (i < nblocks) row[i] = running + incl - x;
    running += total;
  }
}

// exclusive scan of a[0 .. N) in place by ONE workgroup; the total goes to total_dev / total_host when given
__global__ __launch_bounds__(1024) void scan_excl_kernel(unsigned* __restrict__ a, int N, int* __restrict__ total_dev, int* __restrict__ total_host) {
  __shared__ unsigned wsum[16];
  const int chunk = (N + 1023) / 1024;
  const int lo = min((int)threadIdx.x * chunk, N), hi = min(lo + chunk, N);
  unsigned s = 0;
  for (int i = lo; i < hi; i++) s += a[i];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned incl = s;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const unsigned o = __shfl_up(incl, off, 64); if (lane >= off) incl += o; }
  if (lane == 63) wsum[wv] = incl;
  __syncthreads();
  unsigned before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < 16; w++) { const unsigned x = wsum[w]; if (w < wv) before += x; total += x; }
  unsigned run = before + incl - s;
  for (int i = lo; i < hi; i++) { const unsigned t = a[i]; a[i] = run; run += t; }
  if (threadIdx.x == 0) { if (total_dev) *total_dev = (int)total; if (total_host) *total_host = (int)total; }
}

// A wavefront takes 1024 consecutive keys in 16 rounds of 64, lane = position: a key's rank among the keys of its digit is the wavefront's running count of that
// digit plus the number of lower lanes of this round that hold the same digit (eight ballots). Then digit d of wavefront w of tile b starts at
// scanned hist[d][b] + the counts of the wavefronts before w: rounds, lanes, wavefronts and tiles all follow the input order, so the pass is stable.
__global__ __launch_bounds__(SM_THREADS) void sort_scatter_kernel(const unsigned* __restrict__ kin, const int* __restrict__ vin, unsigned* __restrict__ kout,
                                                                  int* __restrict__ vout, int n, int shift, const unsigned* __restrict__ hist, int nblocks) {
  __shared__ unsigned cnt_[SM_THREADS / 64][256];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int w = 0; w < SM_THREADS / 64; w++) cnt_[w][threadIdx.x] = 0;
  __syncthreads();
  volatile unsigned* cnt = cnt_[wv];
  const int base = blockIdx.x * SORT_TILE + wv * (64 * SORT_ITEMS);
  unsigned key[SORT_ITEMS], rank[SORT_ITEMS];
#pragma unroll
  for (int r = 0; r < SORT_ITEMS; r++) {
    const int i = base + r * 64 + lane;
    const bool valid = i < n;
    key[r] = valid ? kin[i] : 0xffffffffu;
    const unsigned d = (key[r] >> shift) & 255u;
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; b++) { const bool bit = (d >> b) & 1u; const unsigned long long bal = __ballot(bit); m &= bit ? bal : ~bal; }
    const unsigned below = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    const unsigned prev = cnt[d];
    __builtin_amdgcn_wave_barrier();
    if (valid && below == 0) cnt[d] = prev + (unsigned)__popcll(m);   // the first lane of each digit of this round
    __builtin_amdgcn_wave_barrier();
    rank[r] = prev + below;
  }
  __syncthreads();
  {   // thread = digit: where each wavefront's keys of this digit start
    const int d = threadIdx.x;
    unsigned g = hist[(size_t)d * nblocks + blockIdx.x];
#pragma unroll
    for (int w = 0; w < SM_THREADS / 64; w++) { const unsigned c = cnt_[w][d]; cnt_[w][d] = g; g += c; }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < SORT_ITEMS; r++) {
    const int i = base + r * 64 + lane;
    if (i < n) {
      const unsigned pos = cnt_[wv][(key[r] >> shift) & 255u] + rank[r];   // < n: the scanned counts of all n keys
      kout[pos] = key[r];
      vout[pos] = vin[i];
    }
  }
}

__device__ __forceinline__ int lower_bound_u32(const unsigned* __restrict__ a, int n, unsigned key) {
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (a[mid] < key) lo = mid + 1; else hi = mid; }
  return lo;
}

// ---- host: how the kernels above are launched -----------------------------------------------------------------------------------------------------------------
// the sort's two key / value buffers, the tiles' digit counts and the digit totals of its four passes; they only grow, in the owner's store
struct SortScratch {
  unsigned* keys[2] = {nullptr, nullptr}; size_t keys_cap[2] = {0, 0};
  int* vals[2] = {nullptr, nullptr}; size_t vals_cap[2] = {0, 0};
  unsigned* hist = nullptr; size_t hist_cap = 0;
  unsigned* dtot = nullptr; size_t dtot_cap = 0;   // [4 passes][256 digits]

  int reserve(DevStore& store, size_t n) {
    const size_t nblocks = (n + SORT_TILE - 1) / SORT_TILE;
    int rc;
    for (int b = 0; b < 2; b++) {
      if ((rc = store.grow(keys[b], keys_cap[b], n))) return rc;
      if ((rc = store.grow(vals[b], vals_cap[b], n))) return rc;
    }
    if ((rc = store.grow(hist, hist_cap, 256 * nblocks))) return rc;
    return store.grow(dtot, dtot_cap, (size_t)4 * 256);
  }
  // the stable sort of keys[0] / vals[0] (n pairs) by the keys' low `bits` bits, 8 per pass: the result in keys[*cur] / vals[*cur]
  int sort_pairs(hipStream_t s, int n, int bits, int* cur_out) {
    const int nblocks = (n + SORT_TILE - 1) / SORT_TILE;
    int cur = 0;
    HIPCHK(hipMemsetAsync(dtot, 0, sizeof(unsigned) * 4 * 256, s));
    for (int shift = 0; shift < bits; shift += 8) {
      unsigned* dt = dtot + 256 * (shift / 8);
      sort_hist_kernel<<<nblocks, SM_THREADS, 0, s>>>(keys[cur], n, shift, hist, nblocks, dt);
      HIPCHK(hipGetLastError());
      sort_scan_kernel<<<256, SM_THREADS, 0, s>>>(hist, nblocks, dt);
      HIPCHK(hipGetLastError());
      sort_scatter_kernel<<<nblocks, SM_THREADS, 0, s>>>(keys[cur], vals[cur], keys[cur ^ 1], vals[cur ^ 1], n, shift, hist, nblocks);
      HIPCHK(hipGetLastError());
      cur ^= 1;
    }
    *cur_out = cur;
    return ROLO_OK;
  }
};

// key bits the sort has to look at for cells 0 .. cells - 1
inline int sort_bits_for_cells(long long cells) {
  int bits = 1;
  while (bits < 31 && (1ll << bits) < cells) bits++;
  return bits;
}

// the box of pts[0 .. n) into h_box[0..6] (pinned; valid after the stream has been waited for); box_part: 8 * BOX_BLOCKS_MAX floats
inline int enqueue_box(hipStream_t s, const float4* pts, int n, float* box_part, float* h_box) {
  if (n <= 0) return ROLO_OK;
  const int blocks = std::min((n + SM_THREADS - 1) / SM_THREADS, BOX_BLOCKS_MAX);
  vg_box_kernel<<<blocks, SM_THREADS, 0, s>>>(pts, n, box_part);
  HIPCHK(hipGetLastError());
  vg_box_final_kernel<<<1, SM_THREADS, 0, s>>>(box_part, blocks, h_box);
  HIPCHK(hipGetLastError());
  return ROLO_OK;
}

}  // namespace
}  // namespace rolo
