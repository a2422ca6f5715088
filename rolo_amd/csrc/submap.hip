// The back end's sub-map assembly on gfx950: a device-resident key-frame store (rolo_keymap_*), extractCloud and pcl::VoxelGrid for clouds of any size.
// Replaces (reference src/backMapping.cpp) extractNearby :575-614 (rolo_keyposes_select_nearby, host), extractCloud :617-658 with transformPointCloud :301-320
// (rolo_keymap_extract), downsampleCurrentScan :666-678 (rolo_keymap_downsample) and the key-frame bookkeeping of saveKeyFramesAndFactor :1140-1181 /
// correctPoses :1287-1320 (rolo_keymap_add_keyframe / rolo_keymap_set_pose), and the clouds of the exports: publishGlobalMap :1611-1665 (rolo_keymap_global_map)
// and saveGlobalPCDs' cloudGlobal.pcd :1546-1557 (rolo_keymap_global_cloud), past ROLO_KEYMAP_MAX_POINTS through the streamed form of the filter (gm_* below).
//
// pcl::VoxelGrid<PointXYZI>::filter, bit-identical to the oracle's orc_voxelgrid (oracle/rolo_oracle_front.cpp): float min / max of the cloud, the integer
// cell index as written there, cells in ascending index order, and per cell the four float sums taken SERIALLY IN ORIGINAL POINT ORDER, divided by the float
// count. Float addition is not associative: a cell's sum is never split into partial sums and never made with atomics. Every point is stored once under its
// cell by a STABLE sort of (cell, point index), then one lane per cell walks its points:
//   vg_box_kernel / vg_box_final_kernel   min / max (exact in any order) and the non-finite flag -> host (div_b, min_b, the "too many cells" copy-through)
//   vg_key_kernel                         the cell index of every point (at most 31 bits; 32 with the sign flipped if div_b's product wraps, as the int does)
//   sort_hist / sort_scan / sort_scatter  LSD radix sort, 8 bits per pass, only the passes the largest index needs; stable: ranks by wavefront match, in point order
//   run_heads_kernel<0>, scan_excl, <1>   a cell starts where the sorted index changes; the scan gives its output slot and the number of cells
//   vg_runsum_kernel                      one lane per cell: the serial sums through the sorted point indices, the division, the output record
// A clumped cell is one long serial chain in one lane; the summation order is the contract, so it stays that way.
// The box, sort and scan kernels live in sort_dev.hpp, which groundprior.hip includes too.
//
// transformPointCloud: the oracle's float statement p0 + (p1 + (p2 + c3)) per row (orc_transform_cloud_f, the parity target of the tests), no contraction.
#include "keymap.hpp"
#include "dev_rows.hpp"
#include "sort_dev.hpp"
#include "pcl_affine.hpp"
#include <algorithm>
#include <array>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace rolo {
namespace {

constexpr int RUN_ITEMS = 4;
constexpr int RUN_TILE = SM_THREADS * RUN_ITEMS;
constexpr int KM_MAX_POINTS = ROLO_KEYMAP_MAX_POINTS;
constexpr size_t CHUNK_POINTS = 1u << 20;              // the store grows in chunks of 16 MiB (or one cloud, if larger): nothing is ever moved or freed

// *cloudOut = T * cloudIn of every listed key frame, written at its place in the concatenation (list order); intensity copied
__global__ __launch_bounds__(SM_THREADS) void km_transform_kernel(const Seg* __restrict__ segs, float4* __restrict__ out) {
  const Seg s = segs[blockIdx.y];
  for (int i = blockIdx.x * SM_THREADS + threadIdx.x; i < s.n; i += gridDim.x * SM_THREADS) {
    out[(size_t)s.dst + i] = transform12(s.T, s.src[i]);
  }
}

struct VgGrid { float inv; int min_b[3]; unsigned mul[3]; unsigned flip; };

// ijk = floor(p * inv) - min_b; idx = ijk0 * 1 + ijk1 * div_b0 + ijk2 * div_b0 * div_b1 (VoxelGrid::applyFilter), in wrapping 32-bit arithmetic
__global__ __launch_bounds__(SM_THREADS) void vg_key_kernel(const float4* __restrict__ pts, int n, VgGrid G, unsigned* __restrict__ keys, int* __restrict__ vals) {
  const int i = blockIdx.x * SM_THREADS + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  const int i0 = (int)floorf(p.x * G.inv) - G.min_b[0], i1 = (int)floorf(p.y * G.inv) - G.min_b[1], i2 = (int)floorf(p.z * G.inv) - G.min_b[2];
  keys[i] = ((unsigned)i0 * G.mul[0] + (unsigned)i1 * G.mul[1] + (unsigned)i2 * G.mul[2]) ^ G.flip;
  vals[i] = i;
}

// a cell starts at sorted position i when i = 0 or the index differs from its predecessor's. WRITE = 0: heads per tile -> bcnt[block];
// WRITE = 1 (bcnt scanned): starts[slot] = i for every head
template <int WRITE>
__global__ __launch_bounds__(SM_THREADS) void run_heads_kernel(const unsigned* __restrict__ keys, int n, unsigned* __restrict__ bcnt, int* __restrict__ starts) {
  __shared__ unsigned wsum[SM_THREADS / 64];
  const int i0 = blockIdx.x * RUN_TILE + threadIdx.x * RUN_ITEMS;
  bool head[RUN_ITEMS];
  unsigned c = 0;
  unsigned prev = (i0 > 0 && i0 - 1 < n) ? keys[i0 - 1] : 0u;
#pragma unroll
  for (int k = 0; k < RUN_ITEMS; k++) {
    const int i = i0 + k;
    const unsigned cur = i < n ? keys[i] : 0u;
    head[k] = i < n && (i == 0 || cur != prev);
    c += head[k] ? 1u : 0u;
    prev = cur;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned incl = c;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const unsigned o = __shfl_up(incl, off, 64); if (lane >= off) incl += o; }
  if (lane == 63) wsum[wv] = incl;
  __syncthreads();
  unsigned before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < SM_THREADS / 64; w++) { const unsigned x = wsum[w]; if (w < wv) before += x; total += x; }
  if (!WRITE) { if (threadIdx.x == 0) bcnt[blockIdx.x] = total; return; }
  unsigned pos = bcnt[blockIdx.x] + before + incl - c;   // < number of heads <= n
#pragma unroll
  for (int k = 0; k < RUN_ITEMS; k++) if (head[k]) starts[pos++] = i0 + k;
}

// one lane per cell: the centroid's four float sums in original point order (the stable sort keeps a cell's points in that order), then / float(count)
__global__ __launch_bounds__(SM_THREADS) void vg_runsum_kernel(const float4* __restrict__ pts, const int* __restrict__ idx, const int* __restrict__ starts,
                                                               const int* __restrict__ m_ptr, int n, float4* __restrict__ out) {
  const int r = blockIdx.x * SM_THREADS + threadIdx.x;
  const int m = *m_ptr;
  if (r >= m) return;
  const int s = starts[r], e = r + 1 < m ? starts[r + 1] : n;
  float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
  for (int j = s; j < e; j++) { const float4 p = pts[idx[j]]; sx += p.x; sy += p.y; sz += p.z; si += p.w; }
  const float cnt = (float)(e - s);
  out[r] = make_float4(sx / cnt, sy / cnt, sz / cnt, si / cnt);
}

// ---- the streamed filter (rolo_keymap_global_map): a batch's runs merged into a table of (cell, running sums, count) kept in cell order -------------------
// The table carries every cell's serial chain from batch to batch: a run of a cell the table holds starts from the kept sums and adds its points in order, so the
// sums are those of one pass over the whole concatenation. Two tables in turn: every old entry and every run writes its own place in the other one, no
// atomics, no workgroup waits for another; each seam is a launch.
//   gm_find_kernel        one lane per run: the lower bound of its cell in the table, found or new; new cells per workgroup -> ncnt (scanned by scan_excl_kernel)
//   gm_merge_runs_kernel  one lane per run: its place = lower bound + the new runs before it; sums continued from the table's, or from 0, through the run's points
//   gm_move_old_kernel    one lane per old entry no run continues: its place = its index + the new runs below its cell
//   gm_finish_kernel      sums / float(count)
// rkey[r]: the run's cell; lbv[r]: its lower bound in the table, as ~bound when the table does not hold the cell
__global__ __launch_bounds__(SM_THREADS) void gm_find_kernel(const unsigned* __restrict__ keys, const int* __restrict__ starts, const int* __restrict__ nruns_ptr,
                                                             const unsigned* __restrict__ tkey, int m_old, unsigned* __restrict__ rkey, int* __restrict__ lbv,
                                                             unsigned* __restrict__ ncnt) {
  __shared__ unsigned wsum[SM_THREADS / 64];
  const int r = blockIdx.x * SM_THREADS + threadIdx.x;
  bool isnew = false;
  if (r < *nruns_ptr) {
    const unsigned key = keys[starts[r]];
    const int lb = lower_bound_u32(tkey, m_old, key);
    isnew = !(lb < m_old && tkey[lb] == key);
    rkey[r] = key;
    lbv[r] = isnew ? ~lb : lb;
  }
  const unsigned long long b = __ballot(isnew);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (unsigned)__popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) { unsigned t = 0; for (int w = 0; w < SM_THREADS / 64; w++) t += wsum[w]; ncnt[blockIdx.x] = t; }
}

struct GmTable { unsigned* key; float4* sum; int* cnt; };

__global__ __launch_bounds__(SM_THREADS) void gm_merge_runs_kernel(const float4* __restrict__ pts, const int* __restrict__ idx, const int* __restrict__ starts,
                                                                   const int* __restrict__ nruns_ptr, int n, const unsigned* __restrict__ rkey,
                                                                   const int* __restrict__ lbv, const unsigned* __restrict__ ncnt /* scanned */, GmTable told,
                                                                   GmTable tnew, int* __restrict__ npre) {
  __shared__ unsigned wsum[SM_THREADS / 64];
  const int r = blockIdx.x * SM_THREADS + threadIdx.x, nruns = *nruns_ptr;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int code = r < nruns ? lbv[r] : 0;
  const bool isnew = code < 0;
  const unsigned long long b = __ballot(isnew);
  if (lane == 0) wsum[wv] = (unsigned)__popcll(b);
  __syncthreads();
  unsigned before = 0;
  for (int w = 0; w < wv; w++) before += wsum[w];
  if (r >= nruns) return;
  const int pre = (int)(ncnt[blockIdx.x] + before + (unsigned)__popcll(b & ((1ull << lane) - 1ull)));
  npre[r] = pre;
  if (r == nruns - 1) npre[nruns] = pre + (isnew ? 1 : 0);
  const int lb = isnew ? ~code : code;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  int c = 0;
  if (!isnew) { s = told.sum[lb]; c = told.cnt[lb]; }
  const int j0 = starts[r], j1 = r + 1 < nruns ? starts[r + 1] : n;
  for (int j = j0; j < j1; j++) { const float4 p = pts[idx[j]]; s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w; }
  const size_t dst = (size_t)lb + (size_t)pre;   // < old entries + new cells: the lower bound counts the old cells below, pre the new ones
  tnew.key[dst] = rkey[r]; tnew.sum[dst] = s; tnew.cnt[dst] = c + (j1 - j0);
}

__global__ __launch_bounds__(SM_THREADS) void gm_move_old_kernel(GmTable told, int m_old, const unsigned* __restrict__ rkey, const int* __restrict__ nruns_ptr,
                                                                 const int* __restrict__ npre, GmTable tnew) {
  const int i = blockIdx.x * SM_THREADS + threadIdx.x;
  if (i >= m_old) return;
  const int nruns = *nruns_ptr;
  const unsigned key = told.key[i];
  const int j = lower_bound_u32(rkey, nruns, key);
  if (j < nruns && rkey[j] == key) return;   // continued by a run: gm_merge_runs_kernel writes it
  const size_t dst = (size_t)i + (size_t)npre[j];
  tnew.key[dst] = key; tnew.sum[dst] = told.sum[i]; tnew.cnt[dst] = told.cnt[i];
}

__global__ __launch_bounds__(SM_THREADS) void gm_finish_kernel(const float4* __restrict__ sum, const int* __restrict__ cnt, int m, float4* __restrict__ out) {
  const int i = blockIdx.x * SM_THREADS + threadIdx.x;
  if (i >= m) return;
  const float4 s = sum[i];
  const float c = (float)cnt[i];
  out[i] = make_float4(s.x / c, s.y / c, s.z / c, s.w / c);
}

// ---- host restatement of the same filter (the key poses of extractNearby: a few hundred points) ------------------------------------------------------------
int host_voxelgrid(const std::vector<std::array<float, 4>>& in, float leaf, std::vector<std::array<float, 4>>& out) {
  out.clear();
  const int n = (int)in.size();
  if (n == 0) return 0;
  const float inv = 1.0f / leaf;
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (const auto& p : in) for (int d = 0; d < 3; d++) { mn[d] = std::min(mn[d], p[d]); mx[d] = std::max(mx[d], p[d]); }
  long long ext[3];
  for (int d = 0; d < 3; d++) { const float e = (mx[d] - mn[d]) * inv; ext[d] = e < 4e18f ? (long long)e + 1 : (long long)INT32_MAX + 1; }
  if (ext[0] > INT32_MAX || ext[1] > INT32_MAX || ext[0] * ext[1] > INT32_MAX || ext[0] * ext[1] * ext[2] > INT32_MAX) { out = in; return n; }
  int lo[3], div[3];
  for (int d = 0; d < 3; d++) { lo[d] = (int)std::floor(mn[d] * inv); div[d] = (int)std::floor(mx[d] * inv) - lo[d] + 1; }
  std::vector<std::pair<int, int>> cell(n);
  for (int i = 0; i < n; i++) {
    int c[3];
    for (int d = 0; d < 3; d++) c[d] = (int)std::floor(in[i][d] * inv) - lo[d];
    cell[i] = {(int)((unsigned)c[0] + (unsigned)c[1] * (unsigned)div[0] + (unsigned)c[2] * ((unsigned)div[0] * (unsigned)div[1])), i};
  }
  std::sort(cell.begin(), cell.end());
  for (int a = 0; a < n;) {
    int b = a;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    while (b < n && cell[b].first == cell[a].first) { for (int d = 0; d < 4; d++) s[d] += in[cell[b].second][d]; b++; }
    const float cnt = (float)(b - a);
    out.push_back({s[0] / cnt, s[1] / cnt, s[2] / cnt, s[3] / cnt});
    a = b;
  }
  return (int)out.size();
}

}  // namespace
}  // namespace rolo

using namespace rolo;

namespace {

int km_sort_scratch(rolo_keymap* km, int n) {
  const int nrun = (n + RUN_TILE - 1) / RUN_TILE;
  int rc;
  if ((rc = km->sort.reserve(km->store, (size_t)n))) return rc;
  if ((rc = km->store.grow(km->bcnt, km->bcnt_cap, (size_t)nrun))) return rc;
  if ((rc = km->store.grow(km->starts, km->starts_cap, (size_t)n))) return rc;
  return km->store.grow(km->box_part, km->box_part_cap, 2 * 8 * (size_t)BOX_BLOCKS_MAX);
}

// first half of the filter: the cloud's box into h_box[slot] (valid after the stream has been waited for)
int vg_enqueue_box(rolo_keymap* km, const float4* pts, int n, int slot) {
  return enqueue_box(km->stream, pts, n, km->box_part + 8 * (size_t)BOX_BLOCKS_MAX * slot, km->h_box + 8 * slot);
}

// the grid of a box (h_box's 7 floats) at a leaf: false for PCL's "leaf size is too small" (more than INT32_MAX cells by the extents). *bits: what the sort needs
bool vg_grid_of_box(const float* hb, float leaf, VgGrid* G, int* bits) {
  const float inv = 1.0f / leaf;
  long long ext[3];
  for (int d = 0; d < 3; d++) { const float e = (hb[3 + d] - hb[d]) * inv; ext[d] = e < 4e18f ? (long long)e + 1 : (long long)INT32_MAX + 1; }
  if (ext[0] > INT32_MAX || ext[1] > INT32_MAX || ext[0] * ext[1] > INT32_MAX || ext[0] * ext[1] * ext[2] > INT32_MAX) return false;
  *G = VgGrid{};
  G->inv = inv;
  int div[3];
  for (int d = 0; d < 3; d++) { G->min_b[d] = (int)std::floor(hb[d] * inv); div[d] = (int)std::floor(hb[3 + d] * inv) - G->min_b[d] + 1; }
  G->mul[0] = 1u; G->mul[1] = (unsigned)div[0]; G->mul[2] = (unsigned)div[0] * (unsigned)div[1];
  const long long cells = (long long)div[0] * div[1] * div[2];
  *bits = 32;
  if (cells <= (long long)INT32_MAX) { *bits = sort_bits_for_cells(cells); G->flip = 0u; }
  else G->flip = 0x80000000u;   // div_b's product wraps the int (the extents' product did not): signed order through the flipped sign bit
  return true;
}

// keys of pts[0 .. n), the stable sort by cell, the run heads: sorted keys / point indices in km->sort.keys[*cur] / km->sort.vals[*cur], km->starts, the number of runs in
// d_m[slot] and h_m[slot] (valid after the stream has been waited for)
int vg_enqueue_sort_runs(rolo_keymap* km, const float4* pts, int n, const VgGrid& G, int bits, int slot, int* cur_out) {
  hipStream_t s = km->stream;
  const int nrun = (n + RUN_TILE - 1) / RUN_TILE;
  vg_key_kernel<<<(n + SM_THREADS - 1) / SM_THREADS, SM_THREADS, 0, s>>>(pts, n, G, km->sort.keys[0], km->sort.vals[0]);
  HIPCHK(hipGetLastError());
  int cur = 0, rc;
  if ((rc = km->sort.sort_pairs(s, n, bits, &cur))) return rc;
  run_heads_kernel<0><<<nrun, SM_THREADS, 0, s>>>(km->sort.keys[cur], n, km->bcnt, km->starts);
  HIPCHK(hipGetLastError());
  scan_excl_kernel<<<1, 1024, 0, s>>>(km->bcnt, nrun, km->d_m + slot, km->h_m + slot);
  HIPCHK(hipGetLastError());
  run_heads_kernel<1><<<nrun, SM_THREADS, 0, s>>>(km->sort.keys[cur], n, km->bcnt, km->starts);
  HIPCHK(hipGetLastError());
  *cur_out = cur;
  return ROLO_OK;
}

// second half: keys, sort, cells, centroids into out; the number of cells lands in h_m[slot] (valid after the stream has been waited for).
// *direct: the result is known without the device (n = 0, or PCL's "leaf size is too small": the input copied through)
int vg_enqueue_filter(rolo_keymap* km, const float4* pts, int n, float leaf, int slot, float4* out, bool* direct, int* m_direct) {
  *direct = false;
  if (n <= 0) { *direct = true; *m_direct = 0; return ROLO_OK; }
  const float* hb = km->h_box + 8 * slot;
  if (hb[6] != 0.f) { ctx_set_error("a non-finite coordinate reached the voxel grid filter"); return ROLO_ENONFINITE; }
  VgGrid G; int bits = 0;
  if (!vg_grid_of_box(hb, leaf, &G, &bits)) {
    HIPCHK(hipMemcpyAsync(out, pts, sizeof(float4) * (size_t)n, hipMemcpyDeviceToDevice, km->stream));
    *direct = true; *m_direct = n;
    return ROLO_OK;
  }
  int cur = 0;
  const int rc = vg_enqueue_sort_runs(km, pts, n, G, bits, slot, &cur);
  if (rc) return rc;
  vg_runsum_kernel<<<(n + SM_THREADS - 1) / SM_THREADS, SM_THREADS, 0, km->stream>>>(pts, km->sort.vals[cur], km->starts, km->d_m + slot, n, out);
  HIPCHK(hipGetLastError());
  return ROLO_OK;
}

// kdtree->radiusSearch(cloud->back(), radius) over the key poses, the one statement of its rule (extractNearby :585, detectLoopClosureDistance :2496): the poses whose
// squared float distance to the LAST one is below radius^2, ascending by (distance, index)
std::vector<std::pair<float, int>> radius_hits_last(const float* xyz, int n, float radius) {
  std::vector<std::pair<float, int>> near;
  if (n <= 0) return near;
  const float* last = xyz + 3 * (size_t)(n - 1);
  const float r2 = radius * radius;
  for (int i = 0; i < n; i++) {
    const float* a = xyz + 3 * (size_t)i;
    const float dx = a[0] - last[0], dy = a[1] - last[1], dz = a[2] - last[2];
    const float d = dx * dx + dy * dy + dz * dz;
    if (d < r2) near.push_back({d, i});
  }
  std::sort(near.begin(), near.end());
  return near;
}

int km_alloc_points(rolo_keymap* km, size_t n, float4** out) {
  *out = nullptr;
  if (n == 0) return ROLO_OK;
  if (km->chunks.empty() || km->chunks.back().cap - km->chunks.back().used < n) {
    rolo_keymap::Chunk c{nullptr, std::max(CHUNK_POINTS, n), 0};
    if (const int rc = km->store.alloc(c.p, c.cap)) return rc;
    km->chunks.push_back(c);
  }
  rolo_keymap::Chunk& c = km->chunks.back();
  *out = c.p + c.used;
  c.used += n;
  return ROLO_OK;
}

// ---- the global map's concatenation: per listed key frame its corner, then its surface cloud; never held as a whole -----------------------------------------
struct GmPiece { const float4* src; int n; int frame; long long off; };   // one non-empty cloud and where it starts in the concatenation

int gm_list(rolo_keymap* km, const int32_t* indices, int n, const char* who, std::vector<GmPiece>& pieces, long long* total) {
  pieces.clear();
  long long off = 0;
  for (int i = 0; i < n; i++) {
    if (indices[i] < 0 || indices[i] >= (int)km->frames.size()) { ctx_set_error((std::string(who) + ": key-frame index out of range").c_str()); return ROLO_EINVAL; }
    const rolo_keymap::Frame& f = km->frames[indices[i]];
    for (int t = 0; t < 2; t++) {
      if (!f.n[t]) continue;
      pieces.push_back({f.pts[t], f.n[t], indices[i], off});
      off += f.n[t];
    }
    if (off > (long long)INT32_MAX) { ctx_set_error((std::string(who) + ": more than 2^31 - 1 points listed").c_str()); return ROLO_EINVAL; }
  }
  *total = off;
  return ROLO_OK;
}

int gm_batch_of(const rolo_keymap* km) { return km->gm_batch > 0 ? km->gm_batch : ROLO_KEYMAP_GLOBAL_BATCH; }

// scratch of one batch: the transformed points, the segment table (a batch of nb points holds at most nb non-empty clouds)
int gm_batch_scratch(rolo_keymap* km, int nb, size_t npieces) {
  const size_t nsegs = std::max<size_t>(std::min<size_t>(npieces, (size_t)nb), 1);
  int rc;
  if ((rc = km->store.grow_pinned(km->h_segs, km->h_segs_cap, nsegs, 64))) return rc;
  if ((rc = km->store.grow(km->segs, km->segs_cap, nsegs))) return rc;
  return km->store.grow(km->cat[0], km->cat_cap[0], (size_t)nb);
}

// points [b0, b0 + nb) of the concatenation, moved by their frames' poses, into cat[0]: a Seg with an offset source is a slice, so a batch may begin and end inside
// a cloud. *cursor: the first piece that reaches b0 or beyond (batches are taken in order). The pinned segment table is reused: the stream has been waited for
// since the last batch's copy
int gm_enqueue_batch(rolo_keymap* km, const std::vector<GmPiece>& pieces, size_t* cursor, long long b0, int nb) {
  while (*cursor < pieces.size() && pieces[*cursor].off + pieces[*cursor].n <= b0) ++*cursor;
  size_t nsegs = 0;
  int max_n = 1;
  for (size_t q = *cursor; q < pieces.size() && pieces[q].off < b0 + nb; q++) {
    const GmPiece& pc = pieces[q];
    const long long lo = std::max(pc.off, b0), hi = std::min(pc.off + pc.n, b0 + nb);
    Seg& g = km->h_segs[nsegs++];
    g.src = pc.src + (lo - pc.off); g.n = (int)(hi - lo); g.dst = (int)(lo - b0);
    pcl_rows_of_rpyxyz(km->frames[pc.frame].pose, g.T);
    max_n = std::max(max_n, g.n);
  }
  hipStream_t s = km->stream;
  HIPCHK(hipMemcpyAsync(km->segs, km->h_segs, nsegs * sizeof(Seg), hipMemcpyHostToDevice, s));
  const int gx = std::min((max_n + SM_THREADS - 1) / SM_THREADS, 128);
  for (size_t y0 = 0; y0 < nsegs; y0 += 32768) {
    km_transform_kernel<<<dim3(gx, (unsigned)std::min<size_t>(nsegs - y0, 32768)), SM_THREADS, 0, s>>>(km->segs + y0, km->cat[0]);
    HIPCHK(hipGetLastError());
  }
  return ROLO_OK;
}

// the streamed form: total > batch points. The events 1 .. 3 are recorded here
int gm_streamed(rolo_keymap* km, const std::vector<GmPiece>& pieces, long long total, int batch, float leaf, int* m_out) {
  hipStream_t s = km->stream;
  const long long nbatches = (total + batch - 1) / batch;
  int rc;
  if ((rc = km_sort_scratch(km, batch))) return rc;
  if ((rc = gm_batch_scratch(km, batch, pieces.size()))) return rc;
  const int nblk = (batch + SM_THREADS - 1) / SM_THREADS;
  if ((rc = km->store.grow(km->gm_ncnt, km->gm_ncnt_cap, (size_t)nblk))) return rc;
  if ((rc = km->store.grow(km->gm_npre, km->gm_npre_cap, (size_t)batch + 1))) return rc;
  // pass 1: the box of the whole concatenation; min, max and the flag are exact in any order
  float box[7] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX, 0.f};
  size_t cursor = 0;
  for (long long b = 0; b < nbatches; b++) {
    const long long b0 = b * batch;
    const int nb = (int)std::min<long long>(batch, total - b0);
    if ((rc = gm_enqueue_batch(km, pieces, &cursor, b0, nb))) return rc;
    if ((rc = vg_enqueue_box(km, km->cat[0], nb, 0))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    for (int k = 0; k < 3; k++) { box[k] = std::min(box[k], km->h_box[k]); box[3 + k] = std::max(box[3 + k], km->h_box[3 + k]); }
    if (km->h_box[6] != 0.f) box[6] = 1.f;
  }
  HIPCHK(hipEventRecord(km->gm_ev[1], s));
  if (box[6] != 0.f) { ctx_set_error("a non-finite coordinate reached the voxel grid filter"); return ROLO_ENONFINITE; }
  VgGrid G; int bits = 0;
  if (!vg_grid_of_box(box, leaf, &G, &bits)) {
    ctx_set_error("rolo_keymap_global_map: leaf size is too small for the listed clouds (more than INT32_MAX cells): the streamed form does not return the whole input");
    return ROLO_EINVAL;
  }
  // pass 2: the same points again, batch by batch: keys with the global grid, sort, runs, merge into the other table
  int m_tab = 0, tcur = 0;
  long long m_peak = 0;
  cursor = 0;
  for (long long b = 0; b < nbatches; b++) {
    const long long b0 = b * batch;
    const int nb = (int)std::min<long long>(batch, total - b0);
    if ((rc = gm_enqueue_batch(km, pieces, &cursor, b0, nb))) return rc;
    int cur = 0;
    if ((rc = vg_enqueue_sort_runs(km, km->cat[0], nb, G, bits, 0, &cur))) return rc;
    const int blocks = (nb + SM_THREADS - 1) / SM_THREADS;
    unsigned* rkey = km->sort.keys[cur ^ 1];   // the sort's other pair is free now: the runs' cells and their lower bounds
    int* lbv = km->sort.vals[cur ^ 1];
    gm_find_kernel<<<blocks, SM_THREADS, 0, s>>>(km->sort.keys[cur], km->starts, km->d_m, km->gt_key[tcur], m_tab, rkey, lbv, km->gm_ncnt);
    HIPCHK(hipGetLastError());
    scan_excl_kernel<<<1, 1024, 0, s>>>(km->gm_ncnt, blocks, km->gm_d, km->gm_h);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    const int nruns = km->h_m[0], nnew = km->gm_h[0];
    if (nruns <= 0 || nruns > nb || nnew < 0 || nnew > nruns || (long long)m_tab + nnew > (long long)INT32_MAX) {
      ctx_set_error("the key map's streamed voxel filter returned an inconsistent cell count"); return ROLO_ESTATE;
    }
    const int tn = tcur ^ 1;
    const size_t m_new = (size_t)m_tab + (size_t)nnew;
    if ((rc = km->store.grow(km->gt_key[tn], km->gt_key_cap[tn], m_new))) return rc;
    if ((rc = km->store.grow(km->gt_sum[tn], km->gt_sum_cap[tn], m_new))) return rc;
    if ((rc = km->store.grow(km->gt_cnt[tn], km->gt_cnt_cap[tn], m_new))) return rc;
    const GmTable told{km->gt_key[tcur], km->gt_sum[tcur], km->gt_cnt[tcur]}, tnew{km->gt_key[tn], km->gt_sum[tn], km->gt_cnt[tn]};
    gm_merge_runs_kernel<<<blocks, SM_THREADS, 0, s>>>(km->cat[0], km->sort.vals[cur], km->starts, km->d_m, nb, rkey, lbv, km->gm_ncnt, told, tnew, km->gm_npre);
    HIPCHK(hipGetLastError());
    if (m_tab > 0) {
      gm_move_old_kernel<<<(m_tab + SM_THREADS - 1) / SM_THREADS, SM_THREADS, 0, s>>>(told, m_tab, rkey, km->d_m, km->gm_npre, tnew);
      HIPCHK(hipGetLastError());
    }
    m_tab = (int)m_new; tcur = tn;
    m_peak = std::max<long long>(m_peak, m_tab);
  }
  HIPCHK(hipEventRecord(km->gm_ev[2], s));
  if ((rc = km->store.grow(km->gmap, km->gmap_cap, (size_t)std::max(m_tab, 1)))) return rc;
  gm_finish_kernel<<<(m_tab + SM_THREADS - 1) / SM_THREADS, SM_THREADS, 0, s>>>(km->gt_sum[tcur], km->gt_cnt[tcur], m_tab, km->gmap);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(km->gm_ev[3], s));
  HIPCHK(hipStreamSynchronize(s));
  km->gm_info[1] = nbatches; km->gm_info[2] = m_tab; km->gm_info[3] = 1; km->gm_info[4] = m_peak;
  *m_out = m_tab;
  return ROLO_OK;
}

}  // namespace

namespace rolo {
int keymap_device_submap(rolo_keymap* km, const float** d_corner, int* m_corner, const float** d_surf, int* m_surf, hipEvent_t* ready, hipEvent_t* consumed, int* device) {
  if (!km->have_submap) { ctx_set_error("the key map holds no sub-map: call rolo_keymap_extract first"); return ROLO_ESTATE; }
  *d_corner = reinterpret_cast<const float*>(km->sub[0]); *m_corner = km->m_sub[0];
  *d_surf = reinterpret_cast<const float*>(km->sub[1]); *m_surf = km->m_sub[1];
  *ready = km->ready; *consumed = km->consumed; *device = km->device;
  return ROLO_OK;
}
void keymap_mark_consumed(rolo_keymap* km) { km->consumer_pending = true; }

int keymap_stage_cloud(rolo_keymap* km, const float* pts, int n, float leaf, const float4** d_out, int* n_out) {
  HIPCHK(hipSetDevice(km->device));
  hipStream_t s = km->stream;
  int rc;
  if ((rc = km->store.grow(km->cat[0], km->cat_cap[0], (size_t)n))) return rc;
  if (!(leaf > 0.f)) {
    HIPCHK(hipMemcpyAsync(km->cat[0], pts, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    *d_out = km->cat[0]; *n_out = n;
    return ROLO_OK;
  }
  if ((rc = km_sort_scratch(km, n))) return rc;
  if ((rc = km->store.grow(km->ds_out, km->ds_cap, (size_t)n))) return rc;
  HIPCHK(hipMemcpyAsync(km->cat[0], pts, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, s));
  if ((rc = vg_enqueue_box(km, km->cat[0], n, 0))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  bool direct; int m_direct = 0;
  if ((rc = vg_enqueue_filter(km, km->cat[0], n, leaf, 0, km->ds_out, &direct, &m_direct))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  const int mm = direct ? m_direct : km->h_m[0];
  if (mm < 0 || mm > n) { ctx_set_error("the key map's voxel filter returned an inconsistent cell count"); return ROLO_ESTATE; }
  *d_out = km->ds_out; *n_out = mm;
  return ROLO_OK;
}

int keymap_filter_resident(rolo_keymap* km, const float4* pts, int n, float leaf, const float4** d_out, int* n_out) {
  HIPCHK(hipSetDevice(km->device));
  hipStream_t s = km->stream;
  int rc;
  if ((rc = km_sort_scratch(km, n))) return rc;
  if ((rc = km->store.grow(km->ds_out, km->ds_cap, (size_t)n))) return rc;
  if ((rc = vg_enqueue_box(km, pts, n, 0))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  bool direct; int m_direct = 0;
  if ((rc = vg_enqueue_filter(km, pts, n, leaf, 0, km->ds_out, &direct, &m_direct))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  const int mm = direct ? m_direct : km->h_m[0];
  if (mm < 0 || mm > n) { ctx_set_error("the key map's voxel filter returned an inconsistent cell count"); return ROLO_ESTATE; }
  *d_out = km->ds_out; *n_out = mm;
  return ROLO_OK;
}

int keymap_scan_downsample(rolo_keymap* km, const float* corner, int n_corner, float corner_leaf, const float* surf, int n_surf, float surf_leaf, const float* raw,
                           int n_raw, bool on_device) {
  if (n_corner < 0 || n_surf < 0 || n_raw < 0 || (n_corner && !corner) || (n_surf && !surf) || n_corner > KM_MAX_POINTS || n_surf > KM_MAX_POINTS || n_raw > KM_MAX_POINTS ||
      !(corner_leaf > 0.f) || !(surf_leaf > 0.f))
    return ROLO_EINVAL;
  HIPCHK(hipSetDevice(km->device));
  hipStream_t s = km->stream;
  if (!km->scan_ready) HIPCHK(hipEventCreateWithFlags(&km->scan_ready, hipEventDisableTiming));
  const float* src[2] = {corner, surf};
  const int n[2] = {n_corner, n_surf};
  const float leaf[2] = {corner_leaf, surf_leaf};
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  int rc;
  if (std::max(n[0], n[1]) > 0 && (rc = km_sort_scratch(km, std::max(n[0], n[1])))) return rc;
  for (int t = 0; t < 2; t++) {
    if ((rc = km->store.grow(km->cat[t], km->cat_cap[t], (size_t)std::max(n[t], 1)))) return rc;
    if ((rc = km->store.grow(km->scan_ds[t], km->scan_ds_cap[t], (size_t)std::max(n[t], 1)))) return rc;
  }
  if (raw && n_raw && (rc = km->store.grow(km->scan_raw, km->scan_raw_cap, (size_t)n_raw))) return rc;
  for (int t = 0; t < 2; t++) {
    if (n[t]) HIPCHK(hipMemcpyAsync(km->cat[t], src[t], sizeof(float4) * (size_t)n[t], kind, s));
    if ((rc = vg_enqueue_box(km, km->cat[t], n[t], t))) return rc;
  }
  if (raw && n_raw) HIPCHK(hipMemcpyAsync(km->scan_raw, raw, sizeof(float4) * (size_t)n_raw, kind, s));
  HIPCHK(hipStreamSynchronize(s));   // the boxes are on the host, and the caller's arrays are free again
  bool direct[2]; int m_direct[2] = {0, 0};
  for (int t = 0; t < 2; t++)
    if ((rc = vg_enqueue_filter(km, km->cat[t], n[t], leaf[t], t, km->scan_ds[t], &direct[t], &m_direct[t]))) return rc;
  HIPCHK(hipEventRecord(km->scan_ready, s));
  HIPCHK(hipStreamSynchronize(s));
  int mm[2];
  for (int t = 0; t < 2; t++) {
    mm[t] = direct[t] ? m_direct[t] : km->h_m[t];
    if (mm[t] < 0 || mm[t] > n[t]) { ctx_set_error("the key map's voxel filter returned an inconsistent cell count"); return ROLO_ESTATE; }
  }
  km->n_scan_ds[0] = mm[0]; km->n_scan_ds[1] = mm[1];
  km->n_scan_raw = raw ? n_raw : 0;
  return ROLO_OK;
}

int keymap_reserve_keyframe(rolo_keymap* km, int n_corner, int n_surf) {
  if (km->frames.size() >= (size_t)INT_MAX) return ROLO_EINVAL;
  HIPCHK(hipSetDevice(km->device));
  const size_t need = (size_t)n_corner + (size_t)n_surf;
  if (need && (km->chunks.empty() || km->chunks.back().cap - km->chunks.back().used < need)) {
    rolo_keymap::Chunk c{nullptr, std::max(CHUNK_POINTS, need), 0};
    if (const int rc = km->store.alloc(c.p, c.cap)) return rc;
    km->chunks.push_back(c);
  }
  km->frames.reserve(km->frames.size() + 1);
  return ROLO_OK;
}

int keymap_append_scan(rolo_keymap* km, const float* pose6, double time) {
  HIPCHK(hipSetDevice(km->device));
  rolo_keymap::Frame f{};
  for (int t = 0; t < 2; t++) {
    float4* d = nullptr;
    const int rc = km_alloc_points(km, (size_t)km->n_scan_ds[t], &d);
    if (rc) return rc;
    if (km->n_scan_ds[t]) HIPCHK(hipMemcpyAsync(d, km->scan_ds[t], sizeof(float4) * (size_t)km->n_scan_ds[t], hipMemcpyDeviceToDevice, km->stream));
    f.pts[t] = d; f.n[t] = km->n_scan_ds[t];
  }
  std::memcpy(f.pose, pose6, sizeof(f.pose));
  f.time = time;
  km->frames.push_back(f);   // (the copies are ordered before every later reader on the key map's stream: no host wait)
  return (int)km->frames.size() - 1;
}

int keymap_registered(rolo_keymap* km, const float4* const* pieces, const int* n, int count, const float* pose6, float* out) {
  HIPCHK(hipSetDevice(km->device));
  hipStream_t s = km->stream;
  size_t total = 0, nsegs = 0;
  int max_n = 1;
  for (int k = 0; k < count; k++) { total += (size_t)n[k]; max_n = std::max(max_n, n[k]); }
  if (total == 0) return ROLO_OK;
  int rc;
  if ((rc = km->store.grow_pinned(km->h_segs, km->h_segs_cap, (size_t)count, 64))) return rc;
  if ((rc = km->store.grow(km->segs, km->segs_cap, (size_t)count))) return rc;
  if ((rc = km->store.grow(km->reg, km->reg_cap, total))) return rc;
  int dst = 0;
  for (int k = 0; k < count; k++) {
    if (!n[k]) continue;
    Seg& g = km->h_segs[nsegs++];
    g.src = pieces[k]; g.n = n[k]; g.dst = dst;
    pcl_rows_of_rpyxyz(pose6, g.T);
    dst += n[k];
  }
  HIPCHK(hipMemcpyAsync(km->segs, km->h_segs, nsegs * sizeof(Seg), hipMemcpyHostToDevice, s));
  km_transform_kernel<<<dim3(std::min((max_n + SM_THREADS - 1) / SM_THREADS, 128), (unsigned)nsegs), SM_THREADS, 0, s>>>(km->segs, km->reg);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, km->reg, sizeof(float4) * total, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return ROLO_OK;
}
}  // namespace rolo

extern "C" {

int rolo_keymap_create(int device, rolo_keymap** out) {
  if (!out) return ROLO_EINVAL;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { ctx_set_error("no HIP device"); return ROLO_EHIP; }
  if (device < 0 || device >= ndev) return ROLO_EINVAL;
  HIPCHK(hipSetDevice(device));
  rolo_keymap* km = new rolo_keymap();
  km->device = device;
  hipError_t e = hipStreamCreateWithFlags(&km->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&km->ready, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&km->consumed, hipEventDisableTiming);
  if (e != hipSuccess) { ctx_set_error((std::string("rolo_keymap_create: ") + hipGetErrorString(e)).c_str()); rolo_keymap_destroy(km); return ROLO_EHIP; }
  km->store.stream = km->stream; km->store.who = "keymap";
  int rc = km->store.alloc_pinned(km->h_box, 16);
  if (!rc) rc = km->store.alloc_pinned(km->h_m, 2);
  if (!rc) rc = km->store.alloc(km->d_m, 2);
  if (!rc) rc = km->store.alloc_pinned(km->gm_h, 2);
  if (!rc) rc = km->store.alloc(km->gm_d, 2);
  if (rc) { rolo_keymap_destroy(km); return rc; }
  *out = km;
  return ROLO_OK;
}

void rolo_keymap_destroy(rolo_keymap* km) {
  if (!km) return;
  (void)hipSetDevice(km->device);
  if (km->stream) (void)hipStreamSynchronize(km->stream);
  if (km->consumer_pending && km->consumed) (void)hipEventSynchronize(km->consumed);
  if (km->sc) { sc_store_destroy(km->sc); km->sc = nullptr; }
  if (km->loop_ctx) { rolo_ctx_release(km->loop_ctx); km->loop_ctx = nullptr; }
  km->store.release();
  if (km->ready) (void)hipEventDestroy(km->ready);
  if (km->consumed) (void)hipEventDestroy(km->consumed);
  if (km->scan_ready) (void)hipEventDestroy(km->scan_ready);
  if (km->loop_t0) (void)hipEventDestroy(km->loop_t0);
  if (km->loop_t1) (void)hipEventDestroy(km->loop_t1);
  for (hipEvent_t e : km->gm_ev) if (e) (void)hipEventDestroy(e);
  if (km->stream) (void)hipStreamDestroy(km->stream);
  delete km;
}

int rolo_keymap_size(rolo_keymap* km) { return km ? (int)km->frames.size() : ROLO_EINVAL; }

int rolo_keymap_add_keyframe(rolo_keymap* km, const float* corner, int n_corner, const float* surf, int n_surf, const float* pose6, double time) {
  if (!km || !pose6 || n_corner < 0 || n_surf < 0 || (n_corner && !corner) || (n_surf && !surf) || n_corner > KM_MAX_POINTS || n_surf > KM_MAX_POINTS) return ROLO_EINVAL;
  if (km->frames.size() >= (size_t)INT_MAX) return ROLO_EINVAL;
  HIPCHK(hipSetDevice(km->device));
  rolo_keymap::Frame f{};
  const float* src[2] = {corner, surf};
  const int n[2] = {n_corner, n_surf};
  for (int t = 0; t < 2; t++) {
    float4* d = nullptr;
    const int rc = km_alloc_points(km, (size_t)n[t], &d);
    if (rc) return rc;
    if (n[t]) HIPCHK(hipMemcpyAsync(d, src[t], sizeof(float4) * (size_t)n[t], hipMemcpyHostToDevice, km->stream));
    f.pts[t] = d; f.n[t] = n[t];
  }
  HIPCHK(hipStreamSynchronize(km->stream));   // the caller's arrays are free again
  std::memcpy(f.pose, pose6, sizeof(f.pose));
  f.time = time;
  km->frames.push_back(f);
  return (int)km->frames.size() - 1;
}

int rolo_keymap_set_pose(rolo_keymap* km, int index, const float* pose6) {
  if (!km || !pose6 || index < 0 || index >= (int)km->frames.size()) return ROLO_EINVAL;
  std::memcpy(km->frames[index].pose, pose6, sizeof(float) * 6);
  km->pose_epoch++;
  return ROLO_OK;
}

int rolo_keymap_set_poses(rolo_keymap* km, const float* pose6, int n) {
  if (!km || n < 0 || (n && !pose6) || n > (int)km->frames.size()) return ROLO_EINVAL;
  for (int k = 0; k < n; k++) std::memcpy(km->frames[k].pose, pose6 + 6 * (size_t)k, sizeof(float) * 6);
  km->pose_epoch++;
  return ROLO_OK;
}

int rolo_keymap_extract(rolo_keymap* km, const int32_t* indices, int n, float corner_leaf, float surf_leaf, int* m_corner, int* m_surf) {
  if (!km || n < 0 || (n && !indices) || !(corner_leaf > 0.f) || !(surf_leaf > 0.f)) return ROLO_EINVAL;
  long long total[2] = {0, 0};
  int nseg[2] = {0, 0}, max_n = 1;
  for (int i = 0; i < n; i++) {
    if (indices[i] < 0 || indices[i] >= (int)km->frames.size()) { ctx_set_error("rolo_keymap_extract: key-frame index out of range"); return ROLO_EINVAL; }
    for (int t = 0; t < 2; t++) { const int c = km->frames[indices[i]].n[t]; total[t] += c; if (c) nseg[t]++; max_n = std::max(max_n, c); }
  }
  if (total[0] > KM_MAX_POINTS || total[1] > KM_MAX_POINTS) { ctx_set_error("rolo_keymap_extract: more than ROLO_KEYMAP_MAX_POINTS points in one fused cloud"); return ROLO_EINVAL; }
  HIPCHK(hipSetDevice(km->device));
  hipStream_t s = km->stream;
  if (km->consumer_pending) { HIPCHK(hipStreamWaitEvent(s, km->consumed, 0)); km->consumer_pending = false; }   // the last reader of the sub-map this call overwrites
  km->have_submap = false;
  int rc;
  const int nmax = (int)std::max(total[0], total[1]);
  if (nmax > 0 && (rc = km_sort_scratch(km, nmax))) return rc;
  const size_t nsegs = (size_t)nseg[0] + nseg[1];
  if (nsegs) {
    if ((rc = km->store.grow_pinned(km->h_segs, km->h_segs_cap, nsegs, 64))) return rc;
    if ((rc = km->store.grow(km->segs, km->segs_cap, nsegs))) return rc;
  }
  for (int t = 0; t < 2; t++) {
    if ((rc = km->store.grow(km->cat[t], km->cat_cap[t], (size_t)std::max<long long>(total[t], 1)))) return rc;
    if ((rc = km->store.grow(km->sub[t], km->sub_cap[t], (size_t)std::max<long long>(total[t], 1)))) return rc;
  }
  // the segment table: corner segments, then surface segments, each in list order
  size_t k = 0;
  for (int t = 0; t < 2; t++) {
    int dst = 0;
    for (int i = 0; i < n; i++) {
      const rolo_keymap::Frame& f = km->frames[indices[i]];
      if (!f.n[t]) continue;
      Seg& g = km->h_segs[k++];
      g.src = f.pts[t]; g.n = f.n[t]; g.dst = dst;
      pcl_rows_of_rpyxyz(f.pose, g.T);
      dst += f.n[t];
    }
  }
  if (nsegs) HIPCHK(hipMemcpyAsync(km->segs, km->h_segs, nsegs * sizeof(Seg), hipMemcpyHostToDevice, s));
  const int gx = std::min((max_n + SM_THREADS - 1) / SM_THREADS, 128);
  for (int t = 0; t < 2; t++) {
    const Seg* base = km->segs + (t ? nseg[0] : 0);
    for (int y0 = 0; y0 < nseg[t]; y0 += 32768) {
      km_transform_kernel<<<dim3(gx, std::min(nseg[t] - y0, 32768)), SM_THREADS, 0, s>>>(base + y0, km->cat[t]);
      HIPCHK(hipGetLastError());
    }
    if ((rc = vg_enqueue_box(km, km->cat[t], (int)total[t], t))) return rc;
  }
  HIPCHK(hipStreamSynchronize(s));
  bool direct[2]; int m_direct[2] = {0, 0};
  const float leaf[2] = {corner_leaf, surf_leaf};
  for (int t = 0; t < 2; t++)
    if ((rc = vg_enqueue_filter(km, km->cat[t], (int)total[t], leaf[t], t, km->sub[t], &direct[t], &m_direct[t]))) return rc;
  HIPCHK(hipEventRecord(km->ready, s));
  HIPCHK(hipStreamSynchronize(s));
  for (int t = 0; t < 2; t++) km->m_sub[t] = direct[t] ? m_direct[t] : km->h_m[t];
  km->have_submap = true;
  if (m_corner) *m_corner = km->m_sub[0];
  if (m_surf) *m_surf = km->m_sub[1];
  return ROLO_OK;
}

int rolo_keymap_get_submap(rolo_keymap* km, float* corner_out, int cap_corner, float* surf_out, int cap_surf) {
  if (!km || cap_corner < 0 || cap_surf < 0) return ROLO_EINVAL;
  if (!km->have_submap) { ctx_set_error("the key map holds no sub-map: call rolo_keymap_extract first"); return ROLO_ESTATE; }
  if (km->m_sub[0] > cap_corner || km->m_sub[1] > cap_surf || (km->m_sub[0] && !corner_out) || (km->m_sub[1] && !surf_out)) return ROLO_EINVAL;
  HIPCHK(hipSetDevice(km->device));
  if (km->m_sub[0]) HIPCHK(hipMemcpyAsync(corner_out, km->sub[0], sizeof(float4) * (size_t)km->m_sub[0], hipMemcpyDeviceToHost, km->stream));
  if (km->m_sub[1]) HIPCHK(hipMemcpyAsync(surf_out, km->sub[1], sizeof(float4) * (size_t)km->m_sub[1], hipMemcpyDeviceToHost, km->stream));
  HIPCHK(hipStreamSynchronize(km->stream));
  return ROLO_OK;
}

int rolo_keymap_downsample(rolo_keymap* km, const float* pts, int n, float leaf, float* out, int* m) {
  if (!km || !m || n < 0 || (n && (!pts || !out)) || !(leaf > 0.f) || n > KM_MAX_POINTS) return ROLO_EINVAL;
  *m = 0;
  if (n == 0) return ROLO_OK;
  const float4* d = nullptr; int mm = 0;
  const int rc = keymap_stage_cloud(km, pts, n, leaf, &d, &mm);
  if (rc) return rc;
  if (mm) HIPCHK(hipMemcpy(out, d, sizeof(float4) * (size_t)mm, hipMemcpyDeviceToHost));
  *m = mm;
  return ROLO_OK;
}

int rolo_keyposes_select_nearby(const float* xyz, const double* times, int n, float search_radius, float density, double time_cur, double recent_seconds,
                                int32_t* out_indices, int cap) {
  if (n < 0 || cap < 0 || (n && (!xyz || !times)) || (cap && !out_indices) || !(density > 0.f) || !(search_radius >= 0.f)) return ROLO_EINVAL;
  if (n == 0) return 0;
  auto d2 = [&](const float* a, const float* b) { const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2]; return dx * dx + dy * dy + dz * dz; };
  const float* last = xyz + 3 * (size_t)(n - 1);
  // radiusSearch(cloudKeyPoses3D->back(), radius) :585
  const std::vector<std::pair<float, int>> near = radius_hits_last(xyz, n, search_radius);
  // downSizeFilterSurroundingKeyPoses :592-593 (intensity = index of the key pose)
  std::vector<std::array<float, 4>> poses, ds;
  for (const auto& e : near) poses.push_back({xyz[3 * (size_t)e.second], xyz[3 * (size_t)e.second + 1], xyz[3 * (size_t)e.second + 2], (float)e.second});
  host_voxelgrid(poses, density, ds);
  // :595-600 — each down-sampled pose takes the index of the nearest key pose
  for (auto& p : ds) {
    int best = 0; float bd = d2(p.data(), xyz);
    for (int i = 1; i < n; i++) { const float d = d2(p.data(), xyz + 3 * (size_t)i); if (d < bd) { bd = d; best = i; } }
    p[3] = (float)best;
  }
  // :604-611 — the key poses of the last recent_seconds, newest first
  for (int i = n - 1; i >= 0; --i) {
    if (time_cur - times[i] < recent_seconds) ds.push_back({xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], (float)i});
    else break;
  }
  // :626 — "if (pointDistance(cloudToExtract->points[i], cloudKeyPoses3D->back()) > surroundingKeyframeSearchRadius) continue"
  int count = 0;
  for (const auto& p : ds) {
    if (std::sqrt(d2(p.data(), last)) > search_radius) continue;
    if (count < cap) out_indices[count] = (int32_t)p[3];
    count++;
  }
  return count;
}

int rolo_keyposes_detect_loop_distance(const float* xyz, const double* times, int n, float search_radius, double time_diff, double time_cur, int32_t* loop_key_pre) {
  if (!loop_key_pre || n < 0 || (n && (!xyz || !times)) || !(search_radius >= 0.f)) return ROLO_EINVAL;
  *loop_key_pre = -1;
  // :2498-2506 — the first hit, nearest first, that is old enough; :2508 — none, or the last key itself
  for (const auto& e : radius_hits_last(xyz, n, search_radius))
    if (std::fabs(times[e.second] - time_cur) > time_diff) { if (e.second != n - 1) *loop_key_pre = e.second; break; }
  return ROLO_OK;
}

int rolo_keymap_loop_cloud(rolo_keymap* km, int slot, int key, int search_num, int wrt_key, float leaf, int* m) {
  if (!km || slot < 0 || slot > 1 || search_num < 0 || !(leaf > 0.f)) return ROLO_EINVAL;
  const int size = (int)km->frames.size();
  if (size > 0 && (key < 0 || key >= size)) { ctx_set_error("rolo_keymap_loop_cloud: key outside the store"); return ROLO_EINVAL; }
  if (wrt_key >= size) { ctx_set_error("rolo_keymap_loop_cloud: wrt_key outside the store"); return ROLO_EINVAL; }
  km->have_loop[slot] = false; km->m_loop[slot] = 0;
  // :2577-2585 / :2605-2611 — keyNear = key - searchNum .. key + searchNum inside the store; corner, then surface, of each
  const int lo = size ? (int)std::max<long long>((long long)key - search_num, 0) : 0, hi = size ? (int)std::min<long long>((long long)key + search_num, size - 1) : -1;
  long long total = 0;
  size_t nsegs = 0;
  int max_n = 1;
  for (int k = lo; k <= hi; k++) for (int t = 0; t < 2; t++) { const int c = km->frames[k].n[t]; total += c; if (c) nsegs++; max_n = std::max(max_n, c); }
  if (total > KM_MAX_POINTS) { ctx_set_error("rolo_keymap_loop_cloud: more than ROLO_KEYMAP_MAX_POINTS points in one loop cloud"); return ROLO_EINVAL; }
  HIPCHK(hipSetDevice(km->device));
  hipStream_t s = km->stream;
  if (!km->loop_t0) { HIPCHK(hipEventCreate(&km->loop_t0)); HIPCHK(hipEventCreate(&km->loop_t1)); }
  km->loop_ms[slot] = 0.f;
  if (total == 0) { km->have_loop[slot] = true; if (m) *m = 0; return ROLO_OK; }   // :2587 — "if (nearKeyframes->empty()) return"
  int rc;
  const int n = (int)total;
  if ((rc = km_sort_scratch(km, n))) return rc;
  if ((rc = km->store.grow_pinned(km->h_segs, km->h_segs_cap, nsegs, 64))) return rc;
  if ((rc = km->store.grow(km->segs, km->segs_cap, nsegs))) return rc;
  if ((rc = km->store.grow(km->cat[0], km->cat_cap[0], (size_t)n))) return rc;
  if ((rc = km->store.grow(km->loop[slot], km->loop_cap[slot], (size_t)n))) return rc;
  size_t q = 0;
  int dst = 0;
  for (int k = lo; k <= hi; k++) {
    const rolo_keymap::Frame& f = km->frames[k];
    for (int t = 0; t < 2; t++) {
      if (!f.n[t]) continue;
      Seg& g = km->h_segs[q++];
      g.src = f.pts[t]; g.n = f.n[t]; g.dst = dst;
      pcl_rows_of_rpyxyz(wrt_key >= 0 ? km->frames[wrt_key].pose : f.pose, g.T);
      dst += f.n[t];
    }
  }
  HIPCHK(hipEventRecord(km->loop_t0, s));
  HIPCHK(hipMemcpyAsync(km->segs, km->h_segs, nsegs * sizeof(Seg), hipMemcpyHostToDevice, s));
  const int gx = std::min((max_n + SM_THREADS - 1) / SM_THREADS, 128);
  for (size_t y0 = 0; y0 < nsegs; y0 += 32768) {
    km_transform_kernel<<<dim3(gx, (unsigned)std::min<size_t>(nsegs - y0, 32768)), SM_THREADS, 0, s>>>(km->segs + y0, km->cat[0]);
    HIPCHK(hipGetLastError());
  }
  if ((rc = vg_enqueue_box(km, km->cat[0], n, 0))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  // :2593-2595 — ONE downSizeFilterICP over corner and surface together
  bool direct; int m_direct = 0;
  if ((rc = vg_enqueue_filter(km, km->cat[0], n, leaf, 0, km->loop[slot], &direct, &m_direct))) return rc;
  HIPCHK(hipEventRecord(km->loop_t1, s));
  HIPCHK(hipStreamSynchronize(s));
  const int mm = direct ? m_direct : km->h_m[0];
  if (mm < 0 || mm > n) { ctx_set_error("the key map's voxel filter returned an inconsistent cell count"); return ROLO_ESTATE; }
  (void)hipEventElapsedTime(&km->loop_ms[slot], km->loop_t0, km->loop_t1);
  km->m_loop[slot] = mm; km->have_loop[slot] = true;
  if (m) *m = mm;
  return ROLO_OK;
}

int rolo_keymap_get_loop_cloud(rolo_keymap* km, int slot, float* out, int cap) {
  if (!km || slot < 0 || slot > 1 || cap < 0) return ROLO_EINVAL;
  if (!km->have_loop[slot]) { ctx_set_error("the key map holds no loop cloud in this slot: call rolo_keymap_loop_cloud first"); return ROLO_ESTATE; }
  const int mm = km->m_loop[slot];
  if (mm > cap || (mm && !out)) return ROLO_EINVAL;
  HIPCHK(hipSetDevice(km->device));
  if (mm) HIPCHK(hipMemcpyAsync(out, km->loop[slot], sizeof(float4) * (size_t)mm, hipMemcpyDeviceToHost, km->stream));
  HIPCHK(hipStreamSynchronize(km->stream));
  return mm;
}

// publishGlobalMap :1656-1663 — every listed frame's corner, then surface cloud moved by its pose, ONE downSizeFilterGlobalMapKeyFrames over all of them
int rolo_keymap_global_map(rolo_keymap* km, const int32_t* indices, int n, float leaf, int* m) {
  if (!km || n < 0 || (n && !indices) || !(leaf > 0.f)) return ROLO_EINVAL;
  km->have_gmap = false; km->m_gmap = 0;
  for (long long& v : km->gm_info) v = 0;
  for (float& v : km->gm_ms) v = 0.f;
  std::vector<GmPiece> pieces;
  long long total = 0;
  int rc;
  if ((rc = gm_list(km, indices, n, "rolo_keymap_global_map", pieces, &total))) return rc;
  km->gm_info[0] = total;
  if (total == 0) { km->have_gmap = true; if (m) *m = 0; return ROLO_OK; }
  HIPCHK(hipSetDevice(km->device));
  hipStream_t s = km->stream;
  for (hipEvent_t& e : km->gm_ev) if (!e) HIPCHK(hipEventCreate(&e));
  const int batch = gm_batch_of(km);
  int mm = 0;
  HIPCHK(hipEventRecord(km->gm_ev[0], s));
  if (total > batch) {
    if ((rc = gm_streamed(km, pieces, total, batch, leaf, &mm))) return rc;
  } else {   // the one-shot form: rolo_keymap_loop_cloud's route, no new arithmetic
    const int np = (int)total;
    if ((rc = km_sort_scratch(km, np))) return rc;
    if ((rc = gm_batch_scratch(km, np, pieces.size()))) return rc;
    if ((rc = km->store.grow(km->gmap, km->gmap_cap, (size_t)np))) return rc;
    size_t cursor = 0;
    if ((rc = gm_enqueue_batch(km, pieces, &cursor, 0, np))) return rc;
    if ((rc = vg_enqueue_box(km, km->cat[0], np, 0))) return rc;
    HIPCHK(hipEventRecord(km->gm_ev[1], s));
    HIPCHK(hipStreamSynchronize(s));
    bool direct; int m_direct = 0;
    if ((rc = vg_enqueue_filter(km, km->cat[0], np, leaf, 0, km->gmap, &direct, &m_direct))) return rc;
    HIPCHK(hipEventRecord(km->gm_ev[2], s));
    HIPCHK(hipEventRecord(km->gm_ev[3], s));
    HIPCHK(hipStreamSynchronize(s));
    mm = direct ? m_direct : km->h_m[0];
    if (mm < 0 || mm > np) { ctx_set_error("the key map's voxel filter returned an inconsistent cell count"); return ROLO_ESTATE; }
    km->gm_info[1] = 1; km->gm_info[2] = mm; km->gm_info[3] = 0; km->gm_info[4] = 0;
  }
  for (int k = 0; k < 3; k++) (void)hipEventElapsedTime(&km->gm_ms[k], km->gm_ev[k], km->gm_ev[k + 1]);
  km->m_gmap = mm; km->have_gmap = true;
  if (m) *m = mm;
  return ROLO_OK;
}

int rolo_keymap_get_global_map(rolo_keymap* km, float* out, int cap) {
  if (!km || cap < 0) return ROLO_EINVAL;
  if (!km->have_gmap) { ctx_set_error("the key map holds no global map: call rolo_keymap_global_map first"); return ROLO_ESTATE; }
  const int mm = km->m_gmap;
  if (mm > cap || (mm && !out)) return ROLO_EINVAL;
  HIPCHK(hipSetDevice(km->device));
  if (mm) HIPCHK(hipMemcpyAsync(out, km->gmap, sizeof(float4) * (size_t)mm, hipMemcpyDeviceToHost, km->stream));
  HIPCHK(hipStreamSynchronize(km->stream));
  return mm;
}

int rolo_keymap_global_set_batch(rolo_keymap* km, int points) {
  if (!km || points < 0 || points > KM_MAX_POINTS) return ROLO_EINVAL;
  km->gm_batch = points;
  return ROLO_OK;
}

int rolo_keymap_global_info(rolo_keymap* km, long long* out, int n) {
  if (!km || n < 0 || (n && !out)) return ROLO_EINVAL;
  for (int k = 0; k < std::min(n, 5); k++) out[k] = km->gm_info[k];
  return ROLO_OK;
}

int rolo_keymap_global_last_ms(rolo_keymap* km, float* ms3) {
  if (!km || !ms3) return ROLO_EINVAL;
  for (int k = 0; k < 3; k++) ms3[k] = km->gm_ms[k];
  return ROLO_OK;
}

// saveGlobalPCDs :1546-1557 — cloudGlobal.pcd's cloud: a batch at a time through the scratch into the caller's array
long long rolo_keymap_global_cloud(rolo_keymap* km, const int32_t* indices, int n, float* out, long long cap) {
  if (!km || n < 0 || (n && !indices) || cap < 0) return ROLO_EINVAL;
  std::vector<GmPiece> pieces;
  long long total = 0;
  int rc;
  if ((rc = gm_list(km, indices, n, "rolo_keymap_global_cloud", pieces, &total))) return rc;
  if (total > cap || (total && !out)) { ctx_set_error("rolo_keymap_global_cloud: the output array is smaller than the listed clouds"); return ROLO_EINVAL; }
  if (total == 0) return 0;
  HIPCHK(hipSetDevice(km->device));
  const int batch = (int)std::min<long long>(gm_batch_of(km), total);
  if ((rc = gm_batch_scratch(km, batch, pieces.size()))) return rc;
  size_t cursor = 0;
  for (long long b0 = 0; b0 < total; b0 += batch) {
    const int nb = (int)std::min<long long>(batch, total - b0);
    if ((rc = gm_enqueue_batch(km, pieces, &cursor, b0, nb))) return rc;
    HIPCHK(hipMemcpyAsync(out + 4 * b0, km->cat[0], sizeof(float4) * (size_t)nb, hipMemcpyDeviceToHost, km->stream));
    HIPCHK(hipStreamSynchronize(km->stream));
  }
  return total;
}

}  // extern "C"
