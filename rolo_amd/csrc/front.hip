// K1-K4 — the front end on gfx950.
// Replaces ImageProjection::projectPointCloud / cloudExtraction (reference src/imageProjection.cpp:399-505) and
// FeatureExtraction::calculateSmoothness / markOccludedPoints / extractFeatures incl. pcl::VoxelGrid
// (reference src/featureExtraction.cpp:87-266). De-skew (deskewPoint :368-396, off in every shipped config) is applied when
// armed with rolo_front_set_deskew: per-point times from the caller, from the message, or interpolated from the azimuth
// (deskewCloudInfo :270-327) when the cloud carries none.
//
// MI355X design. The reference's three serial loops become:
//   K1  one thread per raw point; "first point to claim a pixel wins" (imageProjection.cpp:451) is an atomicMin of
//       the raw point index on a per-pixel owner word — the smallest index is exactly the serial winner;
//   K2  row-major stream compaction: one workgroup per ring does an LDS prefix scan of its valid pixels, a second
//       pass adds the ring offsets and scatters (x,y,z,intensity), column and range — coalesced on both sides;
//   K3  a stencil kernel (11-tap float sum in the reference's written order) plus a mark kernel — the marks only
//       ever store 1 and depend only on ranges / columns, so the serial loop is order-free;
//   K4  (front_extract.hpp, with K3 inside) one workgroup of 1024 threads per ring, everything for the ring staged in LDS: all six sectors in one segmented bitonic sort of
//       packed (curvature bits << 32 | index) keys; the greedy corner / surface picks — a serial walk in the reference — as the equivalent
//       fixed point "picked iff no better-ranked candidate that reaches it is picked", every lane owning a position, a few rounds per
//       sector (only the two sectors touching the cloud ends keep the serial walk); the label<=0 collection is a ballot
//       compaction, and pcl::VoxelGrid is a second bitonic sort of (cell << 32 | order) keys followed by per-run centroids.
// fp32 arithmetic follows the reference expression by expression; this file is compiled with -ffp-contract=off.
#include "ctx_access.hpp"
#include <atomic>
#include "dev_math.hpp"
#include "front_extract.hpp"   // K3 + K4: extract_kernel in phases, FeatArgs, XT, the ring's working set (front_ring_bytes, FRONT_GUARD)
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

namespace rolo {

constexpr int FRONT_MAX_H = 2048;      // Horizon_SCAN up to here: one ring's working set lives in LDS (shipped configs: 1024, 1800, 2048)
constexpr int FRONT_MAX_H_BIG = 4096;  // ... and up to here in a per-ring scratch area in HBM (the same kernel through global pointers: correct, several times slower;
                                       // no sensor the reference accepts has that many columns — its params.yaml mentions a Livox Horizon at 4000)

namespace {

// ---- sensor_msgs/PointCloud2 payload -> x, y, z / ring / per-point time -----------------------------------------------
// What pcl::moveFromROSMsg + the Ouster conversion loop do on the host in ImageProjection::cachePointCloud
// (imageProjection.cpp:188-212): fields are found by their byte offsets in the message, Velodyne "time" is a float in
// seconds, Ouster "t" a uint32 in nanoseconds (dst.time = src.t * 1e-9f), ring is uint16 (Velodyne) or uint8 (Ouster).
// Byte-wise loads: a point_step of 22 (the velodyne driver's packed layout) has no alignment to offer.
ROLO_DEV unsigned load_u32_bytes(const unsigned char* p) { return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24); }

__global__ __launch_bounds__(256) void unpack_cloud_kernel(const unsigned char* __restrict__ data, rolo_cloud_layout L, int n, float* __restrict__ xyz,
                                                          unsigned short* __restrict__ ring, float* __restrict__ rel_time) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned char* p = data + (size_t)i * L.point_step;
  xyz[3 * (size_t)i] = __uint_as_float(load_u32_bytes(p + L.off_x));
  xyz[3 * (size_t)i + 1] = __uint_as_float(load_u32_bytes(p + L.off_y));
  xyz[3 * (size_t)i + 2] = __uint_as_float(load_u32_bytes(p + L.off_z));
  ring[i] = L.ring_bytes == 1 ? (unsigned short)p[L.off_ring] : (unsigned short)(p[L.off_ring] | (p[L.off_ring + 1] << 8));
  float t = 0.f;
  if (L.time_kind == 1) t = __uint_as_float(load_u32_bytes(p + L.off_time));
  else if (L.time_kind == 2) t = (float)load_u32_bytes(p + L.off_time) * 1e-9f;   // :209
  rel_time[i] = fabsf(t);                                                          // deskewCloudInfo :358-359
}

// ---- per-point times of a cloud without a time field: deskewCloudInfo, timeFlag == -1 (imageProjection.cpp:270-327) ----
// The reference interpolates the time from the azimuth in a serial loop with one flag, halfPassed, that flips at the first
// point whose (first-half-adjusted) azimuth is more than pi past the start: a prefix property. Kernel 1 finds that point
// (atomicMin), kernel 2 applies the first-half rule up to and including it and the second-half rule after it.
// Every angle is the CORRECTLY ROUNDED float atan2 — (float)atan2((double)y, (double)x), K1's remedy (below) without the guard: the rule compares the angle with
// seven thresholds, and on adjacent floats planted on either side of them the device's atan2f, one ulp off, takes the other side on a large share
// (tests/test_gpu_deskew_cases.py) — a time a whole scan period off, or the other rule for every later point — and where it takes the right side the bits of the time
// still follow the angle. The fp64 function is good to a few fp64 ulps, so its rounding to float is the correctly rounded float unless the true value lies within
// ~2^-50 of the midpoint of two floats. These kernels run only for a de-skew armed without times.
ROLO_DEV float azimuth_of(const float* __restrict__ pts, int stride, int i) {
  return -(float)atan2((double)pts[(size_t)i * stride + 1], (double)pts[(size_t)i * stride]);   // point.x = in.y, point.z = in.x (:303-307)
}
struct AzimuthRef { float start, end, diff; };
ROLO_DEV AzimuthRef azimuth_ref(const float* __restrict__ pts, int stride, int n) {
  float start = azimuth_of(pts, stride, 0);                                                        // :272
  float end = (float)((double)azimuth_of(pts, stride, n - 1) + 2 * M_PI);                          // :273
  if ((double)(end - start) > 3 * M_PI) end = (float)((double)end - 2 * M_PI);                     // :274-277
  else if ((double)(end - start) < M_PI) end = (float)((double)end + 2 * M_PI);
  return AzimuthRef{start, end, end - start};
}
ROLO_DEV float azimuth_first_half(float ori, float start) {
  if ((double)ori < (double)start - M_PI / 2) ori = (float)((double)ori + 2 * M_PI);
  else if ((double)ori > (double)start + M_PI * 3 / 2) ori = (float)((double)ori - 2 * M_PI);
  return ori;
}
__global__ __launch_bounds__(256) void azimuth_flag_kernel(const float* __restrict__ pts, int stride, int n, int* __restrict__ first_passed) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const AzimuthRef r = azimuth_ref(pts, stride, n);
  const float a = azimuth_first_half(azimuth_of(pts, stride, i), r.start);
  if ((double)(a - r.start) > M_PI) atomicMin(first_passed, i);
}
__global__ __launch_bounds__(256) void azimuth_time_kernel(const float* __restrict__ pts, int stride, int n, float scan_period,
                                                          const int* __restrict__ first_passed, float* __restrict__ rel_time) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const AzimuthRef r = azimuth_ref(pts, stride, n);
  float ori = azimuth_of(pts, stride, i);
  if (i <= *first_passed) {
    ori = azimuth_first_half(ori, r.start);
  } else {                                                                                          // :316-322
    ori = (float)((double)ori + 2 * M_PI);
    if ((double)ori < (double)r.end - M_PI * 3 / 2) ori = (float)((double)ori + 2 * M_PI);
    else if ((double)ori > (double)r.end + M_PI / 2) ori = (float)((double)ori - 2 * M_PI);
  }
  const float relTime = (ori - r.start) / r.diff;                                                   // :324
  rel_time[i] = scan_period * relTime;                                                              // :325
}

// ---- K1 ------------------------------------------------------------------------------------------------
// The column of a point is the reference's expression on the CORRECTLY ROUNDED float atan2(x, y) — what a correctly rounded libm's atan2f returns by definition,
// and the only value two machines can agree on. The device's atan2f is not that: on adjacent floats planted on either side of a column edge it is one ulp away on
// nearly half of them, and there one ulp is the neighbouring pixel (tests/test_gpu_projection_cases.py). As voxel_dev.hpp does for the POLAR key, the fast function
// decides except where the quotient q whose rounding gives the column lies within a guard of a half-integer; there the angle is taken again as
// (float)atan2((double)x, (double)y): the fp64 function is good to a few fp64 ulps, so its rounding to float is the correctly rounded float unless the true value lies
// within ~2^-50 of the midpoint of two floats.
// The guard. Let the fast angle be E float ulps from the correctly rounded one: |da| <= E 2^-22 rad (|a| <= pi < 4). t = fl(a * 180) < 1024 moves by at most
// 180 |da| + 2^-14 (one ulp of t for the two roundings), horizonAngle = fl(t / pi) by at most 180 / pi |da| + 2^-14 / pi + 2^-16 (one ulp of an angle < 256 deg)
// = (0.895 E + 2.27) ulp(180 deg) with ulp(180 deg) = 2^-16 deg, and q by that over ang_res_x. HIP's math API reference lists atan2f at 1 ulp — a largest OBSERVED
// error, so E = 2 here — and the guard is (E + 3) ulp(180 deg) / ang_res_x >= the bound: 9e-4 of a column at H = 4096, so one point in 600 takes the fp64 function.
constexpr double COLUMN_GUARD_DEG = (2 + 3) * 0x1p-16;
ROLO_DEV int column_of_angle(float angle, float ang_res_x, int H, double& q) {
  const float horizonAngle = angle * 180 / M_PI;                  // imageProjection.cpp:437
  q = (horizonAngle - 90.0) / ang_res_x;
  return -round(q) + H / 2;                                       // :440
}

__global__ __launch_bounds__(256) void project_kernel(const float* __restrict__ pts, int stride, const unsigned short* __restrict__ ring,
                                                     int n_raw, rolo_front_params P, int* __restrict__ owner) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_raw) return;
  const float x = pts[(size_t)i * stride], y = pts[(size_t)i * stride + 1], z = pts[(size_t)i * stride + 2];
  const float range = sqrtf(x * x + y * y + z * z);  // utility.h:462-465
  if (range < P.lidar_min_range || range > P.lidar_max_range) return;
  // NaN coordinates (the node refuses clouds that are not is_dense, :226-231): the reference's column index is then the int
  // conversion of NaN — INT_MIN on x86, i.e. the point is dropped; the device conversion would give 0
  if (range != range) return;
  const int rowIdn = ring[i];
  if (rowIdn < 0 || rowIdn >= P.n_scan) return;
  if (rowIdn % P.downsample_rate != 0) return;
  const int H = P.horizon_scan;
  const float ang_res_x = 360.0 / float(H);                       // :438
  double q;
  int columnIdn = column_of_angle(atan2f(x, y), ang_res_x, H, q);
  if (fabs(q - floor(q) - 0.5) < COLUMN_GUARD_DEG / ang_res_x) columnIdn = column_of_angle((float)atan2((double)x, (double)y), ang_res_x, H, q);
  if (columnIdn >= H) columnIdn -= H;
  if (columnIdn < 0 || columnIdn >= H) return;
  atomicMin(&owner[rowIdn * H + columnIdn], i);  // first point wins (:451)
}

// ---- K2 pass A: per ring, local index of every valid pixel + ring count ----
__global__ __launch_bounds__(256) void ring_scan_kernel(const int* __restrict__ owner, int H, int* __restrict__ local_idx, int* __restrict__ ring_count) {
  __shared__ int wsum[4];
  __shared__ int carry;
  const int row = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < H; base += 256) {
    const int j = base + t;
    const int v = (j < H && owner[row * H + j] != INT_MAX) ? 1 : 0;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { int o = __shfl_up(inc, off, 64); if (lane >= off) inc += o; }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wv; w++) woff += wsum[w];
    const int c = carry;
    if (j < H) local_idx[row * H + j] = v ? (c + woff + inc - 1) : -1;
    __syncthreads();
    if (t == 255) carry = c + woff + inc;
    __syncthreads();
  }
  if (t == 0) ring_count[row] = carry;
}

// ---- K2 pass B: ring offsets, start/end ring index, scatter ----
// ImageProjection::deskewPoint (imageProjection.cpp:368-396), rotation only, for clouds with a per-point time:
// rel_time[i] = fabs(point.time) (what deskewCloudInfo :358-359 leaves in deskewCloud->points[i].intensity)
struct DeskewArgs { const float* rel_time; float incre_r, incre_p, incre_y, scan_period; double odom_time_diff; };

ROLO_DEV void deskew_point(const DeskewArgs& d, float rel_time_f, float& x, float& y, float& z) {
  const double relTime = (double)rel_time_f;
  const float ratio = relTime / d.scan_period;                     // :380 double / float, stored float
  const float s1 = (float)(d.scan_period / d.odom_time_diff);      // :383 float / double; Eigen casts the scalar to float
  const float roll = -(d.incre_r * s1 * ratio), pitch = -(d.incre_p * s1 * ratio), yaw = -(d.incre_y * s1 * ratio);
  // pcl::getTransformation(0, 0, 0, roll, pitch, yaw), float (:386)
  const float A = cosf(yaw), B = sinf(yaw), C = cosf(pitch), D = sinf(pitch), E = cosf(roll), F = sinf(roll), DE = D * E, DF = D * F;
  const float nx = (A * C) * x + (A * DF - B * E) * y + (B * F + A * DE) * z + 0.f;   // :389-391
  const float ny = (B * C) * x + (A * E + B * DF) * y + (B * DE - A * F) * z + 0.f;
  const float nz = (-D) * x + (C * F) * y + (C * E) * z + 0.f;
  x = nx; y = ny; z = nz;
}

__global__ __launch_bounds__(256) void ring_scatter_kernel(const float* __restrict__ pts, int stride, const unsigned short* __restrict__ ring,
                                                          const int* __restrict__ owner, const int* __restrict__ local_idx,
                                                          const int* __restrict__ ring_count, int n_scan, int H, float4* __restrict__ extracted,
                                                          int* __restrict__ col_ind, float* __restrict__ point_range, int* __restrict__ start_ring,
                                                          int* __restrict__ end_ring, float* __restrict__ range_mat, int* __restrict__ n_valid,
                                                          DeskewArgs dsk) {
  __shared__ int s_off;
  const int row = blockIdx.x, t = threadIdx.x;
  if (t == 0) {
    int off = 0;
    for (int r = 0; r < row; r++) off += ring_count[r];
    s_off = off;
    start_ring[row] = off - 1 + 5;                     // imageProjection.cpp:485
    end_ring[row] = off + ring_count[row] - 1 - 5;     // :503
    if (row == n_scan - 1) *n_valid = off + ring_count[row];
  }
  __syncthreads();
  const int off = s_off;
  for (int j = t; j < H; j += 256) {
    const int o = owner[row * H + j];
    float rng = FLT_MAX;
    if (o != INT_MAX) {
      const float x = pts[(size_t)o * stride], y = pts[(size_t)o * stride + 1], z = pts[(size_t)o * stride + 2];
      rng = sqrtf(x * x + y * y + z * z);
      const int dst = off + local_idx[row * H + j];
      float sx = x, sy = y, sz = z;
      if (dsk.rel_time) deskew_point(dsk, dsk.rel_time[o], sx, sy, sz);  // :454 — range and pixel come from the raw point
      extracted[dst] = make_float4(sx, sy, sz, ring[o] * z);  // intensity <- ring * z (:410)
      col_ind[dst] = j;
      point_range[dst] = rng;
    }
    if (range_mat) range_mat[row * H + j] = rng;
  }
}

// ---- K3 (calculateSmoothness, markOccludedPoints) and K4: extract_kernel, front_extract.hpp (K3 is its window load) ----

// concatenate per-ring / per-sector staging areas in order
__global__ __launch_bounds__(256) void concat_kernel(const float4* __restrict__ stage, const int* __restrict__ cnt, int n_groups, int group_cap,
                                                    float4* __restrict__ out, int* __restrict__ total) {
  __shared__ int s_off, s_part[4];
  const int g = blockIdx.x, t = threadIdx.x;
  // offset of this group = sum of the counts before it: all 256 threads share the (up to n_scan * 6) loads
  int part = 0;
  for (int r = t; r < g; r += 256) part += cnt[r];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
  if ((t & 63) == 0) s_part[t >> 6] = part;
  __syncthreads();
  if (t == 0) {
    const int off = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    s_off = off;
    if (g == n_groups - 1) *total = off + cnt[g];
  }
  __syncthreads();
  const int c = cnt[g];
  for (int i = t; i < c; i += 256) out[s_off + i] = stage[(size_t)g * group_cap + i];
}

// fused frame path: corner groups (n_scan x 6 sectors, <= 20 each) then surface groups (one per ring) straight into *featureLast =
// corner ++ surface (lidarOdometry.cpp:521-523) — the two concat launches and feature_concat_kernel in one; counts to counters[1], [2]
__global__ __launch_bounds__(256) void feature_gather_kernel(const float4* __restrict__ corner_stage, const int* __restrict__ corner_cnt, int n_cgroups,
                                                            const float4* __restrict__ surf_stage, const int* __restrict__ surf_cnt, int n_sgroups, int surf_cap,
                                                            float4* __restrict__ out, int* __restrict__ counters, int* __restrict__ pub3) {
  __shared__ int s_part[2][4], s_off;
  const int g = blockIdx.x, t = threadIdx.x;
  const bool is_surf = g >= n_cgroups;
  const int gs = is_surf ? g - n_cgroups : g;
  // corners before this group (every corner for a surface group) + surface points before this group
  int pc = 0, ps = 0;
  for (int r = t; r < (is_surf ? n_cgroups : gs); r += 256) pc += corner_cnt[r];
  if (is_surf) for (int r = t; r < gs; r += 256) ps += surf_cnt[r];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { pc += __shfl_xor(pc, off, 64); ps += __shfl_xor(ps, off, 64); }
  if ((t & 63) == 0) { s_part[0][t >> 6] = pc; s_part[1][t >> 6] = ps; }
  __syncthreads();
  if (t == 0) {
    const int oc = s_part[0][0] + s_part[0][1] + s_part[0][2] + s_part[0][3], os = s_part[1][0] + s_part[1][1] + s_part[1][2] + s_part[1][3];
    s_off = oc + os;
    // pub3: the caller's pinned (n_valid, n_corner, n_surface) — written here instead of by a copy launch behind this kernel
    if (g == n_cgroups - 1) { const int v = oc + corner_cnt[gs]; counters[1] = v; if (pub3) { pub3[1] = v; pub3[0] = counters[0]; } }
    if (is_surf && gs == n_sgroups - 1) { const int v = os + surf_cnt[gs]; counters[2] = v; if (pub3) pub3[2] = v; }
  }
  __syncthreads();
  const int c = is_surf ? surf_cnt[gs] : corner_cnt[gs];
  const float4* __restrict__ src = is_surf ? surf_stage + (size_t)gs * surf_cap : corner_stage + (size_t)gs * 20;
  for (int i = t; i < c; i += 256) out[s_off + i] = src[i];
}

// one launch instead of six fills per frame: owner = INT_MAX (npix), and zeros for col / range / curv / picked / label incl. their guard cells (np)
__global__ __launch_bounds__(256) void front_clear_kernel(int* owner, size_t npix, int* col, float* range, float* curv, int* picked, int* label, size_t np) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (size_t)gridDim.x * blockDim.x;
  for (size_t i = t; i < np; i += nt) {
    if (i < npix) owner[i] = INT_MAX;
    col[i] = 0; range[i] = 0.f; curv[i] = 0.f; picked[i] = 0; label[i] = 0;
  }
}

__global__ void fill_int_kernel(int* p, int n, int v) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = v;
}


struct Front {
  int device = 0;
  DevStore store;   // every buffer below; none of them is part of a captured frame
  size_t cap_pix = 0, cap_scan = 0;   // the pixel and the ring group: set once every buffer of the group is allocated
  float* raw = nullptr; size_t cap_raw = 0; unsigned short* ring = nullptr; size_t cap_ring = 0;   // staged records (floats) and their rings (points)
  int *owner = nullptr, *local_idx = nullptr, *ring_count = nullptr, *start_ring = nullptr, *end_ring = nullptr, *counters = nullptr;
  float4* extracted = nullptr; int* col = nullptr; float* range = nullptr; float* range_mat = nullptr;
  float* curv = nullptr; int *picked = nullptr, *label = nullptr;
  float4 *corner_stage = nullptr, *surf_stage = nullptr, *corner_out = nullptr, *surf_out = nullptr;
  int *corner_cnt = nullptr, *surf_cnt = nullptr;
  int* paths = nullptr; bool paths_valid = false;   // per-ring path words of the last extraction (rolo_debug_extract_paths)
  unsigned char* big = nullptr; int maxh = FRONT_MAX_H, cap_maxh = 0;   // Horizon_SCAN > 2048: per-ring scratch of the extract kernel, staging pitch
  int n_valid = 0; int n_scan = 0, H = 0;
  bool projected = false;
  bool extract_cleared = false;   // the projection's clear launch already zeroed curv / picked / label for the extraction that follows
  size_t precleared_np = 0;       // fused frames: the per-point arrays (np elements) were cleared BEHIND the previous frame's features, off the next frame's critical path (0: not)
  // rolo_front_set_deskew: armed for the next projection only
  bool deskew_armed = false;
  int deskew_n = 0;   // length of the armed per-point time array
  DeskewArgs deskew{};
  float* rel_time = nullptr; size_t cap_time = 0;   // staging when the times come from the host
  const float* last_times = nullptr; int last_times_n = 0; bool last_times_azimuth = false;   // what the last projection de-skewed with (rolo_debug_front_times); nullptr: it did not
  bool deskew_from_msg = false;                      // armed without times: the next message brings them
  // message-level entry: raw payload and what the unpack kernel makes of it
  unsigned char* msg_raw = nullptr; size_t cap_msg = 0;
  float* msg_xyz = nullptr; unsigned short* msg_ring = nullptr; float* msg_time = nullptr; size_t cap_msg_xyz = 0, cap_msg_ring = 0, cap_msg_time = 0;
};

thread_local std::string g_ferr;

}  // namespace

namespace {

// the front-end state of a context, created on first use
Front* front_of(rolo_ctx* c) {
  void** slot = ctx_front_slot(c);
  if (!*slot) {
    Front* f = new Front();
    f->store.stream = ctx_stream(c); f->store.who = "front end";
    *slot = f;
  }
  return static_cast<Front*>(*slot);
}

// device buffers for frames of up to n_raw points / n_scan x horizon_scan pixels
int front_prepare(rolo_ctx* c, const rolo_front_params* P, int n_raw, int stride, bool stage_raw, Front** out) {
  if (P->n_scan <= 0 || P->horizon_scan <= 0 || P->downsample_rate <= 0) { ctx_set_error("bad front params"); return ROLO_EINVAL; }
  if (P->horizon_scan > FRONT_MAX_H_BIG) { ctx_set_error("Horizon_SCAN above the limit of this build (4096)"); return ROLO_EUNSUPPORTED; }
  HIPCHK(hipSetDevice(ctx_device(c)));
  Front* f = front_of(c);
  f->device = ctx_device(c);
  f->projected = false; f->paths_valid = false; f->last_times = nullptr;   // (before the buffers change: what an earlier frame left is gone either way)
  const int NS = P->n_scan, H = P->horizon_scan;
  const size_t npix = (size_t)NS * H;
  DevStore& st = f->store;
  int rc;
  // two capacities: floats of the staged records (n_raw * stride) and points (ring) — a later frame with a smaller stride can hold
  // more points inside the same float capacity
  if (stage_raw && ((rc = st.grow(f->raw, f->cap_raw, (size_t)n_raw * stride)) || (rc = st.grow(f->ring, f->cap_ring, (size_t)n_raw)))) return rc;
  // a group's capacity is set once every buffer of the group is there: after a failed allocation the next call allocates the group again
  if (npix > f->cap_pix) {
    const size_t np = npix + 2 * FRONT_GUARD;
    f->cap_pix = 0; f->precleared_np = 0;   // fresh buffers: not cleared
    if ((rc = st.alloc(f->owner, npix)) || (rc = st.alloc(f->local_idx, npix)) || (rc = st.alloc(f->extracted, np)) || (rc = st.alloc(f->col, np)) ||
        (rc = st.alloc(f->range, np)) || (rc = st.alloc(f->range_mat, npix)) || (rc = st.alloc(f->curv, np)) || (rc = st.alloc(f->picked, np)) ||
        (rc = st.alloc(f->label, np)) || (rc = st.alloc(f->corner_out, npix)) || (rc = st.alloc(f->surf_out, npix))) return rc;
    f->cap_pix = npix;
  }
  const int maxh = H > FRONT_MAX_H ? FRONT_MAX_H_BIG : FRONT_MAX_H;   // pitch of the per-ring staging rows, and which extract kernel runs
  if ((size_t)NS > f->cap_scan || maxh > f->cap_maxh) {
    const size_t ns = (size_t)NS;
    f->cap_scan = 0; f->cap_maxh = 0;
    if ((rc = st.alloc(f->ring_count, ns)) || (rc = st.alloc(f->start_ring, ns)) || (rc = st.alloc(f->end_ring, ns)) || (rc = st.alloc(f->counters, 8)) ||
        (rc = st.alloc(f->corner_stage, ns * 6 * 20)) || (rc = st.alloc(f->corner_cnt, ns * 6)) || (rc = st.alloc(f->surf_stage, ns * maxh)) ||
        (rc = st.alloc(f->surf_cnt, ns)) || (rc = st.alloc(f->paths, ns)) ||
        (maxh > FRONT_MAX_H && (rc = st.alloc(f->big, ns * front_ring_bytes(FRONT_MAX_H_BIG))))) return rc;
    f->cap_scan = ns; f->cap_maxh = maxh;
  }
  f->maxh = maxh;
  f->n_scan = NS; f->H = H;
  *out = f;
  return ROLO_OK;
}

// K1 + K2 on raw points that are on the device; N lands in counters[0]. No host synchronisation.
int front_project_enqueue(Front* f, const rolo_front_params* P, const float* d_pts, int stride, const unsigned short* d_ring, int n_raw, bool want_range_mat,
                          hipStream_t s) {
  const int NS = f->n_scan, H = f->H;
  const size_t npix = (size_t)NS * H;
  bool from_azimuth = false;
  if (f->deskew_from_msg) {   // armed without times and no time field came with the points: interpolate them from the azimuth
    f->deskew_from_msg = false;
    if (n_raw > 0) {
      if (int rc = f->store.grow(f->rel_time, f->cap_time, (size_t)n_raw)) return rc;
      fill_int_kernel<<<1, 64, 0, s>>>(f->counters + 4, 1, INT_MAX);
      azimuth_flag_kernel<<<(n_raw + 255) / 256, 256, 0, s>>>(d_pts, stride, n_raw, f->counters + 4);
      azimuth_time_kernel<<<(n_raw + 255) / 256, 256, 0, s>>>(d_pts, stride, n_raw, f->deskew.scan_period, f->counters + 4, f->rel_time);
      f->deskew.rel_time = f->rel_time;
      f->deskew_armed = true; f->deskew_n = n_raw;
      from_azimuth = true;
    }
  }
  if (f->deskew_armed && f->deskew_n < n_raw) {   // ring_scatter_kernel reads rel_time[o] for every raw point of this frame
    f->deskew_armed = false;
    ctx_set_error("de-skew armed with fewer per-point times than the frame has points");
    return ROLO_EINVAL;
  }
  // guard cells of the per-point arrays are zero; the three arrays of the extraction stage are cleared in the same launch
  if (f->precleared_np != npix + 2 * FRONT_GUARD)   // (a fused frame leaves the arrays cleared for its successor)
    front_clear_kernel<<<512, 256, 0, s>>>(f->owner, npix, f->col, f->range, f->curv, f->picked, f->label, npix + 2 * FRONT_GUARD);
  f->precleared_np = 0;
  f->extract_cleared = true;
  if (n_raw > 0) project_kernel<<<(n_raw + 255) / 256, 256, 0, s>>>(d_pts, stride, d_ring, n_raw, *P, f->owner);
  ring_scan_kernel<<<NS, 256, 0, s>>>(f->owner, H, f->local_idx, f->ring_count);
  ring_scatter_kernel<<<NS, 256, 0, s>>>(d_pts, stride, d_ring, f->owner, f->local_idx, f->ring_count, NS, H, f->extracted + FRONT_GUARD,
                                        f->col + FRONT_GUARD, f->range + FRONT_GUARD, f->start_ring, f->end_ring, want_range_mat ? f->range_mat : nullptr,
                                        f->counters, f->deskew_armed ? f->deskew : DeskewArgs{});
  f->last_times = f->deskew_armed ? f->deskew.rel_time : nullptr; f->last_times_n = n_raw; f->last_times_azimuth = from_azimuth;
  f->deskew_armed = false;
  HIPCHK(hipGetLastError());
  return ROLO_OK;
}

// K3 + K4 on what front_project_enqueue left on the device; n_corner / n_surface land in counters[1] / [2]
int front_extract_enqueue(Front* f, const rolo_front_params* P, hipStream_t s, float4* fused_out = nullptr, int* pub3 = nullptr) {
  const int NS = f->n_scan;
  const size_t npix = f->cap_pix;
  // guards of curvature / picked / label are zero; live entries are written by the smoothness kernel
  const size_t np = npix + 2 * FRONT_GUARD;
  if (!f->extract_cleared) {   // a projection loaded from the host (rolo_front_load_projection): nobody cleared them yet
    HIPCHK(hipMemsetAsync(f->curv, 0, sizeof(float) * np, s));
    HIPCHK(hipMemsetAsync(f->picked, 0, sizeof(int) * np, s));
    HIPCHK(hipMemsetAsync(f->label, 0, sizeof(int) * np, s));
  }
  f->extract_cleared = false;
  // (K3 — calculateSmoothness + markOccludedPoints — runs inside extract_kernel; curv / picked / label are zero at this point)
  FeatArgs A;
  A.extracted = f->extracted + FRONT_GUARD; A.col = f->col + FRONT_GUARD; A.range = f->range + FRONT_GUARD; A.curv = f->curv + FRONT_GUARD; A.picked = f->picked + FRONT_GUARD;
  A.label = f->label + FRONT_GUARD; A.start_ring = f->start_ring; A.end_ring = f->end_ring; A.n_ptr = f->counters; A.n_scan = NS;
  A.edge_threshold = P->edge_threshold; A.surf_threshold = P->surf_threshold; A.leaf = P->odometry_surf_leaf_size;
  A.corner_stage = f->corner_stage; A.corner_cnt = f->corner_cnt; A.surf_stage = f->surf_stage; A.surf_cnt = f->surf_cnt;
  A.big = reinterpret_cast<unsigned char*>(f->big); A.paths = f->paths;
  if (f->maxh > FRONT_MAX_H) {
    extract_kernel<FRONT_MAX_H_BIG, true><<<NS, XT, 0, s>>>(A);   // the ring's working set in HBM scratch
  } else {
    constexpr size_t lds = front_ring_bytes(FRONT_MAX_H);
    static std::atomic<unsigned long long> attr_set{0};   // per device ordinal (bit d): the attribute belongs to the device's code object
    const unsigned long long dev_bit = 1ull << (f->device & 63);
    if (!(attr_set.load() & dev_bit)) { HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(extract_kernel<FRONT_MAX_H, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); attr_set.fetch_or(dev_bit); }
    extract_kernel<FRONT_MAX_H, false><<<NS, XT, lds, s>>>(A);
  }
  if (fused_out) {
    feature_gather_kernel<<<NS * 7, 256, 0, s>>>(f->corner_stage, f->corner_cnt, NS * 6, f->surf_stage, f->surf_cnt, NS, f->maxh, fused_out, f->counters, pub3);
  } else {
    concat_kernel<<<NS * 6, 256, 0, s>>>(f->corner_stage, f->corner_cnt, NS * 6, 20, f->corner_out, f->counters + 1);
    concat_kernel<<<NS, 256, 0, s>>>(f->surf_stage, f->surf_cnt, NS, f->maxh, f->surf_out, f->counters + 2);
  }
  HIPCHK(hipGetLastError());
  f->paths_valid = true;
  return ROLO_OK;
}

}  // namespace

// Fused K1-K4 for the device-resident pipeline (rolo_odom_frame): raw frame -> *featureLast = corner ++ surface in
// d_feat (capacity front_feature_capacity floats4), one host synchronisation for the three counts.
size_t front_feature_capacity(const rolo_front_params* P) { return (size_t)P->n_scan * P->horizon_scan + (size_t)P->n_scan * 6 * 20; }

// No host synchronisation: `done` is recorded on the context's stream behind the read-back of the three counts into
// h_counts3 (pinned host memory), so the caller can keep another stream busy meanwhile.
int front_frame_features_enqueue(rolo_ctx* c, const rolo_front_params* P, const float* pts, int stride, const uint16_t* ring, int n_raw,
                                 bool on_device, float4* d_feat, int* h_counts3, hipEvent_t done) {
  Front* f = nullptr;
  int rc = front_prepare(c, P, n_raw, stride, !on_device, &f);
  if (rc) return rc;
  hipStream_t s = ctx_stream(c);
  const float* d_pts = pts; const unsigned short* d_ring = ring;
  if (!on_device) {
    HIPCHK(hipMemcpyAsync(f->raw, pts, sizeof(float) * (size_t)n_raw * stride, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(f->ring, ring, sizeof(uint16_t) * (size_t)n_raw, hipMemcpyHostToDevice, s));
    d_pts = f->raw; d_ring = f->ring;
  }
  if ((rc = front_project_enqueue(f, P, d_pts, stride, d_ring, n_raw, false, s))) return rc;
  if ((rc = front_extract_enqueue(f, P, s, d_feat, h_counts3))) return rc;   // h_counts3 is pinned: the gather kernel writes the counts there itself
  HIPCHK(hipGetLastError());
  if (done) HIPCHK(hipEventRecord(done, s));
  // the next frame's clear, behind this frame's features: nobody reads the per-point arrays of a fused frame any more (its outputs are d_feat
  // and the three counts), and the front-end stream is idle until the next frame arrives — 3.6 us and a kernel boundary off its critical path
  {
    const size_t npix = f->cap_pix;
    front_clear_kernel<<<512, 256, 0, s>>>(f->owner, npix, f->col, f->range, f->curv, f->picked, f->label, npix + 2 * FRONT_GUARD);
    HIPCHK(hipGetLastError());
    f->precleared_np = npix + 2 * FRONT_GUARD;
  }
  f->projected = false;  // the staged rolo_extract_features must not run on top of a fused frame
  return ROLO_OK;
}

// Message-level entry of the fused path: the PointCloud2 payload goes to the device as it is (one copy), the field
// extraction the node does on the host runs as a kernel, and the frame continues device-resident.
int front_frame_features_from_msg(rolo_ctx* c, const rolo_front_params* P, const unsigned char* data, const rolo_cloud_layout* L, int n_raw,
                                  bool on_device, float4* d_feat, int* h_counts3, hipEvent_t done) {
  if (L->point_step <= 0 || (L->ring_bytes != 1 && L->ring_bytes != 2) || L->time_kind < 0 || L->time_kind > 2) { ctx_set_error("bad cloud layout"); return ROLO_EINVAL; }
  const int need = std::max(std::max(L->off_x, L->off_y), L->off_z) + 4;
  if (L->off_x < 0 || L->off_y < 0 || L->off_z < 0 || L->off_ring < 0 || need > L->point_step || L->off_ring + L->ring_bytes > L->point_step ||
      (L->time_kind && (L->off_time < 0 || L->off_time + 4 > L->point_step))) { ctx_set_error("cloud layout: field outside the point record"); return ROLO_EINVAL; }
  Front* f = nullptr;
  int rc = front_prepare(c, P, n_raw, 3, false, &f);
  if (rc) return rc;
  hipStream_t s = ctx_stream(c);
  const size_t bytes = (size_t)n_raw * L->point_step;
  if ((rc = f->store.grow(f->msg_xyz, f->cap_msg_xyz, 3 * (size_t)n_raw)) || (rc = f->store.grow(f->msg_ring, f->cap_msg_ring, (size_t)n_raw)) ||
      (rc = f->store.grow(f->msg_time, f->cap_msg_time, (size_t)n_raw))) return rc;
  const unsigned char* d_data = data;
  if (!on_device) {
    if ((rc = f->store.grow(f->msg_raw, f->cap_msg, bytes))) return rc;
    HIPCHK(hipMemcpyAsync(f->msg_raw, data, bytes, hipMemcpyHostToDevice, s));
    d_data = f->msg_raw;
  }
  if (n_raw > 0) unpack_cloud_kernel<<<(n_raw + 255) / 256, 256, 0, s>>>(d_data, *L, n_raw, f->msg_xyz, f->msg_ring, f->msg_time);
  HIPCHK(hipGetLastError());
  if (f->deskew_from_msg && L->time_kind != 0) {   // without a time field the projection interpolates the times from the azimuth
    f->deskew_from_msg = false;
    f->deskew.rel_time = f->msg_time;
    f->deskew_armed = true; f->deskew_n = n_raw;
  }
  return front_frame_features_enqueue(c, P, f->msg_xyz, 3, f->msg_ring, n_raw, true, d_feat, h_counts3, done);
}

}  // namespace rolo

using namespace rolo;

namespace rolo {
// rolo_ctx_release: a recycled context is a fresh object — a projection, an armed de-skew or cleared arrays of its previous owner must not carry over
// (a staged rolo_extract_features on a recycled context returns ROLO_ESTATE until its new owner has projected a frame)
void front_reset_object_state(rolo_ctx* c) {
  void** slot = ctx_front_slot(c);
  if (!*slot) return;
  Front* f = static_cast<Front*>(*slot);
  f->projected = false; f->extract_cleared = false; f->precleared_np = 0;
  f->deskew_armed = false; f->deskew_from_msg = false; f->deskew_n = 0;
  f->n_valid = 0; f->paths_valid = false; f->last_times = nullptr;
}
}  // namespace rolo

extern "C" {

void rolo_front_destroy(rolo_ctx* c) {
  void** slot = ctx_front_slot(c);
  if (*slot) { Front* f = static_cast<Front*>(*slot); f->store.release(); delete f; *slot = nullptr; }   // (rolo_ctx_destroy has drained the stream)
}

int rolo_front_set_deskew(rolo_ctx* c, const rolo_deskew* d, const float* rel_time, int n_raw, int on_device) {
  if (!c || !d) return ROLO_EINVAL;
  HIPCHK(hipSetDevice(ctx_device(c)));
  Front* f = front_of(c);
  f->deskew_armed = false; f->deskew_from_msg = false;
  if (!d->enabled) return ROLO_OK;   // deskewPoint returns the point as is (:371-372)
  if (!(d->odom_time_diff != 0.0) || !(d->scan_period != 0.f)) { ctx_set_error("de-skew: zero scan period / odometry time difference"); return ROLO_EINVAL; }
  if (!rel_time) {   // the times come with the next message (rolo_odom_submit_msg)
    f->deskew = DeskewArgs{nullptr, d->odom_incre_rpy[0], d->odom_incre_rpy[1], d->odom_incre_rpy[2], d->scan_period, d->odom_time_diff};
    f->deskew_from_msg = true;
    return ROLO_OK;
  }
  if (n_raw < 0) { ctx_set_error("de-skew needs the per-point times"); return ROLO_EINVAL; }
  const float* dt = rel_time;
  if (!on_device) {
    if (int rc = f->store.grow(f->rel_time, f->cap_time, (size_t)n_raw)) return rc;
    HIPCHK(hipMemcpyAsync(f->rel_time, rel_time, sizeof(float) * (size_t)n_raw, hipMemcpyHostToDevice, ctx_stream(c)));
    dt = f->rel_time;
  }
  f->deskew = DeskewArgs{dt, d->odom_incre_rpy[0], d->odom_incre_rpy[1], d->odom_incre_rpy[2], d->scan_period, d->odom_time_diff};
  f->deskew_armed = true; f->deskew_n = n_raw;
  return ROLO_OK;
}

void rolo_front_default_params(rolo_front_params* p) {  // config/params.yaml:20-36
  p->n_scan = 32; p->horizon_scan = 1024; p->downsample_rate = 1;
  p->lidar_min_range = 2.0f; p->lidar_max_range = 1000.0f;
  p->edge_threshold = 0.8f; p->surf_threshold = 0.1f; p->odometry_surf_leaf_size = 0.4f;
}

int rolo_project_frame(rolo_ctx* c, const rolo_front_params* P, const float* pts, int stride, const uint16_t* ring, int n_raw,
                       float* extracted, int32_t* point_col_ind, float* point_range, int32_t* start_ring, int32_t* end_ring,
                       float* range_mat, int* n_valid) {
  if (!c || !P || !pts || !ring || stride < 3 || n_raw < 0 || !n_valid) return ROLO_EINVAL;
  Front* f = nullptr;
  int rc = front_prepare(c, P, n_raw, stride, true, &f);
  if (rc) return rc;
  hipStream_t s = ctx_stream(c);
  const int NS = P->n_scan;
  const size_t npix = (size_t)NS * P->horizon_scan;
  HIPCHK(hipMemcpyAsync(f->raw, pts, sizeof(float) * (size_t)n_raw * stride, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(f->ring, ring, sizeof(uint16_t) * (size_t)n_raw, hipMemcpyHostToDevice, s));
  if ((rc = front_project_enqueue(f, P, f->raw, stride, f->ring, n_raw, true, s))) return rc;
  int nv = 0;
  HIPCHK(hipMemcpyAsync(&nv, f->counters, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  f->n_valid = nv;
  *n_valid = nv;
  if (extracted && nv) HIPCHK(hipMemcpyAsync(extracted, f->extracted + FRONT_GUARD, sizeof(float4) * (size_t)nv, hipMemcpyDeviceToHost, s));
  if (point_col_ind && nv) HIPCHK(hipMemcpyAsync(point_col_ind, f->col + FRONT_GUARD, sizeof(int) * (size_t)nv, hipMemcpyDeviceToHost, s));
  if (point_range && nv) HIPCHK(hipMemcpyAsync(point_range, f->range + FRONT_GUARD, sizeof(float) * (size_t)nv, hipMemcpyDeviceToHost, s));
  if (start_ring) HIPCHK(hipMemcpyAsync(start_ring, f->start_ring, sizeof(int) * (size_t)NS, hipMemcpyDeviceToHost, s));
  if (end_ring) HIPCHK(hipMemcpyAsync(end_ring, f->end_ring, sizeof(int) * (size_t)NS, hipMemcpyDeviceToHost, s));
  if (range_mat) HIPCHK(hipMemcpyAsync(range_mat, f->range_mat, sizeof(float) * npix, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  f->projected = true;
  return ROLO_OK;
}

// FeatureExtraction::laserCloudInfoHandler's input when the node runs in its own process: the arrays of the received
// rolo/cloud_info (fromROSMsg(cloud_projected) + pointColInd / pointRange / start- / endRingIndex) go to the device buffers
// rolo_project_frame would have left there; rolo_extract_features then runs as usual.
int rolo_front_load_projection(rolo_ctx* c, const rolo_front_params* P, const float* extracted, const int32_t* point_col_ind, const float* point_range,
                               const int32_t* start_ring, const int32_t* end_ring, int n_valid) {
  if (!c || !P || n_valid < 0 || !start_ring || !end_ring || (n_valid > 0 && (!extracted || !point_col_ind || !point_range))) return ROLO_EINVAL;
  if ((size_t)n_valid > (size_t)P->n_scan * P->horizon_scan) { ctx_set_error("more valid points than range-image pixels"); return ROLO_EINVAL; }
  // The kernels use these values as array indices: a malformed message (or an N_SCAN / Horizon_SCAN mismatch between the projection and the
  // feature process) must not become an out-of-bounds device access that takes the whole GPU context down. cloudExtraction writes
  // startRingIndex[i] = count - 1 + 5 before ring i and endRingIndex[i] = count - 1 - 5 after it (imageProjection.cpp:481-503), count running
  // from 0 to N; pointColInd is a column of the range image.
  {
    int prev = 0;
    for (int i = 0; i < P->n_scan; i++) {
      const long long before = (long long)start_ring[i] - 4, after = (long long)end_ring[i] + 6;
      if (before < prev || after < before || after > n_valid) { ctx_set_error("startRingIndex / endRingIndex are not the running counts of a projection of n_valid points"); return ROLO_EINVAL; }
      // extract_kernel sizes its ring window and its sector sort for a ring of at most Horizon_SCAN points (one per column)
      if (after - before > P->horizon_scan) { ctx_set_error("a ring holds more than Horizon_SCAN points"); return ROLO_EINVAL; }
      prev = (int)after;
    }
    for (int i = 0; i < n_valid; i++)
      if (point_col_ind[i] < 0 || point_col_ind[i] >= P->horizon_scan) { ctx_set_error("pointColInd outside [0, Horizon_SCAN)"); return ROLO_EINVAL; }
  }
  Front* f = nullptr;
  int rc = front_prepare(c, P, 0, 4, false, &f);
  if (rc) return rc;
  hipStream_t s = ctx_stream(c);
  const int NS = P->n_scan;
  const size_t np = (size_t)NS * P->horizon_scan + 2 * FRONT_GUARD;
  // guard cells and everything behind N are zero, as after a projection
  HIPCHK(hipMemsetAsync(f->col, 0, sizeof(int) * np, s));
  HIPCHK(hipMemsetAsync(f->range, 0, sizeof(float) * np, s));
  if (n_valid) {
    HIPCHK(hipMemcpyAsync(f->extracted + FRONT_GUARD, extracted, sizeof(float4) * (size_t)n_valid, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(f->col + FRONT_GUARD, point_col_ind, sizeof(int) * (size_t)n_valid, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(f->range + FRONT_GUARD, point_range, sizeof(float) * (size_t)n_valid, hipMemcpyHostToDevice, s));
  }
  HIPCHK(hipMemcpyAsync(f->start_ring, start_ring, sizeof(int) * (size_t)NS, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(f->end_ring, end_ring, sizeof(int) * (size_t)NS, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(f->counters, &n_valid, sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));   // n_valid is a stack variable; pageable copies are staged anyway
  f->n_valid = n_valid;
  f->projected = true;
  f->extract_cleared = false; f->precleared_np = 0;   // the arrays hold this projection now
  return ROLO_OK;
}

int rolo_extract_features(rolo_ctx* c, const rolo_front_params* P, float* corner, int* n_corner, float* surface, int* n_surface,
                          float* curvature, int32_t* neighbor_picked, int32_t* label) {
  if (!c || !P || !n_corner || !n_surface) return ROLO_EINVAL;
  void** slot = ctx_front_slot(c);
  Front* f = static_cast<Front*>(*slot);
  if (!f || !f->projected) { ctx_set_error("rolo_extract_features needs a preceding rolo_project_frame"); return ROLO_ESTATE; }
  HIPCHK(hipSetDevice(ctx_device(c)));
  hipStream_t s = ctx_stream(c);
  const int n = f->n_valid;
  int rc = front_extract_enqueue(f, P, s);
  if (rc) return rc;
  int cnts[3] = {0, 0, 0};
  HIPCHK(hipMemcpyAsync(cnts, f->counters, sizeof(int) * 3, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *n_corner = cnts[1]; *n_surface = cnts[2];
  if (corner && cnts[1]) HIPCHK(hipMemcpyAsync(corner, f->corner_out, sizeof(float4) * (size_t)cnts[1], hipMemcpyDeviceToHost, s));
  if (surface && cnts[2]) HIPCHK(hipMemcpyAsync(surface, f->surf_out, sizeof(float4) * (size_t)cnts[2], hipMemcpyDeviceToHost, s));
  if (curvature && n) HIPCHK(hipMemcpyAsync(curvature, f->curv + FRONT_GUARD, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, s));
  if (neighbor_picked && n) HIPCHK(hipMemcpyAsync(neighbor_picked, f->picked + FRONT_GUARD, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, s));
  if (label && n) HIPCHK(hipMemcpyAsync(label, f->label + FRONT_GUARD, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return ROLO_OK;
}

// the path word of every ring (ROLO_XPATH_*, rolo_hip.h) as the last rolo_extract_features on this context left it
int rolo_debug_extract_paths(rolo_ctx* c, int32_t* out, int n_scan) {
  if (!c || !out || n_scan <= 0) return ROLO_EINVAL;
  void** slot = ctx_front_slot(c);
  Front* f = static_cast<Front*>(*slot);
  if (!f || !f->paths_valid) { ctx_set_error("rolo_debug_extract_paths needs a preceding extraction"); return ROLO_ESTATE; }
  if (n_scan != f->n_scan) { ctx_set_error("rolo_debug_extract_paths: n_scan is not the last projection's"); return ROLO_EINVAL; }
  HIPCHK(hipSetDevice(ctx_device(c)));
  hipStream_t s = ctx_stream(c);
  HIPCHK(hipMemcpyAsync(out, f->paths, sizeof(int) * (size_t)n_scan, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return ROLO_OK;
}

// the per-point times the last projection on this context de-skewed with — the caller's, the message's or the azimuth-interpolated ones — and the index of
// the point that set halfPassed in the azimuth route (INT_MAX: no point did, or the times did not come from the azimuth)
int rolo_debug_front_times(rolo_ctx* c, float* out, int n, int32_t* first_passed) {
  if (!c || n < 0 || (n > 0 && !out)) return ROLO_EINVAL;
  void** slot = ctx_front_slot(c);
  Front* f = static_cast<Front*>(*slot);
  if (!f || !f->last_times) { ctx_set_error("rolo_debug_front_times needs a preceding de-skewed projection"); return ROLO_ESTATE; }
  if (n != f->last_times_n) { ctx_set_error("rolo_debug_front_times: n is not the last projection's number of raw points"); return ROLO_EINVAL; }
  HIPCHK(hipSetDevice(ctx_device(c)));
  hipStream_t s = ctx_stream(c);
  int fp = INT_MAX;
  if (n) HIPCHK(hipMemcpyAsync(out, f->last_times, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, s));
  if (f->last_times_azimuth) HIPCHK(hipMemcpyAsync(&fp, f->counters + 4, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (first_passed) *first_passed = fp;
  return ROLO_OK;
}

}  // extern "C"
