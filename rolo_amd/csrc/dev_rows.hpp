// Device-side row helpers of the back end (scan2map.hip, submap.hip, loopicp.hip): the fixed-order sum of per-workgroup rows, its segmented form and the float
// row transform.
#pragma once
#include "dev_math.hpp"

namespace rolo {

// The workgroups' rows (nblocks x NV doubles, NV <= 32) summed in a fixed order, deterministic for a given grid; ONE workgroup of 256 threads: 8 strided groups of
// 32 lanes, group q adds rows q, q + 8, q + 16, ... from +0.0, then the groups are added in order. The NV sums may go straight to pinned host memory.
// INFLIGHT rows are loaded before they are added (1: the plain loop). The in-flight form adds +0.0 for a row past the end: the running sum starts at +0.0 and a
// sum is -0.0 only when both terms are, so it is never -0.0 and the added +0.0 leaves its bits as they are — every INFLIGHT gives the same bits.
template <int NV, int INFLIGHT>
__global__ __launch_bounds__(256) void sum_rows(const double* __restrict__ partials, int nblocks, double* __restrict__ out) {
  __shared__ double part[8][32];
  const int v = threadIdx.x & 31, q = threadIdx.x >> 5;
  double s = 0;
  if (v < NV) {
    for (int b0 = q; b0 < nblocks; b0 += 8 * INFLIGHT) {
      double r[INFLIGHT];
#pragma unroll
      for (int u = 0; u < INFLIGHT; u++) { const int b = b0 + 8 * u; const double x = partials[(size_t)min(b, nblocks - 1) * NV + v]; r[u] = b < nblocks ? x : 0.0; }
#pragma unroll
      for (int u = 0; u < INFLIGHT; u++) s += r[u];
    }
  }
  part[q][v] = s;
  __syncthreads();
  if (threadIdx.x < NV) {
    double t = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) t += part[k][threadIdx.x];
    out[threadIdx.x] = t;
  }
}

// sum_rows<NV, 1> once per segment in one launch: workgroup g adds rows [seg[g].x, seg[g].x + seg[g].y) in exactly that order into out + g * NV (pinned host
// memory). A segment whose skip word (skip[g * skip_stride]) equals skip_value is neither read nor written.
template <int NV>
__global__ __launch_bounds__(256) void sum_rows_segmented(const double* __restrict__ partials, const int2* __restrict__ seg, const int* __restrict__ skip, int skip_stride,
                                                          int skip_value, double* __restrict__ out) {
  __shared__ double part[8][32];
  const int g = blockIdx.x;
  if (skip[(size_t)g * skip_stride] == skip_value) return;   // (workgroup-uniform)
  const int2 sg = seg[g];
  const double* __restrict__ rows = partials + (size_t)sg.x * NV;
  const int v = threadIdx.x & 31, q = threadIdx.x >> 5;
  double s = 0;
  if (v < NV)
    for (int b = q; b < sg.y; b += 8) s += rows[(size_t)b * NV + v];
  part[q][v] = s;
  __syncthreads();
  if (threadIdx.x < NV) {
    double t = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) t += part[k][threadIdx.x];
    out[(size_t)g * NV + threadIdx.x] = t;
  }
}

// T p with each row as T0 x + (T1 y + (T2 z + T3)) in float, w carried: pcl::transformPointCloud as the oracle states it (orc_transform_cloud_f). The bits hold
// only without contraction: its users are built with -ffp-contract=off.
ROLO_DEV float4 transform12(const float* T, float4 p) {
  float4 o;
  o.x = T[0] * p.x + (T[1] * p.y + (T[2] * p.z + T[3]));
  o.y = T[4] * p.x + (T[5] * p.y + (T[6] * p.z + T[7]));
  o.z = T[8] * p.x + (T[9] * p.y + (T[10] * p.z + T[11]));
  o.w = p.w;
  return o;
}

}  // namespace rolo
