// Box tests of the tree walks (knn_packet.hpp, loopicp.hip, scan2map.hip) — plain C++, host and device: the squared distance from a query to a box, the same for
// BOTH child boxes of a node at once, and the "does this lane's search sphere reach the box" compare. Every includer is compiled with -ffp-contract=off: the IEEE
// operations per component and their order are those of the point distances, so a box distance is a true lower bound of every point distance inside, bit for bit.
// tests/cpp/box_pair_test.cpp checks the pair against the scalar form and the one-compare reach test against the two-compare one on the host.
#pragma once
#include <cfloat>
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ROLO_BOX_FN __host__ __device__ __forceinline__
#else
#define ROLO_BOX_FN inline
#endif

namespace rolo {

// two floats that the compiler may keep in one 64-bit register pair (v_pk_add_f32 / v_pk_mul_f32): [0] = the left child's value, [1] = the right child's
#if defined(__clang__)
typedef float box_f2 __attribute__((ext_vector_type(2)));
#else
typedef float box_f2 __attribute__((vector_size(8)));
#endif

// squared distance from q to the box [lo, hi] in the operation order of the point distances (V4: anything with float x, y, z)
template <class V4>
ROLO_BOX_FN float box_d2(const V4& lo, const V4& hi, const V4& q) {
  const float dx = fmaxf(fmaxf(lo.x - q.x, q.x - hi.x), 0.f);
  const float dy = fmaxf(fmaxf(lo.y - q.y, q.y - hi.y), 0.f);
  const float dz = fmaxf(fmaxf(lo.z - q.z, q.z - hi.z), 0.f);
  return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// box_d2 of the left and the right child of one node record (left lo, left hi, right lo, right hi), the two children in the two halves of every operand: six
// packed subtractions, six three-way maxima, three packed multiplies and two packed adds where two calls of box_d2 issue twelve single subtractions
template <class V4>
ROLO_BOX_FN box_f2 box_d2_pair(const V4& llo, const V4& lhi, const V4& rlo, const V4& rhi, const V4& q) {
  const box_f2 qx = {q.x, q.x}, qy = {q.y, q.y}, qz = {q.z, q.z};
  const box_f2 lox = {llo.x, rlo.x}, loy = {llo.y, rlo.y}, loz = {llo.z, rlo.z};
  const box_f2 hix = {lhi.x, rhi.x}, hiy = {lhi.y, rhi.y}, hiz = {lhi.z, rhi.z};
  const box_f2 ax = lox - qx, bx = qx - hix, ay = loy - qy, by = qy - hiy, az = loz - qz, bz = qz - hiz;
  const box_f2 dx = {fmaxf(fmaxf(ax[0], bx[0]), 0.f), fmaxf(fmaxf(ax[1], bx[1]), 0.f)};
  const box_f2 dy = {fmaxf(fmaxf(ay[0], by[0]), 0.f), fmaxf(fmaxf(ay[1], by[1]), 0.f)};
  const box_f2 dz = {fmaxf(fmaxf(az[0], bz[0]), 0.f), fmaxf(fmaxf(az[1], bz[1]), 0.f)};
  return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// A lane reaches a box at squared distance d (>= 0, +inf for a padding box: lo = +inf, hi = -inf) under its bound bd (the d2 of its k-th best: -1 for an idle lane,
// +inf while its list is not full) if (d <= bd) && (d < INFINITY). With the bound clamped to the largest finite float that is ONE compare — the ballot's own operand.
// (the clamp as a SIGNED INTEGER minimum of the bit patterns: for bd >= 0 their order is the floats', -1 has the sign bit and stays — one v_min_i32, where fminf
// puts a canonicalising v_max_f32 in front of its v_min_f32. bd is never NaN.)
ROLO_BOX_FN float box_bound_clamp(float bd) {
  int b, m;
  const float fmax = FLT_MAX;
  __builtin_memcpy(&b, &bd, 4); __builtin_memcpy(&m, &fmax, 4);
  b = b < m ? b : m;
  float r;
  __builtin_memcpy(&r, &b, 4);
  return r;
}
ROLO_BOX_FN bool box_reached(float d, float bd_clamped) { return d <= bd_clamped; }
ROLO_BOX_FN bool box_reached_two_compares(float d, float bd) { return (d <= bd) && (d < INFINITY); }

}  // namespace rolo
