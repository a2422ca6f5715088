// The pcl / Eigen pose rules the host drivers share, each written once: pcl::getTransformation, pcl::getTranslationAndEulerAngles (pcl/common/impl/eigen.hpp),
// Eigen::Affine3f::inverse() and the Affine3f product. PCL and Eigen are not in the reference tree; these are bit-level contracts with
// the oracle, one float operation for each of theirs, in their order. odometry.hip, fusion.hip, mapper.hip, submap.hip and scan2map.hip call them;
// tests/test_pcl_affine.py holds every function to the oracle and the twins bit for bit.
//
// Pure host C++ (no HIP include): tests/cpp/pcl_affine_test.cpp compiles it with g++ alone.
//
// Not here on purpose, each a different rule with different bits: front.hip's de-skew rotation (device code on cosf / sinf), posegraph.hip's double Euler angles
// with a clamped asin, groundprior.hip's gp_rot* and its angles, backend.py's _mul34 and its kin; the oracle and the Python twins under oracle/ and tests/ stay
// independent statements, or they would check nothing.
#pragma once
#include <cmath>

namespace rolo {

struct Aff { float m[16]; };   // an Affine3f as a row-major 4 x 4, last row 0 0 0 1

inline Aff aff_identity() { Aff a; for (int i = 0; i < 16; i++) a.m[i] = (i % 5 == 0) ? 1.f : 0.f; return a; }

// pcl::getTransformation(x, y, z, roll, pitch, yaw), rows 0..2 at stride 4 (12 entries: an Aff's, a 12-float kernel argument, the top of a double 4 x 4).
// S = float is pcl's own overload; S = double is the same formula on widened floats (gtsam::Rot3::RzRyRx, mapper.hip).
template <typename S>
inline void pcl_rows_of_xyzrpy(S x, S y, S z, S roll, S pitch, S yaw, S* T) {
  const S A = std::cos(yaw), B = std::sin(yaw), C = std::cos(pitch), D = std::sin(pitch), E = std::cos(roll), F = std::sin(roll);
  const S DE = D * E, DF = D * F;
  T[0] = A * C; T[1] = A * DF - B * E; T[2] = B * F + A * DE; T[3] = x;
  T[4] = B * C; T[5] = A * E + B * DF; T[6] = B * DE - A * F; T[7] = y;
  T[8] = -D;    T[9] = C * F;          T[10] = C * E;         T[11] = z;
}
inline Aff aff_of_xyzrpy(float x, float y, float z, float roll, float pitch, float yaw) {
  Aff t;
  pcl_rows_of_xyzrpy(x, y, z, roll, pitch, yaw, t.m);
  t.m[12] = 0; t.m[13] = 0; t.m[14] = 0; t.m[15] = 1;
  return t;
}
// the back end's pose order (transformTobeMapped, a key pose): roll pitch yaw x y z. trans2Affine3f, backMapping.cpp:339-342
inline void pcl_rows_of_rpyxyz(const float* p, float* T) { pcl_rows_of_xyzrpy(p[3], p[4], p[5], p[0], p[1], p[2], T); }
inline Aff aff_of_rpyxyz(const float* p) { return aff_of_xyzrpy(p[3], p[4], p[5], p[0], p[1], p[2]); }

// pcl::getTranslationAndEulerAngles: x y z roll pitch yaw
inline void xyzrpy_of(const Aff& t, float* o) {
  o[0] = t.m[3]; o[1] = t.m[7]; o[2] = t.m[11];
  o[3] = std::atan2(t.m[9], t.m[10]);
  o[4] = std::asin(-t.m[8]);
  o[5] = std::atan2(t.m[4], t.m[0]);
}

// Eigen::Transform<float, 3, Affine>::inverse(): the cofactor inverse of the linear part, translation -(L^-1 t)
inline Aff aff_inverse(const Aff& T) {
  const float* a = T.m;
  float c[9];
  c[0] = a[5] * a[10] - a[6] * a[9]; c[1] = a[2] * a[9] - a[1] * a[10]; c[2] = a[1] * a[6] - a[2] * a[5];
  c[3] = a[6] * a[8] - a[4] * a[10]; c[4] = a[0] * a[10] - a[2] * a[8]; c[5] = a[2] * a[4] - a[0] * a[6];
  c[6] = a[4] * a[9] - a[5] * a[8];  c[7] = a[1] * a[8] - a[0] * a[9];  c[8] = a[0] * a[5] - a[1] * a[4];
  const float det = a[0] * c[0] + a[1] * c[3] + a[2] * c[6];
  const float inv = 1.0f / det;
  Aff o;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) o.m[i * 4 + j] = c[i * 3 + j] * inv;
  for (int i = 0; i < 3; i++) o.m[i * 4 + 3] = -(o.m[i * 4] * a[3] + o.m[i * 4 + 1] * a[7] + o.m[i * 4 + 2] * a[11]);
  o.m[12] = o.m[13] = o.m[14] = 0; o.m[15] = 1;
  return o;
}

// Two products a b, both kept: they are not the same function of their bits.
//   aff_mul         the affine form: an entry is its three terms summed left to right, the translation column adds a's translation last; the last row is
//                   never read. The back end uses it (mapper.hip; tests/mapper_twin.py states it).
//   aff_mul_padded  the 4 x 4 form: every entry is 0 + four terms, the last row taking part. The front end and the fusion node use it (odometry.hip,
//                   fusion.hip), because the oracle's mat4f_mul (oracle/rolo_oracle_front.cpp) is this sum and their poses match the oracle's bit for bit.
// Where they differ: the sign of a zero ((-0) + (-0) is -0, but 0 + (-0) is +0, so a sum of negative zeros comes out -0 from aff_mul and +0 from
// aff_mul_padded; the sign goes on into atan2 and asin and so into a published pose), and entries that are not finite (the padded form's fourth term in the linear part
// is a_i3 * 0, NaN for a translation that is not finite, where the affine form never multiplies a translation by the last row). Whether a reachable pose tells
// them apart is not known; every caller stays on the form it has always used.
inline Aff aff_mul(const Aff& a, const Aff& b) {
  Aff c;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) c.m[i * 4 + j] = a.m[i * 4] * b.m[j] + a.m[i * 4 + 1] * b.m[4 + j] + a.m[i * 4 + 2] * b.m[8 + j];
    c.m[i * 4 + 3] = a.m[i * 4] * b.m[3] + a.m[i * 4 + 1] * b.m[7] + a.m[i * 4 + 2] * b.m[11] + a.m[i * 4 + 3];
  }
  c.m[12] = 0; c.m[13] = 0; c.m[14] = 0; c.m[15] = 1;
  return c;
}
inline Aff aff_mul_padded(const Aff& a, const Aff& b) {
  Aff c;
  for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) { float s = 0; for (int k = 0; k < 4; k++) s += a.m[i * 4 + k] * b.m[k * 4 + j]; c.m[i * 4 + j] = s; }
  return c;
}

}  // namespace rolo
