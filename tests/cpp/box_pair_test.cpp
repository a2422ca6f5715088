// CPU test of rolo_amd/csrc/knn_box_pair.hpp (the box tests of the tree walks): no GPU.
//   g++ -std=c++17 -O2 -ffp-contract=off -I rolo_amd/csrc tests/cpp/box_pair_test.cpp -o box_pair_test && ./box_pair_test     (exit code 0 and "all held")
// box_d2_pair (both child boxes of a node record at once, the children in the halves of two-float vectors) against the scalar box_d2 and against a restatement of
// it written out here, BIT FOR BIT: random boxes and queries, degenerate boxes (lo = hi), queries inside, on faces and at corners, padding boxes (lo = +inf,
// hi = -inf) on either side and on both. The one-compare reach test with the clamped bound against the two-compare form over
// d in {0, denormal, 1, FLT_MAX, +inf} x bd in {-1, 0, 1, FLT_MAX, +inf}, and over random pairs.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include "knn_box_pair.hpp"

struct V4 { float x, y, z, w; };

static int fails = 0;
#define CHECK(c, what) do { if (!(c)) { if (fails < 20) std::printf("FAILED: %s (%s)\n", what, #c); fails++; } } while (0)

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// the scalar form restated: one axis after the other, the order of the point distances
static float box_d2_restated(const V4& lo, const V4& hi, const V4& q) {
  const float l[3] = {lo.x, lo.y, lo.z}, h[3] = {hi.x, hi.y, hi.z}, p[3] = {q.x, q.y, q.z};
  float d[3];
  for (int a = 0; a < 3; a++) { const float below = l[a] - p[a], above = p[a] - h[a]; d[a] = fmaxf(fmaxf(below, above), 0.f); }
  const float xx = d[0] * d[0], yy = d[1] * d[1], zz = d[2] * d[2];
  const float xy = xx + yy;
  return xy + zz;
}

static int n_pairs = 0;
static void check_pair(const V4& llo, const V4& lhi, const V4& rlo, const V4& rhi, const V4& q, const char* what) {
  const rolo::box_f2 d = rolo::box_d2_pair(llo, lhi, rlo, rhi, q);
  const float l = rolo::box_d2(llo, lhi, q), r = rolo::box_d2(rlo, rhi, q);
  CHECK(bits(d[0]) == bits(l) && bits(d[1]) == bits(r), what);
  CHECK(bits(l) == bits(box_d2_restated(llo, lhi, q)) && bits(r) == bits(box_d2_restated(rlo, rhi, q)), what);
  n_pairs++;
}

int main() {
  std::mt19937 rng(20261019u);
  const float inf = std::numeric_limits<float>::infinity();
  const V4 pad_lo = {inf, inf, inf, 0.f}, pad_hi = {-inf, -inf, -inf, 0.f};
  auto uni = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
  auto box = [&](float scale, V4& lo, V4& hi) {
    const V4 a = {uni(-scale, scale), uni(-scale, scale), uni(-scale, scale), 0.f}, b = {uni(-scale, scale), uni(-scale, scale), uni(-scale, scale), 0.f};
    lo = {fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z), 0.f};
    hi = {fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), 0.f};
  };
  // random boxes and queries at three scales (metres of a lidar scan, millimetres, a far-away cloud)
  for (float scale : {100.f, 1e-3f, 1e6f})
    for (int t = 0; t < 20000; t++) {
      V4 llo, lhi, rlo, rhi;
      box(scale, llo, lhi); box(scale, rlo, rhi);
      const V4 q = {uni(-1.5f * scale, 1.5f * scale), uni(-1.5f * scale, 1.5f * scale), uni(-1.5f * scale, 1.5f * scale), 1.f};
      check_pair(llo, lhi, rlo, rhi, q, "random boxes");
    }
  for (int t = 0; t < 20000; t++) {
    V4 llo, lhi, rlo, rhi;
    box(50.f, llo, lhi); box(50.f, rlo, rhi);
    // degenerate boxes: a point, and a box flat in one axis
    const V4 pt = {uni(-50.f, 50.f), uni(-50.f, 50.f), uni(-50.f, 50.f), 0.f};
    V4 flat_lo = rlo, flat_hi = rhi; flat_hi.y = flat_lo.y;
    const V4 q = {uni(-60.f, 60.f), uni(-60.f, 60.f), uni(-60.f, 60.f), 1.f};
    check_pair(pt, pt, flat_lo, flat_hi, q, "degenerate boxes");
    check_pair(pt, pt, pt, pt, pt, "query on a point box");
    // queries inside the left box, on its faces, at its corners (the right box wherever it fell)
    const V4 in = {uni(llo.x, lhi.x), uni(llo.y, lhi.y), uni(llo.z, lhi.z), 1.f};
    check_pair(llo, lhi, rlo, rhi, in, "query inside");
    CHECK(rolo::box_d2(llo, lhi, in) == 0.f, "inside: distance 0");
    for (int f = 0; f < 6; f++) {
      V4 on = in;
      (f < 2 ? on.x : f < 4 ? on.y : on.z) = f & 1 ? (f < 2 ? lhi.x : f < 4 ? lhi.y : lhi.z) : (f < 2 ? llo.x : f < 4 ? llo.y : llo.z);
      check_pair(llo, lhi, rlo, rhi, on, "query on a face");
      check_pair(rlo, rhi, llo, lhi, on, "query on a face (right child)");
      CHECK(rolo::box_d2(llo, lhi, on) == 0.f, "face: distance 0");
    }
    for (int c = 0; c < 8; c++) {
      const V4 corner = {c & 1 ? lhi.x : llo.x, c & 2 ? lhi.y : llo.y, c & 4 ? lhi.z : llo.z, 1.f};
      check_pair(llo, lhi, rlo, rhi, corner, "query at a corner");
      check_pair(rlo, rhi, llo, lhi, corner, "query at a corner (right child)");
    }
    // padding boxes: +inf whatever the query, and no NaN beside a real box
    check_pair(llo, lhi, pad_lo, pad_hi, q, "padding right");
    check_pair(pad_lo, pad_hi, rlo, rhi, q, "padding left");
    check_pair(pad_lo, pad_hi, pad_lo, pad_hi, q, "padding both");
    const rolo::box_f2 d = rolo::box_d2_pair(llo, lhi, pad_lo, pad_hi, q);
    CHECK(d[1] == inf && d[0] < inf, "padding box at +inf");
    // a padding lane's query (+inf): every box, real or padding, at +inf
    const V4 qpad = {inf, inf, inf, 0.f};
    check_pair(llo, lhi, pad_lo, pad_hi, qpad, "padding query");
    const rolo::box_f2 dp = rolo::box_d2_pair(llo, lhi, rlo, rhi, qpad);
    CHECK(dp[0] == inf && dp[1] == inf, "padding query at +inf from real boxes");
  }
  std::printf("box pairs: %d\n", n_pairs);

  // the clamped compare
  const float ds[5] = {0.f, std::numeric_limits<float>::denorm_min(), 1.f, FLT_MAX, inf}, bds[5] = {-1.f, 0.f, 1.f, FLT_MAX, inf};
  int n_cmp = 0;
  for (float d : ds)
    for (float bd : bds) {
      CHECK(rolo::box_reached(d, rolo::box_bound_clamp(bd)) == rolo::box_reached_two_compares(d, bd), "clamped compare: table");
      n_cmp++;
    }
  std::printf("clamped compare table: %d\n", n_cmp);
  CHECK(bits(rolo::box_bound_clamp(-1.f)) == bits(-1.f) && bits(rolo::box_bound_clamp(inf)) == bits(FLT_MAX) && bits(rolo::box_bound_clamp(0.f)) == bits(0.f)
        && bits(rolo::box_bound_clamp(FLT_MAX)) == bits(FLT_MAX), "clamp values");
  for (int t = 0; t < 200000; t++) {
    // random non-negative bit patterns up to +inf for d; the same, or -1, for the bound
    const uint32_t ub = std::uniform_int_distribution<uint32_t>(0u, 0x7f800000u)(rng), ud = std::uniform_int_distribution<uint32_t>(0u, 0x7f800000u)(rng);
    float d, bd; std::memcpy(&d, &ud, 4); std::memcpy(&bd, &ub, 4);
    if (t % 7 == 0) bd = -1.f;
    if (t % 11 == 0) d = bd < 0.f ? 0.f : bd;   // equality must reach
    CHECK(rolo::box_reached(d, rolo::box_bound_clamp(bd)) == rolo::box_reached_two_compares(d, bd), "clamped compare: random");
    if (bd >= 0.f) CHECK(bits(rolo::box_bound_clamp(bd)) == bits(fminf(bd, FLT_MAX)), "clamp = fminf(bd, FLT_MAX)");
  }
  if (fails) { std::printf("%d checks FAILED\n", fails); return 1; }
  std::printf("all held\n");
  return 0;
}
