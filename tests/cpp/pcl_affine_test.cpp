// CPU test of rolo_amd/csrc/pcl_affine.hpp (the pcl / Eigen pose rules of the host drivers): answers requests read from standard input, one per line, every float
// given and answered as the 8 hex digits of its bits (a double: 16); tests/test_pcl_affine.py holds the answers to the oracle and the twins bit for bit.
//   X x y z roll pitch yaw   aff_of_xyzrpy [16], xyzrpy_of of it [6], aff_of_rpyxyz of the same pose [16], pcl_rows_of_rpyxyz [12], then a second line:
//                            pcl_rows_of_xyzrpy<double> on the widened floats [12 doubles]
//   E m[16]                  xyzrpy_of [6]
//   I m[16]                  aff_inverse [16]
//   M a[16] b[16]            aff_mul [16]
//   P a[16] b[16]            aff_mul_padded [16]
//   D front[6] back[6]       xyzrpy_of(aff_mul_padded(aff_inverse(aff_of_xyzrpy(front)), aff_of_xyzrpy(back))) [6]: the odometry increment
//   1                        aff_identity [16]
//   g++ -std=c++17 -Wall -Werror -I rolo_amd/csrc tests/cpp/pcl_affine_test.cpp -o pcl_affine_test      (also with -fsanitize=address,undefined)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "pcl_affine.hpp"

static std::vector<float> floats(const char* s) {
  std::vector<float> v;
  for (;;) {
    char* end = nullptr;
    const uint32_t u = (uint32_t)std::strtoul(s, &end, 16);
    if (end == s) break;
    float f;
    std::memcpy(&f, &u, sizeof(f));
    v.push_back(f);
    s = end;
  }
  return v;
}
static void put(const float* f, int n) {
  for (int i = 0; i < n; i++) { uint32_t u; std::memcpy(&u, f + i, sizeof(u)); std::printf("%08x ", (unsigned)u); }
}
static void put(const double* d, int n) {
  for (int i = 0; i < n; i++) { uint64_t u; std::memcpy(&u, d + i, sizeof(u)); std::printf("%016llx ", (unsigned long long)u); }
}
static rolo::Aff aff(const float* m) { rolo::Aff a; std::memcpy(a.m, m, sizeof(a.m)); return a; }

int main() {
  static const struct { char op; size_t n; } ops[] = {{'X', 6}, {'E', 16}, {'I', 16}, {'M', 32}, {'P', 32}, {'D', 12}, {'1', 0}};
  char buf[8192];
  while (std::fgets(buf, sizeof(buf), stdin)) {
    if (buf[0] == '\n') continue;
    const std::vector<float> v = floats(buf + 1);
    size_t want = (size_t)-1;
    for (const auto& o : ops) if (o.op == buf[0]) want = o.n;
    if (v.size() != want) { std::printf("error: request %c with %zu numbers\n", buf[0], v.size()); return 1; }
    float o6[6];
    switch (buf[0]) {
      case 'X': {
        const rolo::Aff t = rolo::aff_of_xyzrpy(v[0], v[1], v[2], v[3], v[4], v[5]);
        rolo::xyzrpy_of(t, o6);
        const float p[6] = {v[3], v[4], v[5], v[0], v[1], v[2]};
        float rows[12];
        rolo::pcl_rows_of_rpyxyz(p, rows);
        put(t.m, 16); put(o6, 6); put(rolo::aff_of_rpyxyz(p).m, 16); put(rows, 12);
        double d[12];
        rolo::pcl_rows_of_xyzrpy<double>(v[0], v[1], v[2], v[3], v[4], v[5], d);
        std::printf("\n"); put(d, 12);
      } break;
      case 'E': rolo::xyzrpy_of(aff(&v[0]), o6); put(o6, 6); break;
      case 'I': put(rolo::aff_inverse(aff(&v[0])).m, 16); break;
      case 'M': put(rolo::aff_mul(aff(&v[0]), aff(&v[16])).m, 16); break;
      case 'P': put(rolo::aff_mul_padded(aff(&v[0]), aff(&v[16])).m, 16); break;
      case 'D': {
        const rolo::Aff F = rolo::aff_of_xyzrpy(v[0], v[1], v[2], v[3], v[4], v[5]), B = rolo::aff_of_xyzrpy(v[6], v[7], v[8], v[9], v[10], v[11]);
        rolo::xyzrpy_of(rolo::aff_mul_padded(rolo::aff_inverse(F), B), o6);
        put(o6, 6);
      } break;
      case '1': put(rolo::aff_identity().m, 16); break;
    }
    std::printf("\n");
  }
  return 0;
}
