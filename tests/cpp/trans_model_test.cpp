// CPU test of rolo_amd/csrc/trans_model.hpp (the translation stage's trial cost as a quadratic in the translation, from the sums of the stage's linearisation): answers
// requests read from standard input, one per line, numbers as %.17g; tests/test_trans_model.py feeds it the oracle's t3_linearize sums and holds the costs to
// compute_t_error, and replays whole stages from it.
//   B lam_over_n inv_dtn g[3] lastA_q[3] lastB_q[3] t0[3] H[36] b[6] y0    build the model          -> "valid 0|1"
//   C tt[3]                                                              its cost at tt            -> "cost <%.17g | nan>"
//   g++ -std=c++17 -Wall -Werror -I rolo_amd/csrc tests/cpp/trans_model_test.cpp -o trans_model_test      (also with -fsanitize=address,undefined)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "trans_model.hpp"

static std::vector<double> numbers(const char* s) {
  std::vector<double> v;
  while (*s) {
    char* end = nullptr;
    const double x = std::strtod(s, &end);   // accepts "nan" and "inf"
    if (end == s) break;
    v.push_back(x);
    s = end;
  }
  return v;
}

int main() {
  rolo::TransModel m{};
  rolo::TransModelConsts K{};
  bool have = false;
  char buf[8192];
  while (std::fgets(buf, sizeof(buf), stdin)) {
    if (buf[0] == 'B') {
      const std::vector<double> v = numbers(buf + 1);
      if (v.size() != 2 + 12 + 36 + 6 + 1) { std::printf("error B takes 57 numbers, got %zu\n", v.size()); std::fflush(stdout); continue; }
      K.lam_over_n = v[0]; K.inv_dtn = v[1];
      for (int i = 0; i < 3; i++) { K.g[i] = v[2 + i]; K.lastA_q[i] = v[5 + i]; K.lastB_q[i] = v[8 + i]; }
      rolo::trans_model_build(m, &v[14], &v[50], v[56], K, &v[11]);
      have = true;
      std::printf("valid %d\n", m.valid);
    } else if (buf[0] == 'C') {
      const std::vector<double> v = numbers(buf + 1);
      if (!have || v.size() != 3) { std::printf("error C takes 3 numbers after a B\n"); std::fflush(stdout); continue; }
      const double y = rolo::trans_model_cost(m, K, v.data());
      if (y == y) std::printf("cost %.17g\n", y); else std::printf("cost nan\n");
    } else if (buf[0] != '\n') {
      std::printf("error unknown request\n");
    }
    std::fflush(stdout);
  }
  return 0;
}
