// CPU test of rolo_amd/csrc/knn_seed_net.hpp (the sorting / merging networks that build the neighbour search's seed lists): integer keys, no GPU.
//   g++ -std=c++17 -I rolo_amd/csrc tests/cpp/seed_net_test.cpp -o seed_net_test && ./seed_net_test      (exit code 0 and "all held" = every case passed)
// A comparator network that sorts every 0-1 input sorts every input (0-1 principle), so sort8 / sort4 are checked on all 2^8 / 2^4 inputs and the merges on
// every pair (ascending 0-1 list of 20, ascending 0-1 list of NB); random distinct integers with +inf padding against std::sort + truncate come on top.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "knn_seed_net.hpp"

namespace sn = rolo::seednet;
using key_t_ = long long;
static const auto mn = [](key_t_ a, key_t_ b) { return a < b ? a : b; };
static const auto mx = [](key_t_ a, key_t_ b) { return a < b ? b : a; };

static int fails = 0;
#define CHECK(c, what) do { if (!(c)) { if (fails < 20) std::printf("FAILED: %s (%s)\n", what, #c); fails++; } } while (0)

template <int NB> static void sort_chunk(key_t_ (&b)[NB]) { if constexpr (NB == 8) sn::sort8(b, mn, mx); else sn::sort4(b, mn, mx); }

template <int NB> static int zero_one_sort() {
  int n = 0;
  for (unsigned m = 0; m < (1u << NB); m++, n++) {
    key_t_ b[NB];
    for (int i = 0; i < NB; i++) b[i] = (m >> i) & 1u;
    sort_chunk<NB>(b);
    CHECK(std::is_sorted(b, b + NB) && std::count(b, b + NB, 1) == __builtin_popcount(m), "sort: 0-1 input");
  }
  return n;
}

template <int NB> static int zero_one_merge() {
  int n = 0;
  for (int zk = 0; zk <= 20; zk++)       // K = zk zeros, then ones
    for (int zb = 0; zb <= NB; zb++, n++) {   // b = zb zeros, then ones
      key_t_ K[20], b[NB];
      for (int i = 0; i < 20; i++) K[i] = i >= zk;
      for (int i = 0; i < NB; i++) b[i] = i >= zb;
      sn::merge_chunk<NB>(K, b, mn, mx);
      const int z = std::min(zk + zb, 20);
      bool ok = true;
      for (int i = 0; i < 20; i++) ok = ok && K[i] == (i >= z);
      CHECK(ok, "merge: 0-1 lists");
    }
  return n;
}

// a list grown chunk by chunk from all-padding, as the seed phase grows it: distinct keys, +inf (repeated) for the padding of the list and of the chunks
template <int NB> static int random_lists(unsigned seed, int rounds) {
  std::mt19937_64 rng(seed);
  const key_t_ INF = LLONG_MAX;
  int n = 0;
  for (int r = 0; r < rounds; r++) {
    key_t_ K[20];
    std::vector<key_t_> all;
    for (int i = 0; i < 20; i++) K[i] = INF;
    const int chunks = 1 + (int)(rng() % 12);
    const key_t_ range = (rng() & 1) ? 64 : (key_t_)1 << 40;   // a narrow range forces many near keys; distinctness is enforced below
    for (int c = 0; c < chunks; c++, n++) {
      key_t_ b[NB];
      const int pad = (rng() % 4 == 0) ? (int)(rng() % (NB + 1)) : 0;
      for (int i = 0; i < NB; i++) {
        if (i < pad) { b[i] = INF; continue; }
        key_t_ v;
        do v = (key_t_)(rng() % (uint64_t)range) * 1024 + (key_t_)(all.size() % 1024); while (std::find(all.begin(), all.end(), v) != all.end());
        b[i] = v; all.push_back(v);
      }
      std::shuffle(b, b + NB, rng);
      sort_chunk<NB>(b);
      CHECK(std::is_sorted(b, b + NB), "random: chunk sorted");
      sn::merge_chunk<NB>(K, b, mn, mx);
      std::vector<key_t_> want = all;
      std::sort(want.begin(), want.end());
      want.resize(20, INF);
      CHECK(std::equal(K, K + 20, want.begin()), "random: list = sort + truncate");
    }
  }
  return n;
}

int main() {
  std::printf("sort8 0-1 inputs: %d\n", zero_one_sort<8>());
  std::printf("sort4 0-1 inputs: %d\n", zero_one_sort<4>());
  std::printf("merge8 0-1 pairs: %d\n", zero_one_merge<8>());
  std::printf("merge4 0-1 pairs: %d\n", zero_one_merge<4>());
  {  // merge8 by its own name, and the cleaner on its own in both directions: every bitonic 0-1 run of 20 ascending, of 8 descending
    key_t_ K[20], b[8] = {3, 5, 8, 13, 21, 34, 55, 89};
    for (int i = 0; i < 20; i++) K[i] = 4 * i;
    sn::merge8(K, b, mn, mx);
    const key_t_ want[20] = {0, 3, 4, 5, 8, 8, 12, 13, 16, 20, 21, 24, 28, 32, 34, 36, 40, 44, 48, 52};
    CHECK(std::equal(K, K + 20, want), "merge8: worked example");
    int n = 0;
    for (int a = 0; a <= 20; a++) for (int l = 0; a + l <= 20; l++, n++) {   // 0..1..0 only: behind the -inf padding in front a run must rise, then fall
      key_t_ R[20];
      for (int i = 0; i < 20; i++) R[i] = (i >= a && i < a + l) ? 1 : 0;
      const long ones = std::count(R, R + 20, 1);
      sn::bitonic_clean<20, 0, false>(R, mn, mx);
      CHECK(std::is_sorted(R, R + 20) && std::count(R, R + 20, 1) == ones, "cleaner: 20 ascending");
    }
    for (int a = 0; a <= 8; a++) for (int l = 0; a + l <= 8; l++) for (int v = 0; v < 2; v++, n++) {   // no padding at 8: 0..1..0 and 1..0..1
      key_t_ R[20];
      for (int i = 0; i < 20; i++) R[i] = i < 12 ? -1 : (((i - 12) >= a && (i - 12) < a + l) ? 1 - v : v);
      const long ones = std::count(R, R + 20, 1);
      sn::bitonic_clean<8, 12, true>(R, mn, mx);
      CHECK(std::is_sorted(R + 12, R + 20, [](key_t_ x, key_t_ y) { return x > y; }) && std::count(R, R + 20, 1) == ones && std::count(R, R + 12, -1) == 12, "cleaner: 8 descending in place");
    }
    std::printf("cleaner 0-1 runs: %d\n", n);
  }
  std::printf("random chunks of 8: %d\n", random_lists<8>(20261, 600));
  std::printf("random chunks of 4: %d\n", random_lists<4>(20262, 600));
  if (fails) { std::printf("%d checks FAILED\n", fails); return 1; }
  std::printf("all held\n");
  return 0;
}
