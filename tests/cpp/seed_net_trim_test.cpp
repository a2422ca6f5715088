// CPU test of the trimmed seed networks of rolo_amd/csrc/knn_seed_net.hpp: merge_chunk without a sort of the tail (the list is bitonic after the element-wise
// minimum), the comparators of the 20-cleaner that cannot swap behind a chunk of 4, and first_two_chunks (the first seed leaf, into a list of sentinels). Integer keys.
//   g++ -std=c++17 -I rolo_amd/csrc tests/cpp/seed_net_trim_test.cpp -o seed_net_trim_test && ./seed_net_trim_test      (exit code 0 and "all held" = every case passed)
// 0-1 principle: a min / max network that gives the right answer on every pair of ascending 0-1 lists gives it on every pair of ascending lists. On top: random
// distinct keys with +inf padding and lists with ties, against std::sort + truncate; and the number of min / max calls, so that a step that creeps back in fails.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "knn_seed_net.hpp"

namespace sn = rolo::seednet;
using key_t_ = long long;
static long n_min = 0, n_max = 0;
static const auto mn = [](key_t_ a, key_t_ b) { n_min++; return a < b ? a : b; };
static const auto mx = [](key_t_ a, key_t_ b) { n_max++; return a < b ? b : a; };
static const key_t_ INF = LLONG_MAX;

static int fails = 0;
#define CHECK(c, what) do { if (!(c)) { if (fails < 20) std::printf("FAILED: %s (%s)\n", what, #c); fails++; } } while (0)

template <int NB> static void sort_chunk(key_t_ (&b)[NB]) { if constexpr (NB == 8) sn::sort8(b, mn, mx); else sn::sort4(b, mn, mx); }

template <int NB> static int zero_one_merge() {
  int n = 0;
  for (int zk = 0; zk <= 20; zk++)
    for (int zb = 0; zb <= NB; zb++, n++) {
      key_t_ K[20], b[NB];
      for (int i = 0; i < 20; i++) K[i] = i >= zk;
      for (int i = 0; i < NB; i++) b[i] = i >= zb;
      sn::merge_chunk<NB>(K, b, mn, mx);
      const int z = std::min(zk + zb, 20);
      bool ok = true;
      for (int i = 0; i < 20; i++) ok = ok && K[i] == (i >= z);
      CHECK(ok, "merge_chunk: 0-1 lists");
    }
  return n;
}

// every pair of ascending 0-1 chunks into a list of sentinels (2: above both 0 and 1), and the same pair through merge_chunk twice
static int zero_one_first() {
  int n = 0;
  for (int z0 = 0; z0 <= 8; z0++)
    for (int z1 = 0; z1 <= 8; z1++, n++) {
      key_t_ K[20], M[20], b0[8], b1[8];
      for (int i = 0; i < 20; i++) K[i] = M[i] = 2;
      for (int i = 0; i < 8; i++) { b0[i] = i >= z0; b1[i] = i >= z1; }
      sn::first_two_chunks(K, b0, b1, mn, mx);
      sn::merge_chunk<8>(M, b0, mn, mx);
      sn::merge_chunk<8>(M, b1, mn, mx);
      bool ok = true;
      for (int i = 0; i < 20; i++) ok = ok && K[i] == (i < z0 + z1 ? 0 : i < 16 ? 1 : 2);
      CHECK(ok, "first_two_chunks: 0-1 chunks");
      CHECK(std::equal(K, K + 20, M), "first_two_chunks = merge_chunk twice");
    }
  return n;
}

// a list grown chunk by chunk from all-padding, as the seed phase grows it. ties = false: distinct keys, +inf (repeated) for the padding of the chunks;
// ties = true: keys drawn from a handful of values (a min / max network does not care which of two equal keys it moves)
template <int NB> static int random_lists(unsigned seed, int rounds, bool ties, bool first_form) {
  std::mt19937_64 rng(seed);
  int n = 0;
  for (int r = 0; r < rounds; r++) {
    key_t_ K[20];
    std::vector<key_t_> all;
    for (int i = 0; i < 20; i++) K[i] = INF;
    const int chunks = 2 + (int)(rng() % 11);
    const key_t_ range = ties ? 6 : ((rng() & 1) ? 64 : (key_t_)1 << 40);
    key_t_ held[8];
    for (int c = 0; c < chunks; c++, n++) {
      key_t_ b[NB];
      const int pad = (rng() % 4 == 0) ? (int)(rng() % (NB + 1)) : 0;
      for (int i = 0; i < NB; i++) {
        if (i < pad) { b[i] = INF; continue; }
        key_t_ v;
        if (ties) v = (key_t_)(rng() % (uint64_t)range);
        else do v = (key_t_)(rng() % (uint64_t)range) * 1024 + (key_t_)(all.size() % 1024); while (std::find(all.begin(), all.end(), v) != all.end());
        b[i] = v; all.push_back(v);
      }
      std::shuffle(b, b + NB, rng);
      sort_chunk<NB>(b);
      if constexpr (NB == 8) {
        if (first_form && c == 0) { std::copy(b, b + 8, held); continue; }   // the first two chunks go in together
        if (first_form && c == 1) { sn::first_two_chunks(K, held, b, mn, mx); }
        else sn::merge_chunk<NB>(K, b, mn, mx);
      } else {
        sn::merge_chunk<NB>(K, b, mn, mx);
      }
      std::vector<key_t_> want = all;
      std::sort(want.begin(), want.end());
      want.resize(20, INF);
      CHECK(std::equal(K, K + 20, want.begin()), "random: list = sort + truncate");
    }
  }
  return n;
}

int main() {
  std::printf("merge_chunk<8> 0-1 pairs: %d\n", zero_one_merge<8>());
  std::printf("merge_chunk<4> 0-1 pairs: %d\n", zero_one_merge<4>());
  std::printf("first_two_chunks 0-1 pairs: %d\n", zero_one_first());
  std::printf("random chunks of 8: %d\n", random_lists<8>(20271, 500, false, false));
  std::printf("random chunks of 4: %d\n", random_lists<4>(20272, 500, false, false));
  std::printf("random chunks of 8, first two together: %d\n", random_lists<8>(20273, 500, false, true));
  std::printf("tied chunks of 8: %d\n", random_lists<8>(20274, 300, true, false));
  std::printf("tied chunks of 4: %d\n", random_lists<4>(20275, 300, true, false));
  std::printf("tied chunks of 8, first two together: %d\n", random_lists<8>(20276, 300, true, true));
  {  // the price of each form in min / max calls: 8 + 2 x 40 for a chunk of 8 (no sort of the tail), 4 + 2 x 36 for a chunk of 4 (four dead comparators), 2 x 32 for the first leaf's merge
    key_t_ K[20], b8[8] = {1, 2, 3, 4, 5, 6, 7, 8}, c8[8] = {0, 2, 4, 6, 8, 10, 12, 14}, b4[4] = {1, 2, 3, 4};
    for (int i = 0; i < 20; i++) K[i] = 3 * i;
    n_min = n_max = 0; sn::merge_chunk<8>(K, b8, mn, mx);
    std::printf("merge_chunk<8> min/max calls: %ld\n", n_min + n_max);
    CHECK(n_min + n_max == 88 && n_min == 48, "merge_chunk<8>: 88 calls");
    n_min = n_max = 0; sn::merge_chunk<4>(K, b4, mn, mx);
    std::printf("merge_chunk<4> min/max calls: %ld\n", n_min + n_max);
    CHECK(n_min + n_max == 76 && n_min == 40, "merge_chunk<4>: 76 calls");
    for (int i = 0; i < 20; i++) K[i] = INF;
    n_min = n_max = 0; sn::first_two_chunks(K, b8, c8, mn, mx);
    std::printf("first_two_chunks min/max calls: %ld\n", n_min + n_max);
    CHECK(n_min + n_max == 64 && n_min == 32, "first_two_chunks: 64 calls");
    CHECK(std::is_sorted(K, K + 20) && K[15] == 14 && K[16] == INF, "first_two_chunks: worked example");
  }
  if (fails) { std::printf("%d checks FAILED\n", fails); return 1; }
  std::printf("all held\n");
  return 0;
}
