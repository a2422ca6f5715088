// Sorting and merging networks of the neighbour search's seed phase (knn_packet.hpp, knn_walk.hpp) — plain C++, host and device, everything unrolls to
// straight-line compare-exchanges. The keys are distinct (d2, index) pairs (equal ones only among the padding's sentinels), so a correct network leaves
// exactly the list that one sorted insert per candidate leaves. Every function takes the key's min and max as function objects: the device passes
// v_min_f64 / v_max_f64 on the packed keys, tests/cpp/seed_net_test.cpp integer min / max (by the 0-1 principle a network that sorts every 0-1 input sorts).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ROLO_NET_FN __host__ __device__ __forceinline__
#define ROLO_NET_UNROLL _Pragma("unroll")
#else
#define ROLO_NET_FN inline
#define ROLO_NET_UNROLL
#endif

namespace rolo {
namespace seednet {

// a <- the smaller, b <- the larger
template <class T, class Min, class Max>
ROLO_NET_FN void cx(T& a, T& b, Min mn, Max mx) {
  const T lo = mn(a, b);
  b = mx(a, b);
  a = lo;
}

// 8 keys ascending: the optimal 19-comparator network
template <class T, class Min, class Max>
ROLO_NET_FN void sort8(T (&b)[8], Min mn, Max mx) {
  constexpr int net[19][2] = {{0, 2}, {1, 3}, {4, 6}, {5, 7}, {0, 4}, {1, 5}, {2, 6}, {3, 7}, {0, 1}, {2, 3}, {4, 5}, {6, 7}, {2, 4}, {3, 5}, {1, 4}, {3, 6}, {1, 2}, {3, 4}, {5, 6}};
ROLO_NET_UNROLL
  for (int c = 0; c < 19; c++) cx(b[net[c][0]], b[net[c][1]], mn, mx);
}

// 4 keys ascending: 5 comparators
template <class T, class Min, class Max>
ROLO_NET_FN void sort4(T (&b)[4], Min mn, Max mx) {
  cx(b[0], b[1], mn, mx); cx(b[2], b[3], mn, mx); cx(b[0], b[2], mn, mx); cx(b[1], b[3], mn, mx); cx(b[1], b[2], mn, mx);
}

// The cleaner of a bitonic merge over K[OFF .. OFF + N): sorts a bitonic run ascending (DESC: descending). N need not be a power of two: an ascending clean
// pads the run IN FRONT with -inf up to the next one (a descending one with +inf), which keeps it bitonic, and the padding never moves — only the comparators
// between real positions are issued (N = 20: 40 of the 80, N = 8: 12).
template <int N, int OFF, bool DESC, class T, int KN, class Min, class Max>
ROLO_NET_FN void bitonic_clean(T (&K)[KN], Min mn, Max mx) {
  constexpr int P2 = N <= 4 ? 4 : N <= 8 ? 8 : N <= 16 ? 16 : 32, PAD = P2 - N;
  static_assert(N <= 32 && OFF + N <= KN, "run inside the list");
ROLO_NET_UNROLL
  for (int d = P2 / 2; d >= 1; d >>= 1) {
ROLO_NET_UNROLL
    for (int p = PAD; p < P2; p++) {
      if ((p & d) == 0) {
        if (DESC) cx(K[OFF + p + d - PAD], K[OFF + p - PAD], mn, mx);
        else cx(K[OFF + p - PAD], K[OFF + p + d - PAD], mn, mx);
      }
    }
  }
}

// K (ascending, 20) <- the 20 smallest of K and the ascending chunk b (NB = 8 or 4), ascending.
//  1. K[20 - NB + i] = min(K[20 - NB + i], b[NB - 1 - i]): every K[i] below has NB larger keys inside K, so the 20 smallest of the 20 + NB are those and the NB
//     smallest of K's tail and b — which this step leaves in the tail, as a bitonic run;
//  2. the tail sorted DESCENDING by its cleaner;
//  3. K rises for 20 - NB keys and falls for NB: bitonic, and the cleaner of the whole list sorts it.
// NB = 8: 8 min + 12 + 40 compare-exchanges.
template <int NB, class T, class Min, class Max>
ROLO_NET_FN void merge_chunk(T (&K)[20], const T (&b)[NB], Min mn, Max mx) {
  static_assert(NB == 8 || NB == 4, "chunk size");
ROLO_NET_UNROLL
  for (int i = 0; i < NB; i++) K[20 - NB + i] = mn(K[20 - NB + i], b[NB - 1 - i]);
  bitonic_clean<NB, 20 - NB, true>(K, mn, mx);
  bitonic_clean<20, 0, false>(K, mn, mx);
}
template <class T, class Min, class Max>
ROLO_NET_FN void merge8(T (&K)[20], const T (&b)[8], Min mn, Max mx) { merge_chunk<8>(K, b, mn, mx); }

}  // namespace seednet
}  // namespace rolo
