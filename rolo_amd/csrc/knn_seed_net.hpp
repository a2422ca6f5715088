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
// between real positions are issued (N = 20: 40 of the 80, N = 16: 32, N = 8: 12).
// ASC (ascending cleans, merge_chunk): the run's first ASC keys are known to be ascending already. Until a stage has moved one of its two keys, a comparator inside that
// prefix cannot swap and is not issued: of the 20-cleaner the stride-16 stage touches 0..3 and 16..19 only, so the stride-8 comparators (i, i + 8) with i >= 4 and
// i + 8 < ASC are dead — (4,12) (5,13) (6,14) (7,15) for ASC = 16, none for ASC <= 12. Every later stage works on keys that have moved.
template <int N, int OFF, bool DESC, int ASC, class T, int KN, class Min, class Max>
ROLO_NET_FN void bitonic_clean_known(T (&K)[KN], Min mn, Max mx) {
  constexpr int P2 = N <= 4 ? 4 : N <= 8 ? 8 : N <= 16 ? 16 : 32, PAD = P2 - N;
  static_assert(N <= 32 && OFF + N <= KN, "run inside the list");
  static_assert(ASC == 0 || (!DESC && N == 20), "the dead comparators are worked out for the ascending 20-cleaner");
ROLO_NET_UNROLL
  for (int d = P2 / 2; d >= 1; d >>= 1) {
ROLO_NET_UNROLL
    for (int p = PAD; p < P2; p++) {
      if ((p & d) == 0) {
        if (d == 8 && p - PAD >= 4 && p + d - PAD < ASC) continue;   // both keys still where the ascending prefix had them
        if (DESC) cx(K[OFF + p + d - PAD], K[OFF + p - PAD], mn, mx);
        else cx(K[OFF + p - PAD], K[OFF + p + d - PAD], mn, mx);
      }
    }
  }
}
template <int N, int OFF, bool DESC, class T, int KN, class Min, class Max>
ROLO_NET_FN void bitonic_clean(T (&K)[KN], Min mn, Max mx) { bitonic_clean_known<N, OFF, DESC, 0>(K, mn, mx); }

// K (ascending, 20) <- the 20 smallest of K and the ascending chunk b (NB = 8 or 4), ascending.
//  1. K[20 - NB + i] = min(K[20 - NB + i], b[NB - 1 - i]): every K[i] below has NB larger keys inside K, so the 20 smallest of the 20 + NB are those and the NB
//     smallest of K's tail and b — which this step leaves in the tail;
//  2. the whole list is bitonic already: K's tail is ascending and b reversed is descending, so their element-wise minimum follows K up to the crossover and the
//     reversed chunk after it — it rises, then falls — and it starts at min(K[20 - NB], b[NB - 1]) >= K[20 - NB - 1], above the untouched ascending keys in front of it.
//     The cleaner of the whole list sorts it (merge20 of knn_walk.hpp relies on the same fact); the tail needs no sort of its own.
// NB = 8: 8 min + 40 compare-exchanges = 88 min / max; NB = 4: 4 + 36 (four comparators inside the untouched prefix are dead: bitonic_clean_known) = 76.
template <int NB, class T, class Min, class Max>
ROLO_NET_FN void merge_chunk(T (&K)[20], const T (&b)[NB], Min mn, Max mx) {
  static_assert(NB == 8 || NB == 4, "chunk size");
ROLO_NET_UNROLL
  for (int i = 0; i < NB; i++) K[20 - NB + i] = mn(K[20 - NB + i], b[NB - 1 - i]);
  bitonic_clean_known<20, 0, false, 20 - NB>(K, mn, mx);
}
// The first two chunks of 8 into a list that holds nothing but sentinels (twenty equal keys no candidate is above: the seed phase's first leaf). Merging a chunk into
// sentinels leaves the chunk itself, so b0 IS the list after the first merge; b1 reversed behind it makes K[0 .. 16) rise, then fall, and the 16-cleaner (no padding,
// 32 compare-exchanges) sorts it. K[16 .. 20) are not touched: they stay sentinels, which no key of either chunk is above (a padding point's key EQUALS the sentinel
// and lands among them in value, wherever it sits). 64 min / max where two merge_chunk<8> take 176.
template <class T, class Min, class Max>
ROLO_NET_FN void first_two_chunks(T (&K)[20], const T (&b0)[8], const T (&b1)[8], Min mn, Max mx) {
ROLO_NET_UNROLL
  for (int i = 0; i < 8; i++) { K[i] = b0[i]; K[8 + i] = b1[7 - i]; }
  bitonic_clean<16, 0, false>(K, mn, mx);
}
template <class T, class Min, class Max>
ROLO_NET_FN void merge8(T (&K)[20], const T (&b)[8], Min mn, Max mx) { merge_chunk<8>(K, b, mn, mx); }

}  // namespace seednet
}  // namespace rolo
