// The packet walk of the exact k-nearest-neighbour search, as device functions: packed (d2, index) keys and their min / max sorted insert, wave-uniform
// fetches, leaf scoring and the walk itself. Included by knn_walk.hpp (K5: the queries are the cloud's own points) and by scan2map.hip (8f.4: its own walk for foreign
// queries takes the keys, insert_slot, sub_*, sload_node, xcd_contiguous_block and WALK_STACK from here, not packet_walk; the box tests are knn_box_pair.hpp's). Design notes: knn_walk.hpp.
#pragma once
#include "rolo_internal.hpp"
#include "dev_math.hpp"
#include "knn_seed_net.hpp"
#include "knn_box_pair.hpp"   // box_d2, box_d2_pair, the one-compare reach test
#include <cfloat>
#include <climits>

#ifndef KNN_STAT
#ifdef ROLO_KNN_STATS   // (the instrumented build: every includer sees the same definition — scan2map.hip includes this file without knn_walk.hpp, and calls none of the counted functions)
#define KNN_STAT(x) x
#else
#define KNN_STAT(x)
#endif
#endif

namespace rolo {
namespace {

constexpr int WALK_STACK = KNN_WALK_STACK;

ROLO_DEV double key_pack(float d2, int idx) {
  return __longlong_as_double((long long)(((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)idx));
}
ROLO_DEV float key_d2(double k) { return __uint_as_float((unsigned)((unsigned long long)__double_as_longlong(k) >> 32)); }
ROLO_DEV int key_idx(double k) { return (int)(unsigned)((unsigned long long)__double_as_longlong(k) & 0xffffffffull); }

// raw v_min_f64 / v_max_f64: fmin/fmax would add a canonicalising v_max_f64 x,x in front of every operand (sNaN
// quieting) — our operands are never NaN by construction. Pure VALU, no memory: safe as inline asm.
ROLO_DEV double vmin_f64(double a, double b) { double r; asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
ROLO_DEV double vmax_f64(double a, double b) { double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
// one slot of the sorted insert, K[s] = max(K[s-1], min(c, K[s])), as ONE asm statement: between two statements the compiler puts an s_nop for the
// read-after-write it cannot see into (20 per full insert); inside one statement the hardware interlock does the same job without the slot
#ifndef ROLO_KNN_SPLIT_MINMAX
// ("+&v": the first instruction writes %0 before the second reads %2 — without the early-clobber mark the compiler may give K[s-1] the register of K[s]
// whenever it knows the two hold the same value, e.g. two sentinels of a fresh list: seen in knn_walk_sub_kernel as lists full of repeated keys)
ROLO_DEV void insert_slot(double& ks, double ksm1, double c) { asm("v_min_f64 %0, %1, %0\n\tv_max_f64 %0, %2, %0" : "+&v"(ks) : "v"(c), "v"(ksm1)); }
#else
ROLO_DEV void insert_slot(double& ks, double ksm1, double c) { ks = vmax_f64(ksm1, vmin_f64(c, ks)); }
#endif
// sorted insert of ck into the ascending K[0 .. KMAX), in four tiers (see knn_score_leaf): the lower tiers run only if some lane's candidate sorts below them
#ifndef ROLO_KNN_B1
#define ROLO_KNN_B1 15
#define ROLO_KNN_B2 10
#define ROLO_KNN_B3 5
#endif
template <int KMAX>
ROLO_DEV void insert_tiered(double (&K)[KMAX], double ck) {
  constexpr int B1 = KMAX == 20 ? ROLO_KNN_B1 : 3 * (KMAX / 4), B2 = KMAX == 20 ? ROLO_KNN_B2 : 2 * (KMAX / 4), B3 = KMAX == 20 ? ROLO_KNN_B3 : KMAX / 4;
#pragma unroll
  for (int s = KMAX - 1; s >= B1; s--) insert_slot(K[s], K[s - 1], ck);
  if (__any(ck < K[B1 - 1])) {
#pragma unroll
    for (int s = B1 - 1; s >= B2; s--) insert_slot(K[s], K[s - 1], ck);
    if (__any(ck < K[B2 - 1])) {
#pragma unroll
      for (int s = B2 - 1; s >= B3; s--) insert_slot(K[s], K[s - 1], ck);
      if (__any(ck < K[B3 - 1])) {
#pragma unroll
        for (int s = B3 - 1; s >= 1; s--) insert_slot(K[s], K[s - 1], ck);
        K[0] = vmin_f64(ck, K[0]);
      }
    }
  }
}

// ---- wave-uniform fetches ----------------------------------------------------------------------------------------------------------------
// Node boxes and leaf points are fetched through wave-uniform addresses: one scalar load per 64 bytes per WAVE instead of a vector load per lane. The
// compiler emits scalar loads only while it can prove that nothing in the kernel may have written memory before them. Hence THE CLOBBER RULE
// (profiles/ANALYSIS.md, kernel notes): no store, atomic, fence, clock builtin or volatile asm may come ahead of the walk loop, nor on any path that
// reaches it again. After one of them the leaf's 64 floats become vector loads: 64 more VGPRs, spills, a 5-10 x slower walk. Every kernel that walks
// writes its results after the loop. (Loads written as inline asm are scalar whatever the kernel does, but cost the walk 2-3 %: DEAD_ENDS, round 4.)
ROLO_DEV void sload_leaf(const float4* __restrict__ p, float4 (&pts)[KNN_LEAF]) {
#pragma unroll
  for (int u = 0; u < KNN_LEAF; u++) pts[u] = p[u];
}
// the two child boxes of node h: boxes[4h .. 4h + 3] = left lo, left hi, right lo, right hi (64 bytes)
ROLO_DEV void sload_node(const float4* __restrict__ p, float4& llo, float4& lhi, float4& rlo, float4& rhi) { llo = p[0]; lhi = p[1]; rlo = p[2]; rhi = p[3]; }

// k = 20 without a lower bound (the headline's walk): kk = KMAX, so the lane's bound IS the list's last slot — the walk reads K[19] and keeps no copies of it
// (bkey, bd: a v_mov_b64 and a v_mov_b32 after every insert execution). A padding lane's list is zeroed after the seeds (knn_walk.hpp): no key is below (0, 0).
template <int KMAX, bool LOWER> constexpr bool walk_bound_in_list() { return KMAX == 20 && !LOWER; }

// score the KNN_LEAF (16) points of leaf g against this lane's query and insert the ones that beat its current k-th best
template <int KMAX, bool LOWER = false>
ROLO_DEV void knn_score_leaf(const float4* __restrict__ sorted, int g, const float4& q, double (&K)[KMAX], int kk, double& bkey, float& bd,
                             unsigned& n_ins, unsigned& lane_acc, unsigned& rounds, double lo = 0.0) {
  // fetch the whole leaf first: the address is wave-uniform, so these are KNN_LEAF scalar loads in flight behind ONE wait
  // (loading inside the loop serialised the scalar-cache round trips of a leaf behind the insert branch)
  float4 pts[KNN_LEAF];
  sload_leaf(sorted + KNN_LEAF * (size_t)g, pts);
  constexpr bool IN_LIST = walk_bound_in_list<KMAX, LOWER>();
  KNN_STAT(const double bkey0 = IN_LIST ? K[KMAX - 1] : bkey; unsigned my_acc = 0;)   // accepted against the bound at leaf entry: what a per-lane queue would hold
#ifdef ROLO_KNN_STATS2
  unsigned my_cur = 0;
#endif
#pragma unroll
  for (int u = 0; u < KNN_LEAF; u++) {
    const float4 c = pts[u];
    const float dx = q.x - c.x, dy = q.y - c.y, dz = q.z - c.z;
    const float cd = ((dx * dx) + (dy * dy)) + (dz * dz);  // file is compiled with -ffp-contract=off (the compiler already pairs x and y into v_pk_add_f32 / v_pk_mul_f32)
    const double ck0 = key_pack(cd, __float_as_int(c.w));
    const double ck = (LOWER && !(ck0 > lo)) ? key_pack(INFINITY, INT_MAX) : ck0;   // LOWER: a point of an earlier round's 64 is no candidate
    const bool better = IN_LIST ? ck < K[KMAX - 1] : ck < bkey;
    KNN_STAT(if (__any(better)) { n_ins++; lane_acc += (unsigned)__popcll(__ballot(better)); })
    KNN_STAT(if (ck < bkey0) my_acc++;)
#ifdef ROLO_KNN_STATS2
    if (better) my_cur++;   // accepted against the CURRENT bound: this lane's own inserts
#endif
    if (better) {
      // sorted insert, descending slot order so every step reads not-yet-overwritten neighbours — in four tiers: a slot whose lower
      // neighbour is already <= the candidate in EVERY lane keeps its value (min(ck, K[s]) = K[s] and K[s-1] <= K[s]), so the lower tiers
      // run only if some lane's candidate sorts below them. Late in the walk candidates barely beat the k-th best: most executions stop
      // after the first tier (the insert is two thirds of the walk's VALU instructions; v_min_f64 / v_max_f64 issue at the fp32 rate, profiles/tools/valu_rate.hip).
      insert_tiered<KMAX>(K, ck);
      if constexpr (!IN_LIST) {
#pragma unroll
        for (int s = 0; s < KMAX; s++) if (s == kk - 1) bkey = K[s];
        bd = key_d2(bkey);
      }
    }
  }
#ifdef ROLO_KNN_STATS
#ifdef ROLO_KNN_STATS2
  rounds += my_cur;   // per LANE (record [7] becomes the wave maximum of a lane's inserts over the whole walk: what a cross-leaf queue would execute at least)
  (void)my_acc;
#else
  { unsigned m = my_acc;   // wave maximum: the drain iterations of a per-lane queue for this leaf
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off, 64));
    rounds += m; }
#endif
#endif
}

// ---- seed leaves: sort and merge, not one insert each ---------------------------------------------------------------------------------------
// Before the tree walk a wavefront scores its own leaves and their curve neighbours. There "insert if some lane's candidate beats its bound" buys nothing: a
// lane's own point is at distance 0, so nearly every candidate is accepted by some lane, and deep (curve neighbours sort to the low slots: up to 48 VALU per
// execution, plus the bound's compare, ballot and branch). The networks of knn_seed_net.hpp take a chunk of 8 candidates into the list in 126 min / max (38 to sort it, 88 to
// merge it; the first leaf's two chunks, which meet a list of sentinels, in 140 together) with no compare and no branch; the keys are distinct (d2, index) pairs, so the list is the one the inserts would have left, bit for bit. Padding points (INFINITY
// coordinates, index INT_MAX) give exactly the sentinel key, and equal sentinels are harmless in a min / max network. (k = 20, no lower bound; the tree phase
// keeps the tiered insert: there the hungriest lane accepts about 5 of a leaf's 16, and a network over masked keys costs more.)
struct KeyMin { ROLO_DEV double operator()(double a, double b) const { return vmin_f64(a, b); } };
struct KeyMax { ROLO_DEV double operator()(double a, double b) const { return vmax_f64(a, b); } };

// NB candidates p[0], p[STRIDE], ... -> keys (the distance in the oracle's operation order) -> sorted -> merged into the ascending K
template <int NB, int STRIDE, class P>
ROLO_DEV void seed_keys(const P& p, int first, const float4& q, double (&b)[NB]) {
#pragma unroll
  for (int u = 0; u < NB; u++) {
    const float4 c = p[first + u * STRIDE];
    const float dx = q.x - c.x, dy = q.y - c.y, dz = q.z - c.z;
    const float cd = ((dx * dx) + (dy * dy)) + (dz * dz);   // (-ffp-contract=off)
    b[u] = key_pack(cd, __float_as_int(c.w));
  }
  if constexpr (NB == 8) seednet::sort8(b, KeyMin(), KeyMax()); else seednet::sort4(b, KeyMin(), KeyMax());
}
template <int NB, int STRIDE, class P>
ROLO_DEV void seed_chunk(const P& p, int first, const float4& q, double (&K)[20]) {
  double b[NB];
  seed_keys<NB, STRIDE>(p, first, q, b);
  seednet::merge_chunk<NB>(K, b, KeyMin(), KeyMax());
}

// the KNN_LEAF (16) points of seed leaf g against this lane's query, in two chunks of 8; the caller takes its bound from K once after the last seed.
// FIRST: K holds twenty sentinels (the first seed of a packet) — the two sorted chunks are the list, one 16-cleaner apart (seednet::first_two_chunks)
template <bool FIRST>
ROLO_DEV void knn_seed_leaf(const float4* __restrict__ sorted, int g, const float4& q, double (&K)[20]) {
  static_assert(KNN_LEAF == 16, "two chunks of 8");
  float4 pts[KNN_LEAF];
  sload_leaf(sorted + KNN_LEAF * (size_t)g, pts);
  if constexpr (FIRST) {
    double b0[8], b1[8];
    seed_keys<8, 1>(pts, 0, q, b0);
    seed_keys<8, 1>(pts, 8, q, b1);
    seednet::first_two_chunks(K, b0, b1, KeyMin(), KeyMax());
  } else {
    seed_chunk<8, 1>(pts, 0, q, K);
    seed_chunk<8, 1>(pts, 8, q, K);
  }
}

// ---- SUB lanes per query (round 4): exchanges among 2 / 4 / 8 adjacent lanes by DPP -------------------------------------------------------------------
template <int CTRL>
ROLO_DEV double dpp_f64(double x) {
  const long long v = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_mov_dpp((int)(unsigned)(unsigned long long)v, CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp((int)(unsigned)((unsigned long long)v >> 32), CTRL, 0xF, 0xF, true);
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
// exchange step `st` (0, 1, 2) of a reduction over SUB = 2, 4, 8 adjacent lanes: lane ^ 1, lane ^ 2 (quad_perm), then the mirror of the 8-lane half row
// (which maps each quad onto the other one)
template <int ST> ROLO_DEV double sub_xchg(double x) { return ST == 0 ? dpp_f64<0xB1>(x) : ST == 1 ? dpp_f64<0x4E>(x) : dpp_f64<0x141>(x); }
template <int SUB> ROLO_DEV double sub_min(double x) {
  x = vmin_f64(x, sub_xchg<0>(x));
  if (SUB >= 4) x = vmin_f64(x, sub_xchg<1>(x));
  if (SUB >= 8) x = vmin_f64(x, sub_xchg<2>(x));
  return x;
}
template <int SUB> ROLO_DEV double sub_max(double x) {
  x = vmax_f64(x, sub_xchg<0>(x));
  if (SUB >= 4) x = vmax_f64(x, sub_xchg<1>(x));
  if (SUB >= 8) x = vmax_f64(x, sub_xchg<2>(x));
  return x;
}

// Workgroup b of a launch runs on XCD b % 8 (round-robin dispatch), each XCD with its own 4 MB L2. Neighbouring packets of the
// Hilbert-sorted cloud read the same leaves and boxes, so give every XCD a CONTIGUOUS eighth of the packets: what one wavefront
// pulled in from HBM (1-2 us per cold fetch — the walk's real bound on the ~48k-point feature clouds) the next ones find in L2.
// Small launches (<= 512 blocks: the ~48k-point feature clouds of the odometry pipeline, where every fetch is a cold miss and the walk is
// pure latency) give each XCD ONE contiguous eighth (pipeline frame latency 0.787 -> 0.731 ms, 1552 -> 1769 frames/s); big launches deal
// runs of 64 blocks round-robin instead, because the work per packet varies along the curve and whole eighths balance worse
// (2 x 131 072 points: 0.226 ms contiguous, 0.199 ms in runs, 0.207 ms unmapped). Both are bijections on [0, G).
// wpb = wavefronts (packets) per block: the thresholds are in packets, whatever the workgroup size
ROLO_DEV int xcd_contiguous_block(int b, int G, int wpb = 4) {
#ifdef ROLO_KNN_NO_XCD_REMAP
  return b;
#else
  if (G * wpb <= 2048) {
    const int x = b & 7, k = b >> 3, q = G >> 3, r = G & 7;   // XCD x owns G / 8 (+1 for x < G % 8) consecutive blocks
    return x * q + min(x, r) + k;
  }
  const int RUN = 256 / wpb, GROUP = 8 * RUN;                  // runs of 256 packets
  if (b >= G / GROUP * GROUP) return b;                       // the whole groups are permuted, the remainder stays put
  const int grp = b / GROUP, o = b - grp * GROUP;             // o = k * 8 + x : the k-th block this group sends to XCD x
  return grp * GROUP + (o & 7) * RUN + (o >> 3);
#endif
}

// ---- the packet walk proper --------------------------------------------------------------------------------------------------------------
// One wavefront, 64 queries, from node h down; the far children wait on a small per-wave stack in LDS. Every control decision is wave-uniform.
typedef __attribute__((address_space(3))) int lds_int;

template <int KMAX, bool LOWER>
ROLO_DEV void packet_walk(const float4* __restrict__ sorted, const float4* __restrict__ boxes, int P, int g_own0, int g_own1, const float4& q, double (&K)[KMAX], int kk,
                          double& bkey, float& bd, double lo, lds_int* stk, int& sp, int h,
                          unsigned& st_nodes, unsigned& st_leaves, unsigned& st_ins, unsigned& st_lane, unsigned& st_rounds, unsigned& st_push) {
  (void)st_push;
  while (true) {
    h = __builtin_amdgcn_readfirstlane(h);
    if (h < P) {
      st_nodes++;
      float4 llo, lhi, rlo, rhi;
      sload_node(boxes + 4 * (size_t)h, llo, lhi, rlo, rhi);
      const box_f2 d = box_d2_pair(llo, lhi, rlo, rhi, q);
      const float bl = d[0], br = d[1], bdc = box_bound_clamp(walk_bound_in_list<KMAX, LOWER>() ? key_d2(K[KMAX - 1]) : bd);
      const bool okl = box_reached(bl, bdc), okr = box_reached(br, bdc);
      const unsigned long long ml = __ballot(okl), mr = __ballot(okr);
      if (ml != 0ull && mr != 0ull) {
        // nearer child first, by majority vote of the lanes that reach either child (a "lane with the largest
        // radius decides" rule needed a 6-step cross-lane max per node and did not reduce the nodes visited)
        const unsigned long long pref = __ballot((okl || okr) && (bl <= br));
        const bool left_first = 2 * __popcll(pref) >= __popcll(ml | mr);
        if (sp < WALK_STACK) { stk[sp] = left_first ? 2 * h + 1 : 2 * h; sp++; KNN_STAT(st_push++;) }
        h = left_first ? 2 * h : 2 * h + 1;
        continue;
      }
      if (ml != 0ull) { h = 2 * h; continue; }
      if (mr != 0ull) { h = 2 * h + 1; continue; }
    } else {
      const int g = h - P;
      if (g < g_own0 || g >= g_own1) {   // (the wavefront's own leaves and their neighbours along the curve were scored as seeds)
        knn_score_leaf<KMAX, LOWER>(sorted, g, q, K, kk, bkey, bd, st_ins, st_lane, st_rounds, lo);
        st_leaves++;
      }
    }
    if (sp == 0) return;
    sp--;
    h = stk[sp];
  }
}

// The walk of a packet whose own leaves were scored as seeds: CLIMB from their common ancestor a = (P + g_mine0) >> 2 (g_mine0 is a multiple of 4: the four own
// leaves are a's whole subtree) instead of descending from the root. On every level the SIBLING of a — its box is one half of the parent's record — is tested
// against the lanes' current bounds, and walked (packet_walk: it is an internal node, two levels above the leaves at least) if some lane reaches it. A descent from
// the root visits the same path: a full node visit per level whose near child is always live, the sibling pushed and popped later in this very order (nearest
// first), and two more visits that lead to leaves it then skips. A sibling is tested when its turn comes, against bounds that only shrank meanwhile, which can only
// prune more; the search is exact either way, so the list is the twenty smallest distinct keys in both forms. P < 4: a <= 1, nothing to climb — all leaves are seeds.
template <int KMAX, bool LOWER>
ROLO_DEV void packet_climb(const float4* __restrict__ sorted, const float4* __restrict__ boxes, int P, int g_mine0, int g_own0, int g_own1, const float4& q, double (&K)[KMAX], int kk,
                           double& bkey, float& bd, double lo, lds_int* stk,
                           unsigned& st_nodes, unsigned& st_leaves, unsigned& st_ins, unsigned& st_lane, unsigned& st_rounds, unsigned& st_push) {
  for (int a = (P + g_mine0) >> 2; a > 1; a >>= 1) {
    const int s = a ^ 1;
    const float4* __restrict__ rec = boxes + 4 * (size_t)(a >> 1) + 2 * (s & 1);   // the sibling's half of the parent's record: lo, hi
    const float4 slo = rec[0], shi = rec[1];
    const float d = box_d2(slo, shi, q);
    const float bdc = box_bound_clamp(walk_bound_in_list<KMAX, LOWER>() ? key_d2(K[KMAX - 1]) : bd);
    KNN_STAT(st_nodes++;)
    if (__ballot(box_reached(d, bdc)) != 0ull) {
      int sp = 0;
      packet_walk<KMAX, LOWER>(sorted, boxes, P, g_own0, g_own1, q, K, kk, bkey, bd, lo, stk, sp, s, st_nodes, st_leaves, st_ins, st_lane, st_rounds, st_push);
    }
  }
}

}  // namespace
}  // namespace rolo
