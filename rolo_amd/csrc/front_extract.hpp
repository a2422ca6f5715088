// K3 + K4 — extract_kernel, one workgroup per ring, as named phases (device only; front.hip includes this and nothing else does).
// The design is in front.hip's file comment; the kernel at the end of this file reads as the list of its phases:
//   load_window        K3: curvature and occlusion marks of the ring's window, gathered from range / col
//   break_reach        column breaks and how far a pick's marks go from every cell
//   sector_keys        the six sectors' (curvature, index) keys, then one segmented bitonic sort
//   ring_picks         all twelve pick stages of the ring as one fixed point (rings away from the cloud's ends, no sector over the corner cap)
//   sector_parallel    ... else sector by sector: a corner and a surface fixed point,
//   sector_serial      or, at the cloud's ends where the stale entries do not reduce to that, the reference's walk on one lane
//   write_back         the window's picked / label cells to the global arrays
//   voxel_grid         pcl::VoxelGrid of the ring's surface scan
// The rules that several phases share have one definition each: sector_bounds, cand_at / cand_curv, pick_fixed_point, mark_reach,
// walk_get / walk_set / walk_marks, scan_append. Every phase's head comment says what it reads, what it writes and which barrier it ends on;
// every branch around a barrier is uniform over the workgroup.
#pragma once
#include "rolo_internal.hpp"   // rolo_hip.h: the ROLO_XPATH_* words
#include "dev_math.hpp"
#include <cfloat>
#include <climits>

namespace rolo {

constexpr int FRONT_GUARD = 8;       // guard cells in front of / behind the per-point arrays (reference reads index -1.. )
// bitonic capacity (elements) for a Horizon_SCAN limit of maxh: 6 sector segments of <= maxh / 4, which also holds one ring's surface scan (<= maxh)
constexpr int front_sort_cap(int maxh) { return 6 * (maxh / 4); }
constexpr int front_win(int maxh) { return maxh + 2 * 16; }   // cells of a ring window: the ring's points and 16 on either side
constexpr int FRONT_WIN_ARRAYS = 8;                           // l_picked, l_col, l_label, l_curv, l_brk, l_rank, l_stat, l_reach
// one ring's working set (RingWin below carves it, and asserts that it carves exactly this): LDS up to FRONT_MAX_H, else a scratch area per ring
constexpr size_t front_ring_bytes(int maxh) { return sizeof(unsigned long long) * (size_t)front_sort_cap(maxh) + sizeof(int) * (size_t)front_win(maxh) * FRONT_WIN_ARRAYS + sizeof(int) * (size_t)(maxh + 16); }
constexpr int ST_OUT = 0, ST_UNDECIDED = 1, ST_PICKED = 2;

namespace {

// Ascending bitonic sort of every aligned `seg`-element segment of key[0, total) in LDS (seg a power of two, total a
// multiple of seg; NT threads). Exchange distances >= 64 are block-wide steps with a barrier each; the distances
// 32..1 that close every merge stage stay inside an aligned 64-element chunk, so one wavefront takes the chunk into
// registers and finishes the stage with cross-lane exchanges (DPP / permlane swaps) — one barrier per stage instead of
// one per step.
template <int J2>
ROLO_DEV void bitonic_lane_step(unsigned long long& v, int lane, bool up) {
  const unsigned long long o = lane_xor_u64<J2>(v);   // DPP / v_permlane*_swap: no LDS crossbar (dev_math.hpp)
  const bool take_min = ((lane & J2) == 0) == up;     // the lane with the smaller index of the pair keeps the minimum when ascending
  v = take_min ? (o < v ? o : v) : (o > v ? o : v);
}
template <int NT>
ROLO_DEV void bitonic_sort_lds_seg(unsigned long long* key, int total, int seg) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int n_chunks = (total + 63) >> 6;
  for (int k = 2; k <= seg; k <<= 1) {
    int jj = k >> 1;
    for (; jj >= 64; jj >>= 1) {
      for (int i = t; i < total; i += NT) {
        const int ixj = i ^ jj;
        if (ixj > i) {
          const unsigned long long a = key[i], b = key[ixj];
          const bool up = ((i & (seg - 1)) & k) == 0;
          if ((a > b) == up) { key[i] = b; key[ixj] = a; }
        }
      }
      __syncthreads();
    }
    for (int c = wv; c < n_chunks; c += NT / 64) {
      const int i = (c << 6) + lane;
      unsigned long long v = i < total ? key[i] : ~0ull;
      const bool up = ((i & (seg - 1)) & k) == 0;
      if (jj >= 32) bitonic_lane_step<32>(v, lane, up);
      if (jj >= 16) bitonic_lane_step<16>(v, lane, up);
      if (jj >= 8) bitonic_lane_step<8>(v, lane, up);
      if (jj >= 4) bitonic_lane_step<4>(v, lane, up);
      if (jj >= 2) bitonic_lane_step<2>(v, lane, up);
      bitonic_lane_step<1>(v, lane, up);
      if (i < total) key[i] = v;
    }
    __syncthreads();
  }
}
template <int NT>
ROLO_DEV void bitonic_sort_lds(unsigned long long* key, int n_pow2) { bitonic_sort_lds_seg<NT>(key, n_pow2, n_pow2); }

struct FeatArgs {
  const float4* extracted; const int* col; const float* range; float* curv; int* picked; int* label;  // global, guard-offset pointers
  const int* start_ring; const int* end_ring;
  const int* n_ptr; int n_scan; float edge_threshold, surf_threshold, leaf;
  float4* corner_stage; int* corner_cnt;  // [n_scan][6][20], [n_scan][6]
  float4* surf_stage; int* surf_cnt;      // [n_scan][MAXH], [n_scan]
  unsigned char* big;                     // Horizon_SCAN > 2048: front_ring_bytes(MAXH) of scratch per ring
  int* paths;                             // [n_scan]: which way the ring's picks were made (ROLO_XPATH_*, rolo_hip.h) — one lane's store per ring
};

// One workgroup of XT = 1024 threads per ring: 128 rings are only 128 workgroups, so the parallelism has to come from inside —
// 16 wavefronts (4 per SIMD) hide the LDS / cross-lane latency of the sorts that 4 wavefronts (1 per SIMD) exposed.
#ifndef ROLO_XT
#define ROLO_XT 1024
#endif
constexpr int XT = ROLO_XT, XW = XT / 64;   // threads, wavefronts
#ifdef ROLO_XT_STATS
__device__ unsigned long long g_xt[128][8];   // per ring: phase time stamps of extract_kernel (shader clock)
#define XT_STAMP(k) do { if (threadIdx.x == 0 && blockIdx.x < 128) g_xt[blockIdx.x][k] = clock64(); } while (0)
extern "C" int rolo_debug_extract_times(unsigned long long* out /* 128 x 8 */) {
  (void)hipDeviceSynchronize();
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_xt), sizeof(unsigned long long) * 128 * 8) == hipSuccess ? 0 : -1;
}
#else
#define XT_STAMP(k)
#endif

// ---- the ring's working set, carved once ----
// layout of raw (LDS, or the ring's scratch area): keys[SORT_CAP] u64 | l_picked | l_col | l_label | l_curv (ring window, WIN cells each) | list[MAXH + 16] |
// l_brk | l_rank | l_stat | l_reach (window) — front_ring_bytes(MAXH) in all, asserted below
template <int MAXH>
struct RingWin {
  static constexpr int SORT_CAP = front_sort_cap(MAXH), SEGMAX = MAXH / 4, WIN = front_win(MAXH);
  static constexpr int UP = (SEGMAX + XT - 1) / XT;        // positions of one sector per thread
  static constexpr int UPG = (6 * SEGMAX + XT - 1) / XT;   // entries (sector, position) of the whole ring per thread
  unsigned long long* keys;   // the sort's keys: six sector segments, later the VoxelGrid's (load_window borrows it as scratch)
  int* l_picked; int* l_col; int* l_label; float* l_curv;   // cloudNeighborPicked, column, cloudLabel, cloudCurvature of the window's cells
  int* list;                  // the ring's surface scan: global indices, in order
  int* l_brk;                 // the suppression marks of a pick stop between window cells i and i + 1 (|columnDiff| > 10, :199-210)
  int* l_rank; int* l_stat;   // a fixed point's rank and ST_* state per cell; INT_MAX / ST_OUT between stages
  int* l_reach;               // how far a pick's suppression marks go from this cell: forward | backward << 4 (0..5 each)
  int ring, s, e, n;          // this ring, its start_ring / end_ring, points in the cloud
  int w0, wlen;               // the window holds the global indices [w0, w0 + wlen)

  ROLO_DEV RingWin(unsigned char* raw, const FeatArgs& A) {
    keys = reinterpret_cast<unsigned long long*>(raw);
    l_picked = reinterpret_cast<int*>(keys + SORT_CAP);
    l_col = l_picked + WIN;
    l_label = l_col + WIN;
    l_curv = reinterpret_cast<float*>(l_label + WIN);
    list = reinterpret_cast<int*>(l_curv + WIN);
    l_brk = list + (MAXH + 16);
    l_rank = l_brk + WIN;
    l_stat = l_rank + WIN;
    l_reach = l_stat + WIN;
    static_assert(sizeof(unsigned long long) * SORT_CAP + sizeof(int) * ((size_t)WIN * FRONT_WIN_ARRAYS + MAXH + 16) == front_ring_bytes(MAXH),
                  "RingWin carves what front_ring_bytes reserves");
    ring = blockIdx.x;
    s = A.start_ring[ring]; e = A.end_ring[ring];
    n = *A.n_ptr;
    w0 = s - 16;
    wlen = (e - s) + 32 + 1;
    if (wlen < 0) wlen = 0;
    if (wlen > WIN) wlen = WIN;  // guarded by the host (ring population <= MAXH)
  }
};

// ---- the shared rules ----
// sector j of a ring (featureExtraction.cpp:171-172): the sorted range is [sp, ep), the walks visit sp .. ep
struct Sector { int sp, ep; };
ROLO_DEV Sector sector_bounds(int s, int e, int j) { return Sector{(s * (6 - j) + e * j) / 6, (s * (5 - j) + e * (j + 1)) / 6 - 1}; }

// The candidate at position k of a sector's walk: the point it names and that point's window cell. Position ep is outside the sorted range:
// cloudSmoothness[ep] is {curvature, ep} as calculateSmoothness left it for ep in [5, n - 5), else the zero-initialised {0, 0}.
struct Cand { int ind, li; bool in_win; };
template <int MAXH>
ROLO_DEV Cand cand_at(const RingWin<MAXH>& W, const unsigned long long* skeys, Sector sec, int k) {
  Cand c;
  c.ind = (k == sec.ep) ? ((sec.ep >= 5 && sec.ep < W.n - 5) ? sec.ep : 0) : (int)(unsigned)(skeys[k - sec.sp] & 0xffffffffull);
  c.li = c.ind - W.w0;
  c.in_win = c.li >= 0 && c.li < W.wlen;   // a stale entry of a tail ring names point 0, far outside this ring's window
  return c;
}
// ... and its curvature for the fixed points (c.in_win): a stale {0, 0} entry has curvature 0 whatever the window holds for point 0
template <int MAXH>
ROLO_DEV float cand_curv(const RingWin<MAXH>& W, Cand c) { return c.ind == 0 ? 0.f : W.l_curv[c.li]; }

// The greedy picks of one or more stages as a fixed point: "picked iff no better-ranked candidate that reaches it is picked". Every lane owns U
// candidates (window cell my_li[u], -1: none; rank my_rank[u]). Reads l_reach, and l_rank / l_stat as the caller wrote them before its barrier;
// moves every ST_UNDECIDED cell of l_stat to ST_PICKED or ST_OUT. Ends on the barrier of the round that left nothing undecided.
template <int U, int MAXH>
ROLO_DEV void pick_fixed_point(const RingWin<MAXH>& W, const int (&my_li)[U], const int (&my_rank)[U]) {
  // which of the ten neighbours can suppress this candidate: within reach and better ranked — fixed for the stage
  unsigned my_nb[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    my_nb[u] = 0u;
    const int li = my_li[u];
    if (li < 0) continue;
    const int rc = W.l_reach[li], fr = rc & 15, br = rc >> 4;
#pragma unroll
    for (int d = 1; d <= 5; d++) {
      const int rf = W.l_rank[li + d], rb = W.l_rank[li - d];
      if (d <= fr && rf < my_rank[u]) my_nb[u] |= 1u << (d - 1);
      if (d <= br && rb < my_rank[u]) my_nb[u] |= 1u << (4 + d);
    }
  }
  // Every round decides the candidates whose better-ranked reaching candidates are all decided; the chains are a handful of links long, so a
  // stage takes a few rounds of ~20 LDS reads instead of ~10^3 dependent LDS steps on one lane.
  while (true) {   // states only ever move UNDECIDED -> final, so a neighbour's state read mid-update is either still valid
    int undecided = 0;
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int li = my_li[u];
      if (li < 0 || W.l_stat[li] != ST_UNDECIDED) continue;
      bool any_sel = false, any_und = false;
#pragma unroll
      for (int d = 1; d <= 5; d++) {   // ten independent LDS reads
        const int sf = W.l_stat[li + d], sb = W.l_stat[li - d];
        if (my_nb[u] & (1u << (d - 1))) { any_sel |= sf == ST_PICKED; any_und |= sf == ST_UNDECIDED; }
        if (my_nb[u] & (1u << (4 + d))) { any_sel |= sb == ST_PICKED; any_und |= sb == ST_UNDECIDED; }
      }
      if (any_sel) W.l_stat[li] = ST_OUT;
      else if (!any_und) W.l_stat[li] = ST_PICKED;
      else undecided = 1;
    }
    if (!__syncthreads_or(undecided)) break;
  }
}
// leave the rank / state cells of this lane's candidates neutral for the next stage (no barrier)
template <int U, int MAXH>
ROLO_DEV void clear_rank_state(const RingWin<MAXH>& W, const int (&my_li)[U]) {
#pragma unroll
  for (int u = 0; u < U; u++) if (my_li[u] >= 0) { W.l_rank[my_li[u]] = INT_MAX; W.l_stat[my_li[u]] = ST_OUT; }
}
// a pick of the fixed points marks itself and its neighbours up to the column breaks (l_reach) as taken (:196-210)
template <int MAXH>
ROLO_DEV void mark_reach(const RingWin<MAXH>& W, int li) {
  W.l_picked[li] = 1;
  const int rc = W.l_reach[li], fr = rc & 15, br = rc >> 4;
#pragma unroll
  for (int d = 1; d <= 5; d++) { if (d <= fr) W.l_picked[li + d] = 1; if (d <= br) W.l_picked[li - d] = 1; }
}

// The serial walk's cells, by global index g: the window's cell, or else the global array's. Validated input never leaves the window (the head
// of tests/front_rings.py says why); the global side is the reference's access as written, kept as defence.
template <int MAXH, class T>
ROLO_DEV T walk_get(const RingWin<MAXH>& W, const T* win, const T* glob, int g) {
  const int li = g - W.w0;
  return (li >= 0 && li < W.wlen) ? win[li] : glob[g];
}
template <int MAXH, class T>
ROLO_DEV void walk_set(const RingWin<MAXH>& W, T* win, T* glob, int g, T v) {
  const int li = g - W.w0;
  if (li >= 0 && li < W.wlen) win[li] = v; else glob[g] = v;
}
// a pick of the serial walk marks itself and its +-5 neighbours, on either side up to the first column break (:196-210)
template <int MAXH>
ROLO_DEV void walk_marks(const RingWin<MAXH>& W, const FeatArgs& A, int ind) {
  walk_set(W, W.l_picked, A.picked, ind, 1);
  for (int dir = 1; dir >= -1; dir -= 2)
    for (int l = 1; l <= 5; l++) {
      const int a = ind + dir * l, b = a - dir;
      if (abs(walk_get(W, W.l_col, A.col, a) - walk_get(W, W.l_col, A.col, b)) > 10) break;
      walk_set(W, W.l_picked, A.picked, a, 1);
    }
}

// The ring's surface scan so far: its length (every thread keeps the same count) and which half of scan_append's counters the next pass uses.
struct ScanCursor { int cnt, par; };
// Every k of [k0, k1] with label <= 0 joins the ring's surface scan, in k order (:240-252): a ballot compaction. Reads l_label, which the
// caller's barrier has made final; appends to list. One barrier per 1024 cells (the counters alternate), none after the last store to list.
template <int MAXH>
ROLO_DEV void scan_append(const RingWin<MAXH>& W, int k0, int k1, ScanCursor& sc) {
  __shared__ int s_cw[2][XW];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  for (int base = k0; base <= k1; base += XT) {
    const int k = base + t;
    const bool v = k <= k1 && W.l_label[k - W.w0] <= 0;
    const unsigned long long bal = __ballot(v);
    if (lane == 0) s_cw[sc.par][wv] = __popcll(bal);
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < XW; w++) { const int c = s_cw[sc.par][w]; tot += c; if (w < wv) woff += c; }
    if (v) W.list[sc.cnt + woff + __popcll(bal & ((1ull << lane) - 1ull))] = k;
    sc.cnt += tot;
    sc.par ^= 1;
  }
}

// ---- the phases ----
// K3 inside this kernel (was: smoothness_kernel + occlusion_kernel, two launches on the frame's critical path): curvature
// (calculateSmoothness, featureExtraction.cpp:87-110) and the occlusion / parallel-beam marks (markOccludedPoints, :112-149) of the window's
// cells straight from range / col. The reference SCATTERS the marks (point j marks j-5..j or j+1..j+6); here every cell GATHERS the three
// conditions of the points that could mark it — the same set, no write shared between workgroups.
// Reads A.range, A.col. Writes l_picked, l_col, l_label (0), l_curv, and A.curv of the ring's own cells; keys is its scratch.
// Ends on a barrier: the window is whole and keys is free.
template <int MAXH>
ROLO_DEV void load_window(const RingWin<MAXH>& W, const FeatArgs& A) {
  const int t = threadIdx.x, n = W.n, w0 = W.w0, wlen = W.wlen;
  int* l_flag = reinterpret_cast<int*>(W.keys);   // scratch (the sector sort fills keys later): conditions of the points [w0 - 6, w0 + wlen + 6)
  for (int i = t; i < wlen + 12; i += XT) {
    const int j = w0 - 6 + i;
    int fl = 0;
    if (j >= 5 && j < n - 6) {   // :116
      const float depth1 = A.range[j], depth2 = A.range[j + 1];
      const int columnDiff = abs(A.col[j + 1] - A.col[j]);
      if (columnDiff < 10) {
        if (depth1 - depth2 > 0.3) fl |= 1;        // marks j-5 .. j
        else if (depth2 - depth1 > 0.3) fl |= 2;   // marks j+1 .. j+6
      }
      const float diff1 = fabsf(float(A.range[j - 1] - A.range[j]));
      const float diff2 = fabsf(float(A.range[j + 1] - A.range[j]));
      if (diff1 > 0.02 * A.range[j] && diff2 > 0.02 * A.range[j]) fl |= 4;   // marks j
    }
    l_flag[i] = fl;
  }
  __syncthreads();
  for (int i = t; i < wlen; i += XT) {
    const int gi = w0 + i;
    const bool in = gi >= -FRONT_GUARD && gi < n + FRONT_GUARD;
    float c = 0.f;
    if (gi >= 5 && gi < n - 5) {  // :91-99, float sum in the written order
      const float* range = A.range;
      const float diffRange = range[gi - 5] + range[gi - 4] + range[gi - 3] + range[gi - 2] + range[gi - 1] - range[gi] * 10
                            + range[gi + 1] + range[gi + 2] + range[gi + 3] + range[gi + 4] + range[gi + 5];
      c = diffRange * diffRange;
    }
    int pk = (l_flag[i + 6] >> 2) & 1;
#pragma unroll
    for (int k = 0; k <= 5; k++) pk |= l_flag[i + 6 + k] & 1;
#pragma unroll
    for (int k = 1; k <= 6; k++) pk |= (l_flag[i + 6 - k] >> 1) & 1;
    W.l_picked[i] = pk;
    W.l_col[i] = in ? A.col[gi] : 0;
    W.l_label[i] = 0;
    W.l_curv[i] = c;
    if (gi >= W.s - 4 && gi <= W.e + 5 && gi >= 0 && gi < n) A.curv[gi] = c;   // the ring's own cells (rings tile [0, n)): cloudCurvature as the reference leaves it
  }
  __syncthreads();   // keys is scratch no longer
}

// Reads l_col. Writes l_rank / l_stat (neutral), l_brk, l_reach. Two barriers inside; NONE after the l_reach stores — sector_keys' closing barrier
// stands between them and their first reader.
template <int MAXH>
ROLO_DEV void break_reach(const RingWin<MAXH>& W) {
  const int t = threadIdx.x, wlen = W.wlen;
  for (int i = t; i < wlen; i += XT) { W.l_rank[i] = INT_MAX; W.l_stat[i] = ST_OUT; }
  __syncthreads();
  for (int i = t; i + 1 < wlen; i += XT) W.l_brk[i] = abs(W.l_col[i + 1] - W.l_col[i]) > 10 ? 1 : 0;
  __syncthreads();
  for (int i = t; i < wlen; i += XT) {   // once per ring: the rounds of pick_fixed_point then read their neighbours without a dependent chain of break tests
    int fr = 0, br = 0;
    if (i >= 5 && i + 5 < wlen) {
      for (int d = 1; d <= 5; d++) { if (W.l_brk[i + d - 1]) break; fr = d; }
      for (int d = 1; d <= 5; d++) { if (W.l_brk[i - d]) break; br = d; }
    }
    W.l_reach[i] = fr | (br << 4);
  }
}

// The keys of all six sector sorts at once (they depend on the curvatures only): 6 segments of seg keys, seg the power of two that holds the longest
// sector, sector j's [sp, ep) at keys[j * seg ...] and ~0 behind it. Reads l_curv, writes keys, returns seg. Ends on a barrier; the caller sorts.
template <int MAXH>
ROLO_DEV int sector_keys(const RingWin<MAXH>& W) {
  const int t = threadIdx.x;
  int seg = 2, maxlen = 0;
  for (int j = 0; j < 6; j++) {
    const Sector sec = sector_bounds(W.s, W.e, j);
    maxlen = max(maxlen, sec.ep - sec.sp);
  }
  while (seg < maxlen) seg <<= 1;  // <= SEGMAX: a sector holds at most Horizon_SCAN / 6 + 1 points
  for (int i = t; i < 6 * seg; i += XT) {
    const int j = i / seg, li = i - j * seg;
    const Sector sec = sector_bounds(W.s, W.e, j);
    unsigned long long kv = ~0ull;
    if (li < sec.ep - sec.sp) {
      const int k = sec.sp + li;
      // cloudSmoothness[k] = {curvature, k} for k in [5, n-5), else the zero-initialised {0, 0}
      const bool live = k >= 5 && k < W.n - 5;
      const float cv = live ? W.l_curv[k - W.w0] : 0.f;
      const int ind = live ? k : 0;
      kv = ((unsigned long long)__float_as_uint(cv) << 32) | (unsigned)ind;
    }
    W.keys[i] = kv;
  }
  __syncthreads();
  return seg;
}

// ---- all twelve pick stages of the ring as ONE fixed point (rings away from the cloud's two ends, at most 20 corners per sector) ----
// The reference walks sector 0 corners, sector 0 surfaces, sector 1 corners, ... (featureExtraction.cpp:168-252); a pick marks its +-5
// neighbours (up to a column break) and later candidates that are marked are skipped. Order every candidate of the ring by (sector, pass,
// rank in its walk): a candidate is picked iff no candidate EARLIER in that order that reaches it is picked — sector_parallel's stage-by-stage
// rule with the order extended across stages, so the chains of twelve stages resolve together (a stage costs ~4 us of barriers with
// a third of the threads busy). Not covered here and left to the staged code: sectors at the cloud's ends (stale smoothness entries),
// thresholds that let a cell be corner AND surface candidate, and the cap — the corner walk stops after its 20th pick
// (largestPickedNum, :186-193), so a sector with more corner picks than that is redone stage by stage (checked before anything is applied).
// Reads the sorted keys, l_curv, l_picked, l_reach. Returns (uniform over the workgroup)
//   ROLO_XPATH_RING_NONE     not eligible: nothing touched, no barrier;
//   ROLO_XPATH_RING_CAPPED   the cap strikes somewhere: nothing applied but A.corner_cnt (rewritten by the staged code), l_rank / l_stat neutral again, ends on a barrier;
//   ROLO_XPATH_RING_APPLIED  l_label, l_picked, A.corner_stage / corner_cnt written and the whole ring appended to the surface scan (scan_append's ending).
template <int MAXH>
ROLO_DEV int ring_picks(const RingWin<MAXH>& W, const FeatArgs& A, int seg, ScanCursor& sc) {
#ifdef ROLO_XT_STAGED
  return ROLO_XPATH_RING_NONE;
#else
  constexpr int SEGMAX = RingWin<MAXH>::SEGMAX, UPG = RingWin<MAXH>::UPG;
  __shared__ int s_gpk[UPG][XW], s_gep[6], s_gbad;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int s = W.s, e = W.e, n = W.n, w0 = W.w0, wlen = W.wlen, ring = W.ring;
  bool eligible = A.surf_threshold > 0.f && A.edge_threshold >= A.surf_threshold && seg >= 64 && e - s >= 12;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    const Sector sec = sector_bounds(s, e, j);
    eligible = eligible && sec.ep > sec.sp && sec.ep - sec.sp < SEGMAX;
  }
  // the cloud's ends (twin: head_ok / tail_ok of extract_kernel's staged loop, per sector): the head ring's stale {0, 0} entries name point 0 — inside this ring's window,
  // an ordinary surface candidate of curvature 0; a tail ring's name point 0 too, which the first ring marked long ago: out of the window, skipped
  const int ep_first = sector_bounds(s, e, 0).ep, ep_last = sector_bounds(s, e, 5).ep;
  const bool head = s < 5, tail = ep_last >= n - 5;
  if (head) eligible = eligible && !tail && ep_first >= 5 && w0 <= 0 && -w0 < wlen;
  if (tail) eligible = eligible && !head && n >= 64 && A.start_ring[0] == 4 && A.end_ring[0] >= 30;
  if (!eligible) return ROLO_XPATH_RING_NONE;   // uniform
  if (t < 6) s_gep[t] = 0;
  if (t == 0) s_gbad = 0;
  int my_li[UPG], my_rank[UPG];
#pragma unroll
  for (int u = 0; u < UPG; u++) {
    const int i = t + XT * u, j = i / SEGMAX, p = i - j * SEGMAX;
    my_li[u] = -1; my_rank[u] = INT_MAX;
    if (j < 6) {
      const Sector sec = sector_bounds(s, e, j);
      if (p <= sec.ep - sec.sp) {
        const int k = sec.sp + p;
        const Cand c = cand_at(W, W.keys + j * seg, sec, k);
        const float cv = c.in_win ? cand_curv(W, c) : 0.f;
        const bool corner = cv > A.edge_threshold, surf = cv < A.surf_threshold;   // never both: edge_threshold >= surf_threshold
        if (c.in_win && (corner || surf)) {
          const int rank = corner ? ((k == sec.ep) ? 0 : sec.ep - k) : p;   // corners walk k = ep .. sp, surfaces k = sp .. ep
          my_li[u] = c.li; my_rank[u] = ((2 * j + (corner ? 0 : 1)) << 12) | rank;
          W.l_rank[c.li] = my_rank[u];
          W.l_stat[c.li] = W.l_picked[c.li] == 0 ? ST_UNDECIDED : ST_OUT;
        }
      }
    }
  }
  __syncthreads();
  pick_fixed_point<UPG>(W, my_li, my_rank);
  // corner picks per (entry slot, wavefront); the k == ep entry of a sector leads its walk
  bool pk[UPG];
#pragma unroll
  for (int u = 0; u < UPG; u++) {
    const int i = t + XT * u, j = i / SEGMAX, p = i - j * SEGMAX;
    const bool is_corner = my_li[u] >= 0 && ((my_rank[u] >> 12) & 1) == 0;
    pk[u] = is_corner && W.l_stat[my_li[u]] == ST_PICKED;
    bool is_ep = false;
    if (j < 6 && is_corner) { const Sector sec = sector_bounds(s, e, j); is_ep = p == sec.ep - sec.sp; }
    if (is_ep && pk[u]) s_gep[j] = 1;
    const unsigned long long bal = __ballot(pk[u] && !is_ep);
    if (lane == 0) s_gpk[u][wv] = __popcll(bal);
    // ordinal inside the slot: picks at higher positions of this wavefront's 64
    my_rank[u] = (my_rank[u] & ~0xfff) | (is_ep ? 0xfff : __popcll(bal & ~((2ull << lane) - 1ull)));   // rank no longer needed: low 12 bits = picks above in the wave (0xfff: the ep entry)
  }
  __syncthreads();
  // a sector's total and, per entry, the picks at higher positions in other wavefront slots of the same sector
  int higher[UPG];
#pragma unroll
  for (int u = 0; u < UPG; u++) {
    higher[u] = 0;
    const int i0 = wv * 64 + XT * u, j = i0 / SEGMAX;
    int total = j < 6 ? s_gep[min(j, 5)] : 0;
#pragma unroll
    for (int u2 = 0; u2 < UPG; u2++)
#pragma unroll
      for (int w2 = 0; w2 < XW; w2++) {
        const int i2 = w2 * 64 + XT * u2;
        if (i2 / SEGMAX == j) { const int c = s_gpk[u2][w2]; total += c; if (i2 > i0) higher[u] += c; }
      }
    if (j < 6 && total > 20) s_gbad = 1;
    if (j < 6 && lane == 0 && (i0 - j * SEGMAX) == 0) A.corner_cnt[ring * 6 + j] = total;   // (rewritten by the staged code if the cap strikes)
  }
  __syncthreads();
  if (s_gbad != 0) {
    // the cap strikes somewhere on this ring: nothing has been applied; neutral rank / state cells for the staged code
    clear_rank_state<UPG>(W, my_li);
    __syncthreads();
    return ROLO_XPATH_RING_CAPPED;
  }
#pragma unroll
  for (int u = 0; u < UPG; u++) {
    const int li = my_li[u];
    if (li < 0 || W.l_stat[li] != ST_PICKED) continue;
    const int j = (t + XT * u) / SEGMAX;
    if (((my_rank[u] >> 12) & 1) == 0) {
      const int within = my_rank[u] & 0xfff;
      const int ordinal = within == 0xfff ? 0 : s_gep[j] + higher[u] + within;
      W.l_label[li] = 1;
      A.corner_stage[(ring * 6 + j) * 20 + ordinal] = A.extracted[li + w0];
    } else {
      W.l_label[li] = -1;
    }
    mark_reach(W, li);
  }
  __syncthreads();
  scan_append(W, s, ep_last, sc);   // the sectors tile [s, e - 1]
  return ROLO_XPATH_RING_APPLIED;
#endif
}

// ---- one sector, stage by stage: parallel greedy picks ----
// The reference walks the sector in curvature order and a pick marks its +-5 neighbours (up to a column break) as
// taken. Equivalent fixed point: a candidate is picked iff no better-ranked candidate that reaches it is picked (pick_fixed_point),
// once for the corners (:181-211) and once for the surfaces (:213-238).
// Reads sector j's sorted keys, l_curv, l_picked, l_reach. Writes l_label, l_picked, A.corner_stage / corner_cnt; uses l_rank / l_stat and leaves them
// neutral. Every pass ends on a barrier; the closing clear_rank_state has none — the caller's barrier before scan_append follows.
template <int MAXH>
ROLO_DEV void sector_parallel(const RingWin<MAXH>& W, const FeatArgs& A, int j, Sector sec, const unsigned long long* skeys) {
  constexpr int UP = RingWin<MAXH>::UP;
  __shared__ int s_pk[UP][XW], s_ep;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int len = sec.ep - sec.sp;  // sorted range [sp, ep); positions sp..ep take part in the picks
  int my_li[UP], my_rank[UP];
  for (int pass = 0; pass < 2; pass++) {   // 0: corners, 1: surfaces
    const float thr = pass == 0 ? A.edge_threshold : A.surf_threshold;
#pragma unroll
    for (int u = 0; u < UP; u++) {
      const int p = t + XT * u;
      my_li[u] = -1; my_rank[u] = INT_MAX;
      if (p <= len) {
        const int k = sec.sp + p;
        const Cand c = cand_at(W, skeys, sec, k);
        if (c.in_win) {   // a stale entry of the cloud's last sector is a no-op (extract_kernel's staged loop)
          const int rank = pass == 0 ? ((k == sec.ep) ? 0 : sec.ep - k) : p;   // corners walk k = ep .. sp, surfaces k = sp .. ep
          const float cv = cand_curv(W, c);
          const bool cand = W.l_picked[c.li] == 0 && (pass == 0 ? cv > thr : cv < thr);
          my_li[u] = c.li; my_rank[u] = rank;
          W.l_rank[c.li] = rank;
          W.l_stat[c.li] = cand ? ST_UNDECIDED : ST_OUT;
        }
      }
    }
    __syncthreads();
    pick_fixed_point<UP>(W, my_li, my_rank);
    // apply the picks; corners: only the first 20 in walk order exist (largestPickedNum, :186-193)
    int ordinal[UP] = {};
    if (pass == 0) {
      // walk order = position len first, then len - 1 .. 0: a pick's ordinal is the number of picks at higher positions
      int higher[UP];
#pragma unroll
      for (int u = 0; u < UP; u++) {
        const int p = t + XT * u;
        const bool pk = my_li[u] >= 0 && W.l_stat[my_li[u]] == ST_PICKED;
        if (p == len) s_ep = pk ? 1 : 0;
        const unsigned long long bal = __ballot(pk && p != len);
        higher[u] = __popcll(bal & ~((2ull << lane) - 1ull));
        if (lane == 0) s_pk[u][wv] = __popcll(bal);
      }
      __syncthreads();
      int total = s_ep;
#pragma unroll
      for (int u = 0; u < UP; u++) {
#pragma unroll
        for (int w = 0; w < XW; w++) {
          total += s_pk[u][w];
#pragma unroll
          for (int u2 = 0; u2 < UP; u2++) if (u > u2 || (u == u2 && w > wv)) higher[u2] += s_pk[u][w];
        }
      }
#pragma unroll
      for (int u = 0; u < UP; u++) ordinal[u] = (t + XT * u == len) ? 0 : s_ep + higher[u];
      if (t == 0) A.corner_cnt[W.ring * 6 + j] = min(total, 20);
    }
#pragma unroll
    for (int u = 0; u < UP; u++) {
      const int li = my_li[u];
      if (li < 0 || W.l_stat[li] != ST_PICKED) continue;
      if (pass == 0) {
        if (ordinal[u] >= 20) continue;
        W.l_label[li] = 1;
        A.corner_stage[(W.ring * 6 + j) * 20 + ordinal[u]] = A.extracted[li + W.w0];
      } else {
        W.l_label[li] = -1;
      }
      mark_reach(W, li);
    }
    __syncthreads();
  }
  clear_rank_state<UP>(W, my_li);
}

// ---- one sector, stage by stage: the reference's serial walk as written, on the one lane that calls it ----
// For a sector at a cloud end whose stale {0, 0} smoothness entries do not reduce to sector_parallel's case. smooth[ep] is outside the sorted
// range but inside both loops (cand_at). Reads sector j's sorted keys and, through walk_get, picked / curvature / column; writes label, picked,
// A.corner_stage / corner_cnt. No barrier: the caller's follows.
template <int MAXH>
ROLO_DEV void sector_serial(const RingWin<MAXH>& W, const FeatArgs& A, int j, Sector sec, const unsigned long long* skeys) {
  // corners: featureExtraction.cpp:181-211
  int largestPickedNum = 0, ncorner = 0;
  for (int k = sec.ep; k >= sec.sp; k--) {
    const int ind = cand_at(W, skeys, sec, k).ind;
    if (walk_get(W, W.l_picked, A.picked, ind) == 0 && walk_get(W, W.l_curv, A.curv, ind) > A.edge_threshold) {
      largestPickedNum++;
      if (largestPickedNum <= 20) {
        walk_set(W, W.l_label, A.label, ind, 1);
        A.corner_stage[(W.ring * 6 + j) * 20 + ncorner] = A.extracted[ind];
        ncorner++;
      } else break;
      walk_marks(W, A, ind);
    }
  }
  A.corner_cnt[W.ring * 6 + j] = ncorner;
  // surfaces: :213-238
  for (int k = sec.sp; k <= sec.ep; k++) {
    const int ind = cand_at(W, skeys, sec, k).ind;
    if (walk_get(W, W.l_picked, A.picked, ind) == 0 && walk_get(W, W.l_curv, A.curv, ind) < A.surf_threshold) {
      walk_set(W, W.l_label, A.label, ind, -1);
      walk_marks(W, A, ind);
    }
  }
}

// Writes the ring's picked / label window back (the oracle's arrays after extraction). Reads l_picked, l_label; writes A.picked, A.label.
// Ends on a barrier — the one that also makes the surface scan's last stores to list visible.
template <int MAXH>
ROLO_DEV void write_back(const RingWin<MAXH>& W, const FeatArgs& A) {
  for (int i = threadIdx.x; i < W.wlen; i += XT) {
    const int gi = W.w0 + i;
    if (gi >= W.s - 10 && gi <= W.e + 10 && gi >= -FRONT_GUARD && gi < W.n + FRONT_GUARD) {
      if (W.l_picked[i]) A.picked[gi] = 1;
      if (gi >= W.s && gi <= W.e) A.label[gi] = W.l_label[i];
      else if (W.l_label[i] != 0) A.label[gi] = W.l_label[i];
    }
  }
  __syncthreads();
}

// ---- pcl::VoxelGrid on the ring's surface scan (featureExtraction.cpp:254-258) ----
// Reads list[0, m) and A.extracted; keys is free by now and takes the (cell << 32 | order) keys. Writes A.surf_stage's row of the ring and A.surf_cnt.
// Returns early, uniformly, on an empty scan and on PCL's overflow pass-through; nothing follows it in the kernel. XT_STAMP 4 .. 6 are inside.
template <int MAXH>
ROLO_DEV void voxel_grid(const RingWin<MAXH>& W, const FeatArgs& A, int m) {
  __shared__ int s_heads;
  __shared__ float s_red[2][3][XW];
  __shared__ int s_wsum[XW];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, ring = W.ring;
  unsigned long long* keys = W.keys;
  const int* list = W.list;
  if (m == 0) { if (t == 0) A.surf_cnt[ring] = 0; return; }
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (int i = t; i < m; i += XT) {
    const float4 p = A.extracted[list[i]];
    mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
    mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
  }
#pragma unroll
  for (int d = 0; d < 3; d++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { mn[d] = fminf(mn[d], __shfl_xor(mn[d], off, 64)); mx[d] = fmaxf(mx[d], __shfl_xor(mx[d], off, 64)); }
    if (lane == 0) { s_red[0][d][wv] = mn[d]; s_red[1][d][wv] = mx[d]; }
  }
  __syncthreads();
#pragma unroll
  for (int d = 0; d < 3; d++) {
    float lo = s_red[0][d][0], hi = s_red[1][d][0];
#pragma unroll
    for (int w = 1; w < XW; w++) { lo = fminf(lo, s_red[0][d][w]); hi = fmaxf(hi, s_red[1][d][w]); }
    mn[d] = lo; mx[d] = hi;
  }
  const float inv = 1.0f / A.leaf;
  const long long dx = (long long)((mx[0] - mn[0]) * inv) + 1, dy = (long long)((mx[1] - mn[1]) * inv) + 1, dz = (long long)((mx[2] - mn[2]) * inv) + 1;
  float4* out = A.surf_stage + (size_t)ring * MAXH;
  if (dx * dy * dz > (long long)INT_MAX) {  // PCL: warn and copy the input through
    for (int i = t; i < m; i += XT) out[i] = A.extracted[list[i]];
    if (t == 0) A.surf_cnt[ring] = m;
    return;
  }
  const int min_b0 = (int)floorf(mn[0] * inv), min_b1 = (int)floorf(mn[1] * inv), min_b2 = (int)floorf(mn[2] * inv);
  const int div_b0 = (int)floorf(mx[0] * inv) - min_b0 + 1, div_b1 = (int)floorf(mx[1] * inv) - min_b1 + 1;
  int np2 = 2; while (np2 < m) np2 <<= 1;
  for (int i = t; i < np2; i += XT) {
    unsigned long long kv = ~0ull;
    if (i < m) {
      const float4 p = A.extracted[list[i]];
      const int ijk0 = (int)floorf(p.x * inv) - min_b0, ijk1 = (int)floorf(p.y * inv) - min_b1, ijk2 = (int)floorf(p.z * inv) - min_b2;
      const int cell = ijk0 + ijk1 * div_b0 + ijk2 * div_b0 * div_b1;
      kv = ((unsigned long long)(unsigned)cell << 32) | (unsigned)i;
    }
    keys[i] = kv;
  }
  __syncthreads();
  XT_STAMP(4);
  bitonic_sort_lds<XT>(keys, np2);  // std::sort by cell index, ties by point order
  XT_STAMP(5);
  // run heads -> output slot; each head accumulates its run in order with float accumulators (pcl::CentroidPoint)
  if (t == 0) s_heads = 0;
  __syncthreads();
  for (int base = 0; base < m; base += XT) {
    const int i = base + t;
    const bool head = i < m && (i == 0 || (keys[i] >> 32) != (keys[i - 1] >> 32));
    int inc = head ? 1 : 0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { int o = __shfl_up(inc, off, 64); if (lane >= off) inc += o; }
    if (lane == 63) s_wsum[wv] = inc;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wv; w++) woff += s_wsum[w];
    const int c = s_heads;
    if (head) {
      const unsigned cell = (unsigned)(keys[i] >> 32);
      float sx = 0, sy = 0, sz = 0, si = 0;
      int cnt = 0;
      for (int r = i; r < m && (unsigned)(keys[r] >> 32) == cell; r++) {
        const float4 p = A.extracted[list[(int)(unsigned)(keys[r] & 0xffffffffull)]];
        sx += p.x; sy += p.y; sz += p.z; si += p.w; cnt++;
      }
      const float fc = (float)cnt;
      out[c + woff + inc - 1] = make_float4(sx / fc, sy / fc, sz / fc, si / fc);
    }
    __syncthreads();
    if (t == XT - 1) s_heads = c + woff + inc;
    __syncthreads();
  }
  XT_STAMP(6);
  if (t == 0) A.surf_cnt[ring] = s_heads;
}

// ---- the kernel: MAXH <= FRONT_MAX_H with the working set in dynamic LDS, or GLOBAL in the ring's scratch area (A.big) ----
template <int MAXH, bool GLOBAL>
__global__ __launch_bounds__(XT) void extract_kernel(FeatArgs A) {
  extern __shared__ unsigned char smem_lds[];
  XT_STAMP(0);
  const RingWin<MAXH> W(GLOBAL ? A.big + (size_t)blockIdx.x * front_ring_bytes(MAXH) : smem_lds, A);
  const int t = threadIdx.x;
  load_window(W, A);
  break_reach(W);
  const int seg = sector_keys(W);
  XT_STAMP(1);
  bitonic_sort_lds_seg<XT>(W.keys, 6 * seg, seg);   // std::sort(begin+sp, begin+ep) with the (value, ind) tie order
  XT_STAMP(2);
  ScanCursor sc{0, 0};
  int path = ring_picks(W, A, seg, sc);   // uniform, as is every branch below that sets it
  if (path != ROLO_XPATH_RING_APPLIED)
  for (int j = 0; j < 6; j++) {
    const Sector sec = sector_bounds(W.s, W.e, j);
    if (sec.sp >= sec.ep) { if (t == 0) A.corner_cnt[W.ring * 6 + j] = 0; path |= ROLO_XPATH_SECTOR_EMPTY << (2 + 2 * j); continue; }  // uniform
    // Sectors at the two ends of the cloud hold the reference's stale {0, 0} smoothness entries: entries that all name POINT 0,
    // with curvature 0. With sane thresholds (0 is a surface candidate, not a corner) they amount to "point 0 is the best-ranked surface
    // candidate": in the sector that holds point 0 the parallel picks handle that as it stands (the duplicates fold onto one window
    // cell); in the last sector of the cloud point 0 was picked long ago — the ring that holds it ran first in the reference — so the
    // entries do nothing and are skipped. Anything odder (tiny clouds, both ends in one sector, thresholds that flip the argument) takes the
    // serial walk as written. (Both end sectors on the serial walk: 155 us of this kernel's 170 on the OS1-128 frame.) Twin: ring_picks' head / tail
    // conditions — the same two tests on the RING's first and last sector, under its stricter threshold rule; kept apart, they differ in every operand.
    const bool head_sp = sec.sp < 5, tail_sp = sec.ep >= W.n - 5;
    const bool thr_ok = A.surf_threshold > 0.f && A.edge_threshold >= 0.f;
    const bool head_ok = !head_sp || (thr_ok && !tail_sp && sec.ep >= 5 && W.w0 <= 0 && -W.w0 < W.wlen);
    const bool tail_ok = !tail_sp || (thr_ok && !head_sp && W.n >= 64 && A.start_ring[0] == 4 && A.end_ring[0] >= 30);   // ring 0 starts at 0 - 1 + 5 and its stale entry marked point 0
    const bool parallel = head_ok && tail_ok && sec.ep - sec.sp < RingWin<MAXH>::SEGMAX;
    path |= (parallel ? ROLO_XPATH_SECTOR_PARALLEL : ROLO_XPATH_SECTOR_SERIAL) << (2 + 2 * j);
    if (parallel) sector_parallel(W, A, j, sec, W.keys + j * seg);
    else if (t == 0) sector_serial(W, A, j, sec, W.keys + j * seg);
    __syncthreads();
    scan_append(W, sec.sp, sec.ep, sc);
  }
  XT_STAMP(3);
  if (t == 0) A.paths[W.ring] = path;
  write_back(W, A);
  voxel_grid(W, A, sc.cnt);
}

}  // namespace
}  // namespace rolo
