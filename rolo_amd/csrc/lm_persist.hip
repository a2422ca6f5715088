// The resident LM kernel (rolo_params::fused_lm = 2, the default): a frame's whole LM chain — both stages — as ONE launch. Split from passes.hip, whose file comment
// describes the iteration; what a pass does to a point is lm_point.hpp, the scalar step lm_step.hpp, shared with the other two launch forms there.
#include "rolo_internal.hpp"
#include "switches.hpp"
#include <atomic>
#include "lm_point.hpp"
#include "lm_step.hpp"
#include "peer_dev.hpp"
#include <cstddef>

namespace rolo {
namespace {

// ---- ONE launch per frame: the resident LM kernel (round 6; rolo_params::fused_lm = 2) --------------------------------------------------------------------
// A frame's LM chain is ~30 trials = ~60 launches of pass + controller: 60 kernel boundaries, each a dispatch, a cold first fetch and an L2 write-back / invalidate
// that every OTHER kernel on the chip feels (profiles/r06/concurrency.md). Here the whole chain — both stages — is one launch of G <= 128 workgroups that stay
// resident: per trial every workgroup evaluates the pass over ITS points (the same thread owns the same points in every trial, so the correspondence cache never
// crosses a workgroup), leaves its row of 1 / 12 / 30 sums in an exchange buffer as self-validating words {epoch : 32 | half a double : 32} — agent-scope relaxed
// atomic stores, the protocol of the multi-GPU peer exchange (peer_dev.hpp) between workgroups instead of ranks — polls everybody's rows (agent-scope loads: they
// miss the XCD's L2), adds them in row order (the same bits in every workgroup) and runs the scalar LM step on its own copy of the state in LDS. No fence, no
// barrier object, no atomic read-modify-write: nothing but the words crosses. Rows are double-buffered by the epoch's parity (a workgroup can be at most one
// exchange ahead of another); the epoch continues from launch to launch through the buffer's header, so a stale word never matches.
// A poll that lasts longer than timeout_ticks (wall clock, 100 MHz) gives up: the stage ends with ROLO_ECOMM in the state — a workgroup that never became
// resident costs a bounded wait, never a hung GPU. Co-residency: G x THREADS threads with ~30 KB of LDS per workgroup fit the chip several times over (256 CUs),
// and every kernel that can occupy the slots in the meantime terminates by itself.
// ADMISSION. Spinning workgroups never give their slots back, so two resident kernels that each got only part of their workgroups onto the chip — two processes sharing
// the GPU, more contexts in flight than the sizing assumed — would wait for each other forever. Before the first trial the workgroups therefore exchange one EMPTY row under
// a short timeout (admit_ticks, default 1 ms: longer than any kernel of this library that may hold the slots in the meantime): if every row arrives, all G workgroups are
// resident and will stay so; if not, the workgroup that ran out of time raises the bail word of this launch, everybody — whoever is polling now, whoever becomes resident
// later — sees it and leaves, the LM state is untouched (LmState::lmp_bailed = 1 apart), and the host finishes the frame with pass + controller launches. A lost race costs
// the admission time, never a hung GPU and never an error.
constexpr int LMP_HDR = 8;   // words in front of the rows: [0] = last epoch used, [2] = bail word (the admission epoch of the launch that gave up)
#ifdef ROLO_LMP_STATS
// the phases of a trial as workgroup 0 sees them (wall clock, 100 MHz ticks, summed): [0] pass body + block reduction, [1] exchange (publish, poll, row sums), [2] the scalar step, [7] trials
__device__ unsigned long long g_lmp_t[8];
__device__ unsigned long long g_lmp_adm[4];   // admission as workgroup 0 sees it: [0] ticks from its start to everybody admitted, [1] launches, [2] the longest one, [3] ticks from its start to the kernel's end
extern "C" int rolo_debug_lmp_admission(unsigned long long* out4, int reset) {
  if (hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_lmp_adm), sizeof(unsigned long long) * 4) != hipSuccess) return -1;
  if (reset) { unsigned long long z[4] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_lmp_adm), z, sizeof(z)) != hipSuccess) return -1; }
  return 0;
}
extern "C" int rolo_debug_lmp_times(unsigned long long* out8, int reset) {
  (void)hipDeviceSynchronize();
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_lmp_t), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
  if (reset) { unsigned long long z[8] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_lmp_t), z, sizeof(z)) != hipSuccess) return -1; }
  return 0;
}
#define LMP_STAMP(k) const long long lt##k = wall_clock64()
#define LMP_ACC() do { if (wg == 0 && t == 0) { const long long lt3 = wall_clock64(); atomicAdd(&g_lmp_t[0], (unsigned long long)(lt1 - lt0)); atomicAdd(&g_lmp_t[1], (unsigned long long)(lt2 - lt1)); \
                       atomicAdd(&g_lmp_t[2], (unsigned long long)(lt3 - lt2)); atomicAdd(&g_lmp_t[7], 1ull); \
                       if (only_first) { atomicAdd(&g_lmp_t[3], (unsigned long long)(lt1 - lt0)); atomicAdd(&g_lmp_t[4], (unsigned long long)(lt2 - lt1)); \
                                         atomicAdd(&g_lmp_t[5], (unsigned long long)(lt3 - lt2)); atomicAdd(&g_lmp_t[6], 1ull); } } } while (0)   /* [3..6]: the cost-only trials among them */
#else
#define LMP_STAMP(k)
#define LMP_ACC()
#endif
// the scalar step as a CALL: one lane runs ~700 dependent instructions with its own register needs (the LDLT's factors) — inlined into the resident kernel's loop they
// were live across the pass bodies and spilled (620 bytes of scratch per lane)
// (state and sums live in LDS: the round trip through an address_space(3) pointer tells the compiler so — a call boundary hides it, and generic pointers would make every
// one of the step's ~150 state accesses a flat instruction)
// (round 6, second form: state and sums are FILE-scope LDS variables, so that the step — a function of its own — names them directly: every access is a ds_ instruction
// with a constant address. As pointer arguments they arrived generic, and the cast back to LDS cost a null check of three instructions per access — ~1 300 of the
// step's 4 300 instructions, all issued by one lane at four cycles each)
__shared__ LmState lmp_sst;
__shared__ double lmp_sums[NV_MAX];
// (a trial's trace record goes to an LDS slot: written to the buffer by the stepping lane, the store's acknowledgement — the function returns behind s_waitcnt vmcnt(0) — was
// ~0.4 us of workgroup 0's step, for which all the others then wait in the next exchange)
__shared__ rolo_trace_rec lmp_trace_slot;
template <int DOF> __device__ __noinline__ void lmp_rot_step(bool want_trace) { rot_step_t<DOF, true>(&lmp_sst, lmp_sums, want_trace ? &lmp_trace_slot : nullptr); }
__device__ __noinline__ void lmp_trans_step(rolo_trace_rec* trace_g) { trans_step<true>(&lmp_sst, lmp_sums, trace_g ? &lmp_trace_slot : nullptr, trace_g); }
// after the barrier behind a step: the last wavefront of workgroup 0 copies the record the step left (if it left one) — plain stores nobody waits for before the kernel ends
// RUN = false (the translation stage): the slot's record alone — a step that answered further trials from the model wrote their records itself (trans_step)
template <int THREADS, bool RUN = true>
ROLO_DEV void lmp_trace_flush(rolo_trace_rec* __restrict__ trace, int count_before) {
  static_assert(sizeof(rolo_trace_rec) % sizeof(int) == 0, "record copied in dwords");
  constexpr int NWORD = sizeof(rolo_trace_rec) / sizeof(int);
  const int t = (int)threadIdx.x - (THREADS - 64);
  if (t < 0 || t >= NWORD) return;
  // a step leaves one record, or none — or, where it answered the repeats of a converged-but-rejected trial from the kept cost (rot_step_t), that trial's record and a
  // count that advanced once per repeat: repeat j is the slot's record with outer + j and trial = 0 (trace_push_repeat). Beyond TRACE_CAP only the count advances.
  static_assert(offsetof(rolo_trace_rec, outer) == 4 && offsetof(rolo_trace_rec, trial) == 8, "the counter fields of a repeated record");
  const int n = RUN ? min(lmp_sst.trace_count, TRACE_CAP) - count_before : min(min(lmp_sst.trace_count, TRACE_CAP) - count_before, 1);
  const int w = reinterpret_cast<const int*>(&lmp_trace_slot)[t];
  for (int j = 0; j < n; j++) reinterpret_cast<int*>(trace + count_before + j)[t] = (j == 0 || t > 2 || t == 0) ? w : (t == 1 ? w + j : 0);
}

// publish row[0 .. nv) as words of epoch e, collect all G rows, add them in a fixed order into sums[] (V_* slots). Returns false if a row did not arrive in time.
#ifndef ROLO_LMP_SPIN_PRIO
#define ROLO_LMP_SPIN_PRIO 1   // issue priority while a workgroup polls the others' rows (A/B: 0 = the spinning wavefronts step back behind everything else on their SIMD)
#endif
#ifndef ROLO_LMP_SPIN_SLEEP
#define ROLO_LMP_SPIN_SLEEP 1  // s_sleep argument between two polls of a missing word (x 64 clocks)
#endif
template <int THREADS, bool ADMIT = false>
ROLO_DEV bool lmp_exchange(const double* __restrict__ row, int nv, int nh, unsigned e, unsigned long long* __restrict__ xbuf, int G, int wg, unsigned* __restrict__ xw,
                           double (*part)[NV_MAX], double* __restrict__ sums, int* __restrict__ bad, unsigned long long timeout_ticks) {
  const int t = (int)threadIdx.x;
  unsigned long long* rows = xbuf + LMP_HDR + (size_t)(e & 1u) * G * PEER_SLOT_WORDS;
  const int nw = 2 * nv;
  if (t < nw) {
    const double v = row[t >> 1];
    const unsigned half = (t & 1) ? (unsigned)__double2hiint(v) : (unsigned)__double2loint(v);
    __hip_atomic_store(rows + (size_t)wg * PEER_SLOT_WORDS + t, ((unsigned long long)e << 32) | half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const int total = G * nw;
  const long long t0 = wall_clock64();
  if (ROLO_LMP_SPIN_PRIO != ROLO_SHORT_PRIO) __builtin_amdgcn_s_setprio(ROLO_LMP_SPIN_PRIO);
  for (int base = t; base < total; base += THREADS * 4) {
    unsigned long long x[4]; const unsigned long long* q[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = min(base + u * THREADS, total - 1);
      const int r = i / nw, w = i - r * nw;
      q[u] = rows + (size_t)r * PEER_SLOT_WORDS + w;
      x[u] = __hip_atomic_load(q[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = base + u * THREADS;
      if (i >= total) continue;
      while ((unsigned)(x[u] >> 32) != e) {
        if ((unsigned long long)(wall_clock64() - t0) > timeout_ticks) {
          *bad = 1;
          if (ADMIT) __hip_atomic_store(xbuf + 2, (unsigned long long)e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // this launch gives up: tell everybody
          break;
        }
        if (ADMIT && (unsigned)__hip_atomic_load(xbuf + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == e) { *bad = 1; break; }   // somebody gave up
        __builtin_amdgcn_s_sleep(ADMIT ? 8 : ROLO_LMP_SPIN_SLEEP);
        x[u] = __hip_atomic_load(q[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      xw[i] = (unsigned)x[u];
    }
  }
  if (ROLO_LMP_SPIN_PRIO != ROLO_SHORT_PRIO) __builtin_amdgcn_s_setprio(ROLO_SHORT_PRIO);
  if (ADMIT && t == 0 && (unsigned)__hip_atomic_load(xbuf + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == e) *bad = 1;   // (a workgroup that found every row may still be the last to hear)
  __syncthreads();
  if (*bad) return false;
  if (ADMIT) return true;
  {   // row sums in a fixed order (16 groups of rows, then the groups): the same bits in every workgroup
    const int v = t & 31;
    for (int q = t >> 5; q < 16; q += THREADS / 32) {
      double s0 = 0.0;
      if (v < nv) for (int r = q; r < G; r += 16) s0 += __hiloint2double((int)xw[r * nw + 2 * v + 1], (int)xw[r * nw + 2 * v]);
      part[q][v] = s0;
    }
  }
  __syncthreads();
  if (t < nv) {
    double s1 = 0.0;
#pragma unroll
    for (int k = 0; k < 16; k++) s1 += part[k][t];
    sums[row_slot(t, nh)] = s1;
  }
  __syncthreads();
  return true;
}

// The pass bodies of the resident kernel: PPT points per thread, INTERLEAVED — all the record fetches of half (A) first, the first hash probes of half (B) behind them,
// then (A)'s arithmetic while the probes are in flight, (B)'s record fetches, (B)'s arithmetic: a trial costs two dependent round trips whatever PPT is, where a loop over
// the points costs two per point (one launch per trial with 2 / 4 / 8 points per thread: +70 us of frame latency per doubling, DEAD_ENDS rounds 2-3). A thread owns the same
// points in every trial, so the float coordinates, the covariance (as m) and BOTH correspondence ids of a point stay in registers for the whole chain; the ids are still
// written to corr[] — the getters and a later rolo_compute_translation read them there.
struct PtReg { float x, y, z; Vec3 m; };   // m.x is NaN for a point whose covariance is not of the plane form (or when the pass has no m at all): six entries from memory
template <int PPT>
ROLO_DEV void lmp_load_points(const PassArgs& a, int i0, int threads, PtReg (&pt)[PPT], int (&cid)[PPT][2], bool (&valid)[PPT]) {
  const size_t pitch = (size_t)a.n_total;
#pragma unroll
  for (int p = 0; p < PPT; p++) {
    const int i = i0 + p * threads;
    valid[p] = i < a.end;
    pt[p] = PtReg{0.f, 0.f, 0.f, Vec3{__builtin_nan(""), 0.0, 0.0}};
    cid[p][0] = cid[p][1] = -1;
    if (valid[p]) {
      const float4 pf = a.src[i];
      pt[p].x = pf.x; pt[p].y = pf.y; pt[p].z = pf.z;
      if (a.nrm) pt[p].m = Vec3{a.nrm[i], a.nrm[pitch + i], a.nrm[2 * pitch + i]};
      if (a.n_off == 1) { cid[p][0] = a.corr[0][i]; cid[p][1] = a.corr[1][i]; }
    }
  }
}
ROLO_DEV Sym3 lmp_rotated_cov(const PassArgs& a, const double* R, const double* __restrict__ S6, const PtReg& q, int i) {
  if (q.m.x == q.m.x) return rotated_plane_cov(R, S6, q.m);
  const size_t pitch = (size_t)a.n_total;
  return sym3_rotate(R, Sym3{a.cov[i], a.cov[pitch + i], a.cov[2 * pitch + i], a.cov[3 * pitch + i], a.cov[4 * pitch + i], a.cov[5 * pitch + i]});
}
// The reference's per-correspondence Mahalanobis cache (rot_vgicp_impl.hpp:204-222: update_correspondences leaves M = (C_B + R C_A R^T)^-1 of the linearisation point with
// every correspondence, compute_error reads it) — in LDS: mc[k * ms + slot], k = the six entries, slot = this thread's p-th point; a thread only ever touches its own slots.
// The (B) half writes it, the (A) half of the trials that follow reads it (m_hit: wave-uniform, lm_persist_kernel) instead of fetching the voxel covariance, rotating C_A and
// inverting again: a cost-only trial is 26 instead of ~100 fp64 instructions per point. As global memory this cache LOST (48 B written + read per point and pass: DEAD_ENDS
// round 5, entry 1); the resident kernel keeps a thread's points for the whole chain, so it costs no traffic here.
typedef __attribute__((address_space(3))) double lds_f64;
ROLO_DEV void mc_store(lds_f64* mc, int ms, int slot, const Sym3& M) {
  mc[slot] = M.xx; mc[ms + slot] = M.xy; mc[2 * ms + slot] = M.xz; mc[3 * ms + slot] = M.yy; mc[4 * ms + slot] = M.yz; mc[5 * ms + slot] = M.zz;
}
ROLO_DEV Sym3 mc_load(const lds_f64* mc, int ms, int slot) { return Sym3{mc[slot], mc[ms + slot], mc[2 * ms + slot], mc[3 * ms + slot], mc[4 * ms + slot], mc[5 * ms + slot]}; }
struct RecMW { Vec3 mean; double w; };
ROLO_DEV RecMW load_rec_mw(const double* __restrict__ rec, int id) {
  const double* r = rec + (size_t)id * REC_DOUBLES;
  return RecMW{Vec3{r[0], r[1], r[2]}, r[9]};
}
// M of every point of this thread for the pose (R, S6 = R R^T) and the correspondences of buffer `buf`, one point after the other: what a (B) half would have left, had
// it not been overwritten by a rejected trial's speculation (once per rejection), and the translation stage's constant matrices (once per stage)
template <int NP>
ROLO_DEV void lmp_fill_cache(const PassArgs& a, const double* R9, const double* S6, int buf, int i0, int threads, const PtReg* pt, const int (*cid)[2], const bool* valid,
                             lds_f64* mc, int ms, int slot0) {
  double R[9];
#pragma unroll
  for (int k = 0; k < 9; k++) R[k] = uni(R9[k]);
#pragma unroll
  for (int p = 0; p < NP; p++) {
    const int v = buf ? cid[p][1] : cid[p][0];
    if (valid[p] && v >= 0) {
      const double* r = a.tab.rec + (size_t)v * REC_DOUBLES;
      const Sym3 cb{r[3], r[4], r[5], r[6], r[7], r[8]};
      mc_store(mc, ms, slot0 + p * threads, sym3_inverse(sym3_add(cb, lmp_rotated_cov(a, R, S6, pt[p], i0 + p * threads))));
    }
    asm volatile("" ::: "memory"); __builtin_amdgcn_sched_barrier(0);
  }
}
template <int DOF, int PPT, bool MC>
ROLO_DEV void lmp_rot_body(const PassArgs& a, const LmState* __restrict__ st, int i0, int threads, const PtReg* pt, int (*cid)[2], const bool* valid,
                           double (&acc)[3 + DOF * (DOF + 1) / 2 + DOF], lds_f64* mc, int ms, int slot0) {
  const RotUni u(st);
  const int phase = u.phase, cur = u.cur;
  const bool skip_lin = u.skip_lin;
  const int newb = phase == 0 ? cur : (cur ^ 1);
  Vec3 tp[PPT];
#pragma unroll
  for (int p = 0; p < PPT; p++) tp[p] = u.at_trial(Vec3{(double)pt[p].x, (double)pt[p].y, (double)pt[p].z});
  // (A) compute_error(xi): the records of the cached correspondences — their ids are in registers, so these fetches depend on nothing this trial computed
  // (with the cache — mc, filled for x0 by whoever ran before: lm_persist_kernel — only the mean and the weight of a record are fetched here)
  Rec ra[PPT]; bool ha[PPT];
#pragma unroll
  for (int p = 0; p < PPT; p++) {
    const int v = cur ? cid[p][1] : cid[p][0];
    ha[p] = phase == 1 && valid[p] && v >= 0;
    if (ha[p]) {
      if (MC) { const RecMW l = load_rec_mw(a.tab.rec, v); ra[p].mean = l.mean; ra[p].w = l.w; }
      else ra[p] = load_rec(a.tab.rec, v);
    }
  }
  // (B) first probe of every point's voxel
  unsigned long long key[PPT]; unsigned h[PPT]; ulonglong2 sl[PPT]; bool ok[PPT];
  if (!skip_lin) {
#pragma unroll
    for (int p = 0; p < PPT; p++) {
      int kx, ky, kz;
      voxel_coord_dev(a.tab, tp[p].x, tp[p].y, tp[p].z, kx, ky, kz);
      ok[p] = valid[p] && pack_key(kx, ky, kz, key[p]);
      h[p] = hash_key(key[p]) & a.tab.mask;
      if (ok[p]) sl[p] = *reinterpret_cast<const ulonglong2*>(a.tab.keys + 2 * (size_t)h[p]);
    }
  }
#pragma unroll
  for (int p = 0; p < PPT; p++) {
    if (ha[p]) {
      Sym3 M;
      if constexpr (MC) M = mc_load(mc, ms, slot0 + p * threads);
      else M = sym3_inverse(sym3_add(ra[p].cov, lmp_rotated_cov(a, u.R0, st->x0_S, pt[p], i0 + p * threads)));
      rot_cost_term(acc, ra[p].mean, ra[p].w, M, tp[p]);
    }
    if (PPT > 1 && !MC) __builtin_amdgcn_sched_barrier(0);   // the FETCHES of the points are batched, their arithmetic is not: interleaved, four inverses' temporaries are 250 registers
  }
  if (skip_lin) return;
  int vid[PPT];
  int* __restrict__ corr_new = a.corr[newb];
#pragma unroll
  for (int p = 0; p < PPT; p++) {
    vid[p] = -1;
    if (ok[p]) {
      while (true) {   // (the table is at most half full: the first probe answers almost always)
        if (sl[p].x == key[p]) { vid[p] = (int)(unsigned)sl[p].y; break; }
        if (sl[p].x == KEY_EMPTY) break;
        h[p] = (h[p] + 1) & a.tab.mask;
        sl[p] = *reinterpret_cast<const ulonglong2*>(a.tab.keys + 2 * (size_t)h[p]);
      }
    }
    if (newb) cid[p][1] = vid[p]; else cid[p][0] = vid[p];
    if (valid[p]) corr_new[i0 + p * threads] = vid[p];
  }
  Rec rb[PPT];
#pragma unroll
  for (int p = 0; p < PPT; p++) if (vid[p] >= 0) rb[p] = load_rec(a.tab.rec, vid[p]);
#pragma unroll
  for (int p = 0; p < PPT; p++) {
    if (vid[p] >= 0) {
      const Sym3 M = sym3_inverse(sym3_add(rb[p].cov, lmp_rotated_cov(a, u.R1, st->xt_S, pt[p], i0 + p * threads)));
      if (MC) mc_store(mc, ms, slot0 + p * threads, M);
      rot_lin_term<DOF>(acc, rb[p].mean, rb[p].w, M, tp[p]);
    }
    if (PPT > 1) __builtin_amdgcn_sched_barrier(0);
  }
}
template <int PPT, bool MC>
ROLO_DEV void lmp_trans_body(const PassArgs& a, const LmState* __restrict__ st, int i0, int threads, const PtReg* pt, const int (*cid)[2], const bool* valid, double (&acc)[30],
                             lds_f64* mc, int ms, int slot0) {
  const TransUni u(st);
  Rec r[PPT]; bool has[PPT];
#pragma unroll
  for (int p = 0; p < PPT; p++) {
    const int v = u.tr_cur ? cid[p][1] : cid[p][0];
    has[p] = valid[p] && v >= 0;
    if (has[p]) {
      if (MC) { const RecMW l = load_rec_mw(a.tab.rec, v); r[p].mean = l.mean; r[p].w = l.w; }
      else r[p] = load_rec(a.tab.rec, v);
    }
  }
#pragma unroll
  for (int p = 0; p < PPT; p++) {
    if (!has[p]) continue;
    const TransPt q(u, Vec3{(double)pt[p].x, (double)pt[p].y, (double)pt[p].z});
    // (the stage's Mahalanobis matrices are those of the LAST rotation linearisation: constant over all its passes — lm_persist_kernel fills the cache once)
    Sym3 M;
    if constexpr (MC) M = mc_load(mc, ms, slot0 + p * threads);
    else M = sym3_inverse(sym3_add(r[p].cov, lmp_rotated_cov(a, u.R, st->tr_S, pt[p], i0 + p * threads)));
    trans_term(acc, u, q, r[p].mean, r[p].w, M);
    if (u.skip_lin) continue;   // (a cost-only trial's points go without the barrier, as they always did)
    if (PPT > 1) __builtin_amdgcn_sched_barrier(0);
  }
}

// PPT > 0: the interleaved bodies above (DIRECT1 only: one correspondence per point); PPT = 0: any number of points per thread and any neighbour search, one point after the other
// BATCH = points of a thread that go through a body together (interleaved); OCC = wavefronts per SIMD the register budget must allow (2: 256 registers, 4: 128 — then a
// walk's wavefronts fit on the same SIMDs and use the issue slots the resident kernel leaves idle while it exchanges and steps)
// MC: the Mahalanobis cache of lmp_rot_body in LDS (the interleaved bodies only)
template <int DOF, int THREADS, int PPT, int BATCH = (PPT > 0 ? PPT : 1), int OCC = 2, bool MC = (PPT > 0)>
__global__ __launch_bounds__(THREADS, OCC) void lm_persist_kernel(PassArgs a, LmState* st_io, unsigned long long* __restrict__ xbuf, rolo_trace_rec* trace, int ppt, LmState* pub,
                                                                             unsigned long long timeout_ticks, unsigned long long admit_ticks, int max_trials) {
  LmState& sst = lmp_sst;
  double* const sums = lmp_sums;
  __shared__ double row[NV_MAX];
  __shared__ double part[16][NV_MAX];
  __shared__ int bad;
  extern __shared__ unsigned xw[];   // G x 60 halves
  constexpr int NW = LM_STATE_WORDS;
  constexpr int NHR = DOF * (DOF + 1) / 2, NVR = 3 + NHR + DOF;
  constexpr int NP = PPT > 0 ? PPT : 1;
  static_assert(THREADS == 512 || THREADS == 256, "16 summation groups of 32 values, dealt over the workgroup's 32-lane halves");
  const int G = (int)gridDim.x, wg = (int)blockIdx.x, t = (int)threadIdx.x;
  if (PPT > 0) ppt = PPT;
  ROLO_SHORT_KERNEL_PRIO();
#ifdef ROLO_LMP_STATS
  const long long lt_entry = wall_clock64();
#endif
  state_copy<THREADS>(&sst, st_io);
  unsigned e = (unsigned)xbuf[0];   // written by the previous launch on this context (a kernel boundary ago)
  if (t == 0) bad = 0;
  // XCD x (= wg mod 8: the dispatcher deals workgroups round-robin) owns a contiguous eighth of the point blocks — a sector of the cloud whose voxels no other XCD's
  // L2 has to hold (pass_xcd_block); and with no kernel boundary between the trials that L2 stays warm from the second trial on
  const int i0 = a.begin + pass_xcd_block(a, wg, G) * ppt * THREADS + t;
  PtReg pt[NP]; int cid[NP][2]; bool valid[NP];
  if (PPT > 0) lmp_load_points<NP>(a, i0, THREADS, pt, cid, valid);
  // the Mahalanobis cache (lmp_rot_body) behind the G rows of xw: 6 x THREADS x PPT doubles
  constexpr int MS = THREADS * NP;
  static_assert(!MC || PPT > 0, "the cache belongs to the interleaved bodies");
  lds_f64* mc = MC ? (lds_f64*)(__attribute__((address_space(3))) void*)(xw + (size_t)G * 60) : nullptr;
  bool m_valid = false;   // the cache holds M(x0) for the correspondences of buffer `cur` (rotation stage) / M(tr_R) for those of `tr_cur` (translation stage)
  __syncthreads();
  // admission (above): one empty row per workgroup under the short timeout
  if (t == 0) row[0] = 0.0;
  __syncthreads();
  if (admit_ticks == 0 /* test switch: nobody is admitted */ || !lmp_exchange<THREADS, true>(row, 1, 0, ++e, xbuf, G, wg, xw, part, sums, &bad, admit_ticks)) {
    // not everybody is resident: leave the stage to the host, exactly as it was (every leaving workgroup writes the same words)
    if (t == 0) {
      xbuf[0] = admit_ticks == 0 ? e + 1 : e;
      st_io->lmp_bailed = 1;
      if (pub) { int* h = reinterpret_cast<int*>(pub); const int* l = reinterpret_cast<const int*>(&sst); for (int w = 0; w < NW; w++) h[w] = l[w]; pub->lmp_bailed = 1; }
    }
    return;
  }
  if (t == 0) sst.lmp_bailed = 0;
#ifdef ROLO_LMP_STATS
  if (wg == 0 && t == 0) { const unsigned long long dta = (unsigned long long)(wall_clock64() - lt_entry); atomicAdd(&g_lmp_adm[0], dta); atomicAdd(&g_lmp_adm[1], 1ull); atomicMax(&g_lmp_adm[2], dta); }
#endif
  rolo_trace_rec* tr = wg == 0 ? trace : nullptr;   // without a buffer trace_count still advances
  int trial = 0;
  bool ok = true;
  bool cost_end = false;   // the last rotation trial was a cost-only one: the cache it read was written by lmp_fill_cache, as the translation stage's is
  // ---- rotation / 6-dof stage ----
  while (ok && uni(sst.stage) == 1) {
    const bool only_first = uni(sst.phase) == 1 && uni(sst.lin_skip) != 0;
    const int phase_in = uni(sst.phase), cur_in = uni(sst.cur), tc_in = uni(sst.trace_count);
    LMP_STAMP(0);
    if (MC && !m_valid && phase_in == 1) lmp_fill_cache<NP>(a, sst.x0_R, sst.x0_S, cur_in, i0, THREADS, pt, cid, valid, mc, MS, t);
    {
      double acc[NVR]; int slot[NVR];
#pragma unroll
      for (int v = 0; v < NVR; v++) { acc[v] = 0.0; slot[v] = v; }
      if (PPT > 0) {
#pragma unroll
        for (int p0 = 0; p0 < NP; p0 += BATCH) {
          lmp_rot_body<DOF, BATCH, MC>(a, &sst, i0 + p0 * THREADS, THREADS, pt + p0, cid + p0, valid + p0, acc, mc, MS, p0 * THREADS + t);
          if (BATCH < NP) { asm volatile("" ::: "memory"); __builtin_amdgcn_sched_barrier(0); }   // one batch after the other: left alone, the compiler interleaves them all (and spills)
        }
      }
      else pass_slabs<1, DOF, THREADS>(a, &sst, i0, ppt, acc);
      block_reduce_store<NVR, THREADS>(acc, slot, row, only_first);   // compact: yi, y, n, H lower triangle, b
    }
    __syncthreads();
    LMP_STAMP(1);
    ok = lmp_exchange<THREADS>(row, only_first ? 1 : NVR, NHR, ++e, xbuf, G, wg, xw, part, sums, &bad, timeout_ticks) && ++trial <= max_trials;
    LMP_STAMP(2);
    if (ok && t == 0) lmp_rot_step<DOF>(tr != nullptr);
    __syncthreads();
    if (ok && tr) lmp_trace_flush<THREADS>(tr, tc_in);
    // what the cache holds now (rot_step_t): a linearisation pass (phase 0) left M(x0); a trial WITH a (B) half overwrote it with M(xt) — M(x0) of the next trial exactly if
    // the step accepted and took the speculated linearisation (cur flipped); a cost-only trial only read it (if it was accepted, a phase-0 pass follows and writes)
    m_valid = phase_in == 0 || only_first || uni(sst.cur) != cur_in;
    cost_end = only_first;
    LMP_ACC();
  }
  // tr_R is the LAST linearisation point, not always x0: the first translation pass fills the cache — unless it holds those very matrices already. It holds M(x0) of buffer
  // `cur` when the last rotation trial left it so (above); that is M(tr_R) of buffer `tr_cur` exactly if tr_cur is cur and tr_R is x0, bit for bit (tr_S is then x0_S: both are
  // lm_set_rrt of the same matrix) — the stage ended on cost-only trials or on a kept cost, not on an accepted step that moved x0 past its linearisation. Only a cache
  // that lmp_fill_cache wrote is kept (cost_end), so that the matrices are those of the same code as the refill's, not a (B) half's.
  // (keep_cost = 0, the A/B: refilled always, as before the kept cost)
  if (m_valid) {
    bool same = cost_end && uni(sst.keep_cost) != 0 && uni(sst.tr_cur) == uni(sst.cur);
#pragma unroll
    for (int k = 0; k < 9; k++) same = same && __double_as_longlong(sst.tr_R[k]) == __double_as_longlong(sst.x0_R[k]);
    m_valid = same;
  }
  // ---- translation stage ----
  while (ok && uni(sst.stage) == 2) {
    const bool only_first = uni(sst.phase) == 1 && uni(sst.lin_skip) != 0;
    const int tc_in = uni(sst.trace_count);
    LMP_STAMP(0);
    if (MC && !m_valid) lmp_fill_cache<NP>(a, sst.tr_R, sst.tr_S, uni(sst.tr_cur), i0, THREADS, pt, cid, valid, mc, MS, t);
    {
      double acc[30]; int slot[30];
#pragma unroll
      for (int v = 0; v < 30; v++) { acc[v] = 0.0; slot[v] = v; }
      if (PPT > 0) {
#pragma unroll
        for (int p0 = 0; p0 < NP; p0 += BATCH) {
          lmp_trans_body<BATCH, MC>(a, &sst, i0 + p0 * THREADS, THREADS, pt + p0, cid + p0, valid + p0, acc, mc, MS, p0 * THREADS + t);
          if (BATCH < NP) { asm volatile("" ::: "memory"); __builtin_amdgcn_sched_barrier(0); }
        }
      }
      else pass_slabs<2, 6, THREADS>(a, &sst, i0, ppt, acc);
      block_reduce_store<30, THREADS>(acc, slot, row, only_first);
    }
    __syncthreads();
    LMP_STAMP(1);
    ok = lmp_exchange<THREADS>(row, only_first ? 1 : 30, 21, ++e, xbuf, G, wg, xw, part, sums, &bad, timeout_ticks) && ++trial <= max_trials;
    LMP_STAMP(2);
    if (ok && t == 0) lmp_trans_step(tr);
    __syncthreads();
    if (ok && tr) lmp_trace_flush<THREADS, false>(tr, tc_in);
    m_valid = true;
    LMP_ACC();
  }
  if (!ok) {   // a row never arrived (or the stages do not end): an error code instead of waiting forever
    if (t == 0) lm_fail_comm(&sst);
    __syncthreads();
  }
  if (wg == 0) {
    state_copy<THREADS>(st_io, &sst);
    if (pub) state_copy<THREADS>(pub, &sst);
    if (t == 0) xbuf[0] = e;   // the next launch's epochs continue here
#ifdef ROLO_LMP_STATS
    if (t == 0) atomicAdd(&g_lmp_adm[3], (unsigned long long)(wall_clock64() - lt_entry));
#endif
  }
}
}  // namespace

// the largest dynamic LDS a resident launch may take: the `fits` bound of lm_persist_form AND the limit lmp_launch raises the function attribute to. It must stay below a CU's
// 160 KiB minus the kernels' static LDS (the state, the summation rows: 10 328 B at 512 threads, 8 280 B at 256 — lmp_launch checks it before it raises the attribute)
constexpr size_t LMP_DYN_LDS_MAX = 148 * 1024;
constexpr size_t LMP_CU_LDS = 160 * 1024;
// one launch of an instantiation: dynamic LDS = the G rows of the exchange (+ the Mahalanobis cache); above 64 KB the function's limit is raised first — once per
// instantiation (KERN is a template argument: a static per kernel, not per signature) and per device of the process
template <auto KERN, typename... Args>
hipError_t lmp_launch(int nrows, int threads, size_t lds, hipStream_t s, Args... args) {
  if (lds > LMP_DYN_LDS_MAX) return hipErrorInvalidValue;
  if (lds > 64 * 1024) {
    static std::atomic<unsigned long long> raised{0};   // bit d: done on device d
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return hipGetLastError();
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(raised.load(std::memory_order_relaxed) & bit)) {
      hipFuncAttributes fa{};
      hipError_t e = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(KERN));
      if (e != hipSuccess) return e;
      if (fa.sharedSizeBytes + LMP_DYN_LDS_MAX > LMP_CU_LDS) return hipErrorInvalidConfiguration;   // the static LDS grew: LMP_DYN_LDS_MAX must shrink with it
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LMP_DYN_LDS_MAX);
      if (e != hipSuccess) return e;
      raised.fetch_or(bit, std::memory_order_relaxed);
    }
  }
  KERN<<<nrows, threads, lds, s>>>(args...);
  return hipGetLastError();
}
LmpForm lm_persist_form(int dof, int threads, int ppt, int n_off, int nrows) {
  // the interleaved bodies (1, 2 or 4 points per thread in registers) for the reference's own configuration — SO(3) optimiser, DIRECT1; everything else one point after the other
  const bool interleave = switches().lm_persist_interleave;
  // ROLO_LM_PERSIST_MCACHE=0 (A/B): no Mahalanobis cache in LDS — every trial inverts again, as the pass kernels do
  const int mcache_on = switches().lm_persist_mcache;
  // (builds for four wavefronts per SIMD — 128 registers, so that a walk's wavefronts could share the SIMDs — spill 85 / 159 / 270 registers at 1 / 2 / 4 points per thread and are
  // not instantiated: lm_persist_kernel<3, 512, PPT, 1, 4>, profiles/DEAD_ENDS.md round 6)
  const int batch4 = switches().lm_persist_batch;   // four points per thread go through the bodies in batches of 2 (default: 4 087 scans/s with four contexts, final kernels) / 1 (4 046: twice the dependent round trips and the same 6.6 us per linearising body — the bodies are bound by their fp64 issue at two wavefronts per SIMD, not by their fetches) / 4 (3 761: 144 spilled registers)
  LmpForm f;
  f.rows = nrows; f.threads = threads; f.ppt = ppt;
  f.sp = (interleave && dof == 3 && n_off == 1 && (ppt == 1 || ppt == 2 || ppt == 4)) ? ppt : 0;
  const size_t rows_lds = sizeof(unsigned) * (size_t)nrows * 60, cache_lds = sizeof(double) * 6 * (size_t)threads * f.sp;
  // (the A/B form exists for the headline's case; it is also the form of a launch whose rows + cache would not fit a CU's LDS: four points per thread AND more than 221
  // workgroups — a cloud of more than 452 608 points on an idle device — is 52 KB of rows + 96 KB of cache + 10 KB of state)
  const bool fits = rows_lds + cache_lds <= LMP_DYN_LDS_MAX;
  f.mcache = f.sp > 0 && !(f.sp == 4 && threads == 512 && (!mcache_on || !fits));
  f.lds = rows_lds + (f.mcache ? cache_lds : 0);
  // the form without the cache has batches of 2 whatever ROLO_LM_PERSIST_BATCH says (lm_persist_kernel<3, 512, 4, 2, 2, false>: the only one without it)
  f.batch = f.sp == 0 ? 1 : (f.sp != 4 ? f.sp : (threads == 256 || !f.mcache ? 2 : batch4));
  return f;
}
hipError_t launch_lm_persist(int dof, int threads, int ppt, const PassArgs& a, LmState* st, unsigned long long* xbuf, int nrows, rolo_trace_rec* trace, LmState* pub, unsigned long long timeout_ticks,
                             unsigned long long admit_ticks, int max_trials, hipStream_t s) {
  const LmpForm f = lm_persist_form(dof, threads, ppt, a.n_off, nrows);
  const size_t lds = f.lds;
#define LMP_GO(...) lmp_launch<&lm_persist_kernel<__VA_ARGS__>>(nrows, threads, lds, s, a, st, xbuf, trace, ppt, pub, timeout_ticks, admit_ticks, max_trials)
  // (A/B, ROLO_LM_PERSIST_BUSY_THREADS=256: 128 workgroups of 256 threads — one wavefront per SIMD at 256 registers, so that other kernels' wavefronts share the SIMDs
  // instead of finding 64 CUs closed: 3 353 / 3 339 against 3 639 / 3 635 scans/s, profiles/DEAD_ENDS.md round 6)
  if (threads == 256) return (dof == 3 && f.sp == 4 && f.mcache) ? LMP_GO(3, 256, 4, 2) : hipErrorInvalidValue;
  if (dof != 3) return LMP_GO(6, 512, 0);
  if (f.sp == 1) return LMP_GO(3, 512, 1);
  if (f.sp == 2) return LMP_GO(3, 512, 2);
  // (the cache-less form is picked before the batch: every other four-point form reads and writes the cache, which a launch without it has no LDS for)
  if (f.sp == 4 && !f.mcache) return LMP_GO(3, 512, 4, 2, 2, false);
  if (f.sp == 4 && f.batch == 1) return LMP_GO(3, 512, 4, 1);
  if (f.sp == 4 && f.batch == 2) return LMP_GO(3, 512, 4, 2);
  if (f.sp == 4) return LMP_GO(3, 512, 4);
  return LMP_GO(3, 512, 0);
#undef LMP_GO
}
size_t lm_persist_words(int nrows) { return (size_t)LMP_HDR + 2 * (size_t)nrows * PEER_SLOT_WORDS; }

}  // namespace rolo
