// K7-K12 — the Gauss-Newton / Levenberg-Marquardt iteration on gfx950.
// Replaces (reference include/rot_gicp/gicp/impl/rot_vgicp_impl.hpp) update_correspondences :173-222,
// so3_linearize :293-388, linearize :225-290, compute_error :391-417, t3_linearize :499-607, compute_t_error
// :610-658, and (lsq_registration_impl.hpp) the drivers rot_step_lm :273-324, step_lm :225-270, step_gn :208-222,
// step_t_optimize :84-139 with their convergence tests.
//
// MI355X design. One *fused pass* kernel per LM trial replaces the reference's separate linearize and error
// sweeps: for every source point it (A) re-evaluates the cost at the trial pose on the correspondences and
// Mahalanobis matrices of the current linearisation — exactly compute_error — and (B) linearises at the trial pose
// itself (new voxel lookup, new Mahalanobis, residual, Jacobian, H, b, cost) — exactly what the reference's next
// so3_linearize would compute if the trial is accepted. Nothing per-correspondence is cached in HBM except one
// 4-byte voxel id: the 3x3 Mahalanobis is recomputed from the 48-byte source covariance and the 96-byte voxel
// record instead of being stored as a 128-byte Matrix4d. Each point's contributions are summed per thread,
// reduce-scattered across the 64-lane wavefront, combined across the four wavefronts of the workgroup through
// LDS, and written as one row of partials. A one-workgroup controller kernel then sums the rows in a fixed order
// (deterministic) and runs the scalar LM logic on the device: LDLT solve, so3/se3 exponential, gain ratio,
// damping update, convergence — so there is no host round trip inside a solve. All pass / controller launches
// are predicated on the device-side state, so a fixed schedule of launches can be enqueued (or graph-captured)
// without knowing how many trials the data will need.
//
// This unit: the pass, controller, reduce, begin / evaluation and one-launch-per-trial kernels with their launchers. What a pass does to a point is lm_point.hpp, the
// scalar step lm_step.hpp — shared with the third launch form, the resident kernel of lm_persist.hip.
#include "rolo_internal.hpp"
#include "switches.hpp"
#include "lm_point.hpp"
#include "lm_step.hpp"
#include "peer_dev.hpp"

namespace rolo {

namespace {

#ifdef ROLO_PASS_STATS
__device__ unsigned long long g_pass_t[8];   // shader-clock ticks per phase of the rotation stage's pass_body, summed over thread 0 of every workgroup; [7] = count
extern "C" int rolo_debug_pass_times(unsigned long long* out8) {
  (void)hipDeviceSynchronize();
  return hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_pass_t), sizeof(unsigned long long) * 8) == hipSuccess ? 0 : -1;
}
#define PT_STAMP(k) const long long pt##k = clock64()
#else
#define PT_STAMP(k)
#endif
template <int STAGE, int DOF>
ROLO_DEV void pass_body(const PassArgs& a, const LmState* __restrict__ st, const int block) {
  ROLO_SHORT_KERNEL_PRIO();
  PT_STAMP(0);
  if (st->stage != STAGE) return;
  PT_STAMP(1);
  constexpr int NH = DOF * (DOF + 1) / 2;
  constexpr int NV = 3 + NH + DOF;
  double acc[NV];
#pragma unroll
  for (int v = 0; v < NV; v++) acc[v] = 0.0;
  const int i = a.begin + block * PASS_THREADS + threadIdx.x;
  const bool valid = i < a.end;
  PtIn in{};
  if (valid) in = load_pt(a, i);
  pass_compute<STAGE, DOF>(a, st, i, valid, in, acc);
#ifdef ROLO_PASS_STATS
  { double sink = 0; for (int v = 0; v < NV; v++) sink += acc[v]; asm volatile("" :: "v"(sink)); }   // the accumulators are final here
#endif
  PT_STAMP(2);
  int slot[NV];
#pragma unroll
  for (int v = 0; v < NV; v++) slot[v] = row_slot(v, NH);
  block_reduce_store<NV>(acc, slot, a.partials + (size_t)block * NV_MAX, st->phase == 1 && st->lin_skip != 0);
#ifdef ROLO_PASS_STATS
  if (STAGE == 1 && threadIdx.x == 0) {   // state flag known | point data + voxel records in, accumulators final | block reduction + row store
    const long long pt3 = clock64();
    atomicAdd(&g_pass_t[0], (unsigned long long)(pt1 - pt0)); atomicAdd(&g_pass_t[1], (unsigned long long)(pt2 - pt1)); atomicAdd(&g_pass_t[2], (unsigned long long)(pt3 - pt2));
    atomicAdd(&g_pass_t[7], 1ull);
  }
#endif
}

template <int DOF>
__global__ __launch_bounds__(PASS_THREADS) void rot_pass_kernel(PassArgs a, const LmState* __restrict__ st) { pass_body<1, DOF>(a, st, pass_xcd_block(a, blockIdx.x, gridDim.x)); }
__global__ __launch_bounds__(PASS_THREADS) void trans_pass_kernel(PassArgs a, const LmState* __restrict__ st) { pass_body<2, 6>(a, st, pass_xcd_block(a, blockIdx.x, gridDim.x)); }

// Batched form (rolo_batch_*, BASELINE config 5): one launch evaluates the same LM trial of B independent frame
// pairs. Workgroups [s * bps, (s + 1) * bps) belong to slot s; every slot has its own clouds, voxel table,
// correspondence cache, partial rows and LM state, and is predicated individually. The LM chain is a string of tiny
// latency-bound launches, so batching B frames through it costs almost the same wall time as one.
template <int DOF>
__global__ __launch_bounds__(PASS_THREADS) void rot_pass_batch_kernel(const BatchSlot* __restrict__ slots, int bps) {
  const int s = blockIdx.x / bps, lb = blockIdx.x - s * bps;
  if (lb >= slots[s].grid) return;
  pass_body<1, DOF>(slots[s].a, slots[s].st, lb);
}
__global__ __launch_bounds__(PASS_THREADS) void trans_pass_batch_kernel(const BatchSlot* __restrict__ slots, int bps) {
  const int s = blockIdx.x / bps, lb = blockIdx.x - s * bps;
  if (lb >= slots[s].grid) return;
  pass_body<2, 6>(slots[s].a, slots[s].st, lb);
}

// fixed-order sum of the per-workgroup rows (deterministic for a given grid)
// (twin: ctrl_body's inline sum — the same 8 groups x 64 loads in flight and the same order, with the first batch issued before the stage flag is known. Shared
// issue / add / group helpers changed the registers of reduce_kernel and of all eight controller kernels: both copies are kept as they were.)
ROLO_DEV void reduce_rows(const double* __restrict__ partials, int nblocks, double* sums /* shared, NV_MAX */) {
  __shared__ double part[8][NV_MAX];
  const int v = threadIdx.x & 31, q = threadIdx.x >> 5;  // 256 threads = 8 strided groups of 32 values
  // The rows were written by other CUs a moment ago, so every load is a ~1-2 us L2/fabric round trip and this
  // reduction is pure latency: issue 64 independent loads per thread before the first add — one round trip for the
  // 512 rows of a 131k-point cloud (16 in flight: four round trips, half of the controller's time). The combination
  // order is fixed => deterministic for a given grid.
  constexpr int INFLIGHT = 64;
  double s0 = 0;
  for (int b0 = q; b0 < nblocks; b0 += 8 * INFLIGHT) {
    double r[INFLIGHT];
#pragma unroll
    for (int u = 0; u < INFLIGHT; u++) {
      const int b = b0 + 8 * u;
      // an always-valid address and a select: `cond ? load : 0` compiles to one exec-masked branch per load (64 of them in front of the data)
      const double x = partials[(size_t)min(b, nblocks - 1) * NV_MAX + v];
      r[u] = (b < nblocks) ? x : 0.0;
    }
#pragma unroll
    for (int u = 0; u < INFLIGHT; u++) s0 += r[u];
  }
  part[q][v] = s0;
  __syncthreads();
  if (threadIdx.x < NV_MAX) {
    double t = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) t += part[k][threadIdx.x];
    sums[threadIdx.x] = t;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void reduce_kernel(const double* __restrict__ partials, int nblocks, double* out, const LmState* st, int stage) {
  if (stage >= 0 && st->stage != stage) return;
  __shared__ double sums[NV_MAX];
  reduce_rows(partials, nblocks, sums);
  if (threadIdx.x < NV_MAX) out[threadIdx.x] = sums[threadIdx.x];
}

// One workgroup: sums the partial rows in a fixed order (or takes the all-reduced sums on the multi-GPU path) and
// runs the scalar LM step on the device. Measured alternatives that did NOT pay on MI355X: running
// this in the last workgroup of the pass (arrival ticket + agent-scope release: 26.2 us per trial vs 11.7 + 9.9), and
// running it redundantly in the prologue of the next pass (every workgroup re-reduces the rows: faster alone,
// slower when four contexts share the GPU).
#ifdef ROLO_CTRL_STATS
__device__ unsigned long long g_ctrl_t[8];   // accumulated shader-clock ticks per phase of ctrl_body + [7] = launches counted
#define CT_STAMP(k) const long long ct##k = clock64()
#else
#define CT_STAMP(k)
#endif
// pub: pinned host copy of the state, written by the LAST controller launch of a frame's schedule whether or not it has a step to take
// (replaces a device-to-host copy launch per frame)
// MODE: -1 = decided at run time from `stage` and the state's optimizer (batched launches); 0 = rotation stage, SO(3) optimiser; 1 = rotation
// stage, 6-dof optimisers; 2 = translation stage. The specialised instances carry ONE step function instead of four: the generic kernel
// is ~11 k instructions of which a launch executes ~700 along a branchy path — on a cold instruction cache every taken branch is a fetch.
template <bool PEER = false, int MODE = -1>
ROLO_DEV void ctrl_body(LmState* st, const double* __restrict__ partials, int nblocks, const double* __restrict__ sums_in,
                        rolo_trace_rec* trace, int stage, LmState* pub = nullptr, const PeerArgs* peer = nullptr) {
  __shared__ double sums[NV_MAX];
  __shared__ double part[8][NV_MAX];
  __shared__ LmState sst;   // (StateFetch)
  ROLO_SHORT_KERNEL_PRIO();
  CT_STAMP(0);
  constexpr int INFLIGHT = 64;
  const int v = threadIdx.x & 31, q = threadIdx.x >> 5;  // 256 threads = 8 strided groups of 32 values
  // Everything this controller reads was written by other CUs a moment ago: every load is a ~1-2 us L2 / fabric round
  // trip. Issue ALL of them before the first use — the state copy and 64 partial rows per thread (the 512 rows of a
  // 131k-point cloud) — so the launch pays one round trip, not "stage flag, then state, then rows" (three).
  // (the staging and the copies below are the twins of StateFetch<256> and state_copy<256>: through either the controller kernels' register counts move)
  constexpr int NW = LM_STATE_WORDS, NWT = (NW + 255) / 256;
  int sreg[NWT];
  {
    const int* g = reinterpret_cast<const int*>(st);
#pragma unroll
    for (int k = 0; k < NWT; k++) { const int i = threadIdx.x + 256 * k; sreg[k] = i < NW ? g[i] : 0; }
  }
  double r[INFLIGHT];
  if (partials) {   // (twin: reduce_rows)
#pragma unroll
    for (int u = 0; u < INFLIGHT; u++) {   // always-valid address + select: `cond ? load : 0` is an exec-masked branch per load, 64 of them in front of the data
      const int b = q + 8 * u; const double x = partials[(size_t)min(b, nblocks - 1) * NV_MAX + v]; r[u] = (b < nblocks) ? x : 0.0;
    }
  }
  {
    int* l = reinterpret_cast<int*>(&sst);
#pragma unroll
    for (int k = 0; k < NWT; k++) { const int i = threadIdx.x + 256 * k; if (i < NW) l[i] = sreg[k]; }
  }
  __syncthreads();
  if (sst.stage != stage) {  // predicated launch: nothing to do (uniform)
    if (pub) { int* h = reinterpret_cast<int*>(pub); const int* l = reinterpret_cast<const int*>(&sst); for (int i = threadIdx.x; i < NW; i += 256) h[i] = l[i]; }
    return;
  }
  CT_STAMP(1);
  if (partials) {
    // fixed combination order => deterministic for a given grid
    double s0 = 0;
#pragma unroll
    for (int u = 0; u < INFLIGHT; u++) s0 += r[u];
    for (int b0 = q + 8 * INFLIGHT; b0 < nblocks; b0 += 8 * INFLIGHT) {   // clouds above 131k points
#pragma unroll
      for (int u = 0; u < INFLIGHT; u++) { const int b = b0 + 8 * u; const double x = partials[(size_t)min(b, nblocks - 1) * NV_MAX + v]; r[u] = (b < nblocks) ? x : 0.0; }
#pragma unroll
      for (int u = 0; u < INFLIGHT; u++) s0 += r[u];
    }
    part[q][v] = s0;
    __syncthreads();
    if (threadIdx.x < NV_MAX) {
      double t = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) t += part[k][threadIdx.x];
      sums[threadIdx.x] = t;
    }
  } else if (threadIdx.x < NV_MAX) {
    sums[threadIdx.x] = sums_in[threadIdx.x];
  }
  __syncthreads();
  bool peer_ok = true;
  if constexpr (PEER) {
    // multi-GPU: this rank's sums cover its shard of the source points — exchange them through the peers' mailboxes and add all ranks'
    // values in rank order (peer_dev.hpp); every rank then runs the identical scalar step below
    __shared__ unsigned xw[PEER_MAX * PEER_SLOT_WORDS];
    __shared__ int bad;
    peer_ok = peer_allreduce_block<256>(sums, xw, &bad, *peer);
  }
  CT_STAMP(2);
  if (threadIdx.x == 0) {
    // (the step on a private copy of the whole state instead of LDS: 256 VGPRs + 396 B of scratch, 2.2 -> 7.1 us)
    if (!peer_ok) {   // a peer did not answer within the timeout: end the registration with ROLO_ECOMM instead of waiting forever
      lm_fail_comm(&sst);
    } else if constexpr (MODE == 0) rot_step_t<3>(&sst, sums, trace);
    else if constexpr (MODE == 1) rot_step_t<6>(&sst, sums, trace);
    else if constexpr (MODE == 2) trans_step(&sst, sums, trace);
    else if (stage == 1) rot_step(&sst, sums, trace);
    else trans_step(&sst, sums, trace);
  }
  __syncthreads();
  CT_STAMP(3);
  {
    int* g = reinterpret_cast<int*>(st);
    const int* l = reinterpret_cast<const int*>(&sst);
    for (int i = threadIdx.x; i < NW; i += 256) g[i] = l[i];
    if (pub) { int* h = reinterpret_cast<int*>(pub); for (int i = threadIdx.x; i < NW; i += 256) h[i] = l[i]; }
  }
#ifdef ROLO_CTRL_STATS
  if (threadIdx.x == 0) {   // phases of a launch that had a step to take: loads issued -> first use | row sums | scalar step | write-back
    const long long ct4 = clock64();
    atomicAdd(&g_ctrl_t[0], (unsigned long long)(ct1 - ct0)); atomicAdd(&g_ctrl_t[1], (unsigned long long)(ct2 - ct1));
    atomicAdd(&g_ctrl_t[2], (unsigned long long)(ct3 - ct2)); atomicAdd(&g_ctrl_t[3], (unsigned long long)(ct4 - ct3)); atomicAdd(&g_ctrl_t[7], 1ull);
  }
#endif
}
#ifdef ROLO_CTRL_STATS
extern "C" int rolo_debug_ctrl_times(unsigned long long* out8) {
  (void)hipDeviceSynchronize();
  return hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_ctrl_t), sizeof(unsigned long long) * 8) == hipSuccess ? 0 : -1;
}
#endif

template <int MODE>
__global__ __launch_bounds__(256) void ctrl_kernel(LmState* st, const double* __restrict__ partials, int nblocks,
                                                  const double* __restrict__ sums_in, rolo_trace_rec* trace, int stage, LmState* pub) {
  ctrl_body<false, MODE>(st, partials, nblocks, sums_in, trace, stage, pub);
}
template <int MODE>
__global__ __launch_bounds__(256) void ctrl_peer_kernel(LmState* st, const double* __restrict__ partials, int nblocks, rolo_trace_rec* trace, int stage,
                                                       LmState* pub, PeerArgs peer) {
  ctrl_body<true, MODE>(st, partials, nblocks, nullptr, trace, stage, pub, &peer);
}
__global__ __launch_bounds__(256) void ctrl_batch_kernel(const BatchSlot* __restrict__ slots, int stage) {
  const BatchSlot& S = slots[blockIdx.x];
  ctrl_body(S.st, S.a.partials, S.grid, nullptr, S.trace, stage);
}

// ---- one launch per LM trial: controller in the prologue of the pass ---------------------------------------------------------------
// Every workgroup of launch j first finishes trial j-1 — sums the partial rows launch j-1 wrote (fixed order: deterministic, and the
// same bits in every workgroup) and runs the scalar LM step on a copy of the state in LDS — then evaluates the pass the new state asks
// for (rotation / 6-dof or translation stage) over its points and writes ITS row. Workgroup 0 also writes the new state back (and the
// LM trace). State and rows are double-buffered between consecutive launches (a workgroup of launch j may still be reading what a
// faster one would overwrite). Versus pass + ctrl_kernel launches this halves the launches of a solve; versus the first attempt at
// this fusion (every one of 512 workgroups re-reading 512 rows of 256 B) the rows are compact (12 or 30 doubles), there
// are n / THREADS of them with fat workgroups, and the point / covariance loads of the pass are issued before the prologue so that
// they overlap the row reads and the scalar step. do_body = 0: the closing launch of a schedule (one workgroup, no pass).
template <int COLS, int THREADS>
ROLO_DEV void reduce_rows_compact(const double* __restrict__ rows, int nrows, int nv, double* __restrict__ part /* THREADS */, double* __restrict__ sums /* NV_MAX */) {
  constexpr int GROUPS = THREADS / COLS;
  constexpr int INFLIGHT = 16;
  const int v = threadIdx.x % COLS, q = threadIdx.x / COLS;
  double s0 = 0;
  for (int b0 = q; b0 < nrows; b0 += GROUPS * INFLIGHT) {
    double r[INFLIGHT];
#pragma unroll
    for (int u = 0; u < INFLIGHT; u++) { const int b = b0 + GROUPS * u; const double x = rows[(size_t)min(b, nrows - 1) * NV_MAX + v]; r[u] = (b < nrows && v < nv) ? x : 0.0; }
#pragma unroll
    for (int u = 0; u < INFLIGHT; u++) s0 += r[u];
  }
  part[q * COLS + v] = s0;
  __syncthreads();
  if (threadIdx.x < COLS) {
    double t = 0;
#pragma unroll 8
    for (int k = 0; k < GROUPS; k++) t += part[k * COLS + threadIdx.x];
    sums[threadIdx.x] = t;
  }
  __syncthreads();
}

template <int DOF, int THREADS>
__global__ __launch_bounds__(THREADS) void lm_kernel(PassArgs a, const LmState* st_in, LmState* st_out /* the closing launch of an even chunk passes st_in == st_out: no __restrict__ */,
                                                    const double* __restrict__ rows_in, double* __restrict__ rows_out, int nrows,
                                                    rolo_trace_rec* trace, int do_body, int ppt, LmState* pub) {
  __shared__ LmState sst;
  __shared__ double part[THREADS];
  __shared__ double csum[NV_MAX];   // compact: yi, y, n, H (lower triangle), b
  __shared__ double sums[NV_MAX];   // V_* layout of the scalar step
  constexpr int NHR = DOF * (DOF + 1) / 2, NVR = 3 + NHR + DOF;
  StateFetch<THREADS> fetch;
  fetch.issue(st_in);
  // this thread's first point: independent of the state, in flight while the prologue runs. A workgroup owns ppt consecutive
  // slabs of THREADS points (fewer, fatter workgroups leave the rest of the chip to the other contexts' kernels).
  const int i0 = a.begin + (int)blockIdx.x * ppt * THREADS + (int)threadIdx.x;
  const bool valid0 = do_body && i0 < a.end;
  PtIn in{};
  if (valid0) in = load_pt(a, i0);
  fetch.land(&sst);
  __syncthreads();
  if (sst.stage != 0 && sst.pending) {
    const int stage = sst.stage;
    const int nv = stage == 1 ? NVR : 30;
    if (nv <= 16) reduce_rows_compact<16, THREADS>(rows_in, nrows, nv, part, csum);
    else reduce_rows_compact<32, THREADS>(rows_in, nrows, nv, part, csum);
    if (threadIdx.x < NV_MAX) {
      // compact -> V_* slots
      const int nh = stage == 1 ? NHR : 21;
      const int t = threadIdx.x;
      if (t < nv) sums[row_slot(t, nh)] = csum[t];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      rolo_trace_rec* tr = blockIdx.x == 0 ? trace : nullptr;
      if (stage == 1) rot_step(&sst, sums, tr); else trans_step(&sst, sums, tr);   // without a buffer trace_count still advances
    }
    __syncthreads();
  }
  const int stage = sst.stage;
  const bool body = do_body && stage != 0;
  if (threadIdx.x == 0) sst.pending = body ? 1 : 0;
  __syncthreads();
  if (blockIdx.x == 0) {
    state_copy<THREADS>(st_out, &sst);
    if (pub) state_copy<THREADS>(pub, &sst);   // pinned host copy (closing launch)
  }
  if (!body) return;
  double* out_row = rows_out + (size_t)blockIdx.x * NV_MAX;
  // (the slab loops below are pass_slabs' twins: the first point is in flight before the prologue and the point record is carried from slab to slab. As one helper
  // for both stages, or with a fresh record per slab as pass_slabs has it, the 1 024-thread instances' scratch changes: kept as they were.)
  if (stage == 1) {
    double acc[NVR];
    int slot[NVR];
#pragma unroll
    for (int v = 0; v < NVR; v++) { acc[v] = 0.0; slot[v] = v; }
    pass_compute<1, DOF>(a, &sst, i0, valid0, in, acc);
    for (int p = 1; p < ppt; p++) {   // twin: the translation stage's loop below, pass_slabs
      const int i = i0 + p * THREADS;
      const bool valid = i < a.end;
      if (valid) in = load_pt(a, i);
      pass_compute<1, DOF>(a, &sst, i, valid, in, acc);
    }
    block_reduce_store<NVR, THREADS>(acc, slot, out_row, sst.phase == 1 && sst.lin_skip != 0);
  } else {
    double acc[30];
    int slot[30];
#pragma unroll
    for (int v = 0; v < 30; v++) { acc[v] = 0.0; slot[v] = v; }
    pass_compute<2, 6>(a, &sst, i0, valid0, in, acc);
    for (int p = 1; p < ppt; p++) {   // twin: the rotation stage's loop above, pass_slabs
      const int i = i0 + p * THREADS;
      const bool valid = i < a.end;
      if (valid) in = load_pt(a, i);
      pass_compute<2, 6>(a, &sst, i, valid, in, acc);
    }
    block_reduce_store<30, THREADS>(acc, slot, out_row, sst.phase == 1 && sst.lin_skip != 0);
  }
}

__global__ void rot_begin_kernel(LmState* st, RotBegin a) {
  if (threadIdx.x != 0) return;
  rot_begin_dev(st, a);
}

ROLO_DEV void trans_knobs(LmState* st, const TransBegin& a) {   // TransBegin: the stage's knobs as they are when computeTranslation is called
  st->max_iterations = a.max_iterations; st->lm_max = a.lm_max; st->q2_intended = a.q2_intended;
  st->trans_eps = a.trans_eps; st->inv_trans_eps = 1.0 / a.trans_eps; st->lm_init = a.lm_init; st->trans_model = a.trans_model;
}
__global__ void trans_begin_kernel(LmState* st, TransBegin a) {
  if (threadIdx.x != 0) return;
  // (twin: trans_inputs_dev, lm_begin.hpp — through it this kernel takes 46 scalar registers instead of 38)
  for (int i = 0; i < 3; i++) { st->t0[i] = a.t0[i]; st->g[i] = a.g[i]; st->l[i] = a.l[i]; }
  st->dtn = a.dtn; st->dtn1 = a.dtn1; st->ct_lambda = a.ct_lambda; st->pending = 0; st->lmp_bailed = 0;
  trans_knobs(st, a);
  if (a.direct) trans_start(st);
}

__global__ void frame_begin_kernel(LmState* st, const FrameArgs* a) {
  if (threadIdx.x != 0) return;
  frame_begin_dev(st, a);
}

__global__ void frame_begin_batch_kernel(const BatchSlot* __restrict__ slots, const FrameArgs* __restrict__ args, int n) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  frame_begin_dev(slots[s].st, &args[s]);
}

// stage-level evaluation (rolo_so3_linearize & co): mode 0 = linearise at (R,t): phase 0, correspondences into
// buffer 0; mode 1 = error at (R,t) on the cached correspondences: phase 1.
__global__ void eval_begin_kernel(LmState* st, RotBegin a, int mode) {
  if (threadIdx.x != 0) return;
  for (int i = 0; i < 9; i++) st->xt_R[i] = a.R[i];
  lm_set_rrt(st->xt_S, st->xt_R);
  for (int i = 0; i < 3; i++) st->xt_t[i] = a.t[i];
  st->optimizer = a.optimizer; st->q2_intended = a.q2_intended;
  st->stage = 1; st->error = 0; st->lin_skip = 0;
  if (mode == 0) {
    st->phase = 0; st->cur = 0; st->tr_cur = 0;
    for (int i = 0; i < 9; i++) { st->x0_R[i] = a.R[i]; st->tr_R[i] = a.R[i]; }
    for (int i = 0; i < 6; i++) { st->x0_S[i] = st->xt_S[i]; st->tr_S[i] = st->xt_S[i]; }
    for (int i = 0; i < 3; i++) st->x0_t[i] = a.t[i];
  } else {
    st->phase = 1;
  }
}
// after a mode-0 evaluation: remember the correspondence count for later t3 evaluations
__global__ void eval_end_kernel(LmState* st, const double* sums, int mode) {
  if (threadIdx.x != 0) return;
  if (mode == 0) { st->n_corr = (int)(sums[V_N] + 0.5); st->tr_n_corr = st->n_corr; }
  st->stage = 0;
}
__global__ void t3_eval_begin_kernel(LmState* st, TransBegin a, int phase) {
  if (threadIdx.x != 0) return;
  for (int i = 0; i < 3; i++) st->tt[i] = a.t0[i];
  trans_inputs_dev(st, a);
  trans_knobs(st, a);
  st->lam_over_n = (double)(a.ct_lambda / (float)st->tr_n_corr);
  trans_consts(st);
  st->stage = 2; st->phase = phase; st->lin_skip = 0;
}

}  // namespace

hipError_t launch_rot_pass(int dof, const PassArgs& a, const LmState* st, int grid, hipStream_t s) {
  if (dof == 3) rot_pass_kernel<3><<<grid, PASS_THREADS, 0, s>>>(a, st);
  else rot_pass_kernel<6><<<grid, PASS_THREADS, 0, s>>>(a, st);
  return hipGetLastError();
}
hipError_t launch_trans_pass(const PassArgs& a, const LmState* st, int grid, hipStream_t s) {
  trans_pass_kernel<<<grid, PASS_THREADS, 0, s>>>(a, st);
  return hipGetLastError();
}
hipError_t launch_batch_pass(int stage, int dof, const BatchSlot* slots, int n_slots, int bps, hipStream_t s) {
  const int grid = n_slots * bps;
  if (stage == 1) {
    if (dof == 3) rot_pass_batch_kernel<3><<<grid, PASS_THREADS, 0, s>>>(slots, bps);
    else rot_pass_batch_kernel<6><<<grid, PASS_THREADS, 0, s>>>(slots, bps);
  } else {
    trans_pass_batch_kernel<<<grid, PASS_THREADS, 0, s>>>(slots, bps);
  }
  return hipGetLastError();
}
hipError_t launch_batch_ctrl(int stage, const BatchSlot* slots, int n_slots, hipStream_t s) {
  ctrl_batch_kernel<<<n_slots, 256, 0, s>>>(slots, stage);
  return hipGetLastError();
}
hipError_t launch_batch_begin(const BatchSlot* slots, const FrameArgs* args, int n_slots, hipStream_t s) {
  frame_begin_batch_kernel<<<(n_slots + 63) / 64, 64, 0, s>>>(slots, args, n_slots);
  return hipGetLastError();
}
hipError_t launch_lm(int dof, int threads, int ppt, const PassArgs& a, const LmState* st_in, LmState* st_out, const double* rows_in, double* rows_out, int nrows,
                     rolo_trace_rec* trace, int do_body, hipStream_t s, LmState* pub) {
  const int grid = do_body ? nrows : 1;
#define LM_GO(DOF, T) lm_kernel<DOF, T><<<grid, T, 0, s>>>(a, st_in, st_out, rows_in, rows_out, nrows, trace, do_body, ppt, pub)
  if (threads == 1024) { if (dof == 3) LM_GO(3, 1024); else LM_GO(6, 1024); }
  else { if (dof == 3) LM_GO(3, 512); else LM_GO(6, 512); }
#undef LM_GO
  return hipGetLastError();
}
hipError_t launch_reduce(const double* partials, int nblocks, double* sums, const LmState* st, int stage, hipStream_t s) {
  reduce_kernel<<<1, 256, 0, s>>>(partials, nblocks, sums, st, stage);
  return hipGetLastError();
}
template <int MODE>   // one controller launch: through the peers' mailboxes (p) or on this device's rows / the given sums
static void ctrl_go(bool p, LmState* st, const double* partials, int nblocks, const double* sums, rolo_trace_rec* trace, int stage, hipStream_t s, LmState* pub, const PeerArgs* peer) {
  if (p) ctrl_peer_kernel<MODE><<<1, 256, 0, s>>>(st, partials, nblocks, trace, stage, pub, *peer);
  else ctrl_kernel<MODE><<<1, 256, 0, s>>>(st, partials, nblocks, sums, trace, stage, pub);
}
hipError_t launch_ctrl(LmState* st, const double* partials, int nblocks, const double* sums, rolo_trace_rec* trace, int stage, hipStream_t s, LmState* pub,
                       const PeerArgs* peer, int dof) {
  const bool generic = switches().ctrl_generic;   // A/B: the one-size-fits-all kernel of round 2
  const int mode = generic ? -1 : (stage == 2 ? 2 : (dof == 3 ? 0 : (dof == 6 ? 1 : -1)));
  const bool p = peer && peer->world > 1 && partials;
  switch (mode) {
    case 0: ctrl_go<0>(p, st, partials, nblocks, sums, trace, stage, s, pub, peer); break;
    case 1: ctrl_go<1>(p, st, partials, nblocks, sums, trace, stage, s, pub, peer); break;
    case 2: ctrl_go<2>(p, st, partials, nblocks, sums, trace, stage, s, pub, peer); break;
    default: ctrl_go<-1>(p, st, partials, nblocks, sums, trace, stage, s, pub, peer);
  }
  return hipGetLastError();
}
hipError_t launch_rot_begin(LmState* st, const RotBegin& a, hipStream_t s) {
  rot_begin_kernel<<<1, 64, 0, s>>>(st, a);
  return hipGetLastError();
}
// graph-replayable form: both argument blocks come from a device buffer refreshed by a captured H2D copy
hipError_t launch_frame_begin(LmState* st, const FrameArgs* a, hipStream_t s) {
  frame_begin_kernel<<<1, 64, 0, s>>>(st, a);
  return hipGetLastError();
}
hipError_t launch_trans_begin(LmState* st, const TransBegin& a, hipStream_t s) {
  trans_begin_kernel<<<1, 64, 0, s>>>(st, a);
  return hipGetLastError();
}
hipError_t launch_eval_begin(LmState* st, const RotBegin& a, int mode, hipStream_t s) {
  eval_begin_kernel<<<1, 64, 0, s>>>(st, a, mode);
  return hipGetLastError();
}
hipError_t launch_eval_end(LmState* st, const double* sums, int mode, hipStream_t s) {
  eval_end_kernel<<<1, 64, 0, s>>>(st, sums, mode);
  return hipGetLastError();
}
hipError_t launch_t3_eval_begin(LmState* st, const TransBegin& a, int phase, hipStream_t s) {
  t3_eval_begin_kernel<<<1, 64, 0, s>>>(st, a, phase);
  return hipGetLastError();
}

}  // namespace rolo
