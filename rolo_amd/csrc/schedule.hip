// The schedule of one frame (include/rolo_hip.h rolo_align, rolo_compute_translation, rolo_register_async / _wait, rolo_batch_*): which LM launch form a context takes and
// how it is sized, how many predicated trials the first enqueue holds, the hipGraph a fixed schedule is captured into, and the host round trips of a frame that needs more.
#include "ctx.hpp"
#include <chrono>

using namespace rolo;

namespace rolo {

// workgroup size of the fused LM launches and slabs of that many points per workgroup (tuning: ROLO_LM_THREADS = 512 | 1024, ROLO_LM_PPT)
static int lm_threads() { return switches().lm_threads; }
static int lm_ppt() { return switches().lm_ppt; }
// 0: pass + controller launches; 1: one launch per LM trial (lm_kernel); 2: one launch per frame (lm_persist_kernel)
static int lm_mode(const rolo_ctx* c) {
  const int force = switches().lm_fused;   // A/B runs: 0 / 1 / 2 overrides the parameter
  // with a communicator / peers the sums pass through the exchange between pass and controller
  if (c->comm || peers(c)) return 0;
  const int m = force >= 0 ? force : c->P.fused_lm;
  return m == 2 ? 2 : (m != 0 ? 1 : 0);
}
static bool lm_fused(const rolo_ctx* c) { return lm_mode(c) == 1; }
static bool lm_persist(const rolo_ctx* c) { return lm_mode(c) == 2; }
// workgroups of the resident LM kernel: on an idle device one 512-thread workgroup per CU (a point per thread at 131 072 points: the shortest trial, 7.8 us), with other
// contexts' frames in flight 64 — the kernel holds the register files it runs on for the whole chain, and four launches of 64 are what the chip takes at one workgroup per
// CU (profiles/r06/concurrency.md); ROLO_LM_PERSIST_WGS pins it (A/B)
static int lm_persist_max_wgs(const rolo_ctx* c) {
  const int v = switches().lm_persist_wgs;
  return v ? v : (c->device_busy ? 64 : 256);
}
static unsigned long long lm_persist_admit_ticks() {     // how long the resident kernel's workgroups wait for each other to become resident before they leave the frame to the host
  // (ROLO_LM_PERSIST_ADMIT_US=0: a test switch — no launch is ever admitted, every frame takes the bail-out path)
  return (unsigned long long)switches().lm_persist_admit_us * 100ull;   // wall_clock64 runs at 100 MHz
}
static unsigned long long lm_persist_timeout_ticks() { return (unsigned long long)switches().lm_persist_timeout_ms * 100000ull; }   // what a poll may last after that

int prepare_pass(rolo_ctx* c, PassArgs& a, int& grid) {
  const int noff = n_offsets(c->P);
  int rc;
  for (int b = 0; b < 2; b++) if ((rc = c->store.grow(c->corr[b], c->corr_cap[b], (size_t)c->src.n * noff))) return rc;
  int begin, end; shard(c, begin, end);
  grid = std::max(1, (end - begin + PASS_THREADS - 1) / PASS_THREADS);
  c->lm_rows = std::max(1, (end - begin + lm_threads() * lm_ppt() - 1) / (lm_threads() * lm_ppt()));
  if ((rc = c->store.grow(c->partials, c->partials_cap, std::max((size_t)grid, 2 * (size_t)c->lm_rows) * NV_MAX))) return rc;
  if (lm_persist(c)) {
    // ROLO_LM_PERSIST_BUSY_THREADS=256 (A/B): with other frames in flight twice the workgroups of half the size — the same registers held, on twice the CUs, half of each
    int T = c->device_busy ? switches().lm_persist_busy_threads : 512;
    const int npts = std::max(end - begin, 1);
    int maxw = std::min(256, lm_persist_max_wgs(c) * (512 / T));
    int ppt = (npts + T * maxw - 1) / (T * maxw);
    if (ppt == 3) ppt = 4;   // (1, 2 and 4 points per thread have the interleaved bodies)
    if (T == 256 && !(ppt == 4 && c->P.optimizer == ROLO_OPT_SO3_LM && noff == 1)) {   // the A/B form exists for the headline's case only
      T = 512; maxw = lm_persist_max_wgs(c);
      ppt = (npts + T * maxw - 1) / (T * maxw);
      if (ppt == 3) ppt = 4;
    }
    c->lmp_ppt = ppt; c->lmp_threads = T;
    c->lmp_rows = (npts + T * c->lmp_ppt - 1) / (T * c->lmp_ppt);
    const size_t need = lm_persist_words(256);   // sized for the largest grid once: the epochs in it must survive a change of the cloud size
    if (!c->xbuf || c->xbuf_cap < need) {
      if ((rc = c->store.grow(c->xbuf, c->xbuf_cap, need))) return rc;
      HIPCHK(hipMemsetAsync(c->xbuf, 0, c->xbuf_cap * sizeof(unsigned long long), c->stream));
    }
  } else {
    c->lmp_form = LmpForm{};
  }
  a.src = c->src.xyz; a.cov = c->src.cov; a.n_total = c->src.n; a.begin = begin; a.end = end; a.n_off = noff;
  // the source covariances as I - m m^T: only what the library computed itself for THIS cloud under PLANE (ROLO_PASS_NRM=0: the six-entry form always — the A/B)
  a.nrm = (switches().pass_nrm && c->src.have_cov && c->src.have_nrm && !c->src.cov_user && c->src.nrm && c->P.regularization == ROLO_REG_PLANE) ? c->src.nrm : nullptr;
  a.corr[0] = c->corr[0]; a.corr[1] = c->corr[1]; a.partials = c->partials; a.tab = c->tab;
  a.xcd_map = switches().pass_xcd ? 1 : 0;
  return ROLO_OK;
}

// one LM trial: fused pass + controller launch, both predicated on the device state
static int enqueue_pass(rolo_ctx* c, const PassArgs& a, int grid, int stage, bool publish = false) {
  {
    ProfScope ps(c, stage == 1 ? ROLO_PROF_ROT_PASS : ROLO_PROF_TRANS_PASS);
    if (stage == 1) HIPCHK(launch_rot_pass(c->P.optimizer == ROLO_OPT_SO3_LM ? 3 : 6, a, c->state, grid, c->stream));
    else HIPCHK(launch_trans_pass(a, c->state, grid, c->stream));
  }
  ProfScope pc(c, ROLO_PROF_CTRL);
  if (c->comm) {
    HIPCHK(launch_reduce(c->partials, grid, c->sums, c->state, stage, c->stream));
    int e = g_rccl.AllReduce(c->sums, c->sums, NV_MAX, NCCL_FLOAT64, NCCL_SUM, c->comm, c->stream);
    if (e != 0) { g_err = std::string("ncclAllReduce: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(e) : "?"); return ROLO_ECOMM; }
    HIPCHK(launch_ctrl(c->state, nullptr, 0, c->sums, c->trace, stage, c->stream, publish ? c->h_state : nullptr, nullptr, c->P.optimizer == ROLO_OPT_SO3_LM ? 3 : 6));
  } else {
    // with peers the controller itself exchanges its row sums through the mailboxes: still ONE launch, still graph-capturable
    HIPCHK(launch_ctrl(c->state, c->partials, grid, nullptr, c->trace, stage, c->stream, publish ? c->h_state : nullptr, peer_args(c), c->P.optimizer == ROLO_OPT_SO3_LM ? 3 : 6));
  }
  return ROLO_OK;
}

// k fused trials + the closing launch; the state starts and ends in c->state[0] (see passes.hip lm_kernel)
static int enqueue_lm_chunk(rolo_ctx* c, const PassArgs& a, int k, bool publish = false) {
  LmState* sb[2] = {c->state, c->state + 1};
  const int nrows = c->lm_rows;
  double* rb[2] = {c->partials, c->partials + (size_t)nrows * NV_MAX};
  const int dof = c->P.optimizer == ROLO_OPT_SO3_LM ? 3 : 6, T = lm_threads();
  for (int j = 0; j < k; j++) {
    ProfScope ps(c, ROLO_PROF_LM_PASS);
    HIPCHK(launch_lm(dof, T, lm_ppt(), a, sb[j & 1], sb[(j + 1) & 1], rb[(j + 1) & 1], rb[j & 1], nrows, c->trace, 1, c->stream));
  }
  ProfScope ps(c, ROLO_PROF_LM_PASS);
  HIPCHK(launch_lm(dof, T, lm_ppt(), a, sb[k & 1], sb[0], rb[(k + 1) & 1], rb[k & 1], nrows, c->trace, 0, c->stream, publish ? c->h_state : nullptr));
  return ROLO_OK;
}

// both stages (or the one the state is in) to completion in ONE launch (lm_persist.hip lm_persist_kernel); the state starts and ends in c->state[0]
static int enqueue_lm_persist(rolo_ctx* c, const PassArgs& a, bool publish = false) {
  ProfScope ps(c, ROLO_PROF_LM_PASS);
  const int cap = (std::max(c->P.max_iterations, c->P.fixed_iterations) + 2) * (std::max(c->P.lm_max_iterations, 0) + 2) * 2 + 16;
  const int dof = c->P.optimizer == ROLO_OPT_SO3_LM ? 3 : 6;
  c->lmp_form = lm_persist_form(dof, c->lmp_threads, c->lmp_ppt, a.n_off, c->lmp_rows);
  HIPCHK(launch_lm_persist(dof, c->lmp_threads, c->lmp_ppt, a, c->state, c->xbuf, c->lmp_rows, c->trace, publish ? c->h_state : nullptr,
                           lm_persist_timeout_ticks(), lm_persist_admit_ticks(), cap, c->stream));
  return ROLO_OK;
}

RotBegin make_rot_begin(const rolo_ctx* c, const double* R9, const double* t3, int run_trans) {
  RotBegin b{};
  for (int i = 0; i < 9; i++) b.R[i] = R9 ? R9[i] : ((i % 4 == 0) ? 1.0 : 0.0);
  for (int i = 0; i < 3; i++) b.t[i] = t3 ? t3[i] : 0.0;
  b.optimizer = c->P.optimizer; b.max_iterations = c->P.max_iterations; b.fixed_iterations = c->P.fixed_iterations;
  b.lm_max = c->P.lm_max_iterations; b.q2_intended = c->P.q2_intended; b.rot_eps = c->P.rotation_epsilon;
  b.trans_eps = c->P.transformation_epsilon; b.lm_init = c->P.lm_init_lambda_factor; b.run_trans = run_trans;
  b.spec_lin = switches().lm_spec_lin;   // 0: every pass carries both halves (the A/B, rounds 1-4)
  b.keep_cost = switches().lm_keep_cost; // 0: the repeats of a converged-but-rejected trial under forced iterations are passes of their own (the A/B)
  b.trans_model = switches().lm_trans_model;   // 0: every trial of the translation stage is a pass of its own (the A/B)
  return b;
}

void fill_trans_knobs(const rolo_ctx* c, TransBegin& tb) {
  tb.max_iterations = c->P.max_iterations; tb.lm_max = c->P.lm_max_iterations; tb.q2_intended = c->P.q2_intended;
  tb.trans_eps = c->P.transformation_epsilon; tb.lm_init = c->P.lm_init_lambda_factor;
  tb.trans_model = switches().lm_trans_model;
}

void guess_to_Rt(const float* g16, double* R, double* t) {
  for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) R[i * 3 + j] = g16 ? (double)g16[i * 4 + j] : (i == j ? 1.0 : 0.0); t[i] = g16 ? (double)g16[i * 4 + 3] : 0.0; }
}

void fill_rot_outputs(const LmState* s, float* Tf, double* Td, rolo_stats* st) {
  double T[16];
  for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) T[i * 4 + j] = s->x0_R[i * 3 + j]; T[i * 4 + 3] = s->x0_t[i]; }
  T[12] = T[13] = T[14] = 0; T[15] = 1;
  if (Td) memcpy(Td, T, sizeof(T));
  if (Tf) for (int i = 0; i < 16; i++) Tf[i] = (float)T[i];
  if (st) { st->n_outer = s->rot_outer; st->converged = s->rot_converged; st->lm_failed = s->rot_failed; st->n_passes = s->rot_passes; st->n_correspondences = s->rot_ncorr; st->n_cost_only = s->rot_cost_only; }
}

// the translation stage's results (trans_out: 3 doubles, or nullptr)
void fill_trans_outputs(const LmState* s, double* trans_out, rolo_stats* st) {
  if (trans_out) for (int i = 0; i < 3; i++) trans_out[i] = s->t0[i];
  if (st) { st->n_outer = s->trans_outer; st->converged = s->trans_failed ? 0 : 1; st->lm_failed = s->trans_failed; st->n_passes = s->trans_passes; st->n_correspondences = s->tr_n_corr; st->n_cost_only = s->trans_cost_only; }
}

static int rot_first_chunk(const rolo_ctx* c) { return c->P.fixed_iterations > 0 ? c->P.fixed_iterations + 3 : 8; }
// first chunks of a whole frame (rolo_register_async): from the hints once a frame has been seen
static void frame_chunks(const rolo_ctx* c, int& nrot, int& ntrans) {
  nrot = c->hint_rot > 0 ? c->hint_rot : rot_first_chunk(c);
  ntrans = c->hint_trans > 0 ? c->hint_trans : 12;
}
// The first schedule of the next frame holds the most passes any of the last 64 frames needed as predicated pass / controller pairs (fused launches: one more,
// rounded up to an even count); it grows at once and shrinks only when the window's maximum has fallen 6 below it.
// A stream of DIFFERENT frame pairs needs different numbers of LM trials (BASELINE configs[4]: 24 ... 41 per pair). Round 2 followed the last
// frame alone: every other frame either re-captured its hipGraph (the schedule length is part of the graph's key) or topped up through
// host round trips — 351 top-ups, 297 captures and 753 eager frames in 1536. A 16-frame window still re-captured 90 times (the maximum slides
// in and out of a short window) and a capture is milliseconds of host time; a predicated no-op pair costs ~5 us of GPU time.
// Round 5: with pass + controller launches the schedule holds EXACTLY the window's maximum — through round 4 it held one pair more, rounded up to an even count (what
// the fused launches' double-buffered state needs): 22 + 12 pairs for frames that use 21 + 9..10, i.e. six to eight no-op launches of ~2.5 us on every frame's
// critical path. A frame that needs more than any of the last 64 did tops up through one host round trip and raises the hint.
// `used` counts launches that RAN: a rotation trial answered from the kept cost (LmState::rot_kept) is a trial of the solve and no launch — sized from rot_passes, every
// forced-iteration frame would carry a dozen predicated no-op pairs. (The resident kernel has no schedule: its hint only keys the frame's hipGraph, and keeps following the
// solve's trials, which differ less from pair to pair than the launches do — a hint that moves means an eager frame and a new capture.)
static int rot_launches(const rolo_ctx* c, const LmState* s) { return lm_persist(c) ? s->rot_passes : s->rot_passes - s->rot_kept; }
// ... and the same for the translation stage's trials answered from the linearisation's sums (LmState::trans_modelled; trans_lin_extra: the linearise-only launches that
// stand in for the (B) half of a modelled trial's pass, which trans_passes does not count)
static int trans_launches(const rolo_ctx* c, const LmState* s) { return lm_persist(c) ? s->trans_passes : s->trans_passes - s->trans_modelled + s->trans_lin_extra; }
static void update_hint(int& hint, rolo_ctx::NeedWindow& w, int used, bool fused) {
  constexpr int WN = 64;
  w.need[w.pos] = used; w.pos = (w.pos + 1) % WN; if (w.n < WN) w.n++;
  int mx = 0;
  for (int i = 0; i < w.n; i++) mx = std::max(mx, w.need[i]);
  const int want = fused ? std::min((std::max(mx + 1, 2) + 1) & ~1, 96) : std::min(std::max(mx, 2), 96);
  if (hint == 0 || want > hint || want <= hint - 6) hint = want;
}

// drive a stage to completion: enqueue predicated passes in chunks, look at the device flags between chunks
// no_persist: the frame's resident kernel gave the stage back (admission, LmState::lmp_bailed): finish with pass + controller launches
int run_stage(rolo_ctx* c, const PassArgs& a, int grid, int stage, int first_chunk, bool no_persist) {
  int chunk = first_chunk;
  const int hard_cap = (c->P.max_iterations + 2) * (c->P.lm_max_iterations + 1) + 8;
  int issued = 0;
  while (true) {
    if (lm_persist(c) && !no_persist) { int rc = enqueue_lm_persist(c, a); if (rc) return rc; }   // runs until the state says the stage (and what follows it) is over
    else if (lm_fused(c)) { int rc = enqueue_lm_chunk(c, a, chunk); if (rc) return rc; }
    else for (int i = 0; i < chunk; i++) { int rc = enqueue_pass(c, a, grid, stage); if (rc) return rc; }
    issued += chunk;
    c->n_topup_chunks++;
    int rc = fetch_state(c);
    if (rc) return rc;
    const bool done = (stage == 1) ? (c->h_state->rot_done != 0) : (c->h_state->trans_done != 0);
    if (done) return ROLO_OK;
    if (c->h_state->lmp_bailed && !no_persist) { no_persist = true; c->n_persist_bails++; }
    if (issued > hard_cap) { g_err = "LM stage did not terminate"; return ROLO_ESTATE; }
    chunk = 8;
  }
}

// frames in flight per device (rolo_register_async .. rolo_register_wait): a frame enqueued while OTHER contexts of the device have frames in flight takes the
// kernels that share the chip best (throughput), a frame enqueued on an idle device the ones that finish soonest (latency) — launch_knn_walk
static std::atomic<int> g_frames_in_flight[64];
void count_in_flight(rolo_ctx* c, bool on) {
  if (on == c->counted_in_flight || c->device < 0 || c->device >= 64) return;
  c->counted_in_flight = on;
  g_frames_in_flight[c->device].fetch_add(on ? 1 : -1, std::memory_order_relaxed);
}
static bool others_in_flight(const rolo_ctx* c) {
  if (c->device < 0 || c->device >= 64) return false;
  return g_frames_in_flight[c->device].load(std::memory_order_relaxed) - (c->counted_in_flight ? 1 : 0) > 0;
}

// ---- "capture a fixed schedule once, replay it after" (ctx.hpp CapturedSchedule) -------------------------------------------------------------
// ONE comparator for a frame and for a batch. A batch fills only the sizes, buffers, parameters and epoch of its members' keys, and those keys are value-initialised
// (std::vector<GraphKey> keys(b->n)): nrot / ntrans / rank / world / busy are zero on both sides, so the full comparison answers what a comparison of the filled fields would.
static bool same_key(const GraphKey& a, const GraphKey& b) {
  return a.n_src == b.n_src && a.n_tgt == b.n_tgt && a.src_xyz == b.src_xyz && a.tgt_xyz == b.tgt_xyz && a.epoch == b.epoch &&
         a.nrot == b.nrot && a.ntrans == b.ntrans && a.rank == b.rank && a.world == b.world && a.busy == b.busy && memcmp(&a.P, &b.P, sizeof(rolo_params)) == 0;
}
static bool same_key(const std::vector<GraphKey>& a, const std::vector<GraphKey>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++) if (!same_key(a[i], b[i])) return false;
  return true;
}
static unsigned long long key_epoch(const GraphKey& k) { return k.epoch; }
static unsigned long long key_epoch(const std::vector<GraphKey>& k) { return k[0].epoch; }
static void set_key_epoch(GraphKey& k, unsigned long long e) { k.epoch = e; }
static void set_key_epoch(std::vector<GraphKey>& ks, unsigned long long e) { for (GraphKey& k : ks) k.epoch = e; }

template <typename Key> static bool replay_due(const CapturedSchedule<Key>& g, const Key& key) { return g.exec && same_key(key, g.key); }
// the key was seen once, eagerly, and is here again unchanged: this frame is captured (and whatever graph is held goes)
template <typename Key> static bool capture_due(const CapturedSchedule<Key>& g, const Key& key) { return !replay_due(g, key) && g.seen_valid && same_key(key, g.seen); }

enum class Ran { Eager, Captured, Replayed };

// The launches `enqueue` puts on `st` are the same while `key` holds: the first frame with a new key runs eagerly and is remembered, the second is captured into a
// hipGraph and launched, every later one is one hipGraphLaunch. key == nullptr: this frame cannot be captured (event timing, a communicator, ...) and runs eagerly.
//   enqueue(capturing)  the launches, eagerly or into the capture. It must not allocate while capturing: the graph holds raw device pointers, so a capture during
//                       which g_alloc_epoch moved is thrown away. The eager frame before it did the allocations, which is why its key's epoch is refreshed afterwards.
//   captured()          the new graph is about to be launched for the first time: record what a replay will have to restore (graph_nrm_written)
//   discarded()         the capture failed and nothing ran: take back what enqueueing it marked as done (have_cov), the frame is redone eagerly
template <typename Key, typename Enqueue, typename Captured, typename Discarded>
static int run_captured(CapturedSchedule<Key>& g, hipStream_t st, const Key* key, Enqueue&& enqueue, Captured&& captured, Discarded&& discarded, Ran* ran) {
  int rc;
  *ran = Ran::Eager;
  if (key && replay_due(g, *key)) {
    HIPCHK(hipGraphLaunch(g.exec, st));
    *ran = Ran::Replayed;
    return ROLO_OK;
  }
  if (key && capture_due(g, *key)) {
    g.release();
    HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    rc = enqueue(true);
    hipGraph_t gph = nullptr;
    hipError_t e = hipStreamEndCapture(st, &gph);
    const bool epoch_moved = key_epoch(*key) != g_alloc_epoch;  // an allocation inside the capture would be a bug; fall back
    if (rc == ROLO_OK && e == hipSuccess && gph && !epoch_moved && hipGraphInstantiate(&g.exec, gph, nullptr, nullptr, 0) == hipSuccess) {
      g.graph = gph; g.key = *key;
      captured();
      HIPCHK(hipGraphLaunch(g.exec, st));
      *ran = Ran::Captured;
      return ROLO_OK;
    }
    if (gph) (void)hipGraphDestroy(gph);
    g.exec = nullptr;
    (void)hipGetLastError();
    discarded();  // nothing ran: redo eagerly below
    g.seen_valid = false;
  } else if (key) {
    g.seen = *key; g.seen_valid = true;
  }
  if ((rc = enqueue(false))) return rc;
  if (key) set_key_epoch(g.seen, g_alloc_epoch);  // the eager frame did the allocations the capture must not do
  return ROLO_OK;
}

}  // namespace rolo

extern "C" {

// ---- drivers ------------------------------------------------------------------------------------------------
static int enqueue_frame(rolo_ctx* c, bool with_trans);
// One enqueue, one wait (round 4; until then: covariances + voxel map with a host round trip for its counters, then the LM chunks): the frame path of
// rolo_register_async with the rotation stage alone — the voxel map rides inside the search's launches (VoxelFuse), its finalize kernel starts the LM
// state from pinned arguments, the first schedule of predicated trials follows the last frames' need, and the host waits once.
int rolo_align(rolo_ctx* c, const float* guess16, float* Tf, double* Td, rolo_stats* stats) {
  if (!c) return ROLO_EINVAL;
  if (c->async_pending) { g_err = "a registration is in flight on this context"; return ROLO_ESTATE; }
  int rc = set_device(c); if (rc) return rc;
  if (c->src.n <= 0 || c->tgt.n <= 0) { g_err = "source/target not set"; return ROLO_ESTATE; }
  c->have_map = false;  // computeTransformation: voxelmap_.reset() (rot_vgicp_impl.hpp:147)
  double R[9], t[3]; guess_to_Rt(guess16, R, t);
  c->h_args->rot = make_rot_begin(c, R, t, 0);
  c->h_args->trans = TransBegin{}; fill_trans_knobs(c, c->h_args->trans);
  if ((rc = enqueue_frame(c, false))) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  if ((rc = peer_check(c))) return rc;
  if ((rc = take_map_counters(c))) return rc;
  if (!c->h_state->rot_done) {   // the first schedule was too short (or the resident kernel gave the stage back): keep feeding predicated trials
    PassArgs a; int grid;
    const bool bailed = c->h_state->lmp_bailed != 0;
    if (bailed) c->n_persist_bails++;
    if ((rc = prepare_pass(c, a, grid))) return rc;
    if ((rc = run_stage(c, a, grid, 1, 8, bailed))) return rc;
  }
  c->have_corr = true;
  if (!c->h_state->error) { update_hint(c->hint_rot, c->win_rot, rot_launches(c, c->h_state), lm_fused(c)); c->n_kept_trials += c->h_state->rot_kept; }
  fill_rot_outputs(c->h_state, Tf, Td, stats);
  if (c->h_state->error) { g_err = c->h_state->error == ROLO_ENOCORR ? "no correspondences" : "device-side error during align"; return c->h_state->error; }
  return ROLO_OK;
}

int rolo_compute_translation(rolo_ctx* c, double* trans, const double* g3, const double* l3, double dtn, double dtn1, float lam, rolo_stats* stats) {
  if (!c || !trans || !g3 || !l3) return ROLO_EINVAL;
  if (!c->have_corr) { g_err = "computeTranslation needs the correspondences of a previous align"; return ROLO_ENOCORR; }
  int rc = set_device(c); if (rc) return rc;
  PassArgs a; int grid;
  if ((rc = prepare_pass(c, a, grid))) return rc;
  TransBegin tb{};
  for (int i = 0; i < 3; i++) { tb.t0[i] = trans[i]; tb.g[i] = g3[i]; tb.l[i] = l3[i]; }
  tb.dtn = dtn; tb.dtn1 = dtn1; tb.ct_lambda = lam; tb.direct = 1; fill_trans_knobs(c, tb);
  HIPCHK(launch_trans_begin(c->state, tb, c->stream));
  // the first chunk: what the last 64 calls' launches were (12 before the first) — with the trials answered from the model a stage is two or three launches
  if ((rc = run_stage(c, a, grid, 2, c->hint_ct > 0 ? c->hint_ct : 12))) return rc;
  const LmState* s = c->h_state;
  if (!s->error) update_hint(c->hint_ct, c->win_ct, trans_launches(c, s), lm_fused(c));
  c->n_model_trials += s->trans_modelled;
  fill_trans_outputs(s, trans, stats);
  if (s->error) { g_err = "device-side error during computeTranslation"; return s->error; }
  return ROLO_OK;
}

// everything of one frame after the clouds are on the device; per-frame arguments come from c->h_args (pinned)
static bool stamp_env() { return switches().stamp; }
#define STAMP(slot) do { if (stamp_env()) HIPCHK(launch_stamp(c->stamps, slot, c->stream)); } while (0)

static int enqueue_frame(rolo_ctx* c, bool with_trans) {   // with_trans = false: the rotation stage alone (rolo_align as one enqueue)
  int rc;
  if (c->src.n <= 0 || c->tgt.n <= 0) { g_err = "source/target not set"; return ROLO_ESTATE; }
  if (stamp_env()) {
    if (!c->stamps && (rc = c->store.alloc(c->stamps, 8))) return rc;
    if (!c->h_stamps && (rc = c->store.alloc_pinned(c->h_stamps, 8))) return rc;
  }
  STAMP(0);
  // voxel map without the host round trip of ensure_map(): errors are picked up in rolo_register_wait. The table is sized first: when
  // the target's covariances are about to be computed (and are bounded), the search's own launches build the map (VoxelFuse).
  {
    if ((rc = size_voxel_table(c))) return rc;
    c->vf_done = false;
    c->vf = VoxelFuse{};
    if (!c->tgt.have_cov && switches().voxel_fuse && knn_voxel_fuse_supported()) {   // ROLO_VOXEL_FUSE=0: the map as its own launches after the search (the A/B of VoxelFuse)
      c->tgt.cov_user = false;   // about to be computed here
      if (voxel_fixed_cov(c)) { c->vf.enabled = 1; c->vf.tab = c->tab; c->vf.tgt_keys = c->tgt_keys; c->vf.tgt_slot = c->tgt_slot; c->vf.counters = c->counters; }
    }
    rc = ensure_covs(c);
    c->vf.enabled = 0;
    if (rc) return rc;
    STAMP(1);
    note_voxel_build(c, c->vf_done ? ROLO_VOXBUILD_SEARCH : ROLO_VOXBUILD_FRAME);
    { ProfScope ps(c, ROLO_PROF_VOXEL_BUILD); HIPCHK(launch_voxel_build(c->tgt, c->tab, c->tgt_keys, c->tgt_slot, c->counters, voxel_morton_order(c), voxel_fixed_cov(c), c->tgt.bbox6, c->vf_done, c->stream, c->h_counters, c->state, c->h_args)); }   // the finalize kernel leaves the counters in pinned memory and starts the frame's LM state from c->h_args (pinned)
    c->vf_done = false;
  }
  PassArgs a; int grid;
  if ((rc = prepare_pass(c, a, grid))) return rc;
  // (the LM state of the frame was started by the voxel map's finalize kernel above: frame_begin_kernel was a launch of its own until round 3)
  STAMP(2);
  int nrot, ntrans; frame_chunks(c, nrot, ntrans);
  if (!with_trans) ntrans = 0;
  if (lm_persist(c)) {
    if ((rc = enqueue_lm_persist(c, a, true))) return rc;   // one launch for both stages; it leaves the state in pinned memory
  } else if (lm_fused(c)) {
    // both stages are the same launches (the device decides which pass a launch evaluates); each hint carries one spare
    if ((rc = enqueue_lm_chunk(c, a, std::max(nrot + ntrans - 1, 2), true))) return rc;   // the closing launch leaves the state in pinned memory
  } else {
    for (int i = 0; i < nrot; i++) if ((rc = enqueue_pass(c, a, grid, 1))) return rc;
    STAMP(3);
    for (int i = 0; i < ntrans; i++) if ((rc = enqueue_pass(c, a, grid, 2, i + 1 == ntrans && !c->comm))) return rc;   // the last controller publishes the state
  }
  STAMP(4);
  if (stamp_env()) HIPCHK(hipMemcpyAsync(c->h_stamps, c->stamps, sizeof(unsigned long long) * 8, hipMemcpyDeviceToHost, c->stream));
  if (!lm_persist(c) && ((c->comm && !lm_fused(c)) || (!lm_fused(c) && ntrans == 0))) HIPCHK(hipMemcpyAsync(c->h_state, c->state, sizeof(LmState), hipMemcpyDeviceToHost, c->stream));
  return ROLO_OK;
}

static int register_async_impl(rolo_ctx* c, const float* guess16, const double* trans_start, const double* g3, const double* l3, double dtn, double dtn1, float lam) {
  if (!c || !g3 || !l3) return ROLO_EINVAL;
  if (c->async_pending) { g_err = "a registration is already in flight on this context"; return ROLO_ESTATE; }
  int rc = set_device(c); if (rc) return rc;
  if (c->src.n <= 0 || c->tgt.n <= 0) { g_err = "source/target not set"; return ROLO_ESTATE; }
  double R[9], t[3]; guess_to_Rt(guess16, R, t);
  c->h_args->rot = make_rot_begin(c, R, t, 1);
  TransBegin& tb = c->h_args->trans;
  for (int i = 0; i < 3; i++) { tb.t0[i] = trans_start ? trans_start[i] : 0.0; tb.g[i] = g3[i]; tb.l[i] = l3[i]; }
  tb.dtn = dtn; tb.dtn1 = dtn1; tb.ct_lambda = lam; tb.direct = 0; fill_trans_knobs(c, tb);

  // hipGraph: the schedule of a frame is fixed (predicated launches), so with unchanged sizes / buffers / parameters
  // the ~95 launches are captured once and replayed with one hipGraphLaunch (host cost 0.35 ms -> ~0.02 ms per frame)
  const bool graphable = c->P.use_graph && !c->prof_on && !c->comm && !c->want_knn_lists && !c->src.have_cov && !c->tgt.have_cov;
  GraphKey key{};
  if (graphable) {
    key.n_src = c->src.n; key.n_tgt = c->tgt.n; key.src_xyz = c->src.xyz; key.tgt_xyz = c->tgt.xyz; key.P = c->P; key.epoch = g_alloc_epoch;
    key.rank = c->rank; key.world = c->world;   // the captured launches bake the shard range in
    key.busy = c->device_busy ? 1 : 0;          // ... and the walk kernel picked by the device's load
    frame_chunks(c, key.nrot, key.ntrans);
    // the second slot, around the one schedule: a frame of the other load regime is swapped in when it is cached, and kept when its successor is about to be captured
    CapturedSchedule<GraphKey>& g = c->sched;
    if (c->galt.exec && same_key(key, c->galt.key) && !replay_due(g, key)) {   // the other regime's frame is cached: swap
      std::swap(g.graph, c->galt.graph); std::swap(g.exec, c->galt.exec); std::swap(g.key, c->galt.key); std::swap(c->graph_nrm_written, c->galt.nrm);
      std::swap(c->graph_vox_build, c->galt.vox_build);
    } else if (g.exec && g.key.busy != key.busy && capture_due(g, key)) {   // keep the other regime's frame in the second slot (whatever was there goes)
      if (c->galt.exec) (void)hipGraphExecDestroy(c->galt.exec);
      if (c->galt.graph) (void)hipGraphDestroy(c->galt.graph);
      c->galt.graph = g.graph; c->galt.exec = g.exec; c->galt.key = g.key; c->galt.nrm = c->graph_nrm_written;
      std::copy(c->graph_vox_build, c->graph_vox_build + 4, c->galt.vox_build);
      g.graph = nullptr; g.exec = nullptr;
    }
  }
  Ran ran;
  rc = run_captured(c->sched, c->stream, graphable ? &key : nullptr, [&](bool) { return enqueue_frame(c, true); },
                    [&] { c->graph_nrm_written = c->src.have_nrm && c->tgt.have_nrm; std::copy(c->vox_build, c->vox_build + 4, c->graph_vox_build); },
                    [&] { c->src.have_cov = false; c->tgt.have_cov = false; }, &ran);
  if (rc) return rc;
  if (ran == Ran::Replayed) {
    c->n_replays++;
    std::copy(c->graph_vox_build, c->graph_vox_build + 4, c->vox_build);
    c->src.have_cov = true; c->tgt.have_cov = true; c->src.have_sorted = true; c->tgt.have_sorted = true;
    c->src.have_nrm = c->tgt.have_nrm = c->graph_nrm_written;   // what build_clouds decided when this graph was captured (recorded then, not re-derived: advisor, round 5)
  } else if (ran == Ran::Captured) c->n_captures++;
  else c->n_eager++;
  c->async_pending = true;
  return ROLO_OK;
}

int rolo_register_async(rolo_ctx* c, const float* guess16, const double* trans_start, const double* g3, const double* l3, double dtn, double dtn1, float lam) {
  if (c) {
    if (others_in_flight(c)) c->busy_credit = 8; else if (c->busy_credit > 0) c->busy_credit--;
    // (ranks that share ONE frame — peers, a communicator, a shard range — always have each other's frames "in flight": that is cooperation, not load)
    const bool sharded_ctx = c->comm != nullptr || peers(c) || c->world > 1;
    c->device_busy = c->load_hint < 0 ? (!sharded_ctx && c->busy_credit > 0) : c->load_hint != 0;
    // nobody of this process in flight: the learner decides (it may know of load this process cannot count)
    c->frame_auto_idle = c->load_hint < 0 && !sharded_ctx && c->busy_credit == 0 && !c->async_pending;
    if (c->frame_auto_idle) {
      c->learn.sizes(c->src.n, c->tgt.n);
      c->device_busy = c->learn.busy();
    }
    if (!c->async_pending && set_device(c) == ROLO_OK) (void)hipEventRecord(c->ev_start, c->stream);
  }
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = register_async_impl(c, guess16, trans_start, g3, l3, dtn, dtn1, lam);
  if (rc == ROLO_OK && c->async_pending) { c->n_frames++; count_in_flight(c, true); HIPCHK(hipEventRecord(c->ev_done, c->stream)); }
  if (c) c->ns_enqueue += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

int rolo_register_wait(rolo_ctx* c, float* Tf, double* Td, double* trans_out, rolo_stats* rs, rolo_stats* ts) {
  if (!c) return ROLO_EINVAL;
  if (!c->async_pending) { g_err = "no registration in flight"; return ROLO_ESTATE; }
  int rc = set_device(c); if (rc) return rc;
  c->async_pending = false;
  count_in_flight(c, false);
  c->device_busy = c->load_hint == 1;   // the choice belongs to the frame that was enqueued: synchronous entry points (rolo_compute_covariances, rolo_align, ...) run alone
  const auto tw0 = std::chrono::steady_clock::now();
  HIPCHK(hipEventSynchronize(c->ev_done));
  const auto tw1 = std::chrono::steady_clock::now();
  c->ns_wait_blocked += std::chrono::duration_cast<std::chrono::nanoseconds>(tw1 - tw0).count();
  if (c->frame_auto_idle) {   // the learner's signal: how long the frame took on the device (rolo_ctx::LoadLearner)
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->ev_start, c->ev_done) == hipSuccess && ms > 0.f) {
      c->learn.frame((double)ms);
    } else (void)hipGetLastError();
  }
  struct WaitTimer { rolo_ctx* c; std::chrono::steady_clock::time_point t; ~WaitTimer() { c->ns_wait_other += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t).count(); } } wt{c, tw1};
  if ((rc = peer_check(c))) return rc;
  if ((rc = take_map_counters(c))) return rc;
  PassArgs a; int grid;
  if ((rc = prepare_pass(c, a, grid))) return rc;
  // the common case finished inside the first enqueue; otherwise keep feeding predicated passes
  if (!c->h_state->rot_done || (!c->h_state->trans_done && !c->h_state->error)) c->n_topup_frames++;   // the first schedule was too short: host round trips
  const bool bailed = c->h_state->lmp_bailed != 0;   // (read before the top-ups overwrite the host copy)
  if (bailed) { c->n_persist_bails++; c->busy_credit = 64; }   // somebody this process cannot see shares the GPU (another process, a foreign workload): the busy-device sizing for the next frames
  if (!c->h_state->rot_done) { if ((rc = run_stage(c, a, grid, 1, 8, bailed))) return rc; }
  if (!c->h_state->trans_done && !c->h_state->error) { if ((rc = run_stage(c, a, grid, 2, 8, bailed))) return rc; }
  c->have_corr = true;
  const LmState* s = c->h_state;
  if (!s->error) { update_hint(c->hint_rot, c->win_rot, rot_launches(c, s), lm_fused(c)); update_hint(c->hint_trans, c->win_trans, trans_launches(c, s), lm_fused(c)); }
  c->n_kept_trials += s->rot_kept; c->n_model_trials += s->trans_modelled;
  fill_rot_outputs(s, Tf, Td, rs);
  fill_trans_outputs(s, trans_out, ts);
  if (s->error) { g_err = "device-side error during registration"; return s->error; }
  return ROLO_OK;
}

// ---- batches of independent scan pairs (BASELINE config 5; struct rolo_batch: ctx.hpp) -------------------------------------------------------
int rolo_batch_create(int device, int n_members, rolo_batch** out) {
  if (!out || n_members < 1 || n_members > 64) return ROLO_EINVAL;
  rolo_batch* b = new rolo_batch();
  b->device = device; b->n = n_members;
  for (int i = 0; i < n_members; i++) {
    rolo_ctx* c = nullptr;
    int rc = rolo_ctx_create(device, &c);
    if (rc) { rolo_batch_destroy(b); return rc; }
    b->m.push_back(c);
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { g_err = "event creation failed"; rolo_batch_destroy(b); return ROLO_EHIP; }
    b->ev_join.push_back(e);
    e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { g_err = "event creation failed"; rolo_batch_destroy(b); return ROLO_EHIP; }
    b->ev_join.push_back(e);
    e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { g_err = "event creation failed"; rolo_batch_destroy(b); return ROLO_EHIP; }
    b->ev_in.push_back(e);
  }
  if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming) != hipSuccess) {
    g_err = "batch stream / event creation failed"; rolo_batch_destroy(b); return ROLO_EHIP;
  }
  b->store.stream = b->stream; b->store.who = "batch";
  int rc = b->store.alloc_pinned(b->h_slots, (size_t)n_members);
  if (!rc) rc = b->store.alloc_pinned(b->h_args, (size_t)n_members);
  if (!rc) rc = b->store.alloc(b->d_slots, (size_t)n_members);
  if (!rc) rc = b->store.alloc(b->d_args, (size_t)n_members);
  if (rc) { rolo_batch_destroy(b); return rc; }
  *out = b;
  return ROLO_OK;
}

void rolo_batch_destroy(rolo_batch* b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  b->sched.release();
  for (rolo_ctx* c : b->m) rolo_ctx_destroy(c);
  for (hipEvent_t e : b->ev_join) (void)hipEventDestroy(e);
  for (hipEvent_t e : b->ev_in) (void)hipEventDestroy(e);
  if (b->ev_fork) (void)hipEventDestroy(b->ev_fork);
  if (b->stream) (void)hipStreamDestroy(b->stream);
  b->store.release();
  delete b;
}

int rolo_batch_size(rolo_batch* b) { return b ? b->n : 0; }
rolo_ctx* rolo_batch_member(rolo_batch* b, int i) { return (b && i >= 0 && i < b->n) ? b->m[i] : nullptr; }

// everything of one batch step after the clouds are on the device
static int enqueue_batch(rolo_batch* b, bool fork) {
  rolo_ctx* c0 = b->m[0];
  hipStream_t st = b->stream;
  int rc, bps = 1;
  // Eager launches (fork): the per-member front work fans out over the members' two streams — source search on one,
  // target search + voxel map on the other; one search launch fills about half the chip — and joins the batch stream
  // before the shared LM chain. Both streams fork directly from the batch stream. Captured schedule (!fork): a single
  // branch on the batch stream. ROCm 7.2's graph runtime is not safe with forked captures here: a fork of a fork sends
  // hipStreamEndCapture into an endless recursion, and several multi-branch graphs in flight crashed hipGraphLaunch
  // (hip::Graph::UpdateStreams); overlap between frames then comes from keeping several batches in flight.
  if (fork) HIPCHK(hipEventRecord(b->ev_fork, st));
  for (int i = 0; i < b->n; i++) {
    rolo_ctx* c = b->m[i];
    const hipStream_t s1 = fork ? c->stream : st, s2 = fork ? c->stream2 : st;
    if (c->src.n <= 0 || c->tgt.n <= 0) { g_err = "source/target not set"; return ROLO_ESTATE; }
    if (fork) { HIPCHK(hipStreamWaitEvent(s1, b->ev_fork, 0)); HIPCHK(hipStreamWaitEvent(s2, b->ev_fork, 0)); }
    if (!c->src.have_cov && (rc = build_src(c, s1))) return rc;
    if (!c->tgt.have_cov && (rc = build_tgt(c, s2))) return rc;
    if ((rc = size_voxel_table(c))) return rc;
    note_voxel_build(c, ROLO_VOXBUILD_FRAME);
    HIPCHK(launch_voxel_build(c->tgt, c->tab, c->tgt_keys, c->tgt_slot, c->counters, voxel_morton_order(c), voxel_fixed_cov(c), c->tgt.bbox6, false, s2));
    HIPCHK(hipMemcpyAsync(c->h_counters, c->counters, 4 * sizeof(int), hipMemcpyDeviceToHost, s2));
    if (fork) { HIPCHK(hipEventRecord(b->ev_join[2 * i], s1)); HIPCHK(hipEventRecord(b->ev_join[2 * i + 1], s2)); }
    PassArgs a; int grid;
    if ((rc = prepare_pass(c, a, grid))) return rc;
    BatchSlot& S = b->h_slots[i];
    S.a = a; S.st = c->state; S.trace = c->trace; S.grid = grid; S.pad = 0;
    bps = std::max(bps, grid);
  }
  b->bps = bps;
  if (fork) for (hipEvent_t e : b->ev_join) HIPCHK(hipStreamWaitEvent(st, e, 0));
  HIPCHK(hipMemcpyAsync(b->d_slots, b->h_slots, sizeof(BatchSlot) * b->n, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(b->d_args, b->h_args, sizeof(FrameArgs) * b->n, hipMemcpyHostToDevice, st));
  HIPCHK(launch_batch_begin(b->d_slots, b->d_args, b->n, st));
  const int dof = c0->P.optimizer == ROLO_OPT_SO3_LM ? 3 : 6;
  const int nrot = rot_first_chunk(c0);
  for (int k = 0; k < nrot; k++) { HIPCHK(launch_batch_pass(1, dof, b->d_slots, b->n, bps, st)); HIPCHK(launch_batch_ctrl(1, b->d_slots, b->n, st)); }
  for (int k = 0; k < 12; k++) { HIPCHK(launch_batch_pass(2, dof, b->d_slots, b->n, bps, st)); HIPCHK(launch_batch_ctrl(2, b->d_slots, b->n, st)); }
  for (int i = 0; i < b->n; i++) HIPCHK(hipMemcpyAsync(b->m[i]->h_state, b->m[i]->state, sizeof(LmState), hipMemcpyDeviceToHost, st));
  return ROLO_OK;
}

int rolo_batch_register_async(rolo_batch* b, const float* guess16, const double* trans_start, const double* init_guess, const double* last_t0,
                              double dtn, double dtn1, float lam) {
  if (!b || !init_guess || !last_t0) return ROLO_EINVAL;
  if (b->pending) { g_err = "a batch registration is already in flight"; return ROLO_ESTATE; }
  int rc = set_device(b->m[0]); if (rc) return rc;
  bool graphable = true;
  std::vector<GraphKey> keys(b->n);   // value-initialised: see same_key
  for (int i = 0; i < b->n; i++) {
    rolo_ctx* c = b->m[i];
    if (c->src.n <= 0 || c->tgt.n <= 0) { g_err = "batch member without source/target"; return ROLO_ESTATE; }
    if (c->comm || peers(c) || c->async_pending) { g_err = "batch members must be idle single-GPU contexts"; return ROLO_ESTATE; }
    if (c->P.optimizer != b->m[0]->P.optimizer || c->P.fixed_iterations != b->m[0]->P.fixed_iterations) { g_err = "batch members must share optimizer and iteration settings"; return ROLO_EUNSUPPORTED; }
    double R[9], t[3]; guess_to_Rt(guess16 ? guess16 + 16 * (size_t)i : nullptr, R, t);
    b->h_args[i].rot = make_rot_begin(c, R, t, 1);
    TransBegin& tb = b->h_args[i].trans;
    for (int d = 0; d < 3; d++) { tb.t0[d] = trans_start ? trans_start[3 * i + d] : 0.0; tb.g[d] = init_guess[3 * i + d]; tb.l[d] = last_t0[3 * i + d]; }
    tb.dtn = dtn; tb.dtn1 = dtn1; tb.ct_lambda = lam; tb.direct = 0; fill_trans_knobs(c, tb);
    graphable = graphable && c->P.use_graph && !c->prof_on && !c->want_knn_lists && !c->src.have_cov && !c->tgt.have_cov;
    keys[i].n_src = c->src.n; keys[i].n_tgt = c->tgt.n; keys[i].src_xyz = c->src.xyz; keys[i].tgt_xyz = c->tgt.xyz; keys[i].P = c->P; keys[i].epoch = g_alloc_epoch;
  }
  hipStream_t st = b->stream;
  // whatever the caller queued on the members' streams (rolo_set_source/_target pack the clouds there) comes first
  for (int i = 0; i < b->n; i++) { HIPCHK(hipEventRecord(b->ev_in[i], b->m[i]->stream)); HIPCHK(hipStreamWaitEvent(st, b->ev_in[i], 0)); }
  Ran ran;
  rc = run_captured(b->sched, st, graphable ? &keys : nullptr, [&](bool capturing) { return enqueue_batch(b, !capturing); },
                    [&] { for (rolo_ctx* c : b->m) c->graph_nrm_written = c->src.have_nrm && c->tgt.have_nrm; },
                    [&] { for (rolo_ctx* c : b->m) { c->src.have_cov = false; c->tgt.have_cov = false; } }, &ran);
  if (rc) return rc;
  if (ran == Ran::Replayed)
    for (rolo_ctx* c : b->m) { c->src.have_cov = true; c->tgt.have_cov = true; c->src.have_sorted = true; c->tgt.have_sorted = true;
                               c->src.have_nrm = c->tgt.have_nrm = c->graph_nrm_written; }   // as recorded when the batch's graph was captured
  b->pending = true;
  return ROLO_OK;
}

int rolo_batch_register_wait(rolo_batch* b, float* Tf, double* Td, double* trans_out, rolo_stats* rs, rolo_stats* ts) {
  if (!b) return ROLO_EINVAL;
  if (!b->pending) { g_err = "no batch registration in flight"; return ROLO_ESTATE; }
  int rc = set_device(b->m[0]); if (rc) return rc;
  b->pending = false;
  HIPCHK(hipStreamSynchronize(b->stream));
  int first_err = ROLO_OK;
  for (int i = 0; i < b->n; i++) {
    rolo_ctx* c = b->m[i];
    if ((rc = take_map_counters(c))) { if (!first_err) first_err = rc; continue; }
    // a member whose data needed more trials than the fixed schedule holds is finished on its own (rare)
    if (!c->h_state->error && (!c->h_state->rot_done || !c->h_state->trans_done)) {
      PassArgs a; int grid;
      if ((rc = prepare_pass(c, a, grid))) return rc;
      if (!c->h_state->rot_done) { if ((rc = run_stage(c, a, grid, 1, 8))) return rc; }
      if (!c->h_state->trans_done && !c->h_state->error) { if ((rc = run_stage(c, a, grid, 2, 8))) return rc; }
    }
    c->have_corr = true;
    const LmState* s = c->h_state;
    c->n_kept_trials += s->rot_kept; c->n_model_trials += s->trans_modelled;
    fill_rot_outputs(s, Tf ? Tf + 16 * (size_t)i : nullptr, Td ? Td + 16 * (size_t)i : nullptr, rs ? rs + i : nullptr);
    fill_trans_outputs(s, trans_out ? trans_out + 3 * (size_t)i : nullptr, ts ? ts + i : nullptr);
    if (s->error && !first_err) { g_err = "device-side error in a batch member"; first_err = s->error; }
  }
  return first_err;
}

int rolo_set_load_hint(rolo_ctx* c, int mode) {
  if (!c || mode < -1 || mode > 1) return ROLO_EINVAL;
  c->load_hint = mode;
  return ROLO_OK;
}

}  // extern "C"
