// Test and experiment hooks of the C ABI (include/rolo_hip.h): the LM controllers on scripted pass results, captured launch chains, the ROLO_STAMP=1 timeline,
// per-kernel event timing, the LM trace, and the counters a context keeps about its frames.
#include "ctx.hpp"

using namespace rolo;

// ---- test hook: the controller kernels on scripted pass results (include/rolo_hip.h rolo_lm_script) -------------------------------------------
static int script_stage(rolo_ctx* c, const rolo_lm_script* S, int stage, int dof, int generic_ctrl) {
  if (!S || S->n_outer < 1 || S->n_trial < 1 || !S->lin_y || !S->lin_H || !S->lin_b || !S->lin_n || !S->err_y) { g_err = "bad LM script"; return ROLO_EINVAL; }
  int rc = c->store.grow(c->partials, c->partials_cap, (size_t)NV_MAX);
  if (rc) return rc;
  const int hard_cap = (std::max(c->P.max_iterations, c->P.fixed_iterations) + 2) * (std::max(c->P.lm_max_iterations, 0) + 2) + 8;
  for (int it = 0; it <= hard_cap; it++) {
    if ((rc = fetch_state(c))) return rc;
    const LmState* s = c->h_state;
    if (stage == 1 ? s->rot_done != 0 : s->trans_done != 0) return ROLO_OK;
    double row[NV_MAX];
    for (double& v : row) v = __builtin_nan("");
    auto put_lin = [&](int o) {
      o = std::min(std::max(o, 0), S->n_outer - 1);
      row[V_Y] = S->lin_y[o]; row[V_N] = (double)S->lin_n[o];
      int t = 0;
      for (int i = 0; i < dof; i++) for (int j = 0; j <= i; j++) row[V_H + t++] = S->lin_H[(size_t)o * 36 + i * 6 + j];
      for (int i = 0; i < dof; i++) row[V_B + i] = S->lin_b[(size_t)o * 6 + i];
    };
    if (s->phase == 0) put_lin(s->outer);   // a linearise-only pass: the stage's first, or the one after a trial accepted on a cost-only pass
    else {
      row[V_YI] = S->err_y[(size_t)std::min(std::max(s->outer, 0), S->n_outer - 1) * S->n_trial + std::min(std::max(s->trial, 0), S->n_trial - 1)];
      if (!s->lin_skip) put_lin(s->outer + 1);   // half (B) of a full pass: the linearisation at the trial pose = the one that opens the next outer iteration
    }
    HIPCHK(hipMemcpyAsync(c->partials, row, sizeof(row), hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_ctrl(c->state, c->partials, 1, nullptr, c->trace, stage, c->stream, nullptr, nullptr, generic_ctrl ? 0 : dof));
  }
  g_err = "scripted LM stage did not terminate";
  return ROLO_ESTATE;
}
extern "C" int rolo_debug_lm_script_align(rolo_ctx* c, const rolo_lm_script* S, const float* guess16, int generic_ctrl, float* Tf, double* Td, rolo_stats* stats) {
  if (!c) return ROLO_EINVAL;
  if (c->async_pending) { g_err = "a registration is in flight on this context"; return ROLO_ESTATE; }
  int rc = set_device(c); if (rc) return rc;
  double R[9], t[3]; guess_to_Rt(guess16, R, t);
  RotBegin rb = make_rot_begin(c, R, t, 0);
  rb.keep_cost = 0;   // a script names a cost per (outer, trial): the repeat of a converged-but-rejected trial is not bound to return the same one, so each is asked for
  HIPCHK(launch_rot_begin(c->state, rb, c->stream));
  if ((rc = script_stage(c, S, 1, c->P.optimizer == ROLO_OPT_SO3_LM ? 3 : 6, generic_ctrl))) return rc;
  c->have_corr = c->h_state->tr_n_corr > 0;   // what computeTranslation asks for: a linearisation that left correspondences
  fill_rot_outputs(c->h_state, Tf, Td, stats);
  return c->h_state->error;
}
extern "C" int rolo_debug_lm_script_translation(rolo_ctx* c, const rolo_lm_script* S, double* trans, const double* g3, const double* l3, double dtn, double dtn1, float lam,
                                                int generic_ctrl, rolo_stats* stats) {
  if (!c || !trans || !g3 || !l3) return ROLO_EINVAL;
  if (!c->have_corr) { g_err = "computeTranslation needs the correspondences of a previous align"; return ROLO_ENOCORR; }
  int rc = set_device(c); if (rc) return rc;
  TransBegin tb{};
  for (int i = 0; i < 3; i++) { tb.t0[i] = trans[i]; tb.g[i] = g3[i]; tb.l[i] = l3[i]; }
  tb.dtn = dtn; tb.dtn1 = dtn1; tb.ct_lambda = lam; tb.direct = 1; fill_trans_knobs(c, tb);
  tb.trans_model = 0;   // a script names a cost per (outer, trial): every trial is asked for, none answered from the linearisation's sums
  HIPCHK(launch_trans_begin(c->state, tb, c->stream));
  if ((rc = script_stage(c, S, 2, 6, generic_ctrl))) return rc;
  const LmState* s = c->h_state;
  fill_trans_outputs(s, trans, stats);
  return s->error;
}

extern "C" {

int rolo_debug_stamps(rolo_ctx* c, unsigned long long* out8) {   // after rolo_register_wait; zeros unless ROLO_STAMP=1
  if (!c || !out8) return ROLO_EINVAL;
  if (c->h_stamps) memcpy(out8, c->h_stamps, sizeof(unsigned long long) * 8); else memset(out8, 0, sizeof(unsigned long long) * 8);
  return ROLO_OK;
}

// experiment hook (include/rolo_hip.h): a captured chain of launch pairs, replayed `reps` times
int rolo_debug_chain(rolo_ctx* c, int kind, int n_pairs, int grid, int reps) {
  if (!c || kind < 0 || kind > 4 || n_pairs < 1 || n_pairs > 256 || grid < 1 || reps < 1) return ROLO_EINVAL;
  if (c->async_pending) { g_err = "a registration is in flight on this context"; return ROLO_ESTATE; }
  int rc = set_device(c); if (rc) return rc;
  if (kind >= 3 && (!c->have_map || !c->src.have_cov)) { g_err = "the real LM chain needs a finished registration on this context"; return ROLO_ESTATE; }
  if (!c->dbg_chain_exec || c->dbg_chain_key[0] != kind || c->dbg_chain_key[1] != n_pairs || c->dbg_chain_key[2] != grid) {
    if (c->dbg_chain_exec) { (void)hipGraphExecDestroy(c->dbg_chain_exec); c->dbg_chain_exec = nullptr; }
    PassArgs a; int pgrid = 0;
    if (kind >= 3 && (rc = prepare_pass(c, a, pgrid))) return rc;
    HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    hipError_t e = hipSuccess;
    const int dof = c->P.optimizer == ROLO_OPT_SO3_LM ? 3 : 6;
    if (kind >= 3) e = launch_frame_begin(c->state, c->h_args, c->stream);
    for (int i = 0; i < n_pairs && e == hipSuccess; i++) {
      if (kind == 0) { e = launch_empty(1, 256, c->stream); if (e == hipSuccess) e = launch_empty(1, 256, c->stream); }
      else if (kind == 1) { e = launch_empty(grid, 256, c->stream); if (e == hipSuccess) e = launch_empty(grid, 256, c->stream); }
      else if (kind == 2) { e = launch_empty(grid, 256, c->stream); if (e == hipSuccess) e = launch_empty(1, 256, c->stream); }
      else if (kind == 3) {   // the first two thirds of the pairs belong to the rotation stage, the rest to the translation stage (a frame's 21 + 10)
        const int stage = i < (2 * n_pairs + 2) / 3 ? 1 : 2;
        e = stage == 1 ? launch_rot_pass(dof, a, c->state, pgrid, c->stream) : launch_trans_pass(a, c->state, pgrid, c->stream);
        if (e == hipSuccess) e = launch_ctrl(c->state, c->partials, pgrid, nullptr, c->trace, stage, c->stream, nullptr, nullptr, dof);
      } else { e = launch_rot_pass(dof, a, c->state, pgrid, c->stream); if (e == hipSuccess) e = launch_rot_pass(dof, a, c->state, pgrid, c->stream); }
    }
    hipGraph_t gph = nullptr;
    const hipError_t e2 = hipStreamEndCapture(c->stream, &gph);
    if (e != hipSuccess || e2 != hipSuccess || !gph || hipGraphInstantiate(&c->dbg_chain_exec, gph, nullptr, nullptr, 0) != hipSuccess) {
      if (gph) (void)hipGraphDestroy(gph);
      c->dbg_chain_exec = nullptr; (void)hipGetLastError();
      g_err = "rolo_debug_chain: capture failed"; return ROLO_EHIP;
    }
    (void)hipGraphDestroy(gph);
    c->dbg_chain_key[0] = kind; c->dbg_chain_key[1] = n_pairs; c->dbg_chain_key[2] = grid;
  }
  for (int r = 0; r < reps; r++) HIPCHK(hipGraphLaunch(c->dbg_chain_exec, c->stream));
  return ROLO_OK;
}

int rolo_get_trace(rolo_ctx* c, rolo_trace_rec* out, int cap) {
  if (!c) return ROLO_EINVAL;
  int rc = set_device(c); if (rc) return rc;
  if ((rc = fetch_state(c))) return rc;
  const int n = std::min(c->h_state->trace_count, TRACE_CAP);
  const int m = std::min(n, cap);
  if (m > 0 && out) {
    HIPCHK(hipMemcpyAsync(out, c->trace, sizeof(rolo_trace_rec) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return n;
}

int rolo_ctx_counters(rolo_ctx* c, long long* out, int n) {
  if (!c || !out || n < 0) return ROLO_EINVAL;
  const long long v[16] = {c->n_frames, c->n_replays, c->n_captures, c->n_eager, c->n_topup_frames, c->n_topup_chunks, c->hint_rot, c->hint_trans, c->walk_lanes,
                           c->ns_enqueue, c->ns_wait_blocked, c->ns_wait_other, c->n_persist_bails, c->learn.mode, c->n_kept_trials, c->n_model_trials};
  for (int i = 0; i < n && i < 16; i++) out[i] = v[i];
  return ROLO_OK;
}

int rolo_ctx_lm_form(rolo_ctx* c, int* out, int n) {
  if (!c || !out || n < 0) return ROLO_EINVAL;
  const LmpForm& f = c->lmp_form;
  const int v[7] = {f.rows, f.threads, f.ppt, f.sp, f.batch, f.mcache, (int)f.lds};
  for (int i = 0; i < n && i < 7; i++) out[i] = v[i];
  return ROLO_OK;
}

int rolo_debug_voxel_build(rolo_ctx* c, int32_t out[4]) {
  if (!c || !out) return ROLO_EINVAL;
  if (!c->have_map || c->vox_build[0] < 0) { g_err = "rolo_debug_voxel_build needs a built voxel map"; return ROLO_ESTATE; }
  for (int i = 0; i < 4; i++) out[i] = c->vox_build[i];
  return ROLO_OK;
}

// the source's PLANE short form as prepare_pass hands it to the passes (schedule.hip: PassArgs::nrm), row per point; m.x is NaN where the tail poisoned it
int rolo_debug_source_plane_form(rolo_ctx* c, double* m, int n) {
  if (!c || !m) return ROLO_EINVAL;
  if (c->async_pending) { g_err = "a registration is in flight on this context"; return ROLO_ESTATE; }
  int rc = set_device(c); if (rc) return rc;
  if (!(switches().pass_nrm && c->src.have_cov && c->src.have_nrm && !c->src.cov_user && c->src.nrm && c->P.regularization == ROLO_REG_PLANE)) {
    g_err = "the passes do not read the source's plane form (not PLANE, handed-in covariances, ROLO_PASS_NRM=0, or not computed)"; return ROLO_ESTATE;
  }
  if (n != c->src.n) { g_err = "rolo_debug_source_plane_form: n is not the source's size"; return ROLO_EINVAL; }
  std::vector<double> soa(3 * (size_t)n);
  HIPCHK(hipMemcpyAsync(soa.data(), c->src.nrm, sizeof(double) * soa.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int i = 0; i < n; i++) for (int d = 0; d < 3; d++) m[(size_t)i * 3 + d] = soa[(size_t)d * n + i];
  return ROLO_OK;
}

int rolo_prof_enable(rolo_ctx* c, int on) {
  if (!c) return ROLO_EINVAL;
  c->prof_on = on != 0;
  return ROLO_OK;
}

int rolo_prof_read(rolo_ctx* c, int slot, float* ms, int cap) {
  if (!c || slot < 0 || slot >= ROLO_PROF_N) return ROLO_EINVAL;
  int rc = set_device(c); if (rc) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  int n = 0;
  std::vector<rolo_ctx::ProfEv> keep;
  for (auto& e : c->prof) {
    if (e.slot != slot) { keep.push_back(e); continue; }
    float t = 0.f;
    (void)hipEventElapsedTime(&t, e.a, e.b);
    if (ms && n < cap) ms[n] = t;
    n++;
    (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b);
  }
  c->prof.swap(keep);
  return n;
}

}  // extern "C"
