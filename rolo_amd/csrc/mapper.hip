// The mapping node's per-scan step as one call: laserCloudInfoHandler (reference src/backMapping.cpp:420-457) over a key map, a scan-to-submap context and a pose
// graph that the mapper owns. Replaces updateInitialGuess :516-555, the caller's side of extractSurroundingKeyFrames :558-663 and downsampleCurrentScan :666-678,
// scan2MapOptimization's gate :684 and transformUpdate :1060-1068, saveFrame :1071-1091, saveKeyFramesAndFactor :1094-1221 with addOdomFactor / addLoopFactor /
// addPriorFactor :1224-1284, correctPoses :1287-1320, the incremental pose of publishOdometry :1361-1389 and the clouds of publishFrames :1405-1424.
//
// Every number comes from a unit that exists: the voxel filter and the store (submap.hip), the Gauss-Newton loop (scan2map.hip: s2m_optimize_core, the body both
// entries share), Scan Context (scancontext.hip), the graph (posegraph.hip). This unit adds the order of the statements, the node's float pose bookkeeping, and
// residence: the scan's filtered clouds stay in the key map's scan_ds slots from the filter to the key-frame store; streams are ordered by events (scan_ready for the
// registration's pack, the key map's own stream for the append); no host wait beyond those of the composed calls.
//
// The float pose algebra (pcl::getTransformation, pcl::getTranslationAndEulerAngles, Eigen::Affine3f inverse and products) is pcl_affine.hpp's; the products here are
// its aff_mul, the affine form; tests/mapper_twin.py holds the node's bookkeeping to a float64 statement within a derived bound.
#include "keymap.hpp"
#include "pcl_affine.hpp"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

using namespace rolo;

namespace {

// constraintTransformation :282-290
float clamp_sym(float value, float limit) {
  if (value < -limit) value = -limit;
  if (value > limit) value = limit;
  return value;
}

// gtsam::Pose3(Rot3::RzRyRx(double(roll), double(pitch), double(yaw)), Point3(double(x), ...)) :322-332 as a row-major 4 x 4: pcl::getTransformation's
// formula in double on the widened floats
void T16_of_rpyxyz(const float* p, double* T) {
  pcl_rows_of_xyzrpy<double>(p[3], p[4], p[5], p[0], p[1], p[2], T);
  T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
}
// poseFrom.between(poseTo) = poseFrom^-1 poseTo for rigid poses: R = Rf^T Rt, t = Rf^T (tt - tf), every sum over k left to right
void T16_between(const double* Fm, const double* Tm, double* Z) {
  const double d[3] = {Tm[3] - Fm[3], Tm[7] - Fm[7], Tm[11] - Fm[11]};
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) Z[4 * i + j] = Fm[i] * Tm[j] + Fm[4 + i] * Tm[4 + j] + Fm[8 + i] * Tm[8 + j];
    Z[4 * i + 3] = Fm[i] * d[0] + Fm[4 + i] * d[1] + Fm[8 + i] * d[2];
  }
  Z[12] = 0.0; Z[13] = 0.0; Z[14] = 0.0; Z[15] = 1.0;
}

struct QueuedFactor { int from, to; double T[16], var[6], k; };

// what a scan may change before saveKeyFramesAndFactor: committed in one assignment once scan2MapOptimization has succeeded
struct NodeState {
  float tf[6] = {0, 0, 0, 0, 0, 0};                 // transformTobeMapped
  double timeLastProcessing = -1;                    // :434
  float lastOdom[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};   // lastOdomTransformation :535
  int lastOdomAvailable = 0;                         // :534
  float front6[6] = {0, 0, 0, 0, 0, 0};              // the pose incrementalOdometryAffineFront was taken from :519
  float back6[6] = {0, 0, 0, 0, 0, 0};               // the pose incrementalOdometryAffineBack was taken from :1067 (all zero: the identity)
};

bool finite_n(const double* v, int n) { for (int i = 0; i < n; i++) if (!std::isfinite(v[i])) return false; return true; }

}  // namespace

struct rolo_mapper {
  int device = 0;
  rolo_mapper_params P{};
  rolo_keymap* km = nullptr;
  rolo_ctx* ctx = nullptr;      // from the pool: its source / target clouds hold the sub-map's trees
  rolo_pgo* pgo = nullptr;
  NodeState st;
  float incre[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};   // increOdomAffine :1364
  int increStarted = 0;                                      // lastIncreOdomPubFlag :1362
  bool aLoopIsClosed = false;
  std::vector<QueuedFactor> loopQ, priorQ;
  // the sub-map the context holds: the list it was fused from and the key map's pose epoch then
  std::vector<int32_t> list; bool list_valid = false; unsigned long long list_epoch = 0;
  int m_sub[2] = {0, 0};
  // the last processed scan
  bool have_scan = false;
  float pub_tf[6] = {0, 0, 0, 0, 0, 0};
  hipEvent_t ev[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // with timing: 4 pairs and the call's first / last
  float ms[6] = {0, 0, 0, 0, 0, 0};
};

namespace {

int check_queued(const double* T16, const double* var6, double k, const char* who) {
  if (!T16 || !var6) return ROLO_EINVAL;
  for (int r = 0; r < 3; r++) if (!finite_n(T16 + 4 * r, 4)) { ctx_set_error((std::string(who) + ": a non-finite pose").c_str()); return ROLO_EINVAL; }
  for (int i = 0; i < 6; i++) if (!std::isfinite(var6[i]) || !(var6[i] > 0.0)) { ctx_set_error((std::string(who) + ": a variance must be finite and positive").c_str()); return ROLO_EINVAL; }
  if (!(k >= 0.0) || !std::isfinite(k) || !std::isfinite(k * k) || (k > 0.0 && !(k * k > 0.0))) { ctx_set_error((std::string(who) + ": the Cauchy constant must be finite, and positive or 0 for none").c_str()); return ROLO_EINVAL; }
  return ROLO_OK;
}

// extractSurroundingKeyFrames :558-663 and the hand-over (kdtree*FromMap->setInputCloud :689-690): kept when the list and the poses are those of the resident sub-map
int mapper_submap(rolo_mapper* m, double stamp, rolo_mapper_result* out) {
  rolo_keymap* km = m->km;
  const int n = (int)km->frames.size();
  std::vector<float> xyz(3 * (size_t)n);
  std::vector<double> times((size_t)n);
  for (int k = 0; k < n; k++) { for (int d = 0; d < 3; d++) xyz[3 * (size_t)k + d] = km->frames[k].pose[3 + d]; times[k] = km->frames[k].time; }
  std::vector<int32_t> idx(2 * (size_t)n);
  const int cnt = rolo_keyposes_select_nearby(xyz.data(), times.data(), n, m->P.surroundingKeyframeSearchRadius, m->P.surroundingKeyframeDensity, stamp, 10.0, idx.data(),
                                              (int)idx.size());
  if (cnt < 0) return cnt;
  if (cnt > (int)idx.size()) { ctx_set_error("rolo_mapper_scan: the key-frame list is longer than two entries per key pose"); return ROLO_ESTATE; }
  idx.resize((size_t)cnt);
  out->n_listed = cnt;
  if (m->list_valid && m->list_epoch == km->pose_epoch && idx == m->list && km->have_submap) {
    out->submap_rebuilt = 0;
  } else {
    m->list_valid = false;
    int rc;
    if ((rc = rolo_keymap_extract(km, idx.data(), cnt, m->P.mappingCornerLeafSize, m->P.mappingSurfLeafSize, &m->m_sub[0], &m->m_sub[1]))) return rc;
    if ((rc = rolo_scan2map_set_submap_keymap(m->ctx, km))) return rc;
    m->list = idx; m->list_epoch = km->pose_epoch; m->list_valid = true;
    out->submap_rebuilt = 1;
  }
  out->m_corner = m->m_sub[0]; out->m_surf = m->m_sub[1];
  return ROLO_OK;
}

// saveKeyFramesAndFactor :1094-1221 behind its saveFrame gate; S->tf is the pose after transformUpdate and becomes the graph's estimate
int mapper_save_keyframe(rolo_mapper* m, double stamp, NodeState* S, rolo_mapper_result* out) {
  rolo_keymap* km = m->km;
  const int K = (int)km->frames.size();   // the new key
  const size_t nl = m->loopQ.size(), np = m->priorQ.size();
  int chords = 0;
  for (const std::vector<QueuedFactor>* q : {&m->loopQ, &m->priorQ})
    for (const QueuedFactor& f : *q) {
      if (f.from < 0 || f.to < 0 || f.from > K || f.to > K || f.from == f.to) { ctx_set_error("rolo_mapper_scan: a queued factor names a key that is not in the graph"); return ROLO_EINVAL; }
      if (f.from != f.to + 1 && f.to != f.from + 1) chords++;
    }
  int gN = 0;
  int rc;
  if ((rc = rolo_pgo_size(m->pgo, &gN, nullptr, nullptr))) return rc;
  if (gN != K) { ctx_set_error("rolo_mapper_scan: the borrowed graph and key map no longer hold the same number of keys"); return ROLO_ESTATE; }
  // room first: the three stores grow together or not at all
  if ((rc = keymap_reserve_keyframe(km, km->n_scan_ds[0], km->n_scan_ds[1]))) return rc;
  if (m->P.sc_input != 0 && (rc = keymap_sc_reserve(km))) return rc;
  if ((rc = pgo_reserve(m->pgo, 1, 1 + (int)(nl + np), chords))) return rc;
  // the descriptor next: a non-finite raw coordinate is found here, before anything is stored (:1183-1216; an empty cloud is skipped with a warning there)
  HIPCHK(hipEventRecord(m->ev[6], km->stream));
  int sc_index = -1;
  if (m->P.sc_input == 1 && km->n_scan_ds[1] > 0) {
    if ((sc_index = keymap_sc_add_resident(km, km->scan_ds[1], km->n_scan_ds[1])) < 0) return sc_index;
  } else if (m->P.sc_input == 2 && km->n_scan_raw > 0) {
    const float4* d = km->scan_raw; int n = km->n_scan_raw;
    if (m->P.sc_leaf > 0.f && (rc = keymap_filter_resident(km, km->scan_raw, km->n_scan_raw, m->P.sc_leaf, &d, &n))) return rc;
    if (n > 0 && (sc_index = keymap_sc_add_resident(km, d, n)) < 0) return sc_index;
  }
  // addOdomFactor :1224-1243
  double To[16], Z[16];
  T16_of_rpyxyz(S->tf, To);
  if ((rc = rolo_pgo_add_pose(m->pgo, To)) < 0) return rc;
  if (K == 0) {
    const double v[6] = {1e-2, 1e-2, M_PI * M_PI, 1e8, 1e8, 1e8};
    if ((rc = rolo_pgo_add_prior(m->pgo, 0, To, v))) return rc;
  } else {
    const double v[6] = {1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4};
    double From[16];
    T16_of_rpyxyz(km->frames[K - 1].pose, From);   // pclPointTogtsamPose3(cloudKeyPoses6D->points.back())
    T16_between(From, To, Z);
    if ((rc = rolo_pgo_add_between(m->pgo, K - 1, K, Z, v))) return rc;
  }
  // addLoopFactor :1245-1264, addPriorFactor :1266-1284
  for (const QueuedFactor& f : m->loopQ)
    if ((rc = f.k > 0.0 ? rolo_pgo_add_between_robust(m->pgo, f.from, f.to, f.T, f.var, ROLO_PGO_LOSS_CAUCHY, f.k) : rolo_pgo_add_between(m->pgo, f.from, f.to, f.T, f.var))) return rc;
  for (const QueuedFactor& f : m->priorQ)
    if ((rc = rolo_pgo_add_between(m->pgo, f.from, f.to, f.T, f.var))) return rc;
  if (nl) m->aLoopIsClosed = true;
  m->loopQ.clear(); m->priorQ.clear();
  out->loops_added = (int)nl; out->priors_added = (int)np;
  // isam->update ... calculateEstimate :1115-1137
  rolo_pgo_params lm;
  rolo_pgo_default_params(&lm);
  if ((rc = rolo_pgo_optimize(m->pgo, &lm, &out->pgo))) return rc;
  float gms[4] = {0, 0, 0, 0};
  (void)rolo_pgo_last_ms(m->pgo, gms);
  m->ms[4] = gms[0] + gms[1] + gms[2] + gms[3];
  std::vector<float> p6(6 * (size_t)(K + 1));
  if ((rc = rolo_pgo_get_poses(m->pgo, nullptr, p6.data(), K + 1)) < 0) return rc;
  std::memcpy(S->tf, p6.data() + 6 * (size_t)K, sizeof(float) * 6);   // :1141-1170: thisPose6D and transformTobeMapped from latestEstimate
  // cornerCloudKeyFrames / surfCloudKeyFrames .push_back :1173-1181, device to device
  if ((rc = keymap_append_scan(km, S->tf, stamp)) < 0) return rc;
  HIPCHK(hipEventRecord(m->ev[7], km->stream));
  out->keyframe = rc; out->sc_index = sc_index;
  // correctPoses :1287-1320
  if (m->aLoopIsClosed) {
    if ((rc = rolo_keymap_set_poses(km, p6.data(), K + 1))) return rc;
    m->aLoopIsClosed = false;
    out->poses_corrected = 1;
  }
  return ROLO_OK;
}

}  // namespace

extern "C" {

void rolo_mapper_default_params(rolo_mapper_params* p) {
  if (!p) return;
  p->mappingProcessInterval = 0.15;
  p->mappingCornerLeafSize = 0.2f; p->mappingSurfLeafSize = 0.2f;
  p->surroundingKeyframeSearchRadius = 50.0f; p->surroundingKeyframeDensity = 1.0f;
  p->surroundingkeyframeAddingDistThreshold = 1.0f; p->surroundingkeyframeAddingAngleThreshold = 0.2f;
  p->edgeFeatureMinValidNum = 10; p->surfFeatureMinValidNum = 100;
  p->z_tollerance = FLT_MAX; p->rotation_tollerance = FLT_MAX;
  p->sc_input = 1; p->sc_leaf = 0.5f;
}

int rolo_mapper_create(int device, const rolo_mapper_params* params, rolo_mapper** out) {
  if (!out) return ROLO_EINVAL;
  *out = nullptr;
  rolo_mapper_params P;
  rolo_mapper_default_params(&P);
  if (params) P = *params;
  if (!(P.mappingCornerLeafSize > 0.f) || !(P.mappingSurfLeafSize > 0.f) || !(P.surroundingKeyframeDensity > 0.f) || !(P.surroundingKeyframeSearchRadius >= 0.f) ||
      P.sc_input < 0 || P.sc_input > 2 || !(P.sc_leaf >= 0.f) || P.mappingProcessInterval != P.mappingProcessInterval) {
    ctx_set_error("rolo_mapper_create: bad parameters");
    return ROLO_EINVAL;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { ctx_set_error("no HIP device"); return ROLO_EHIP; }
  if (device < 0 || device >= ndev) return ROLO_EINVAL;
  rolo_mapper* m = new rolo_mapper();
  m->device = device; m->P = P;
  int rc = rolo_keymap_create(device, &m->km);
  if (!rc) rc = rolo_ctx_acquire(device, &m->ctx);
  if (!rc) rc = rolo_pgo_create(device, &m->pgo);
  if (!rc && hipSetDevice(device) != hipSuccess) rc = ROLO_EHIP;
  for (hipEvent_t& e : m->ev) if (!rc && hipEventCreate(&e) != hipSuccess) { ctx_set_error("rolo_mapper_create: events"); rc = ROLO_EHIP; }
  if (rc) { rolo_mapper_destroy(m); return rc; }
  *out = m;
  return ROLO_OK;
}

void rolo_mapper_destroy(rolo_mapper* m) {
  if (!m) return;
  if (m->ctx) { (void)hipSetDevice(m->device); (void)hipStreamSynchronize(ctx_stream(m->ctx)); rolo_ctx_release(m->ctx); }
  if (m->pgo) rolo_pgo_destroy(m->pgo);
  if (m->km) rolo_keymap_destroy(m->km);   // (waits for its stream and for the last reader of its sub-map)
  for (hipEvent_t e : m->ev) if (e) (void)hipEventDestroy(e);
  delete m;
}

rolo_keymap* rolo_mapper_keymap(rolo_mapper* m) { return m ? m->km : nullptr; }
rolo_pgo* rolo_mapper_pgo(rolo_mapper* m) { return m ? m->pgo : nullptr; }

int rolo_mapper_queue_loop(rolo_mapper* m, int from, int to, const double* T16, const double* var6, double cauchy_k) {
  if (!m || from < 0 || to < 0 || from == to) return ROLO_EINVAL;
  if (const int rc = check_queued(T16, var6, cauchy_k, "rolo_mapper_queue_loop")) return rc;
  QueuedFactor f{};
  f.from = from; f.to = to; f.k = cauchy_k;
  std::memcpy(f.T, T16, sizeof(f.T)); std::memcpy(f.var, var6, sizeof(f.var));
  m->loopQ.push_back(f);
  return ROLO_OK;
}

int rolo_mapper_queue_prior(rolo_mapper* m, int from, int to, const double* T16, const double* var6) {
  if (!m || from < 0 || to < 0 || from == to) return ROLO_EINVAL;
  if (const int rc = check_queued(T16, var6, 0.0, "rolo_mapper_queue_prior")) return rc;
  QueuedFactor f{};
  f.from = from; f.to = to; f.k = 0.0;
  std::memcpy(f.T, T16, sizeof(f.T)); std::memcpy(f.var, var6, sizeof(f.var));
  m->priorQ.push_back(f);
  return ROLO_OK;
}

int rolo_mapper_scan(rolo_mapper* m, double stamp, const float* corner, int n_corner, const float* surf, int n_surf, const float* raw, int n_raw, int clouds_on_device,
                     const float* initialGuess6, int odomAvailable, rolo_mapper_result* out) {
  if (!m || !out || n_corner < 0 || n_surf < 0 || n_raw < 0 || (n_corner && !corner) || (n_surf && !surf) || (odomAvailable && !initialGuess6) || stamp != stamp) return ROLO_EINVAL;
  *out = rolo_mapper_result{};
  out->keyframe = -1; out->sc_index = -1;
  // :436 — "if (timeLaserInfoCur - timeLastProcessing >= mappingProcessInterval)"
  if (!(stamp - m->st.timeLastProcessing >= m->P.mappingProcessInterval)) return ROLO_OK;
  rolo_keymap* km = m->km;
  HIPCHK(hipSetDevice(m->device));
  NodeState S = m->st;
  S.timeLastProcessing = stamp;
  const bool have_keys = !km->frames.empty();
  int rc;
  HIPCHK(hipEventRecord(m->ev[8], km->stream));
  // updateInitialGuess :516-555
  std::memcpy(S.front6, S.tf, sizeof(S.front6));
  float tf_new[6];
  if ((rc = rolo_mapper_initial_guess(S.tf, have_keys ? 1 : 0, initialGuess6, odomAvailable, S.lastOdom, &S.lastOdomAvailable, tf_new))) return rc;
  std::memcpy(S.tf, tf_new, sizeof(S.tf));
  // extractSurroundingKeyFrames :558-663
  HIPCHK(hipEventRecord(m->ev[2], km->stream));
  if (have_keys && (rc = mapper_submap(m, stamp, out))) { m->list_valid = false; return rc; }
  HIPCHK(hipEventRecord(m->ev[3], km->stream));
  // downsampleCurrentScan :666-678
  HIPCHK(hipEventRecord(m->ev[0], km->stream));
  m->have_scan = false;   // the slots are about to be overwritten; set again when this scan is through
  if ((rc = keymap_scan_downsample(km, corner, n_corner, m->P.mappingCornerLeafSize, surf, n_surf, m->P.mappingSurfLeafSize, raw, n_raw, clouds_on_device != 0))) {
    m->list_valid = false;
    return rc;
  }
  HIPCHK(hipEventRecord(m->ev[1], km->stream));
  out->n_corner_ds = km->n_scan_ds[0]; out->n_surf_ds = km->n_scan_ds[1];
  // scan2MapOptimization :681-711
  hipStream_t cs = ctx_stream(m->ctx);
  HIPCHK(hipEventRecord(m->ev[4], cs));
  if (have_keys) {
    out->s2m_ran = 1;
    rc = s2m_optimize_core(m->ctx, reinterpret_cast<const float*>(km->scan_ds[0]), km->n_scan_ds[0], reinterpret_cast<const float*>(km->scan_ds[1]), km->n_scan_ds[1], true,
                           km->scan_ready, nullptr, 0, nullptr, 0, S.tf, m->P.edgeFeatureMinValidNum, m->P.surfFeatureMinValidNum, &out->s2m, nullptr, nullptr);
    if (rc) { m->list_valid = false; return rc; }
    if (out->s2m.skipped != 1) {   // transformUpdate :1060-1068 (a sub-map too small to search, skipped = 2, is the reference's loop selecting nothing: it still runs)
      S.tf[0] = clamp_sym(S.tf[0], m->P.rotation_tollerance);
      S.tf[1] = clamp_sym(S.tf[1], m->P.rotation_tollerance);
      S.tf[5] = clamp_sym(S.tf[5], m->P.z_tollerance);
      std::memcpy(S.back6, S.tf, sizeof(S.back6));
    }
  }
  HIPCHK(hipEventRecord(m->ev[5], cs));
  // nothing can fail between here and saveKeyFramesAndFactor: the scan is accepted
  m->st = S;
  m->ms[3] = 0.f; m->ms[4] = 0.f;
  bool committed = false;
  const float* last = have_keys ? km->frames.back().pose : nullptr;
  if (rolo_mapper_save_frame(last, m->st.tf, m->P.surroundingkeyframeAddingDistThreshold, m->P.surroundingkeyframeAddingAngleThreshold) == 1) {
    NodeState S2 = m->st;
    if ((rc = mapper_save_keyframe(m, stamp, &S2, out))) { out->keyframe = -1; return rc; }
    m->st = S2;
    committed = true;
  }
  // publishOdometry :1361-1389
  if ((rc = rolo_mapper_incremental(m->st.front6, m->st.back6, m->st.tf, m->increStarted, m->incre, out->incremental6))) return rc;
  m->increStarted = 1;
  std::memcpy(out->transformTobeMapped, m->st.tf, sizeof(m->st.tf));
  std::memcpy(m->pub_tf, m->st.tf, sizeof(m->pub_tf));
  m->have_scan = true;
  out->processed = 1;
  HIPCHK(hipEventRecord(m->ev[9], km->stream));
  HIPCHK(hipEventSynchronize(m->ev[9]));
  HIPCHK(hipEventSynchronize(m->ev[5]));
  (void)hipEventElapsedTime(&m->ms[0], m->ev[0], m->ev[1]);
  (void)hipEventElapsedTime(&m->ms[1], m->ev[2], m->ev[3]);
  (void)hipEventElapsedTime(&m->ms[2], m->ev[4], m->ev[5]);
  if (committed) (void)hipEventElapsedTime(&m->ms[3], m->ev[6], m->ev[7]);
  (void)hipEventElapsedTime(&m->ms[5], m->ev[8], m->ev[9]);
  return ROLO_OK;
}

int rolo_mapper_get_scan(rolo_mapper* m, float* corner_ds, int cap_corner, float* surf_ds, int cap_surf, int* counts2) {
  if (!m || cap_corner < 0 || cap_surf < 0) return ROLO_EINVAL;
  if (!m->have_scan) { ctx_set_error("the mapper has processed no scan yet"); return ROLO_ESTATE; }
  rolo_keymap* km = m->km;
  if (counts2) { counts2[0] = km->n_scan_ds[0]; counts2[1] = km->n_scan_ds[1]; }
  float* dst[2] = {corner_ds, surf_ds};
  const int cap[2] = {cap_corner, cap_surf};
  HIPCHK(hipSetDevice(m->device));
  for (int t = 0; t < 2; t++) {
    if (!dst[t] || !km->n_scan_ds[t]) continue;
    if (km->n_scan_ds[t] > cap[t]) return ROLO_EINVAL;
    HIPCHK(hipMemcpyAsync(dst[t], km->scan_ds[t], sizeof(float4) * (size_t)km->n_scan_ds[t], hipMemcpyDeviceToHost, km->stream));
  }
  HIPCHK(hipStreamSynchronize(km->stream));
  return ROLO_OK;
}

int rolo_mapper_get_registered(rolo_mapper* m, float* out, int cap) {
  if (!m || cap < 0) return ROLO_EINVAL;
  if (!m->have_scan) { ctx_set_error("the mapper has processed no scan yet"); return ROLO_ESTATE; }
  rolo_keymap* km = m->km;
  const int n = km->n_scan_ds[0] + km->n_scan_ds[1];
  if (n > cap || (n && !out)) return ROLO_EINVAL;
  const float4* pieces[2] = {km->scan_ds[0], km->scan_ds[1]};
  if (const int rc = keymap_registered(km, pieces, km->n_scan_ds, 2, m->pub_tf, out)) return rc;
  return n;
}

int rolo_mapper_get_registered_raw(rolo_mapper* m, float* out, int cap) {
  if (!m || cap < 0) return ROLO_EINVAL;
  if (!m->have_scan) { ctx_set_error("the mapper has processed no scan yet"); return ROLO_ESTATE; }
  rolo_keymap* km = m->km;
  if (km->n_scan_raw <= 0) { ctx_set_error("rolo_mapper_get_registered_raw: the last processed scan came without a raw cloud"); return ROLO_ESTATE; }
  if (km->n_scan_raw > cap || !out) return ROLO_EINVAL;
  const float4* pieces[1] = {km->scan_raw};
  if (const int rc = keymap_registered(km, pieces, &km->n_scan_raw, 1, m->pub_tf, out)) return rc;
  return km->n_scan_raw;
}

int rolo_mapper_get_keyposes(rolo_mapper* m, float* pose6, double* times, int cap) {
  if (!m || cap < 0) return ROLO_EINVAL;
  const int n = (int)m->km->frames.size();
  for (int k = 0; k < std::min(n, cap); k++) {
    if (pose6) std::memcpy(pose6 + 6 * (size_t)k, m->km->frames[k].pose, sizeof(float) * 6);
    if (times) times[k] = m->km->frames[k].time;
  }
  return n;
}

int rolo_mapper_last_ms(rolo_mapper* m, float* ms6) {
  if (!m || !ms6) return ROLO_EINVAL;
  for (int k = 0; k < 6; k++) ms6[k] = m->ms[k];
  return ROLO_OK;
}

int rolo_mapper_initial_guess(const float* tf6_in, int have_keyposes, const float* guess6, int odomAvailable, float* lastOdom12, int* lastOdomAvailable, float* tf6_out) {
  if (!tf6_in || !tf6_out || !lastOdom12 || !lastOdomAvailable || (odomAvailable && !guess6)) return ROLO_EINVAL;
  float tf[6];
  std::memcpy(tf, tf6_in, sizeof(tf));
  if (!have_keyposes) {   // :524-531
    tf[0] = 0.f; tf[1] = 0.f; tf[2] = 0.f;
  } else if (odomAvailable) {
    const Aff transBack = aff_of_rpyxyz(guess6);   // :538-539
    if (!*lastOdomAvailable) {                   // :540-543
      std::memcpy(lastOdom12, transBack.m, 12 * sizeof(float));
      *lastOdomAvailable = 1;
    } else {                                     // :545-551
      Aff last = aff_identity();
      std::memcpy(last.m, lastOdom12, 12 * sizeof(float));
      const Aff transIncre = aff_mul(aff_inverse(last), transBack);
      const Aff transFinal = aff_mul(aff_of_rpyxyz(tf), transIncre);
      float o[6];
      xyzrpy_of(transFinal, o);
      tf[0] = o[3]; tf[1] = o[4]; tf[2] = o[5]; tf[3] = o[0]; tf[4] = o[1]; tf[5] = o[2];
      std::memcpy(lastOdom12, transBack.m, 12 * sizeof(float));
    }
  }
  std::memcpy(tf6_out, tf, sizeof(tf));
  return ROLO_OK;
}

int rolo_mapper_save_frame(const float* last_keypose6, const float* tf6, float dist_thr, float angle_thr) {
  if (!tf6) return ROLO_EINVAL;
  if (!last_keypose6) return 1;   // :1073-1074
  const Aff transBetween = aff_mul(aff_inverse(aff_of_rpyxyz(last_keypose6)), aff_of_rpyxyz(tf6));   // :1076-1080
  float o[6];
  xyzrpy_of(transBetween, o);
  if (std::fabs(o[3]) < angle_thr && std::fabs(o[4]) < angle_thr && std::fabs(o[5]) < angle_thr && std::sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]) < dist_thr) return 0;
  return 1;
}

int rolo_mapper_incremental(const float* front6, const float* back6, const float* tf6, int started, float* incre12, float* pose6_out) {
  if (!incre12 || !pose6_out || (!started && !tf6) || (started && (!front6 || !back6))) return ROLO_EINVAL;
  Aff inc;
  if (!started) {   // :1365-1369
    inc = aff_of_rpyxyz(tf6);
  } else {          // :1372-1373
    Aff cur = aff_identity();
    std::memcpy(cur.m, incre12, 12 * sizeof(float));
    inc = aff_mul(cur, aff_mul(aff_inverse(aff_of_rpyxyz(front6)), aff_of_rpyxyz(back6)));
  }
  std::memcpy(incre12, inc.m, 12 * sizeof(float));
  xyzrpy_of(inc, pose6_out);
  return ROLO_OK;
}

}  // extern "C"
