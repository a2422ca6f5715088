/* rolo_hip.h — C ABI of librolo_hip.so, the MI355X-native (gfx950, HIP) implementation of sdwyc/ROLO's
 * per-frame scan-matching hot path. This is the drop-in boundary: plain pointers and sizes, no C++/torch
 * types. Every entry point names the reference interface it replaces (paths relative to the ROLO repository).
 *
 * Operator API replaced: fast_gicp::RotVGICP<pcl::PointXYZI, pcl::PointXYZI> of librot_gicp.so
 *   (include/rot_gicp/gicp/rot_vgicp.hpp:72-104, include/rot_gicp/gicp/lsq_registration.hpp:51-62), as driven by
 *   LidarOdometry::scanRegeistration (src/lidarOdometry.cpp:460-494).
 * Node cores replaced: ImageProjection::projectPointCloud/cloudExtraction (src/imageProjection.cpp:399-505),
 *   FeatureExtraction::calculateSmoothness/markOccludedPoints/extractFeatures (src/featureExtraction.cpp:87-266),
 *   LidarOdometry::cloudHandler (src/lidarOdometry.cpp:503-570).
 *
 * All functions return 0 on success or a negative ROLO_E* code; nothing throws or aborts. A context is
 * single-threaded (like one RotVGICP instance); several contexts may run concurrently on one device.
 * Host pointers unless the name ends in _device. Matrices are row-major.
 */
#ifndef ROLO_HIP_H
#define ROLO_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ROLO_OK 0
#define ROLO_EINVAL (-1)        /* bad argument */
#define ROLO_ETOOFEW (-2)       /* cloud has fewer than k points (reference: FLANN clamps k -> UB) */
#define ROLO_ENOCORR (-4)       /* empty correspondence set (reference: H = 0 -> NaN) */
#define ROLO_ESTATE (-5)        /* call order: a prerequisite stage has not run */
#define ROLO_EHIP (-6)          /* HIP runtime error; see rolo_last_error() */
#define ROLO_EUNSUPPORTED (-7)  /* option of the reference API that this build does not implement */
#define ROLO_EALIAS (-8)        /* reference: std::invalid_argument, rot_vgicp_impl.hpp:150-152 */
#define ROLO_ECOMM (-9)         /* RCCL error */
#define ROLO_EKEYRANGE (-10)    /* voxel coordinate outside +-2^20 (packed 3x21-bit key) */
#define ROLO_ENONFINITE (-11)   /* a non-finite point / covariance (degenerate neighbourhood) reached the voxel map's fixed-point sums. DEVIATION from the
                                   reference, on purpose: vmp_voxel.hpp:169-196 carries the NaN into that ONE voxel and on into H (a degraded or NaN pose, no
                                   error); this library fails the frame with this code instead of returning a finite but wrong pose. When a frame holds
                                   both this and ROLO_EKEYRANGE, this (more negative) code is reported. */

/* enum orders follow include/rot_gicp/gicp/gicp_settings.hpp:6-13 and lsq_registration.hpp:13 */
enum { ROLO_REG_NONE = 0, ROLO_REG_MIN_EIG, ROLO_REG_NORMALIZED_MIN_EIG, ROLO_REG_PLANE, ROLO_REG_FROBENIUS, ROLO_REG_PLANE_S };
enum { ROLO_DIRECT27 = 0, ROLO_DIRECT7, ROLO_DIRECT1 };
enum { ROLO_VOXEL_POLAR = 0, ROLO_VOXEL_UNIFORM };
enum { ROLO_OPT_GN = 0, ROLO_OPT_LM, ROLO_OPT_SO3_LM };

typedef struct rolo_params {
  int k_correspondences;         /* setCorrespondenceRandomness, rot_vgicp_impl.hpp:92-94 (20) */
  int regularization;            /* setRegularizationMethod :97-99 (PLANE) */
  int neighbor_search;           /* setNeighborSearchMethod :58-60 (DIRECT1) */
  int voxel_type;                /* setResolution -> UNIFORM :44-48 ; setPolarResolution -> POLAR :51-55 */
  double voxel_resolution;       /* setResolution (1.0) */
  double polar_resolution[3];    /* setPolarResolution(theta, phi, r); ctor leaves (1,0,0) */
  int optimizer;                 /* setOptimizerType, lsq_registration_impl.hpp:337-340 (SO3_LM) */
  int max_iterations;            /* pcl::Registration::setMaximumIterations; lsq ctor :11 (64) */
  double rotation_epsilon;       /* setRotationEpsilon :30-32 (2e-3) */
  double transformation_epsilon; /* pcl::Registration::setTransformationEpsilon; lsq ctor :13 (5e-4) */
  int lm_max_iterations;         /* lsq ctor :18 (10) */
  double lm_init_lambda_factor;  /* setInitialLambdaFactor :35-37 (1e-9) */
  int fixed_iterations;          /* harness knob: >0 runs exactly this many outer iterations of align() */
  int q2_intended;               /* 0 as written, 1 intended continuous-time term */
  int overlap_knn;               /* tuning knob (default 1): source and target go through ONE chain of search launches (every
                                    kernel works on the pair) instead of one chain per cloud — both searches start together */
  int use_graph;                 /* tuning knob (default 1): rolo_register_async captures the frame's fixed launch schedule in a
                                    hipGraph on the second frame with unchanged sizes / buffers / parameters and replays it */
  int fused_lm;                  /* how the LM chain of a registration is launched (tuning knob, results equal to rounding):
                                    0 = a pass launch + a controller launch per LM trial (rounds 1-5's default: ~60 launches per frame, predicated on the device state);
                                    1 = ONE launch per LM trial (the controller runs in the prologue of the next pass, in every workgroup): the shortest chain of rounds 1-5 for
                                        one frame at a time (the odometry driver turns it on), slower with several contexts in flight (-22 % with four);
                                    2 = ONE launch per FRAME (round 6, the default): 64 (other contexts' frames in flight) ... 256 (idle device) workgroups stay resident for the
                                        whole chain of both stages and exchange their rows through self-validating words between the trials (lm_persist.hip lm_persist_kernel) — no
                                        kernel boundary inside the chain, no schedule that can fall short. Spin-waits are bounded: a launch that cannot get all its workgroups
                                        onto the chip within ROLO_LM_PERSIST_ADMIT_US (1000) leaves the stage untouched and the frame is finished as with 0
                                        (rolo_ctx_counters[12]); a later poll longer than ROLO_LM_PERSIST_TIMEOUT_MS (200) ends the frame with ROLO_ECOMM.
                                        Ranks that share a frame (rolo_peer_*, rolo_comm_*) always run as with 0: their sums cross the exchange between pass and controller */
} rolo_params;

typedef struct rolo_stats {
  int n_outer;        /* outer iterations run (nr_iterations_ + 1) */
  int converged;      /* pcl::Registration::hasConverged() */
  int lm_failed;      /* "lm not converged!!" (lsq_registration_impl.hpp:66-69,168-171); result still returned */
  int n_passes;       /* fused linearize/error passes over the source points */
  int n_correspondences;
  int n_cost_only;    /* of n_passes: passes that evaluated a trial's cost alone (compute_error / compute_t_error without the linearisation half) — counted on the device */
} rolo_stats;

typedef struct rolo_trace_rec { /* one LM trial; lm_debug_print_ table of lsq_registration_impl.hpp:299-305 */
  int stage, outer, trial, accepted; /* accepted: 1 yes, 0 no, 2 rejected-but-converged */
  double y0, yi, rho, lambda, dnorm;
} rolo_trace_rec;

typedef struct rolo_ctx rolo_ctx;

const char* rolo_last_error(void);
int rolo_device_count(void);

/* RotVGICP() / ~RotVGICP(): rot_vgicp_impl.hpp:20-42. `device` = HIP device ordinal. */
int rolo_ctx_create(int device, rolo_ctx** out);
void rolo_ctx_destroy(rolo_ctx* ctx);
/* The same for callers that construct one operator PER FRAME, as the reference does (src/lidarOdometry.cpp:460 — `RotVGICP rot_vgicp;` inside
 * scanRegeistration): rolo_ctx_release parks the context (streams, events, pinned and device buffers, the captured hipGraph of a frame) in a
 * small per-process pool after resetting everything a fresh object would not have — parameters back to the defaults, no clouds, no
 * covariances, no map, no correspondences — and rolo_ctx_acquire hands a parked context of that device out again (or creates one). The C++
 * drop-in class (include/rot_vgicp_hip.hpp) constructs / destructs through this pair, so lidarOdometry.cpp:460-494 runs unchanged WITHOUT a
 * hipMalloc per frame. rolo_ctx_pool_clear destroys what is parked (call before process exit if the HIP runtime should see every free). */
int rolo_ctx_acquire(int device, rolo_ctx** out);
void rolo_ctx_release(rolo_ctx* ctx);
void rolo_ctx_pool_clear(void);
void rolo_default_params(rolo_params* p);
int rolo_set_params(rolo_ctx* ctx, const rolo_params* p);
/* the HIP stream all work of this context is enqueued on (hipStream_t as void*), for event timing */
void* rolo_ctx_stream(rolo_ctx* ctx);

/* setInputTarget / setInputSource (rot_vgicp_impl.hpp:133-143 / :112-120): n records of `stride` floats with
 * x,y,z at float offsets 0,1,2 (pcl::PointXYZI: stride 8). The cloud is copied to the device; cached
 * covariances, voxel map and correspondences are dropped, as in the reference. */
int rolo_set_target(rolo_ctx* ctx, const float* pts, int n, int stride);
int rolo_set_source(rolo_ctx* ctx, const float* pts, int n, int stride);
int rolo_set_target_device(rolo_ctx* ctx, const float* d_pts, int n, int stride);
int rolo_set_source_device(rolo_ctx* ctx, const float* d_pts, int n, int stride);
/* swapSourceAndTarget :69-77, clearSource :102-105, clearTarget :107-110 */
int rolo_swap_source_and_target(rolo_ctx* ctx);
/* The source cloud is the previous target moved by a pure translation (LidarOdometry::stateLinearPropagation zeroes
 * the rotation, lidarOdometry.cpp:707): its covariances are those of the target up to the float rounding of the moved
 * points, so take them over instead of searching again. Call after rolo_set_source*, before rolo_set_target*.
 * Not what the reference does (it recomputes both, :460-466): results differ at the 1e-7 relative level of the
 * covariances; the drop-in default leaves it off. ROLO_ESTATE unless the target holds covariances and n matches. */
int rolo_adopt_target_covariances(rolo_ctx* ctx);
int rolo_clear_source(rolo_ctx* ctx);
int rolo_clear_target(rolo_ctx* ctx);

/* calculate_covariances :421-496 for whichever of source/target has none. */
int rolo_compute_covariances(rolo_ctx* ctx);
/* getSourceCovariances / getTargetCovariances (rot_vgicp.hpp:91-97): n x 16 doubles (Matrix4d, row-major). */
int rolo_get_source_covariances(rolo_ctx* ctx, double* covs);
int rolo_get_target_covariances(rolo_ctx* ctx, double* covs);
/* setSourceCovariances / setTargetCovariances :122-130 */
int rolo_set_source_covariances(rolo_ctx* ctx, const double* covs);
int rolo_set_target_covariances(rolo_ctx* ctx, const double* covs);
/* debug: the k nearest neighbours (indices, squared float distances) of every source / target point */
int rolo_get_knn(rolo_ctx* ctx, int which /*0 source, 1 target*/, int32_t* idx, float* d2);

/* VmfVoxelMap::create_voxelmap (vmp_voxel.hpp:167-197) on the target. */
int rolo_build_voxelmap(rolo_ctx* ctx);
int rolo_num_voxels(rolo_ctx* ctx);
/* target points of the last map build whose POLAR voxel coordinate lies within 1e-12 (in bins) of a bin edge — the only place where the
 * device's atan2 / acos (ulps away from glibc's) could put a point into a different voxel than the reference's CPU does. The synthetic
 * scans of the tests hold a few (the azimuth wrap, atan2(y, x) + pi ~ 1e-16); their keys are checked against the CPU path like all others.
 * UNIFORM keys are correctly rounded on both sides: always 0. */
int rolo_num_edge_points(rolo_ctx* ctx);
/* keys V x 3, counts V, means V x 4, covs V x 16 — voxel order is unspecified (match on keys). */
int rolo_get_voxels(rolo_ctx* ctx, int32_t* keys, int32_t* counts, double* means, double* covs);
/* polar_coord / voxel_coord (vmp_voxel.hpp:199-211) of the target points (n x 3). */
int rolo_get_target_voxel_keys(rolo_ctx* ctx, int32_t* keys);

/* so3_linearize :293-388 / linearize :225-290 (update_correspondences :173-222 fused in), compute_error :391-417.
 * T row-major 4x4. H/b may be NULL. */
int rolo_so3_linearize(rolo_ctx* ctx, const double* T, double* H9, double* b3, double* err);
int rolo_linearize(rolo_ctx* ctx, const double* T, double* H36, double* b6, double* err);
int rolo_compute_error(rolo_ctx* ctx, const double* T, double* err);
/* voxel_correspondences_ of the last linearize: per source point the 3-int key of its voxel, or found[i] = 0. */
int rolo_get_correspondences(rolo_ctx* ctx, int32_t* found /* n_src * n_offsets */, int32_t* keys /* n_src * n_offsets * 3 */);
/* t3_linearize :499-607 / compute_t_error :610-658 on the correspondences cached by the last linearize. */
int rolo_t3_linearize(rolo_ctx* ctx, const double* t3, const double* init_guess3, const double* last_t03,
                      double dtn, double dtn1, float ct_lambda, double* H36, double* b6, double* err);
int rolo_compute_t_error(rolo_ctx* ctx, const double* t3, const double* init_guess3, const double* last_t03,
                         double dtn, double dtn1, float ct_lambda, double* err);

/* pcl::Registration::align(out, guess) -> RotVGICP::computeTransformation :146-160 -> LsqRegistration::
 * computeTransformation (lsq_registration_impl.hpp:152-179). guess16 NULL = Identity. T_out_f16 =
 * getFinalTransformation() (float); T_out_d16 (optional) the double pose it was cast from. The transformed source the
 * reference also writes (pcl::transformPointCloud into `output`) is rolo_transform_cloud with T_out_f16. */
int rolo_align(rolo_ctx* ctx, const float* guess16, float* T_out_f16, double* T_out_d16, rolo_stats* stats);
/* RotVGICP::computeTranslation :163-169 -> lsq :55-80. trans3_io: in = start value, out = result. */
int rolo_compute_translation(rolo_ctx* ctx, double* trans3_io, const double* init_guess3, const double* last_t03,
                             double dtn, double dtn1, float ct_lambda, rolo_stats* stats);
/* Both stages back to back with no host synchronisation in between (scanRegeistration :460-500 as one enqueue).
 * rolo_register_async only enqueues; rolo_register_wait blocks and fetches results. */
int rolo_register_async(rolo_ctx* ctx, const float* guess16, const double* trans3_start, const double* init_guess3,
                        const double* last_t03, double dtn, double dtn1, float ct_lambda);
int rolo_register_wait(rolo_ctx* ctx, float* T_out_f16, double* T_out_d16, double* trans3_out,
                       rolo_stats* rot_stats, rolo_stats* trans_stats);
/* Batches of independent scan pairs (BASELINE config 5 — the reference would loop scanRegeistration over them).
 * A batch owns n member contexts that share one HIP stream; the caller configures every member through the normal
 * API (rolo_set_params, rolo_set_source/_target[_device]) and then registers all of them with ONE call: the members'
 * neighbourhood searches and voxel maps are enqueued back to back and their LM chains run as batched launches (one
 * pass / controller launch per trial for the whole batch), replayed from a hipGraph when nothing changed. Array
 * arguments hold one entry per member (guess16: n x 16 or NULL, vectors: n x 3). Members must share the optimizer
 * and fixed_iterations settings. */
typedef struct rolo_batch rolo_batch;
int rolo_batch_create(int device, int n_members, rolo_batch** out);
void rolo_batch_destroy(rolo_batch* b);
int rolo_batch_size(rolo_batch* b);
rolo_ctx* rolo_batch_member(rolo_batch* b, int i); /* owned by the batch: do not destroy */
int rolo_batch_register_async(rolo_batch* b, const float* guess16, const double* trans3_start, const double* init_guess3,
                              const double* last_t03, double dtn, double dtn1, float ct_lambda);
int rolo_batch_register_wait(rolo_batch* b, float* T_out_f16, double* T_out_d16, double* trans3_out, rolo_stats* rot_stats,
                             rolo_stats* trans_stats);
/* getFinalHessian (lsq_registration_impl.hpp:45-47): 6x6, Identity until a 6-dof LM step accepts */
int rolo_get_final_hessian(rolo_ctx* ctx, double* H36);
int rolo_get_trace(rolo_ctx* ctx, rolo_trace_rec* out, int cap); /* returns the number of records */

/* pcl::transformPointCloud float path used at lidarOdometry.cpp:459,492 and lsq_registration_impl.hpp:78,178 */
int rolo_transform_cloud(rolo_ctx* ctx, const float* in, float* out, int n, int stride, const float* T16);

/* Multi-GPU point sharding: every rank holds the full clouds; rank r evaluates source points
 * [r*n/W, (r+1)*n/W) in the passes and the per-pass sums are all-reduced (fp64, <= 32 values) with RCCL on the
 * context's stream. K5 shards by query point: each rank searches 1/W of the Morton-sorted queries and the 48-byte covariances are
 * all-gathered once per cloud and frame (ncclAllGather). unique_id = the 128-byte ncclUniqueId created by rank 0
 * (rolo_comm_unique_id) and distributed by the caller (e.g. torch.distributed broadcast). */
/* the slice of n source points rank r of `world` evaluates: [n*r/world, n*(r+1)/world) */
void rolo_shard_range(int n, int rank, int world, int* begin, int* end);
/* test hook: shard the passes WITHOUT a communicator — sums returned by the stage-level calls are then partial */
int rolo_set_shard(rolo_ctx* ctx, int rank, int world);
/* test hook: with rolo_set_shard and no communicator, also shard K5 (calculate_covariances, rot_vgicp_impl.hpp:430-496) by query point
 * as a communicator does — every rank sorts the whole cloud, searches only its slice of the Morton-sorted queries (whole 256-query
 * workgroups, equal slices) — but WITHOUT the all-gather: only the covariances of the own slice are valid afterwards (the rest of
 * rolo_get_*_covariances is stale / undefined); the union over the ranks must equal the unsharded result. */
int rolo_set_shard_knn(rolo_ctx* ctx, int on);
/* test hook: the LM drivers of lsq_registration_impl.hpp:55-179, 225-324 — the controller kernels of passes.hip — fed with SCRIPTED pass results instead of pass
 * kernels: the linearisation opened by outer iteration o returns lin_*[o], the trial cost of (o, trial t) returns err_y[o][t] (indices beyond the extents repeat the
 * last entry); slots of a pass row that the step must not read are poisoned with NaN. Every exit of the drivers (LM failure, iteration cap, rejected-but-converged,
 * NaN / infinite gain ratios, the cost-only passes' late linearisation) can be reached with inputs that are the same bits as a CPU statement's.
 * rolo_debug_lm_script_align: computeTransformation from `guess16` with the context's parameters; generic_ctrl != 0 runs the one-size-fits-all controller of the
 * batched launches instead of the specialised one. rolo_debug_lm_script_translation: computeTranslation afterwards (it needs the correspondence count the
 * rotation script left, as the reference's does). Results as rolo_align / rolo_compute_translation; rolo_get_trace reads the trace. */
typedef struct rolo_lm_script {
  int n_outer, n_trial;
  const double* lin_y;    /* [n_outer] */
  const double* lin_H;    /* [n_outer][36] row-major 6 x 6; a 3-dof optimiser reads the top-left 3 x 3 */
  const double* lin_b;    /* [n_outer][6] */
  const int32_t* lin_n;   /* [n_outer] correspondences of that linearisation */
  const double* err_y;    /* [n_outer][n_trial] */
} rolo_lm_script;
int rolo_debug_lm_script_align(rolo_ctx* ctx, const rolo_lm_script* script, const float* guess16, int generic_ctrl, float* T_out_f16, double* T_out_d16, rolo_stats* stats);
int rolo_debug_lm_script_translation(rolo_ctx* ctx, const rolo_lm_script* script, double* trans3_io, const double* init_guess3, const double* last_t03,
                                     double dtn, double dtn1, float ct_lambda, int generic_ctrl, rolo_stats* stats);
/* Which kernels rolo_register_async picks where the best one depends on whether the GPU is shared (not in the reference: its operator owns its CPU threads).
 * -1 (default): decided per frame — other contexts of the device have frames in flight when this one is enqueued => the kernels that share the chip best
 * (throughput); an idle device => the ones that finish soonest (latency). 0 / 1 pin the idle- / busy-device choice (profiling runs, callers that know their
 * load). It selects the neighbour search of large launches — 64-query packets (busy) or two lanes per query (idle): the same lists, bit for bit — and, since round 6, the
 * size of the resident LM kernel (fused_lm = 2: 64 workgroups busy, 256 idle): the sums of a pass then run over other groups of points and poses agree to rounding
 * (1e-12), not bit for bit. A caller that needs run-to-run identical bits under changing load pins the hint (or sets fused_lm = 0). */
int rolo_set_load_hint(rolo_ctx* ctx, int mode);
int rolo_comm_unique_id(void* unique_id128);
int rolo_comm_init(rolo_ctx* ctx, const void* unique_id128, int rank, int world);
int rolo_comm_destroy(rolo_ctx* ctx);
/* rank and size read back from the RCCL communicator itself (ncclCommUserRank / ncclCommCount); world = 0 without one */
int rolo_comm_info(rolo_ctx* ctx, int* rank, int* world);

/* The same exchange WITHOUT a collective library ("every GPU peer-writes its partial into a slot on each peer, fixed-rank-
 * order local sum"): every rank exports one device allocation (its "mailbox": slots for the 32 fp64 sums of an LM pass + the covariance
 * exchange area), the ranks swap the 64-byte handles by any means (torch.distributed all_gather, a file, a pipe), and connect. From then on
 *   - the LM controller kernel of every trial writes its shard's sums into its slot of EVERY rank's mailbox and adds all slots of its own
 *     mailbox in rank order (bit-identical on every rank): no reduce launch, no library call, one launch per trial as on one GPU, and the
 *     frame's launch schedule stays hipGraph-capturable;
 *   - K5's covariances of the own query slice are copied into every peer's exchange area by a kernel (replaces ncclAllGather).
 * Handles come from hipIpcGetMemHandle (processes of one node; HSA_ENABLE_IPC_MODE_LEGACY=0 on this driver); contexts of ONE process
 * (several GPUs driven by one process, or two contexts on one device) are recognised and use each other's pointers directly. A rank that
 * does not answer within ROLO_PEER_TIMEOUT_MS (default 10 000) makes the waiting ranks end the registration with ROLO_ECOMM — a lost peer
 * never hangs the GPU. world <= 8 (one node). max_points >= source + target points of the largest frame (sizes the covariance area).
 * Mutually exclusive with rolo_comm_init (RCCL), which stays as the A/B. Reference loop that is split over the GPUs:
 * rot_vgicp_impl.hpp:313-382 (the per-thread Hs / bs / sum_errors of so3_linearize summed at :377-382). */
#define ROLO_PEER_HANDLE_BYTES 64
int rolo_peer_export(rolo_ctx* ctx, int world, int max_points, void* handle64);
int rolo_peer_connect(rolo_ctx* ctx, const void* handles /* world x 64 bytes, rank order */, int rank, int world);
int rolo_peer_disconnect(rolo_ctx* ctx);
/* Collective self-test of a connected group, to be run by EVERY rank (same reps) before the first frame: `reps` all-reduces of 32 known fp64
 * through the LM mailboxes and one covariance-segment push of known words into every peer's exchange area, verified on every rank. us_out[0] =
 * mean microseconds of one LM exchange launch (first one excluded), us_out[1] = microseconds of the covariance exchange (push + flags + wait).
 * ROLO_ECOMM with a message naming the rank and the words that were wrong or missing — the first crossing of a new transport (hipIpc mapping,
 * peer access, fine-grained memory over xGMI) fails here and not as a wrong pose inside a frame. */
int rolo_peer_selftest(rolo_ctx* ctx, int reps, double* us_out /* [2], optional */);
/* rank / world of the connection (world 0: none); mem_kind16 (optional, 16 chars): "finegrained" | "coarse" */
int rolo_peer_info(rolo_ctx* ctx, int* rank, int* world, char* mem_kind16);

/* Bookkeeping of rolo_register_async / _wait on this context since its creation (what bench.py reports next to the throughput):
 * out[0] frames registered, [1] of them replayed from the hipGraph, [2] captured, [3] enqueued eagerly, [4] frames whose first launch
 * schedule was too short (rolo_register_wait had to top up with host round trips), [5] synchronous chunks of predicated passes enqueued
 * by the drivers (top-ups + rolo_align / rolo_compute_translation), [6] / [7] passes the next frame's first schedule holds per stage, [8] lanes per query
 * of the last neighbour search enqueued (1: 64-query packets, 2 / 4: knn_walk_sub_kernel — picked by launch size, ROLO_KNN_SUB overrides),
 * [9] nanoseconds of HOST time spent inside rolo_register_async (graph launch / capture / eager enqueue) since the context was created or recycled,
 * [10] nanoseconds the host was blocked in rolo_register_wait's hipEventSynchronize, [11] nanoseconds of the rest of rolo_register_wait (std::chrono::steady_clock;
 * bench.py's host_enqueue_us_per_frame — round 5's verdict, item 2a), [12] frames whose resident LM kernel (fused_lm = 2) could not get all its workgroups onto the chip within its
 * admission time and gave the stage back to the host, which finished it with pass + controller launches, [13] what the context has LEARNED about load it cannot count (another
 * process on the GPU): 0 = its frames last what they last alone (idle-device kernels), 1 = trying the busy-device kernels, 2 = keeping them (rolo_set_load_hint -1 only),
 * [14] "kept_trials": rotation-stage trials, summed over the frames, that cost no pass — with fixed_iterations > 0 a converged-but-rejected trial repeats unchanged until the
 * iterations are used up, and the step answers the repeats from the cost it holds (ROLO_LM_KEEP_COST=0: every repeat is a pass again). rolo_stats::n_passes / n_cost_only and
 * the LM trace keep counting the solve's trials, these included,
 * [15] "model_trials": translation-stage trials, summed over the frames and the rolo_compute_translation calls, that cost no pass — within that stage a trial's cost is a
 * quadratic in the translation whose coefficients are in the sums of the stage's own linearisation, and the step answers the trials from it, asking for a pass only to
 * linearise again after an accepted trial (ROLO_LM_TRANS_MODEL=0: every trial is a pass again; the costs then differ in their last bits, the decisions do not). Counted
 * in n_passes / n_cost_only and traced like [14]. */
int rolo_ctx_counters(rolo_ctx* ctx, long long* out, int n);
/* the form of the context's last resident LM launch (fused_lm = 2, one launch per frame): out[0] workgroups, [1] threads per workgroup, [2] points per thread,
 * [3] points per thread of the interleaved body (1, 2, 4; 0: the generic body, one point after the other), [4] points of a thread that go through a body together,
 * [5] 1 if the Mahalanobis cache sits in LDS, [6] dynamic LDS in bytes. All zero if the last LM chain of the context did not use the resident kernel. */
int rolo_ctx_lm_form(rolo_ctx* ctx, int* out, int n);
/* test hook: how the context's current voxel map was built — host-side facts, kept where the build is enqueued (a frame replayed from its hipGraph reports what its capture
 * baked in). out[0] the form: the map's own launches behind rolo_build_voxelmap and the stage-level evaluations, over the target in input order (STAGED_INPUT) or in the
 * order of the search's curve (STAGED_CURVE: chosen from the points per voxel of the context's previous map, before there is one for the POLAR grid); inside the
 * launches of the target's neighbour search (SEARCH: rolo_align / rolo_register_async on a target without covariances); the staged launches as a frame or a batch member
 * enqueues them behind a search that had finished before, or was not needed (FRAME). out[1] 1: the covariance sums are fixed point too, 0: fp64 atomics (handed-in
 * covariances, unbounded regularisations). out[2] where max |coordinate|, which sets the fixed-point scale, came from: 0 the search's bounding box, 1 the points
 * themselves (no search ran on this target). out[3] slots of the hash table. ROLO_ESTATE without a map. */
#define ROLO_VOXBUILD_STAGED_INPUT 0
#define ROLO_VOXBUILD_STAGED_CURVE 1
#define ROLO_VOXBUILD_SEARCH 2
#define ROLO_VOXBUILD_FRAME 3
int rolo_debug_voxel_build(rolo_ctx* ctx, int32_t out[4]);
/* test hook: the source covariances' PLANE short form, C_A = I - m m^T, as the passes would read it: m (n x 3, row per point), m.x NaN where the neighbourhood's
 * SVD did not leave that form (the passes then read the point's six entries). n must be the source's size. ROLO_ESTATE when the passes would not read the form at all:
 * a regularisation other than PLANE, handed-in covariances, ROLO_PASS_NRM=0, or covariances not computed. */
int rolo_debug_source_plane_form(rolo_ctx* ctx, double* m /* n x 3 */, int n);
/* device buffer (re)allocations made so far by the registration contexts of this process (every hipMalloc behind a rolo_ctx's buffers; a captured hipGraph is keyed on it):
 * a steady-state frame loop must stop moving it */
long long rolo_alloc_count(void);
/* experiment hook (profiles/tools/concurrency.py, round 5's verdict item 2b): enqueue `reps` replays of a captured chain of `n_pairs` launch PAIRS on the context's stream —
 * kind 0: empty kernels shaped like a controller (1 workgroup); 1: empty kernels shaped like a pass (`grid` workgroups of 256); 2: empty pass + empty controller
 * alternating (the LM chain's boundaries and dispatches without its instructions or traffic); 3: the context's REAL LM chain (frame begin + predicated pass / controller
 * pairs as rolo_register_async enqueues them, on the map and clouds of its last registration); 4: the real passes without the controller (every launch linearises at
 * the start pose). Asynchronous: synchronise through rolo_ctx_stream. */
int rolo_debug_chain(rolo_ctx* ctx, int kind, int n_pairs, int grid, int reps);

/* Per-kernel timing with HIP events on the context's stream (bench.py's "roofline" object). While enabled, every
 * launch of the listed kernels is bracketed by an event pair; rolo_prof_read synchronises the stream and returns
 * the durations (ms) of one slot in launch order, then forgets them. Returns the number of launches recorded. */
enum { ROLO_PROF_KNN_BUILD = 0, ROLO_PROF_KNN_WALK, ROLO_PROF_VOXEL_BUILD, ROLO_PROF_ROT_PASS, ROLO_PROF_TRANS_PASS, ROLO_PROF_CTRL, ROLO_PROF_KNN_TAIL, ROLO_PROF_LM_PASS /* fused trial: controller prologue + pass */, ROLO_PROF_N };
int rolo_prof_enable(rolo_ctx* ctx, int on);
int rolo_prof_read(rolo_ctx* ctx, int slot, float* ms, int cap);

/* ---- front end ------------------------------------------------------------------------------------------ */
typedef struct rolo_front_params {
  int n_scan, horizon_scan, downsample_rate;       /* include/rolo/utility.h:310-312 */
  float lidar_min_range, lidar_max_range;          /* :313-314 */
  float edge_threshold, surf_threshold;            /* :318-319 */
  float odometry_surf_leaf_size;                   /* :323 */
} rolo_front_params;
void rolo_front_default_params(rolo_front_params* p); /* config/params.yaml values */

/* ImageProjection::projectPointCloud + cloudExtraction (src/imageProjection.cpp:399-505), deskew off.
 * in: n_raw points (x,y,z at float offsets 0..2 of `stride`-float records) + ring[n_raw].
 * out (host, sized n_scan*horizon_scan): extracted[N*4] (x,y,z,intensity), point_col_ind[N], point_range[N],
 * start_ring[n_scan], end_ring[n_scan]; range_mat (optional) n_scan*horizon_scan. *n_valid = N.
 * The column of a point is the reference's expression (:437-444) on the CORRECTLY ROUNDED float atan2(x, y), i.e. the column a CPU run with a correctly
 * rounded libm gives: like the POLAR voxel key (rolo_num_edge_points above), a point within a guard of a column edge — where one ulp of the device's atan2f
 * is the neighbouring pixel — has its angle taken again in fp64. glibc 2.35's atan2f is itself not correctly rounded on about a quarter (27-28 %) of
 * the points planted one ulp from a column edge in tests/projection_cases.py; only on such points can the column differ by one from that CPU's. */
int rolo_project_frame(rolo_ctx* ctx, const rolo_front_params* P, const float* pts, int stride, const uint16_t* ring,
                       int n_raw, float* extracted, int32_t* point_col_ind, float* point_range, int32_t* start_ring,
                       int32_t* end_ring, float* range_mat, int* n_valid);
/* ImageProjection::deskewPoint (src/imageProjection.cpp:368-396; deskewCloudInfo :266-366 prepares its inputs): rotation-only
 * de-skew of every stored point by the front-end odometry increment over the scan, `rolo/deskewEnabled` (off in every
 * shipped config). Arms the NEXT rolo_project_frame / rolo_odom_submit on this context: rel_time[i] = fabs(point.time) of
 * raw point i (what :358-359 stores), odom_incre_rpy = odomIncreRoll/Pitch/Yaw, odom_time_diff = odomTimeDiff (:349-351; rolo_odom_increment does
 * the pose algebra). rel_time == NULL: the times come from the time field of the next message (rolo_odom_submit_msg) or, for
 * points without one (timeFlag == -1), are interpolated from the azimuth as deskewCloudInfo does (:270-327). Range, pixel and every
 * index still come from the raw point, as in the reference (:412-454). */
typedef struct rolo_deskew { int enabled; float odom_incre_rpy[3]; float scan_period; double odom_time_diff; } rolo_deskew;
int rolo_front_set_deskew(rolo_ctx* ctx, const rolo_deskew* d, const float* rel_time, int n_raw, int rel_time_on_device);
/* lidarOdomAffineFront.inverse() * lidarOdomAffineBack -> pcl::getTranslationAndEulerAngles (:345-351); poses and increment as
 * x, y, z, roll, pitch, yaw (float) */
void rolo_odom_increment(const float* front6, const float* back6, float* incre6);
/* Eigen::Affine3f::rotation() of the row-major 4x4 T — what `Rotation = transformation_interpolated.rotation().cast<double>()` reads
 * (src/lidarOdometry.cpp:474, :548; TransformFusion::affineToPose :130). For an Affine (not Isometry) transform this is
 * computeRotationScaling(): JacobiSVD<Matrix3f> of the linear part in float, U V^T with the determinant sign fix — the polar factor, which
 * differs from the linear part in the last float ulps. Host code (the pose chain of the odometry driver uses it); R9 row-major. */
void rolo_affine3f_rotation(const float* T16, float* R9);
/* The input of FeatureExtraction::laserCloudInfoHandler (src/featureExtraction.cpp:71-85) when that node runs as its own process: the arrays
 * of the received rolo/cloud_info — extracted[n_valid*4] = fromROSMsg(cloud_projected) as x, y, z, intensity; pointColInd, pointRange
 * (first n_valid entries), startRingIndex / endRingIndex [n_scan] — go where rolo_project_frame would have left them on the device;
 * rolo_extract_features then runs as usual. The index arrays are used as array indices on the device, so a malformed message is ROLO_EINVAL:
 * start / end indices that are not the running counts of n_valid points, a ring of more than Horizon_SCAN points, a column outside the image. */
int rolo_front_load_projection(rolo_ctx* ctx, const rolo_front_params* P, const float* extracted, const int32_t* point_col_ind,
                               const float* point_range, const int32_t* start_ring, const int32_t* end_ring, int n_valid);
/* FeatureExtraction::calculateSmoothness + markOccludedPoints + extractFeatures (src/featureExtraction.cpp:87-266)
 * on the arrays rolo_project_frame left on the device (call order: project, then extract).
 * out (host): corner[nc*4], surface[ns*4] (sized for N points each); optional curvature/picked/label [N]. */
int rolo_extract_features(rolo_ctx* ctx, const rolo_front_params* P, float* corner, int* n_corner, float* surface,
                          int* n_surface, float* curvature, int32_t* neighbor_picked, int32_t* label);
/* Test hook: which way the last rolo_extract_features on `ctx` made the greedy corner / surface picks of every ring — out[n_scan], one
 * word per ring, n_scan as in the parameters of the rolo_project_frame / rolo_front_load_projection it ran on. The choice depends on the data only
 * (ring population, thresholds, position of the ring in the cloud, number of corner picks), never on the result.
 *   bits 1..0, the ring:       ROLO_XPATH_RING_NONE     the whole-ring fixed point (all twelve pick stages at once) was not attempted
 *                              ROLO_XPATH_RING_CAPPED   attempted and discarded: a sector had more than 20 corner picks, the ring was redone stage by stage
 *                              ROLO_XPATH_RING_APPLIED  attempted and applied; every sector field below is ROLO_XPATH_SECTOR_NOT_STAGED
 *   bits 3+2j..2+2j, sector j = 0..5 of a ring that went stage by stage:
 *                              ROLO_XPATH_SECTOR_EMPTY     skipped (sp >= ep)
 *                              ROLO_XPATH_SECTOR_PARALLEL  corner and surface picks as parallel fixed points
 *                              ROLO_XPATH_SECTOR_SERIAL    the reference's serial walk on one lane
 * A build with -DROLO_XT_STAGED never attempts the whole-ring fixed point: the ring field is always ROLO_XPATH_RING_NONE.
 * ROLO_ESTATE if no extraction has run since the last projection or load, ROLO_EINVAL if n_scan is not that projection's. */
enum { ROLO_XPATH_RING_NONE = 0, ROLO_XPATH_RING_CAPPED = 1, ROLO_XPATH_RING_APPLIED = 2 };
enum { ROLO_XPATH_SECTOR_NOT_STAGED = 0, ROLO_XPATH_SECTOR_EMPTY = 1, ROLO_XPATH_SECTOR_PARALLEL = 2, ROLO_XPATH_SECTOR_SERIAL = 3 };
int rolo_debug_extract_paths(rolo_ctx* ctx, int32_t* out, int n_scan);
/* test hook: the per-point times (seconds, n = the number of raw points) that the last projection on this context de-skewed with — the caller's
 * (rolo_front_set_deskew), fabs(time) of the message, or the ones interpolated from the azimuth (deskewCloudInfo's timeFlag == -1 branch,
 * imageProjection.cpp:270-327) — and in *first_passed (may be NULL) the index of the point that set halfPassed in that branch: INT_MAX if no point did or
 * the times did not come from the azimuth. Times handed over as a device pointer are read through that pointer. ROLO_ESTATE if the last projection was not
 * de-skewed, ROLO_EINVAL if n is not its number of raw points. */
int rolo_debug_front_times(rolo_ctx* ctx, float* out, int n, int32_t* first_passed);

/* ---- per-frame odometry driver -------------------------------------------------------------------------------
 * LidarOdometry (src/lidarOdometry.cpp:325-713) between fromROSMsg and publish, on feature clouds (n x 4 floats:
 * x, y, z, intensity). The driver keeps the node's state (previous features, LaserOdomPose, the last step for
 * the forward prediction) and runs both registration stages on `ctx`, whose registration parameters
 * (setPolarResolution(0.175, 0.175, 2.0) in the reference, :462) the caller sets with rolo_set_params. */
typedef struct rolo_odom rolo_odom;
int rolo_odom_create(rolo_ctx* ctx, float ct_lambda /* rolo/continuousTrajectoryWeight */, rolo_odom** out);
void rolo_odom_destroy(rolo_odom* o);
/* odometryHandler :440-446 — the back end's rolo/mapping/odometry; scan matching is gated on it (:537-541) */
int rolo_odom_backend_odometry(rolo_odom* o, double stamp);
/* cloudHandler :503-570. Returns 0 = first frame stored, 1 = gated (pose propagated, no registration),
 * 2 = registered; <0 error. pose6 = LaserOdomPose (x, y, z, roll, pitch, yaw) as published on
 * odomTopic+"_incremental"; rot9 / trans3 = Rotation / Translation of the frame-to-frame step. */
int rolo_odom_cloud(rolo_odom* o, double stamp, const float* corner, int n_corner, const float* surface, int n_surface,
                    float* pose6, double* rot9, double* trans3);
/* The three node cores fused, device-resident: raw frame (ImageProjection::cloudHandler input, imageProjection.cpp:151)
 * -> projection -> features -> cloudHandler of LidarOdometry, without the CloudInfoStamp hops: the feature clouds, the
 * propagated previous features and both registration inputs never leave HBM; the host sees three counts mid-frame
 * and the pose at the end. Same results and return codes as rolo_project_frame + rolo_extract_features +
 * rolo_odom_cloud. pts/ring may be device pointers (pts_on_device != 0). counts3 (optional) = N, n_corner, n_surface. */
int rolo_odom_frame(rolo_odom* o, const rolo_front_params* P, double stamp, const float* pts, int stride, const uint16_t* ring,
                    int n_raw, int pts_on_device, float* pose6, double* rot9, double* trans3, int* counts3);
/* The same in two halves, for throughput: rolo_odom_submit enqueues K1-K4 of a frame on the driver's own front-end
 * stream and returns at once; rolo_odom_collect finishes the oldest submitted frame (waits for its features, registers,
 * updates the pose). Up to two frames may be in flight, so the features of frame k+1 are extracted while frame k
 * registers — the overlap the reference gets from running its three nodes as separate processes. With host input the
 * caller must keep pts / ring valid until the matching collect. rolo_odom_frame = submit + collect. */
int rolo_odom_submit(rolo_odom* o, const rolo_front_params* P, double stamp, const float* pts, int stride, const uint16_t* ring,
                     int n_raw, int pts_on_device);
int rolo_odom_collect(rolo_odom* o, float* pose6, double* rot9, double* trans3, int* counts3);
/* The same from the message itself: `data` is the payload of the sensor_msgs/PointCloud2 that ImageProjection::cloudHandler
 * receives (n_points records of layout->point_step bytes), `layout` the byte offsets of the fields the node reads — what
 * pcl::moveFromROSMsg and the Ouster conversion loop of cachePointCloud (imageProjection.cpp:188-212) do on the host runs as a
 * kernel: x, y, z (FLOAT32), ring (UINT16 for Velodyne, UINT8 for Ouster), time (time_kind 1: Velodyne "time", FLOAT32 seconds;
 * 2: Ouster "t", UINT32 nanoseconds, * 1e-9f; 0: none). A de-skew armed without times (rolo_odom_set_deskew with rel_time =
 * NULL) takes fabs(time) of this message, or the azimuth-interpolated times when the message has no time field. */
typedef struct rolo_cloud_layout { int point_step, off_x, off_y, off_z, off_ring, ring_bytes, off_time, time_kind; } rolo_cloud_layout;
int rolo_odom_submit_msg(rolo_odom* o, const rolo_front_params* P, double stamp, const uint8_t* data, const rolo_cloud_layout* layout,
                         int n_points, int data_on_device);
/* The feature clouds of the last collected frame of the fused path, for the outgoing rolo/CloudInfoStamp (extracted_corner ++
 * extracted_surface as n x 4 floats: x, y, z, intensity; corners first). features may be NULL to query the counts. */
int rolo_odom_get_features(rolo_odom* o, float* features, int cap_points, int* n_corner, int* n_surface);
/* options of the fused path: ROLO_ODOM_REUSE_COVARIANCES (default 0) = rolo_adopt_target_covariances between frames */
#define ROLO_ODOM_REUSE_COVARIANCES 1
/* ROLO_ODOM_FUSED_LM (default 2; values 0 / 1 / 2 = rolo_params.fused_lm): how the driver's registrations launch their LM chain — it registers one frame at a
 * time, where the shortest chain wins: one launch per frame since round 6 (one launch per trial, 1, through round 5). The driver asserts the option on its context right
 * before each registration it enqueues; it does not depend on, and is not reverted by, the parameter block the caller hands to rolo_set_params. */
#define ROLO_ODOM_FUSED_LM 2
/* ROLO_ODOM_EARLY_SOURCE (default 0): when a frame is submitted with nothing else in flight (rolo_odom_frame, or submit / collect one frame at
 * a time), the propagated previous features — the SOURCE of the coming registration, known at submit time — are moved and searched on the
 * registration stream while K1-K4 of the new frame run on the front-end stream; collect searches the target alone. Same results (the search
 * of a cloud does not depend on what it is launched with), but MEASURED SLOWER on MI355X: the search of a 48 k-point cloud lasts as long
 * as its heaviest packets, alone nearly as long as together with the other cloud — two chains cost 0.68 ms per frame against 0.58 ms for the
 * pair chain after K1-K4. Kept as an A/B (env ROLO_ODOM_EARLY_SOURCE=1 arms it in every driver). */
#define ROLO_ODOM_EARLY_SOURCE 3
int rolo_odom_set_option(rolo_odom* o, int option, int value);
/* rolo_front_set_deskew for the next rolo_odom_submit / rolo_odom_frame of the fused path */
int rolo_odom_set_deskew(rolo_odom* o, const rolo_deskew* d, const float* rel_time, int n_raw, int rel_time_on_device);

/* ---- back end: scan-to-submap optimisation ---------------------------------------------------------------------
 * scan2MapOptimization (src/backMapping.cpp:681-711) with cornerOptimization :720-824, surfOptimization :827-901,
 * combineOptimizationCoeffs :904-925 and LMOptimization :929-1058: the down-sampled corner / surface points of the current scan
 * (laserCloudCornerLastDS / laserCloudSurfLastDS, n x 4 floats) against the corner / surface sub-maps (laserCloud*FromMapDS), starting
 * from and updating transformTobeMapped = (roll, pitch, yaw, x, y, z). Up to 30 Gauss-Newton iterations, each one kernel over the points
 * (exact 5-NN in the sub-map's BVH, line / plane fit, Jacobian row, J^T J reduction) and a 6 x 6 float solve on the host.
 * edge_min / surf_min = edgeFeatureMinValidNum / surfFeatureMinValidNum (utility.h: 10 / 100): with fewer features the call does nothing
 * (stats->skipped = 1); a sub-map with fewer than five points cannot answer the 5-NN association: also nothing (stats->skipped = 2). The context's source / target clouds are used as scratch for the sub-map trees: use a context of its own.
 * transformUpdate()'s clamps (:1060-1068; tolerances FLT_MAX in every shipped config) are left to the caller.
 * selected_out[n_corner + n_surf] / coeff_out[(n_corner + n_surf) * 4] (optional): laserCloudOri*Flag and coeffSel of the LAST iteration. */
typedef struct rolo_scan2map_stats { int skipped, iterations, converged, degenerate, n_selected; } rolo_scan2map_stats;
/* kdtreeCornerFromMap / kdtreeSurfFromMap ->setInputCloud (:690-691) as a call of its own: uploads the sub-map and builds its two search trees once; they stay
 * resident in the context until the next call. rolo_scan2map_optimize with map_corner = map_surf = NULL then registers against the resident sub-map (the
 * surrounding key-frame set changes every few scans, not every scan). */
int rolo_scan2map_set_submap(rolo_ctx* ctx, const float* map_corner, int m_corner, const float* map_surf, int m_surf);
int rolo_scan2map_optimize(rolo_ctx* ctx, const float* corner, int n_corner, const float* surf, int n_surf, const float* map_corner, int m_corner,
                           const float* map_surf, int m_surf, float* transformTobeMapped6, int edge_min, int surf_min, rolo_scan2map_stats* stats,
                           unsigned char* selected_out, float* coeff_out);

/* ---- back end: device-resident key frames and sub-map assembly ---------------------------------------------------------------------
 * What the back end does before scan2MapOptimization, on the device: the key frames' corner / surface clouds (n x 4 floats: x, y, z, intensity) and their
 * poses (transformTobeMapped order: roll, pitch, yaw, x, y, z) stay in a rolo_keymap; rolo_keymap_extract fuses the listed ones into the two sub-maps
 * (transformPointCloud + pcl::VoxelGrid) and rolo_scan2map_set_submap_keymap hands them to the registration without a host round trip.
 * The voxel filter is bit-identical to pcl::VoxelGrid<PointXYZI> as the oracle states it (cells in ascending index order, each centroid's float sums
 * taken serially in point order); a cloud of up to ROLO_KEYMAP_MAX_POINTS points per call; "leaf size too small" (more than INT32_MAX cells) copies the
 * input through as PCL does; a non-finite coordinate is ROLO_ENONFINITE. transformPointCloud evaluates each row as T0 x + (T1 y + (T2 z + T3)) in float
 * without contraction — the order of the oracle's orc_transform_cloud_f (PCL's own transformPointCloud), which the tests hold it to; src/backMapping.cpp:314-316
 * writes the same sum left to right, which can differ in the last bit of a coordinate.
 * A key map is single-threaded like a context and works on a stream of its own; its store and scratch only grow until rolo_keymap_destroy. */
#define ROLO_KEYMAP_MAX_POINTS (1 << 26)   /* largest cloud one filter call / one fused sub-map cloud may hold (67 108 864 points) */
typedef struct rolo_keymap rolo_keymap;
int rolo_keymap_create(int device, rolo_keymap** out);
void rolo_keymap_destroy(rolo_keymap* km);
/* saveKeyFramesAndFactor (src/backMapping.cpp:1140-1181): cornerCloudKeyFrames / surfCloudKeyFrames .push_back and cloudKeyPoses6D.push_back; returns the key frame's index (>= 0) */
int rolo_keymap_add_keyframe(rolo_keymap* km, const float* corner, int n_corner, const float* surf, int n_surf, const float* pose6, double time);
/* correctPoses (:1301-1314): a key frame's pose after a graph update; the next extraction uses it (nothing transformed is cached) */
int rolo_keymap_set_pose(rolo_keymap* km, int index, const float* pose6);
int rolo_keymap_size(rolo_keymap* km);
/* extractNearby (:575-614) with extractCloud's range filter (:626), host only (no device needed): the key frames extractCloud would fuse, in its order.
 * xyz: n x 3 key-pose positions, times: their stamps. Radius search around the LAST pose (squared float distance below search_radius^2, ordered by
 * (distance, index)), VoxelGrid at `density` on those poses, each down-sampled pose re-indexed to its nearest key pose (lowest index on ties), then from the
 * newest backwards every pose with time_cur - time < recent_seconds (10.0 in the reference); entries whose listed position (the centroid, for down-sampled
 * ones) is farther than search_radius from the last pose are dropped. Returns the number of entries (duplicates are possible and meant) and writes the
 * first min(count, cap) of them. Parity unpinned: the strict "<" and the (distance, index) tie order restate FLANN's radius result set from its source as
 * remembered, not from a recorded vector. */
int rolo_keyposes_select_nearby(const float* xyz, const double* times, int n, float search_radius, float density, double time_cur, double recent_seconds,
                                int32_t* out_indices, int cap);
/* extractCloud (:617-658): for the listed key frames in list order (a duplicate's clouds go in twice), *transformPointCloud (:301-320) of the corner and
 * the surface cloud, concatenated, downSizeFilterCorner / downSizeFilterSurf (mappingCornerLeafSize 0.2 / mappingSurfLeafSize 0.4). The two sub-maps stay
 * on the device; m_corner / m_surf receive their sizes. */
int rolo_keymap_extract(rolo_keymap* km, const int32_t* indices, int n, float corner_leaf, float surf_leaf, int* m_corner, int* m_surf);
/* download of the last extraction's sub-maps (laserCloudCornerFromMapDS / laserCloudSurfFromMapDS); caps in points */
int rolo_keymap_get_submap(rolo_keymap* km, float* corner_out, int cap_corner, float* surf_out, int cap_surf);
/* downsampleCurrentScan (:666-678) for one cloud, also usable alone: out holds up to n points, *m receives the count */
int rolo_keymap_downsample(rolo_keymap* km, const float* pts, int n, float leaf, float* out, int* m);
/* kdtree*FromMap->setInputCloud (:690-691) without the host round trip: rolo_scan2map_set_submap on the key map's last extraction (same device) */
int rolo_scan2map_set_submap_keymap(rolo_ctx* ctx, rolo_keymap* km);

/* ---- back end: Scan Context place recognition from the resident key frames ------------------------------------------------------------
 * SCManager (src/scancontext/Scancontext.cpp, include/scancontext/Scancontext.h) as the back end uses it: saveKeyFramesAndFactor (src/backMapping.cpp:1183-1216)
 * turns every key frame into a descriptor, performSCLoopClosure (:2399-2479) asks for a loop candidate and a yaw offset. The descriptors live in the key map,
 * on its stream and under its rules (the store only grows, nothing is freed before rolo_keymap_destroy). Per descriptor: the num_ring x num_sector matrix of
 * maximum heights (float values, as the reference's MatrixXd only widens them), the fp64 column norms, the sector key (column means, fp64) and the ring key (row
 * means, fp64 rounded to float as eig2stdvec :62-66 does).
 * The arithmetic is the reference's statement by statement (rolo_amd/csrc/scancontext.hip lists it); every sum is taken serially in index order.
 * Parity unpinned, stated once: the order in which Eigen's norm(), mean() and dot() add; the order in which the kd-tree returns keys at equal distance (here
 * the lower index first; the candidate SET is the exact K nearest, which nanoflann's tree also returns); which atan overload the reference's build selects
 * for xy2theta's float quotient (here the fp64 one, correctly rounded). The tests hold the kernels bit for bit to the numpy statement tests/sc_twin.py.
 * Limits (ROLO_EINVAL): num_ring * num_sector <= ROLO_SC_MAX_BINS (the bins and the query's matrix sit in one workgroup's LDS), num_sector <=
 * ROLO_SC_MAX_SECTORS, num_candidates <= ROLO_SC_MAX_CANDIDATES or 0 = every searched descriptor is a candidate (the exhaustive form of the original paper,
 * with search_ratio = 1.0 for all shifts). A zero maximum height is stored as +0.0. */
#define ROLO_SC_MAX_BINS 4096
#define ROLO_SC_MAX_SECTORS 1024
#define ROLO_SC_MAX_CANDIDATES 64
typedef struct rolo_sc_params { int num_ring, num_sector; double max_radius, lidar_height;
                                int num_exclude_recent, num_candidates; double search_ratio, dist_thres; } rolo_sc_params;
/* Scancontext.h:80-95: PC_NUM_RING 20, PC_NUM_SECTOR 60, PC_MAX_RADIUS 80.0, LIDAR_HEIGHT 2.0, NUM_EXCLUDE_RECENT 30, NUM_CANDIDATES_FROM_TREE 3,
 * SEARCH_RATIO 0.1, SC_DIST_THRES 0.4; host only (no device needed). num_exclude_recent is carried for the caller (ScanContextManager); the library does not read it. */
void rolo_sc_default_params(rolo_sc_params* p);
/* the geometry (num_ring, num_sector, max_radius, lidar_height) can change only while no descriptor is stored (ROLO_ESTATE otherwise;
 * arrays an earlier, failed add has sized for the old geometry are retired); the rest at any time */
int rolo_keymap_sc_set_params(rolo_keymap* km, const rolo_sc_params* p);
/* the parameters in force (the defaults before the first rolo_keymap_sc_set_params): what sizes rolo_keymap_sc_get's outputs */
int rolo_keymap_sc_get_params(rolo_keymap* km, rolo_sc_params* out);
/* makeAndSaveScancontextAndKeys (:236-250) with makeScancontext :151-195 and the two keys :198-227; both return the new descriptor's index (>= 0). A non-finite
 * coordinate is ROLO_ENONFINITE and an empty cloud ROLO_EINVAL (the reference skips it with a warning): nothing is stored.
 * scInputType scan_feat (src/backMapping.cpp:1213): the key frame's RESIDENT surface cloud, device to device */
int rolo_keymap_sc_add_surface(rolo_keymap* km, int keyframe);
/* scInputType scan_raw (:1186-1196): n x 4 floats from the host; leaf > 0: downSizeFilterSC (0.5) first, on the device with the key map's voxel filter, no
 * round trip; leaf = 0: the cloud as it is */
int rolo_keymap_sc_add_cloud(rolo_keymap* km, const float* pts, int n, float leaf);
int rolo_keymap_sc_size(rolo_keymap* km);
/* download of one descriptor, each part optional: desc[num_ring * num_sector] ring-major (desc[r * num_sector + s], the reference's desc(r, s)),
 * ringkey[num_ring], sectorkey[num_sector], colnorm[num_sector] */
int rolo_keymap_sc_get(rolo_keymap* km, int index, double* desc, float* ringkey, double* sectorkey, double* colnorm);
/* detectLoopClosureID (:253-344) for descriptor `query` against descriptors 0 .. n_search - 1. The caller passes n_search because the reference searches a stale
 * set: its tree is rebuilt every TREE_MAKING_PERIOD_ = 10 calls from all keys but the newest NUM_EXCLUDE_RECENT (:263-282). n_search <= 0 is the early return
 * (loop_id -1, yaw 0). Candidates: the min(num_candidates, n_search) smallest float squared ring-key distances (nanoflann.hpp:383-408: groups of four, left to
 * right), ascending by (distance, index). Per candidate distanceBtnScanContext :116-148: the sector-key alignment over all shifts (first strict minimum), the
 * window of round(0.5 * search_ratio * num_sector) shifts either side of it modulo num_sector, each shift once in ascending order, and the column-wise cosine
 * distance at each (columns with a zero norm on either side not counted; none counted: NaN, never a minimum, so the pair keeps 10 000 000 and shift 0).
 * nn_idx / nn_align / min_dist: the first strict minimum in candidate order (:302-317); loop_id = nn_idx if min_dist < dist_thres, else -1; yaw_diff_rad =
 * deg2rad(nn_align * 360.0 / num_sector) with the reference's float / double mix (:17-20, :339).
 * cand_idx / cand_dist / cand_align (optional, cap entries each): the first min(n_candidates, cap) candidates in candidate order. */
typedef struct rolo_sc_result { int loop_id; float yaw_diff_rad; int nn_idx, nn_align; double min_dist; int n_candidates; } rolo_sc_result;
int rolo_keymap_sc_detect(rolo_keymap* km, int query, int n_search, rolo_sc_result* out, int32_t* cand_idx, double* cand_dist, int32_t* cand_align, int cap);
/* device time of the last rolo_keymap_sc_add_* / rolo_keymap_sc_detect call in milliseconds, between two events on the key map's stream (profiles/tools/sc_time.py) */
float rolo_keymap_sc_last_ms(rolo_keymap* km);

/* ---- back end: loop-closure ICP from the resident key frames ----------------------------------------------------------------------------
 * performRSLoopClosure / performSCLoopClosure (src/backMapping.cpp:2307-2479) without the factor graph: two clouds built from key frames
 * (loopFindNearKeyframes[WithRespectTo] :2572-2624) are aligned with pcl::IterativeClosestPoint as the reference configures it (SVD estimation, no rejectors,
 * no RANSAC) and accepted or rejected on getFitnessScore. PCL is not in the reference tree: the contract is this statement (tests/icp_twin.py restates it in
 * numpy; parity with a PCL build is unpinned).
 *   setup      the source is moved by the guess (each row T0 x + (T1 y + (T2 z + T3)) in float, no contraction; NULL or the identity: not at all), the target gets
 *              the neighbour search's curve-sorted implicit BVH, the moved source is sorted along the same curve once and stays on the device
 *   iteration  every source point's exact nearest target point in float, d2 = ((dx dx) + (dy dy)) + (dz dz) with dx = source - target, ties to the smallest
 *              target index; the pair is kept when (double)d2 <= max_correspondence_distance^2. Over the kept pairs n, sum d2, sum p, sum q and sum p q^T in fp64,
 *              per workgroup and then over the workgroups in a fixed order (no floating-point atomics: the same bits on every run).
 *              n < min_correspondences: state NO_CORRESPONDENCES, not converged, stop. Otherwise Umeyama without scaling in double on the host:
 *              Sigma = sum q p^T / n - mean(q) mean(p)^T, Sigma = U S V^T, R = U diag(1, 1, s) V^T with s = -1 when det U det V < 0 (for a rank-2 Sigma this is
 *              Eigen's rank rule), t = mean(q) - R mean(p); the increment is rounded to float, the moved source is multiplied by it in float (PCL's
 *              progressive form) and final = increment * final in float (each entry a0 b0 + a1 b1 + a2 b2 + a3 b3, left to right).
 *   exit       in this order, with the count of finished iterations: iterations >= max_iterations -> ITERATIONS; cos = 0.5 (tr R - 1) >= rot_thr and |t|^2 <=
 *              transformation_epsilon (R, t of the float increment, in double; rot_thr = rotation_epsilon if > 0, else 1 - transformation_epsilon) -> TRANSFORM;
 *              mse = sum d2 / n < 1e-12 -> ABS_MSE; |mse - prev| / prev < euclidean_fitness_epsilon -> REL_MSE; else prev = mse (prev starts at DBL_MAX).
 *   fitness    getFitnessScore(): one more association of the moved source without a cap; the mean of d2 over the pairs (DBL_MAX without one). */
#define ROLO_ICP_NOT_CONVERGED 0
#define ROLO_ICP_ITERATIONS 1
#define ROLO_ICP_TRANSFORM 2
#define ROLO_ICP_ABS_MSE 3
#define ROLO_ICP_REL_MSE 4
#define ROLO_ICP_NO_CORRESPONDENCES 5
typedef struct rolo_loopicp_params { int max_iterations; double transformation_epsilon, euclidean_fitness_epsilon, rotation_epsilon /* <= 0: not given */;
                                     double max_correspondence_distance; int min_correspondences; } rolo_loopicp_params;
typedef struct rolo_loopicp_result { float T[16]; double fitness; int converged, iterations, state, n_source, n_target, n_last; } rolo_loopicp_result;
/* one association of an alignment: the kept pairs, their mean d2, the 17 sums (n, sum d2, sum p [3], sum q [3], sum p q^T [9] row-major) and the float increment
 * estimated from them (zeros where the alignment stopped before estimating) */
typedef struct rolo_loopicp_trace_rec { int n; double mse; double sums[17]; float increment[16]; } rolo_loopicp_trace_rec;
/* 100 iterations, transformation epsilon 1e-6, fitness epsilon 1e-6 (:2343-2345, :2432-2434), no rotation epsilon, min_correspondences 3; the cap
 * (setMaxCorrespondenceDistance) is the caller's: 2 * historyKeyframeSearchRadius or 150 m in the reference, +infinity here */
void rolo_loopicp_default_params(rolo_loopicp_params* p);
/* loopFindNearKeyframes (wrt_key < 0) / loopFindNearKeyframesWithRespectTo (wrt_key >= 0) into the key map's resident loop cloud `slot` (0: source, 1: target):
 * for keyNear = key - search_num .. key + search_num inside the store, the corner and then the surface cloud of keyNear moved by keyNear's own pose (by wrt_key's
 * pose in the second form), all concatenated in that order, then ONE pcl::VoxelGrid of `leaf` (downSizeFilterICP, mappingSurfLeafSize) over the whole cloud.
 * *m receives the size; 0 is a valid result (an empty store, empty frames). key or a non-negative wrt_key outside the store is ROLO_EINVAL (an empty store
 * takes any key). The clouds stay on the device under the key map's rules: its stream, buffers that only grow. */
int rolo_keymap_loop_cloud(rolo_keymap* km, int slot, int key, int search_num, int wrt_key, float leaf, int* m);
int rolo_keymap_get_loop_cloud(rolo_keymap* km, int slot, float* out, int cap);
/* detectLoopClosureDistance (:2481-2515), host only: radius search around the LAST key pose under rolo_keyposes_select_nearby's rule (squared float distance below
 * radius^2, ascending by (distance, index)); the first hit with |time - time_cur| > time_diff is the candidate. *loop_key_pre receives its index, or -1 when no
 * hit qualifies or the candidate is the last key itself (the "already has a loop" map stays with the caller). */
int rolo_keyposes_detect_loop_distance(const float* xyz, const double* times, int n, float search_radius, double time_diff, double time_cur, int32_t* loop_key_pre);
/* icp.align + getFitnessScore on the key map's two loop clouds (slot 0 onto slot 1); guess16: row-major 4 x 4 or NULL. An empty cloud gives state NO_CORRESPONDENCES.
 * The tree and the walk run in a registration context the key map takes from the pool (rolo_ctx_acquire) and keeps until rolo_keymap_destroy. */
int rolo_keymap_loop_icp(rolo_keymap* km, const rolo_loopicp_params* params, const float* guess16, rolo_loopicp_result* out);
/* the same on two host clouds (n x 4 floats) in a caller's context, whose source / target clouds it overwrites */
int rolo_loopicp_align(rolo_ctx* ctx, const float* source, int n_source, const float* target, int n_target, const rolo_loopicp_params* params, const float* guess16,
                       rolo_loopicp_result* out);
/* the associations of the last alignment in order, the fitness pass last; returns their number and writes the first min(number, cap) */
int rolo_loopicp_get_trace(rolo_ctx* ctx, rolo_loopicp_trace_rec* out, int cap);
int rolo_keymap_loop_trace(rolo_keymap* km, rolo_loopicp_trace_rec* out, int cap);
/* test hook: one association of T16 * source (NULL: source as it is) against target; per source point the target index and d2, or -1 and +infinity beyond the cap */
int rolo_loopicp_associate(rolo_ctx* ctx, const float* source, int n_source, const float* target, int n_target, const float* T16, double max_correspondence_distance,
                           int32_t* index_out, float* d2_out);
/* device time of the last alignment in milliseconds between HIP events: ms4[0] set-up (guess, sort, tree), [1] all iterations, [2] the fitness pass, [3] the whole call;
 * rolo_keymap_loop_last_ms adds ms6[4] / ms6[5]: the last rolo_keymap_loop_cloud of slot 0 / slot 1 */
int rolo_loopicp_last_ms(rolo_ctx* ctx, float* ms4);
int rolo_keymap_loop_last_ms(rolo_keymap* km, float* ms6);
/* The ground-prior association's form (performPriorAssociation, :1943-2158: one ICP per stored patch against the same ground cloud): B sources against ONE target.
 * sources holds the clouds one after another (n_source[b] points of 4 floats each), guess16 B row-major 4 x 4 matrices or NULL, out B results. out[b] and
 * candidate b's trace are those of rolo_loopicp_align(source b, target, params, guess b), bit for bit: the same sort and 256-point workgroups per candidate, the
 * same sums in the same order, the same host step. What differs is the schedule: every candidate's association runs in one launch per iteration, the increment
 * of the previous iteration is applied when that launch loads a point, and the host is waited for once per iteration for all candidates; a candidate that has left
 * the loop gets its fitness pass in the next launch and rests after it. Launches: the largest iteration count + 1, not the sum.
 * B <= ROLO_LOOPICP_MAX_BATCH; the target and the sum of the sources are each at most ROLO_KEYMAP_MAX_POINTS. B == 0 is ROLO_OK and touches nothing; an empty
 * source, or an empty target, gives that candidate NO_CORRESPONDENCES. Null pointers, a negative count or sizes past the limits are ROLO_EINVAL. */
#define ROLO_LOOPICP_MAX_BATCH 256
int rolo_loopicp_align_batch(rolo_ctx* ctx, const float* sources, const int* n_source, int B, const float* target, int n_target, const rolo_loopicp_params* params,
                             const float* guess16_or_null, rolo_loopicp_result* out);
/* candidate b's associations of the last batch call, as rolo_loopicp_get_trace; b outside the last batch is ROLO_EINVAL */
int rolo_loopicp_get_trace_batch(rolo_ctx* ctx, int b, rolo_loopicp_trace_rec* out, int cap);
/* device time of the last batch call in milliseconds between HIP events: ms4[0] set-up (guesses, sorts, tree, tables), [1] all iterations with the fitness passes,
 * [2] 0, [3] the whole call */
int rolo_loopicp_batch_last_ms(rolo_ctx* ctx, float* ms4);

/* ---- back end: the global map (publishGlobalMap, src/backMapping.cpp:1611-1665; saveGlobalPCDs' cloudGlobal.pcd, :1546-1557) --------------------------
 * rolo_keymap_global_map: for every listed key frame, in list order and with repeats, its corner and then its surface cloud moved by the frame's current pose
 * (rolo_keymap_loop_cloud's statement), all concatenated, then ONE pcl::VoxelGrid of `leaf` (:1660-1663). The concatenation may hold up to 2^31 - 1 points: past
 * ROLO_KEYMAP_MAX_POINTS it never exists as a whole. A list of at most `batch` points (rolo_keymap_global_set_batch) goes through the filter of
 * rolo_keymap_extract in one piece (the one-shot form); a longer one is worked through in batches of exactly `batch` points, cut wherever that falls, each sorted
 * by cell and merged into a table of (cell, running sums, count) kept in cell order (the streamed form). A cell's sums are continued from batch to batch in
 * concatenation order, never split into partial sums: both forms return the bits of the filter over the whole cloud. Differences between the forms: PCL's "leaf
 * size is too small" (copy-through in the one-shot form) is ROLO_EINVAL in the streamed form, whose answer would be the whole input; a table that cannot be
 * grown is ROLO_EHIP ("hipMalloc failed"). The map stays on the device in a slot of its own; working memory follows the batch and the number of cells. */
int rolo_keymap_global_map(rolo_keymap* km, const int32_t* indices, int n, float leaf, int* m);
/* the last global map (n x 4 floats) into out; returns its size. ROLO_ESTATE before the first rolo_keymap_global_map, ROLO_EINVAL if cap is too small */
int rolo_keymap_get_global_map(rolo_keymap* km, float* out, int cap);
/* points per batch, 1 .. ROLO_KEYMAP_MAX_POINTS; 0: the default (ROLO_KEYMAP_GLOBAL_BATCH). For callers short of device memory, and for the tests */
#define ROLO_KEYMAP_GLOBAL_BATCH (1 << 24)
int rolo_keymap_global_set_batch(rolo_keymap* km, int points);
/* of the last rolo_keymap_global_map, the first min(n, 5) of: input points, batches, cells, the form (0 one-shot, 1 streamed), the largest table size (cells) */
int rolo_keymap_global_info(rolo_keymap* km, long long* out, int n);
/* device time of the last rolo_keymap_global_map in milliseconds between HIP events: ms3[0] the box pass (one-shot: transform + box), [1] the sort + merge
 * pass (one-shot: the filter), [2] the finish (one-shot: 0) */
int rolo_keymap_global_last_ms(rolo_keymap* km, float* ms3);
/* cloudGlobal.pcd's cloud (:1546-1557): the same concatenation unfiltered, batch by batch through the device into out (cap points of 4 floats on the host); nothing
 * of the list's size lives on the device. Returns the number of points, or an error code; ROLO_EINVAL if cap is smaller */
long long rolo_keymap_global_cloud(rolo_keymap* km, const int32_t* indices, int n, float* out, long long cap);

/* ---- back end: pose-graph optimisation for the loop closures ----------------------------------------------------------------------------
 * saveKeyFramesAndFactor / addOdomFactor / addLoopFactor / addPriorFactor / correctPoses (src/backMapping.cpp:1094-1320) as a BATCH minimiser of the objective
 * the reference hands to iSAM2, built from the same factors and the same noise models. GTSAM is not in the reference tree and iSAM2 is incremental: this is not a
 * restatement of it, and parity with GTSAM is unpinned. The contract is this statement; tests/pgo_twin.py restates it in numpy.
 *   poses      X_k = (R_k, t_k), fp64 everywhere; T16 is a row-major 4 x 4 double matrix (its last row is not read)
 *   factors    prior(i, Z, var6): e = Log(Z^-1 X_i); between(i, j, Z, var6): e = Log(Z^-1 X_i^-1 X_j), i != j in either order. Log is the full SE(3) logarithm,
 *              tangent order [omega, v] (rotation first, as GTSAM's Pose3), coefficient series below an angle of 1e-2; an angle within 1e-6 of pi is outside the
 *              statement. var6: variances in that order (noiseModel::Diagonal::Variances). Objective 1/2 sum |e / sigma|^2.
 *   loss       a between factor may carry a Cauchy loss with constant k > 0, as performSCLoopClosure adds its loop (noiseModel::Robust::Create(
 *              mEstimator::Cauchy::Create(1.0), Diagonal::Variances(v6)), :2464-2470). With e_w = e / sigma and r^2 = |e_w|^2 its cost term is
 *              rho = k^2 / 2 log1p(r^2 / k^2) in place of r^2 / 2 and its weight w = k^2 / (k^2 + r^2): mEstimator::Cauchy::loss and ::weight at distance r.
 *              In the linearisation the whitened error and both whitened Jacobians are scaled by sqrt(w) before the products, as
 *              noiseModel::Robust::WhitenSystem does: the factor's blocks are w J^T J and its gradient parts w J^T e_w, the exact gradient of rho. The outer loop
 *              is unchanged: accept, reject and convergence read the robust cost. w > 0 always, so H + lambda I keeps its definiteness rule. A factor without
 *              loss is computed as before, and a graph without a robust factor gives the results it gave. Priors carry no loss, and Cauchy is the only
 *              M-estimator (the reference configures no other). tests/pgo_robust_twin.py restates this in numpy; parity with GTSAM is unpinned here too.
 *   linearise  retraction X <- X Exp(delta); J_j = Jr^-1(e), J_i = -Jr^-1(e) Ad((X_i^-1 X_j)^-1), prior J_i = Jr^-1(e), with Jr^-1 by its series
 *              I + ad/2 + ad^2/12 - ad^4/720; rows whitened by 1 / sigma. H and g are summed per pose over its factors in factor order (no atomics).
 *   step       (H + lambda I) delta = -g by conjugate gradients preconditioned with T, the block-tridiagonal part of H + lambda I (diagonal blocks and the blocks
 *              between poses k and k + 1; a factor on such a pair in either direction lands there). Everything else, the chords, enters through the
 *              matrix-vector product only. T^-1 by block cyclic reduction (6 x 6 blocks, identity padding to a power of two), factored once per lambda.
 *              Exit when sqrt(r z) <= pcg_tol sqrt(r0 z0), at the cap (pcg_max_iterations, or 0 = automatic: min(12 chords + 2, 1000) since H - T has rank
 *              <= 12 chords; without chords T is the matrix and the cap is 1), or when r z or p A p stops being positive; r0 z0 == 0 returns delta = 0 at once.
 *   outer      Levenberg-Marquardt, GTSAM's LevenbergMarquardtParams defaults. Per trial: iterations >= max_iterations -> ITERATIONS; lambda > lambda_upper ->
 *              LAMBDA; solve, retract, cost. A trial that lowers the cost is accepted: lambda /= factor, iterations += 1, and CONVERGED when the decrease is
 *              <= absolute_error_tol or <= relative_error_tol * cost before; else relinearise. A trial that does not lower it but raises it by less than
 *              absolute_error_tol ends as CONVERGED without moving (a zero gradient ends here: the every-key-frame case). Otherwise lambda *= factor and the
 *              step is retried without relinearising.
 * pose6 (transformTobeMapped order) is taken from R as pcl::getTranslationAndEulerAngles does; GTSAM's rotation().roll()/pitch()/yaw() agree away from gimbal
 * lock (parity unpinned). A graph is single-threaded like a key map, works on a stream of its own and waits for it before returning; its device store only grows.
 * ROLO_EINVAL: an index out of range, i == j, a variance <= 0 or non-finite, a non-finite pose, more than ROLO_PGO_MAX_POSES poses, a solve whose H + lambda I is
 * not positive definite, a loss constant k that is not finite and positive (or whose square is not). ROLO_EUNSUPPORTED: a loss other than
 * ROLO_PGO_LOSS_CAUCHY. ROLO_ESTATE: optimise, linearise or get_factor_errors with no pose or no factor; solve_linear without a linearisation of the graph as
 * it stands. */
#define ROLO_PGO_MAX_POSES (1 << 16)
#define ROLO_PGO_CONVERGED 1
#define ROLO_PGO_ITERATIONS 2
#define ROLO_PGO_LAMBDA 3
#define ROLO_PGO_LOSS_CAUCHY 1
typedef struct rolo_pgo rolo_pgo;
typedef struct rolo_pgo_params { int max_iterations; double absolute_error_tol, relative_error_tol, lambda_initial, lambda_factor, lambda_upper, pcg_tol;
                                 int pcg_max_iterations; } rolo_pgo_params;
typedef struct rolo_pgo_result { int state, iterations, trials; double initial_cost, final_cost, lambda; int pcg_iterations; } rolo_pgo_result;
/* one record per trial: its lambda, the trial's cost, whether it was accepted, the PCG iterations and sqrt(r z) / sqrt(r0 z0) of its solve */
typedef struct rolo_pgo_trace_rec { double lambda, cost; int accepted, pcg_iterations; double residual; } rolo_pgo_trace_rec;
int rolo_pgo_create(int device, rolo_pgo** out);
void rolo_pgo_destroy(rolo_pgo* g);
void rolo_pgo_default_params(rolo_pgo_params* p);
/* initialEstimate.insert; returns the pose's index (>= 0) */
int rolo_pgo_add_pose(rolo_pgo* g, const double* T16);
int rolo_pgo_add_prior(rolo_pgo* g, int i, const double* T16, const double* var6);
int rolo_pgo_add_between(rolo_pgo* g, int i, int j, const double* T16, const double* var6);
/* the same factor under a loss: everything rolo_pgo_add_between checks, and loss == ROLO_PGO_LOSS_CAUCHY with its constant k. A factor on a chain pair
 * (|i - j| == 1) may be robust: it lands in the chain block like any other */
int rolo_pgo_add_between_robust(rolo_pgo* g, int i, int j, const double* T16, const double* var6, int loss, double k);
int rolo_pgo_size(rolo_pgo* g, int* n_poses, int* n_factors, int* n_chords);
int rolo_pgo_optimize(rolo_pgo* g, const rolo_pgo_params* params, rolo_pgo_result* out);
/* the current poses: T16_out (n x 16 doubles) and / or pose6_out (n x 6 floats), the first min(n, cap); returns n */
int rolo_pgo_get_poses(rolo_pgo* g, double* T16_out, float* pose6_out, int cap);
/* every factor's r^2 = |e / sigma|^2 and weight w at the current poses, in the order the factors were added, the first min(F, cap); each output is optional;
 * returns F. w is exactly 1.0 for a factor without loss: after an optimise, a robust loop whose w is near 0 is one the optimum outvoted */
int rolo_pgo_get_factor_errors(rolo_pgo* g, double* r2, double* weight, int cap);
int rolo_pgo_get_trace(rolo_pgo* g, rolo_pgo_trace_rec* out, int cap);
/* test hooks. linearise at the current poses: cost, grad[6N], diag[N x 36], chain[(N - 1) x 36] (the blocks H[k, k+1]), chord[chords x 36] (H[i, j] of the
 * factor as given) and chord_ij[chords x 2], each optional; solve_linear: the step a trial would take on the last linearisation */
int rolo_pgo_linearize(rolo_pgo* g, double* cost, double* grad, double* diag, double* chain, double* chord, int32_t* chord_ij);
/* The solve (of solve_linear and of every trial of optimise) has two forms that return the same bits: delta, the iteration count, the residual and the
 * not-positive-definite flag. ONE_WG runs the factorisation and the whole PCG loop in one workgroup of one launch. GRID cuts the same arithmetic into launches
 * that cover the device, one per level of the reduction and per stage of an iteration; PCG's scalars and its exit live in device memory and the host looks at
 * them once per batch of iterations. Every element is the same expression in both; the dot products keep the one-workgroup form's summation order. */
int rolo_pgo_solve_linear(rolo_pgo* g, double lambda, double pcg_tol, int pcg_max, double* delta, int* pcg_iterations, double* residual);
/* which form a graph's solves take. AUTO (the default): ONE_WG below a measured pose count, GRID from it on (512 poses: DESIGN.md 7). Any other value is ROLO_EINVAL and
 * the form stays as it was. get: the form asked for and the one the latest solve ran (0 before any solve); each output is optional. Per graph, at any time
 * between calls */
#define ROLO_PGO_SOLVE_AUTO 0
#define ROLO_PGO_SOLVE_ONE_WG 1
#define ROLO_PGO_SOLVE_GRID 2
int rolo_pgo_set_solve_form(rolo_pgo* g, int form);
int rolo_pgo_get_solve_form(rolo_pgo* g, int* requested, int* last_used);
/* device milliseconds of the last optimise, summed over its trials: ms4[0] linearise + assemble and [3] retract + cost between HIP events; [1] the cyclic
 * reduction's factorisation and [2] the PCG loop: in the one-workgroup form they share one launch and are read from the device's wall clock inside it, in the
 * grid form they lie between HIP events */
int rolo_pgo_last_ms(rolo_pgo* g, float* ms4);
/* correctPoses (:1301-1314) in one call: poses 0 .. n - 1 of the key map (n x 6 floats); n above the key map's size is ROLO_EINVAL */
int rolo_keymap_set_poses(rolo_keymap* km, const float* pose6, int n);

/* ---- The ground prior: a resident ground cloud with x-y queries and patch cut (reference ground_factor::GroundModel, src/prior_pose/pose_solver.cpp) and the
 * batched terrain pose solver (ground_factor::PoseSolver::Solve, PriorPoseNode::HandlePose prior_pose_node.cpp:164-233). tests/prior_twin.py states all of it in
 * numpy; DESIGN.md 10 has the kernels.
 *   cloud      n records of stride_floats floats (3 .. 8), x y z at floats 0 .. 2; the whole record is kept (a patch carries what GroundPatchType carries). A
 *              non-finite x or y is ROLO_ENONFINITE and the model keeps what it held. n = 0 empties the model; every query on an empty model is ROLO_ESTATE
 *              (ExtractPatch returns false on an empty cloud). The points are binned into a uniform x-y grid on the device: cells of the fit radius (0.6, or
 *              rolo_ground_set_grid), doubled until no side has more than ROLO_GROUND_MAX_SIDE cells and the grid no more than min(max_cells, 4 n + 1024).
 *              The grid only decides which points a query looks at, never its answer.
 *   nearest    the smallest (d2, index) with d2 = dx dx + dy dy in float, as FLANN's L2_Simple adds its terms (the z term is 0). Among equal distances the
 *              reference takes whatever FLANN's tree order gives; here the lowest index. Parity on that choice is unpinned.
 *   radius     { i : d2_i < (float)(r r) }, r r in double (what pcl::KdTreeFLANN::radiusSearch passes down), strict, in ascending (d2, index): a sorted radius
 *              search. Every sum over neighbours below is a serial fp64 sum in that order. A neighbourhood of more than ROLO_GROUND_MAX_NEIGHBOURS points does
 *              not fit a workgroup's list: the debug query returns its true count and no list; a fit or an average height takes its nearest-point fall-back and
 *              sets ROLO_PRIOR_STATUS_OVERFLOW.
 *   patch      ExtractPatch: two pcl::PassThrough passes, x then y; each limit is (float)(c -+ 0.5 size) with the sum in double, both ends inclusive, a point
 *              with a non-finite x, y or z is dropped, the caller's order is kept. With T16 (row-major 4 x 4 floats) the kept points are moved as
 *              pcl::transformPointCloud moves them in float, each row T0 x + (T1 y + (T2 z + T3)); the other fields are copied. *m = 0 is a valid answer; a cap
 *              below the number kept is ROLO_EINVAL and *m still receives that number.
 * One model is single-threaded like a key map, works on a stream of its own and waits for it before returning. */
#define ROLO_GROUND_MAX_POINTS (1 << 26)
#define ROLO_GROUND_MAX_NEIGHBOURS 4096
#define ROLO_GROUND_MAX_CELLS (1 << 22)
#define ROLO_GROUND_MAX_SIDE 2048
#define ROLO_GROUND_MAX_QUERIES 65536
typedef struct rolo_ground rolo_ground;
int rolo_ground_create(int device, rolo_ground** out);
void rolo_ground_destroy(rolo_ground* g);
/* the first cell size (> 0, finite) and the cell limit (1 .. ROLO_GROUND_MAX_CELLS) of the NEXT rolo_ground_set_cloud */
int rolo_ground_set_grid(rolo_ground* g, float cell_size, int max_cells);
int rolo_ground_set_cloud(rolo_ground* g, const float* pts, int n, int stride_floats);
/* out[0] points, [1] cells along x, [2] along y, [3] how often the cell size was doubled, [4] floats per record; the first min(cap, 5) */
int rolo_ground_info(rolo_ground* g, long long* out, int cap);
/* debug entry points, nq <= ROLO_GROUND_MAX_QUERIES queries (x y floats: the reference casts its query to float before it searches). nearest: index and d2 per
 * query. radius: count[q] is the number of hits whatever cap is; the first min(count, cap) (index, d2) pairs of the ordered list go to row q of idx / d2 (cap
 * entries per row), none when count exceeds ROLO_GROUND_MAX_NEIGHBOURS */
int rolo_ground_nearest_xy(rolo_ground* g, const float* xy, int nq, int32_t* idx, float* d2);
int rolo_ground_radius_xy(rolo_ground* g, const float* xy, int nq, double radius, int cap, int32_t* count, int32_t* idx, float* d2);
int rolo_ground_extract_patch(rolo_ground* g, double cx, double cy, double patch_size, const float* T16_or_null, float* out, int cap, int* m);
/* device milliseconds between HIP events of the last grid build [0], patch [1] and solve [2] (0 before the first) */
int rolo_ground_last_ms(rolo_ground* g, float* ms3);

/* PoseSolver::Solve as written, in fp64, for a batch of (x, y, yaw): one workgroup per pose, every pose independent of the others and its result the same bits
 * alone or in any batch.
 *   start      R = RotZ(yaw); z = InitialZ: the least AverageHeightAt over the wheels (the nearest point, then the mean z of the radius search around THAT
 *              point; the nearest point's z when ground_avg_radius <= 0, when the search finds nothing or fewer than ground_min_neighbors) + vehicle_com_z - 1.
 *   residual   per wheel p = R (wx, wy, -com_z) + t and a ground point: FitLocalSurface at (float) p.xy, else the nearest point. The fit: the radius search
 *              (fit_radius); fewer than fit_min_points hits -> no fit; the z-outlier cut with inclusive bounds mean -+ fit_outlier_factor sigma (population
 *              sigma); fewer than fit_min_points (or than 3) inliers -> no fit; centroid and scatter matrix of the inliers, the eigenvector of the smallest
 *              eigenvalue as the normal (a cyclic Jacobi in fp64: the height does not depend on the vector's sign or scale, and Eigen's QL iteration is not
 *              restated); |c| < 1e-6 -> no fit; z = -(a x + b y + d) / c at the double query. d_i = (p - ground) . (R ez); f_i = k d_i if d_i < 0 else 0.
 *              residual = sum_i f_i (1, wy_i, -wx_i) + g ((R ez) . ez, 0, 0); the Jacobian as ComputeResidualAndJacobian writes it. Sums run in wheel order.
 *   loop       A = J^T J + lambda I, b = -J^T r; a 3 x 3 LU with full pivoting and Eigen's rank rule (a pivot counts if |p| > 3 eps |p_max|); singular ->
 *              lambda *= 10 and the next iteration. R_new = RotX(droll) RotY(dpitch) R, then EnforceFixedYaw. Accept when the trial cost is lower: lambda =
 *              max(lambda / 2, 1e-8), converged when |last_cost - c1| < tol_cost and |delta| < tol_step; reject: lambda *= 5. Best-so-far (z, R, cost) is
 *              what comes back. The wheels' signed distances at the end use the NEAREST point, not the fit.
 *   success    FailureDetection: z in [z_min, z_max], |roll| <= roll_max, |pitch| <= pitch_max, every |distance| <= wheel_distance_max, and not max_iters;
 *              cleared too by any status bit. ROLO_PRIOR_STATUS_NONFINITE: a wheel position or a cost stopped being finite and the pose's loop ended there
 *              (the reference would go on searching with it).
 *   lidar pose x y z roll pitch yaw of T_world_body body_to_lidar with T_world_body = (RotZ(yaw) RotY(pitch) RotX(roll), (x, y, z)) and the angles as
 *              tf2::Matrix3x3::getRPY takes them; HandlePose's round trips through quaternions are not restated.
 * Unpinned: FLANN's order among equal distances, Eigen's SelfAdjointEigenSolver and FullPivLU internals, the order of Eigen's matrix-vector sums.
 * ROLO_EINVAL: B outside 1 .. ROLO_PRIOR_MAX_BATCH, n_wheels outside 1 .. ROLO_PRIOR_MAX_WHEELS, max_iters outside 0 .. ROLO_PRIOR_MAX_ITERS, negative
 * neighbour counts; ROLO_ENONFINITE: a non-finite parameter or pose; ROLO_ESTATE: no cloud. */
#define ROLO_PRIOR_MAX_WHEELS 8
#define ROLO_PRIOR_MAX_BATCH 65536
#define ROLO_PRIOR_MAX_ITERS 10000
#define ROLO_PRIOR_END_CONVERGED 0
#define ROLO_PRIOR_END_MAX_ITERS 1
#define ROLO_PRIOR_STATUS_OVERFLOW 1
#define ROLO_PRIOR_STATUS_NONFINITE 2
#define ROLO_PRIOR_FIT_OK 0          /* fall-backs of the fit, in the order FitLocalSurface tests them */
#define ROLO_PRIOR_FIT_FEW_HITS 1
#define ROLO_PRIOR_FIT_FEW_INLIERS 2
#define ROLO_PRIOR_FIT_NO_PLANE 3    /* fewer than 3 inliers */
#define ROLO_PRIOR_FIT_VERTICAL 4    /* |c| < 1e-6 */
#define ROLO_PRIOR_FIT_OVERFLOW 5
typedef struct rolo_priorpose_params {
  int n_wheels; double wheel_xy[2 * ROLO_PRIOR_MAX_WHEELS]; double vehicle_com_z; double body_to_lidar_t[3]; double body_to_lidar_R[9];   /* R row-major */
  double k_spring, g; int max_iters; double lm_lambda, tol_cost, tol_step, ground_avg_radius; int ground_min_neighbors;
  double fit_radius, fit_outlier_factor; int fit_min_points;
  double z_min, z_max, roll_max, pitch_max, wheel_distance_max;
} rolo_priorpose_params;
typedef struct rolo_priorpose_result {
  double z, roll, pitch, R[9], cost; double wheel_distance[ROLO_PRIOR_MAX_WHEELS]; double lidar_pose[6];   /* x y z roll pitch yaw */
  int iterations, end_reason, success, status;
} rolo_priorpose_result;
/* hits: the radius search's count; inliers: after the cut (0 when the fit ended before it); fallback: ROLO_PRIOR_FIT_*; point: the ground point the residual
 * would use, the fit's (x, y, height) or the nearest point; nearest: that point's index, -1 when the fit held */
typedef struct rolo_priorpose_fit { int hits, inliers, fallback, nearest; double point[3]; } rolo_priorpose_fit;
/* the values of config/prior_pose_params.yaml (its four wheels), fit radius 0.6, outlier factor 3, minimum points 15 */
void rolo_priorpose_default_params(rolo_priorpose_params* p);
int rolo_priorpose_solve(rolo_ground* g, const rolo_priorpose_params* params, const double* xyyaw, int B, rolo_priorpose_result* out);
/* the fit alone at nq <= ROLO_GROUND_MAX_QUERIES double queries (x y) */
int rolo_priorpose_fit_surface(rolo_ground* g, const rolo_priorpose_params* params, const double* xy, int nq, rolo_priorpose_fit* out);

/* ---- back end: the mapping node's per-scan step as one device-resident call ---------------------------------------------------------------
 * laserCloudInfoHandler (src/backMapping.cpp:420-457) for one CloudInfoStamp: the interval gate (:436), updateInitialGuess (:516-555), extractSurroundingKeyFrames
 * (:558-663), downsampleCurrentScan (:666-678), scan2MapOptimization (:681-711) with transformUpdate (:1060-1068), saveKeyFramesAndFactor (:1094-1221), correctPoses
 * (:1287-1320), the incremental pose of publishOdometry (:1361-1389) and the clouds of publishFrames (:1405-1424), in that order. A mapper owns a key map, a pooled
 * context for the scan-to-submap registration and a pose graph, and composes the calls above: every result is the bits of the call-by-call route (INTEGRATION.md,
 * "Back end"). What it adds is residence: the scan is uploaded once (or handed over as device clouds), its two filtered clouds stay in slots of their own in the key
 * map, the registration packs its features from there behind an event, and a saved scan is appended to the key-frame store device to device.
 *   pose      transformTobeMapped = (roll, pitch, yaw, x, y, z) in float, as everywhere in this header. The node's Affine3f bookkeeping is restated in float:
 *             pcl::getTransformation, pcl::getTranslationAndEulerAngles, Affine3f::inverse() as the cofactor inverse of the linear part with -L^-1 t, products as
 *             sums over k left to right (Eigen's own order is unpinned).
 *   sub-map   rolo_keyposes_select_nearby on the key map's poses and stamps (10 s of recent poses), rolo_keymap_extract, rolo_scan2map_set_submap_keymap. The
 *             sub-map of the last scan is kept (submap_rebuilt = 0) exactly when the listed indices equal the last list and no key pose has been set since (by the
 *             mapper or through the borrowed key map); nothing transformed is cached, so keeping and rebuilding give the same bits. (A rolo_keymap_extract of the caller's own
 *             through the borrowed key map replaces what rolo_keymap_get_submap returns, not what the registration searches: its trees live in the mapper's context.)
 *   too few   with n_corner_ds <= edgeFeatureMinValidNum or n_surf_ds <= surfFeatureMinValidNum the pose stays the guess, transformUpdate does not run and
 *             incrementalOdometryAffineBack keeps the PREVIOUS scan's value, as in the reference (:687-710): the incremental pose then advances by the previous scan's
 *             step measured from this scan's front. Before transformUpdate has ever run the reference reads an unset matrix; here it is the identity.
 *   graph     key 0 gets the prior (:1229-1233), every later key the odometry factor from the key map's last pose (:1235-1241), then the queued loop factors
 *             (cauchy_k > 0: rolo_pgo_add_between_robust) and prior factors in queue order, ONE rolo_pgo_optimize with the default parameters, and
 *             transformTobeMapped from the newest pose's pose6. poseCovariance (:1161) is not provided: it is read nowhere. A queued factor whose keys are not
 *             in the graph when it is added is ROLO_EINVAL, and the queues keep it.
 *   errors    a non-finite coordinate (ROLO_ENONFINITE) or any other error before saveKeyFramesAndFactor leaves the mapper exactly as it was: pose, odometry
 *             memory, time gate, key frames, graph, queues (the next scan rebuilds its sub-map). saveKeyFramesAndFactor first reserves room in the key map, the
 *             descriptor store and the graph, then computes the descriptor, then changes the three: they grow together or not at all.
 * A mapper is single-threaded like a context: the reference's mtx is the caller's business. Publishing stays with the caller. */
typedef struct rolo_mapper rolo_mapper;
typedef struct rolo_mapper_params {           /* utility.h:320-343 */
  double mappingProcessInterval;              /* 0.15 */
  float  mappingCornerLeafSize, mappingSurfLeafSize;                                       /* 0.2, 0.2 */
  float  surroundingKeyframeSearchRadius, surroundingKeyframeDensity;                      /* 50, 1 */
  float  surroundingkeyframeAddingDistThreshold, surroundingkeyframeAddingAngleThreshold;  /* 1.0, 0.2 */
  int    edgeFeatureMinValidNum, surfFeatureMinValidNum;                                   /* 10, 100 */
  float  z_tollerance, rotation_tollerance;                                                /* FLT_MAX */
  int    sc_input;                            /* 0 none, 1 scan_feat (:1213), 2 scan_raw (:1186-1196) */
  float  sc_leaf;                             /* downSizeFilterSC of scan_raw: 0.5 */
} rolo_mapper_params;
typedef struct rolo_mapper_result {
  int processed;                              /* 0: the interval gate (:436) held the scan back; nothing else is filled */
  float transformTobeMapped[6], incremental6[6];   /* :1348-1351 and :1372-1384 (x y z roll pitch yaw of increOdomAffine) */
  int s2m_ran;                                /* 0: no key frame yet (:684) */
  rolo_scan2map_stats s2m;
  int n_corner_ds, n_surf_ds, m_corner, m_surf, n_listed, submap_rebuilt;
  int keyframe;                               /* index of the key frame this scan became, -1: saveFrame said no */
  int loops_added, priors_added, poses_corrected;   /* poses_corrected 1: correctPoses rewrote the key map */
  int sc_index;                               /* descriptor stored for this key frame, -1 none */
  rolo_pgo_result pgo;                        /* of the optimise behind isam->update, zeroed when keyframe < 0 */
} rolo_mapper_result;
void rolo_mapper_default_params(rolo_mapper_params* p);
int rolo_mapper_create(int device, const rolo_mapper_params* params /* NULL: the defaults */, rolo_mapper** out);
void rolo_mapper_destroy(rolo_mapper* m);
/* borrowed, never destroyed by the caller: for the loop-closure, Scan Context, global-map and ground-prior calls between scans */
rolo_keymap* rolo_mapper_keymap(rolo_mapper* m);
rolo_pgo* rolo_mapper_pgo(rolo_mapper* m);
/* one CloudInfoStamp. corner, surf: n x 4 floats (surf = extracted_surface ++ extracted_normal, :430); raw: cloud_projected (for sc_input 2 and
 * rolo_mapper_get_registered_raw), may be NULL; clouds_on_device != 0: all three are device pointers on the mapper's device whose writers the caller has waited for.
 * initialGuess6: initialGuessRoll / Pitch / Yaw / X / Y / Z, read when odomAvailable != 0. */
int rolo_mapper_scan(rolo_mapper* m, double stamp, const float* corner, int n_corner, const float* surf, int n_surf, const float* raw, int n_raw, int clouds_on_device,
                     const float* initialGuess6, int odomAvailable, rolo_mapper_result* out);
/* loopIndexQueue / loopPoseQueue / loopNoiseQueue .push_back (:2388-2392, :2472-2476): between(from, to, T16, Variances(var6)), under Cauchy(cauchy_k) when cauchy_k > 0.
 * T16, var6 and cauchy_k are checked here as rolo_pgo_add_between[_robust] checks them; the keys when the factor is added */
int rolo_mapper_queue_loop(rolo_mapper* m, int from, int to, const double* T16, const double* var6, double cauchy_k);
/* priorIndexQueue &c (:2129-2133) */
int rolo_mapper_queue_prior(rolo_mapper* m, int from, int to, const double* T16, const double* var6);
/* laserCloudCornerLastDS / laserCloudSurfLastDS of the last processed scan; either output may be NULL to read the sizes; counts2 (optional): the two sizes */
int rolo_mapper_get_scan(rolo_mapper* m, float* corner_ds, int cap_corner, float* surf_ds, int cap_surf, int* counts2);
/* publishFrames :1405-1414: corner_ds ++ surf_ds moved to transformTobeMapped, each row T0 x + (T1 y + (T2 z + T3)) as the key map moves its clouds; returns the size */
int rolo_mapper_get_registered(rolo_mapper* m, float* out, int cap);
/* :1416-1424: the raw cloud of the last processed scan moved the same way; ROLO_ESTATE when that scan came without one */
int rolo_mapper_get_registered_raw(rolo_mapper* m, float* out, int cap);
/* the key poses (n x 6 floats) and stamps of the mapper's key map, the first min(n, cap); returns n */
int rolo_mapper_get_keyposes(rolo_mapper* m, float* pose6, double* times, int cap);
/* device milliseconds of the last processed scan between HIP events: ms6[0] down-sample, [1] sub-map (extraction and hand-over), [2] scan2map, [3] key-frame commit
 * (descriptor and append), [4] graph (rolo_pgo_last_ms summed), [5] the whole call, first event to last */
int rolo_mapper_last_ms(rolo_mapper* m, float* ms6);
/* the node's float bookkeeping, host only (no device needed):
 * updateInitialGuess (:516-555) after incrementalOdometryAffineFront has been taken. tf6_out = tf6_in, with roll = pitch = yaw = 0 while there is no key frame
 * (:524-531); else, when odomAvailable: the first guess is only stored (:540-543), a later one moves the pose by lastOdom^-1 guess (:545-551). lastOdom12 (rows 0..2 of
 * lastOdomTransformation, row-major 3 x 4) and *lastOdomAvailable are read and updated. */
int rolo_mapper_initial_guess(const float* tf6_in, int have_keyposes, const float* guess6, int odomAvailable, float* lastOdom12, int* lastOdomAvailable, float* tf6_out);
/* saveFrame (:1071-1091): 1 save, 0 not; last_keypose6 NULL: no key frame yet, 1 */
int rolo_mapper_save_frame(const float* last_keypose6, const float* tf6, float dist_thr, float angle_thr);
/* publishOdometry :1361-1389. started == 0 (lastIncreOdomPubFlag false): incre12 = trans2Affine3f(tf6). Otherwise incre12 <- incre12 (front^-1 back) with front =
 * trans2Affine3f(front6), the pose before updateInitialGuess (:519), and back = trans2Affine3f(back6), the pose transformUpdate last wrote (:1067). pose6_out =
 * x y z roll pitch yaw of incre12. */
int rolo_mapper_incremental(const float* front6, const float* back6, const float* tf6, int started, float* incre12, float* pose6_out);

#ifdef __cplusplus
}
#endif
#endif /* ROLO_HIP_H */
