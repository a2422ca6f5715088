// Every switch librolo_hip.so reads from the environment: THIS is the list, one line per switch — its field, its parse (default, accepted values, what becomes of any other
// value) and what it selects. The README's "Switches read from the environment" names the same ones. Pure host C++ (no HIP include; tests/cpp/switches_test.cpp compiles it
// with g++ alone). All but three are A/B and tuning switches parsed ONCE, on the first call of switches(); the three at the bottom are read on every call.
// (Compile-time A/B builds — -DROLO_*_STATS, -DROLO_SHORT_PRIO=... — are not listed here: rolo_internal.hpp and the units that read them.)
#pragma once
#include <cstdio>
#include <climits>
#include <cstdlib>
#include <initializer_list>

namespace rolo {

namespace env {
inline const char* str(const char* name) { return getenv(name); }
inline long num(const char* name, long unset) { const char* e = str(name); return e ? atol(e) : unset; }   // NAME as a number, as given
inline bool unless_zero(const char* name) { const char* e = str(name); return !(e && atoi(e) == 0); }   // on by default; NAME=0 turns it off
inline bool if_nonzero(const char* name) { const char* e = str(name); return e && atoi(e) != 0; }       // off by default; NAME=1 turns it on
inline int one_of(const char* name, std::initializer_list<int> accepted, int otherwise) {   // NAME when it is one of `accepted`; unset or anything else: `otherwise`
  const int v = (int)num(name, otherwise);
  for (int a : accepted) if (v == a) return v;
  return otherwise;
}
inline long in_range(long v, long lo, long hi, long otherwise) { return (v >= lo && v <= hi) ? v : otherwise; }
inline int knn_sub() {   // a value that names no kernel is ignored with a warning instead of silently picking one
  const char* e = str("ROLO_KNN_SUB");
  if (!e) return -1;
  const int v = one_of("ROLO_KNN_SUB", {0, 1, 2, 4}, -1);
  if (v < 0) fprintf(stderr, "librolo_hip: ROLO_KNN_SUB=%s is not one of 0 / 1 / 2 / 4: ignored (the walk is picked by size)\n", e);
  return v;
}
}  // namespace env

struct Switches {
  // ---- neighbour search and voxel map (api.hip, schedule.hip, knn_cov.hip) ----
  bool voxel_fuse = env::unless_zero("ROLO_VOXEL_FUSE");     // =0: the voxel map as its own launches after the search, not inside them (VoxelFuse)
  bool knn_moments = env::unless_zero("ROLO_KNN_MOMENTS");   // =0: the walk leaves neighbour indices and the tail gathers through them, not the six centred moments (k = 20)
  int knn_sub = env::knn_sub();                              // 0: 64-query packets at every size | 2: two lanes per query | 4 or 1: four lanes; unset or anything else -1: by size
  int polar_exact = env::unless_zero("ROLO_POLAR_EXACT");    // =0: POLAR keys of target points near a bin edge are counted only, not recomputed with the correctly rounded atan2 / acos
  // ---- LM launch planning (schedule.hip) ----
  int lm_fused = (int)env::num("ROLO_LM_FUSED", -1);                  // 0 | 1 | 2 overrides rolo_params.fused_lm (any other positive value counts as 1; negative or unset: the parameter decides)
  int lm_threads = env::one_of("ROLO_LM_THREADS", {512, 1024}, 512);  // workgroup size of the one-launch-per-trial form
  int lm_ppt = (int)env::in_range((int)env::num("ROLO_LM_PPT", 1), 1, 16, 1);   // 1..16 (anything else 1): slabs of lm_threads points per workgroup of that form
  int lm_spec_lin = env::unless_zero("ROLO_LM_SPEC_LIN");             // =0: every pass carries both halves (no cost-only passes after a rejected trial)
  int lm_keep_cost = env::unless_zero("ROLO_LM_KEEP_COST");           // =0: with forced iterations every repeat of a converged-but-rejected trial is a pass of its own again (the A/B of rot_step_t's kept cost)
  int lm_trans_model = env::unless_zero("ROLO_LM_TRANS_MODEL");       // =0: every trial of the translation stage is a pass of its own again, not answered from the linearisation's sums (the A/B of trans_model.hpp)
  bool pass_nrm = env::unless_zero("ROLO_PASS_NRM");                 // =0: the passes read the six-entry covariances always, never the PLANE form I - m m^T
  bool pass_xcd = env::unless_zero("ROLO_PASS_XCD");                  // =0: point blocks dealt to the XCDs round-robin, not an eighth of the cloud per XCD
  bool stamp = env::if_nonzero("ROLO_STAMP");                         // =1: a device timestamp at five points of every frame (rolo_debug_stamps)
  // ---- the resident LM kernel (schedule.hip, lm_persist.hip) ----
  int lm_persist_wgs = (int)env::in_range((int)env::num("ROLO_LM_PERSIST_WGS", 0), 8, 256, 0);           // 8..256 pins its workgroup count; unset or outside 0: 256 on an idle device, 64 on a busy one
  int lm_persist_busy_threads = env::one_of("ROLO_LM_PERSIST_BUSY_THREADS", {256}, 512);    // =256: on a busy device twice the workgroups of half the size
  long lm_persist_admit_us = env::in_range(env::num("ROLO_LM_PERSIST_ADMIT_US", 1000), 0, LONG_MAX, 1000);     // microseconds its workgroups wait for each other to become resident (negative: 1000; 0: every frame bails out — a test switch)
  long lm_persist_timeout_ms = env::in_range(env::num("ROLO_LM_PERSIST_TIMEOUT_MS", 200), 1, LONG_MAX, 200);   // milliseconds a poll may last after admission (zero or negative: 200)
  bool lm_persist_interleave = env::unless_zero("ROLO_LM_PERSIST_INTERLEAVE");              // =0: the generic body (one point after the other) for the reference's configuration too
  int lm_persist_mcache = env::unless_zero("ROLO_LM_PERSIST_MCACHE");                       // =0: no Mahalanobis cache in LDS, every trial inverts again
  int lm_persist_batch = env::one_of("ROLO_LM_PERSIST_BATCH", {1, 4}, 2);                   // points of a thread that go through a body together at four points per thread
  bool ctrl_generic = env::if_nonzero("ROLO_CTRL_GENERIC");                                 // =1: the one-size-fits-all controller kernel instead of the specialised ones
  // ---- contexts and streams (api.hip, odometry.hip) ----
  int cu_partition = env::one_of("ROLO_CU_PARTITION", {2, 4, 8}, 0);                // groups: the k-th context's main stream is confined to XCD group k % groups (0 = off)
  bool odom_front_priority = env::unless_zero("ROLO_ODOM_FRONT_PRIORITY");          // =0: the odometry driver's front-end stream at normal priority
  // ---- scan-to-submap association (scan2map.hip) ----
  bool s2m_packets = env::unless_zero("ROLO_S2M_PACKETS");       // =0: the cross-check s2m_kernel, one tree walk per lane in the caller's order, features not sorted along the curve
  const char* s2m_stats = env::str("ROLO_S2M_STATS");            // =<path>: per-wavefront walk statistics of s2m_assoc_kernel are written there
};

inline const Switches& switches() {
  static const Switches s;
  return s;
}

// ---- read on every call (never cached: tests and callers set them between two contexts of one process) ----
// ROLO_PEER_TIMEOUT_MS: milliseconds a kernel's poll of the peers' words may last before the rank gives up with ROLO_ECOMM (rolo_peer_connect, which takes at least 1 ms; unset 10 000)
inline double peer_timeout_ms_now() { const char* e = env::str("ROLO_PEER_TIMEOUT_MS"); return e ? atof(e) : 10000.0; }
// ROLO_PEER_MEM = finegrained | coarse forces the mailbox's memory kind (rolo_peer_export; unset: fine-grained, coarse when that cannot be allocated or exported)
inline const char* peer_mem_now() { return env::str("ROLO_PEER_MEM"); }
// ROLO_ODOM_EARLY_SOURCE = 0 | 1 overrides the odometry driver's early hand-over of the source cloud (rolo_odom_create; unset: the driver's default)
inline bool odom_early_source_now(bool unset) { const char* e = env::str("ROLO_ODOM_EARLY_SOURCE"); return e ? atoi(e) != 0 : unset; }

}  // namespace rolo
