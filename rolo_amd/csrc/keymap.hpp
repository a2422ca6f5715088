// The key map's state, shared by the units that work on it: submap.hip (key-frame store, sub-map assembly, voxel filter) and scancontext.hip (Scan Context
// descriptors of the same key frames). One rule for both: the key map's own stream, buffers that only grow (km->store), nothing freed before rolo_keymap_destroy.
#pragma once
#include "ctx_access.hpp"
#include "sort_dev.hpp"

namespace rolo {
struct Seg { const float4* src; int n; int dst; float T[12]; };   // one key frame's cloud in the concatenation
struct ScStore;                                                    // scancontext.hip
void sc_store_destroy(ScStore* sc);                                // frees what the descriptor store holds (rolo_keymap_destroy, after the stream has drained)
}  // namespace rolo

struct rolo_keymap {
  int device = 0;
  hipStream_t stream = nullptr;      // a stream of its own: assembling a sub-map never queues behind a registration
  hipEvent_t ready = nullptr;        // recorded after every extraction: what a consumer's stream waits for
  hipEvent_t consumed = nullptr;     // recorded by the last consumer (rolo_scan2map_set_submap_keymap) after it has read the sub-map
  bool consumer_pending = false;
  // the store: chunks that are never moved or freed before rolo_keymap_destroy
  struct Chunk { float4* p; size_t cap, used; };
  std::vector<Chunk> chunks;
  struct Frame { const float4* pts[2]; int n[2]; float pose[6]; double time; };
  std::vector<Frame> frames;
  // scratch and results: they only grow
  float4* cat[2] = {nullptr, nullptr}; size_t cat_cap[2] = {0, 0};       // the concatenated, transformed clouds (corner, surface); cat[0] also stages rolo_keymap_downsample's input
  float4* sub[2] = {nullptr, nullptr}; size_t sub_cap[2] = {0, 0};       // the sub-map (laserCloud*FromMapDS)
  float4* ds_out = nullptr; size_t ds_cap = 0;                           // rolo_keymap_downsample's result
  // the current scan of a mapper (mapper.hip), resident from its upload to its place in the store: laserCloudCornerLastDS / laserCloudSurfLastDS in slots of
  // their own, the raw cloud (cloud_projected) when one was given, and the scratch of the registered clouds (publishFrames)
  float4* scan_ds[2] = {nullptr, nullptr}; size_t scan_ds_cap[2] = {0, 0};
  int n_scan_ds[2] = {0, 0};
  float4* scan_raw = nullptr; size_t scan_raw_cap = 0; int n_scan_raw = 0;
  float4* reg = nullptr; size_t reg_cap = 0;
  hipEvent_t scan_ready = nullptr;   // recorded after the scan's two filters: what the scan-to-submap helper context's stream waits for; created by the first scan
  unsigned long long pose_epoch = 0; // counts rolo_keymap_set_pose / _set_poses: a mapper keeps its sub-map only while this stands still
  rolo::SortScratch sort;            // the voxel filter's sort of (cell, point index)
  unsigned* bcnt = nullptr; size_t bcnt_cap = 0;
  int* starts = nullptr; size_t starts_cap = 0;
  float* box_part = nullptr; size_t box_part_cap = 0;
  rolo::Seg* segs = nullptr; size_t segs_cap = 0;
  int* d_m = nullptr;                // [2]
  float* h_box = nullptr;            // pinned [2][8]
  int* h_m = nullptr;                // pinned [2]
  rolo::Seg* h_segs = nullptr; size_t h_segs_cap = 0;   // pinned staging of the segment table
  rolo::DevStore store;              // every buffer here and in `sc` is its allocation, on the key map's stream; rolo_keymap_destroy releases it
  int m_sub[2] = {0, 0};
  bool have_submap = false;
  rolo::ScStore* sc = nullptr;       // the Scan Context descriptors (scancontext.hip), created by the first rolo_keymap_sc_* call
  // loop closure (rolo_keymap_loop_cloud in submap.hip, rolo_keymap_loop_icp in loopicp.hip): the two resident loop clouds, 0 source, 1 target. Both calls wait for
  // their streams before they return, so neither needs an event to order the other
  float4* loop[2] = {nullptr, nullptr}; size_t loop_cap[2] = {0, 0};
  int m_loop[2] = {0, 0};
  bool have_loop[2] = {false, false};
  float loop_ms[2] = {0.f, 0.f};     // device time of the last assembly per slot
  hipEvent_t loop_t0 = nullptr, loop_t1 = nullptr;   // with timing, created by the first assembly
  rolo_ctx* loop_ctx = nullptr;      // the pooled registration context whose tree builder and stream the ICP uses; given back by rolo_keymap_destroy
  // the global map (rolo_keymap_global_* in submap.hip): the result, and the streamed form's two ping-pong tables of (cell, running sums, count) in cell order
  int gm_batch = 0;                  // points per batch; 0: ROLO_KEYMAP_GLOBAL_BATCH
  float4* gmap = nullptr; size_t gmap_cap = 0;
  int m_gmap = 0;
  bool have_gmap = false;
  unsigned* gt_key[2] = {nullptr, nullptr}; size_t gt_key_cap[2] = {0, 0};
  float4* gt_sum[2] = {nullptr, nullptr}; size_t gt_sum_cap[2] = {0, 0};
  int* gt_cnt[2] = {nullptr, nullptr}; size_t gt_cnt_cap[2] = {0, 0};
  unsigned* gm_ncnt = nullptr; size_t gm_ncnt_cap = 0;   // new cells per workgroup of the batch's runs, then their exclusive scan
  int* gm_npre = nullptr; size_t gm_npre_cap = 0;        // per run: the new cells among the runs before it; [runs]: all of them
  int* gm_d = nullptr;               // [2] on the device: the batch's new cells
  int* gm_h = nullptr;               // pinned [2]
  long long gm_info[5] = {0, 0, 0, 0, 0};
  float gm_ms[3] = {0.f, 0.f, 0.f};
  hipEvent_t gm_ev[4] = {nullptr, nullptr, nullptr, nullptr};   // with timing, created by the first global map
};

namespace rolo {

// submap.hip: a host cloud (n x 4 floats, 0 < n <= ROLO_KEYMAP_MAX_POINTS) onto the device through the key map's scratch and, with leaf > 0, through the voxel
// filter (vg_enqueue_box / vg_enqueue_filter) without leaving the device. *d_out (n_out points) is valid on the key map's stream until the next call that
// uses the scratch. The stream has been waited for when this returns: the caller's array is free again.
int keymap_stage_cloud(rolo_keymap* km, const float* pts, int n, float leaf, const float4** d_out, int* n_out);

// ---- submap.hip, for mapper.hip: the current scan without a host round trip. on_device: the clouds are device memory whose writers the caller has waited for ----
// downsampleCurrentScan (:666-678): both clouds staged (cat[0], cat[1]) and filtered into scan_ds[0] / scan_ds[1]; raw (may be NULL) is copied into scan_raw as it
// is. Two host waits for the pair, as rolo_keymap_extract has for its pair; scan_ready is recorded behind the filters. An error leaves n_scan_ds as it was.
int keymap_scan_downsample(rolo_keymap* km, const float* corner, int n_corner, float corner_leaf, const float* surf, int n_surf, float surf_leaf, const float* raw,
                           int n_raw, bool on_device);
// the voxel filter on a cloud that is resident already and ordered on the key map's stream, into ds_out (keymap_stage_cloud's result slot)
int keymap_filter_resident(rolo_keymap* km, const float4* pts, int n, float leaf, const float4** d_out, int* n_out);
// room in the store for one more key frame of these sizes: after it keymap_append_scan cannot fail for want of memory
int keymap_reserve_keyframe(rolo_keymap* km, int n_corner, int n_surf);
// cornerCloudKeyFrames / surfCloudKeyFrames .push_back of scan_ds[0] / scan_ds[1], device to device on the key map's stream; returns the key frame's index
int keymap_append_scan(rolo_keymap* km, const float* pose6, double time);
// publishFrames :1405-1424: pieces[k] (n[k] points each, k < count <= 2) moved by pose6 into `reg` one after another and downloaded into out; the transform is
// km_transform_kernel's, T0 x + (T1 y + (T2 z + T3)) per row
int keymap_registered(rolo_keymap* km, const float4* const* pieces, const int* n, int count, const float* pose6, float* out);
// scancontext.hip: room for one more descriptor (creates the store), and the descriptor of a resident cloud on the key map's stream; returns its index
int keymap_sc_reserve(rolo_keymap* km);
int keymap_sc_add_resident(rolo_keymap* km, const float4* d_pts, int n);

}  // namespace rolo
