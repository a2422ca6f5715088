// What the units of librolo_hip.so share without sharing the context's layout (ctx.hpp): every function that crosses a unit boundary and is no part of the C ABI,
// the one HIP check, and the one store for device buffers that only grow. Included by the units that define these functions (api.hip through ctx.hpp, front.hip,
// scan2map.hip, submap.hip, scancontext.hip, loopicp.hip) as well as by their users: the compiler checks every definition against the declaration here.
#pragma once
#include "rolo_internal.hpp"
#include <atomic>
#include <string>
#include <vector>

namespace rolo {
// ---- api.hip ----
void ctx_set_error(const char* msg);   // what rolo_last_error returns on this thread
hipStream_t ctx_stream(rolo_ctx* c);
int ctx_device(rolo_ctx* c);
void** ctx_front_slot(rolo_ctx* c);    // the units' own state hanging off a context: front.hip, scan2map.hip, loopicp.hip
void** ctx_s2m_slot(rolo_ctx* c);
void** ctx_loop_slot(rolo_ctx* c);
unsigned long long ctx_cloud_epoch(rolo_ctx* c);   // changes whenever the context's source / target clouds change hands
void ctx_set_fused_lm(rolo_ctx* c, int mode);
int ctx_create_high_priority(int device, rolo_ctx** out);
int ctx_set_pair_device(rolo_ctx* c, const float* d_src, int n_src, int stride_src, const float* T16_host_or_null, const float* d_tgt, int n_tgt, int stride_tgt);
int ctx_build_map_trees(rolo_ctx* c, const float* corner, int nc, const float* surf, int ns, int stride, KnnPair* out, bool on_device = false);
// ---- front.hip ----
void front_reset_object_state(rolo_ctx* c);
// ---- submap.hip: the resident sub-map as device clouds (n x 4 floats), the event a reader's stream waits for and the one it records when it has read them ----
int keymap_device_submap(rolo_keymap* km, const float** d_corner, int* m_corner, const float** d_surf, int* m_surf, hipEvent_t* ready, hipEvent_t* consumed, int* device);
void keymap_mark_consumed(rolo_keymap* km);
// ---- scan2map.hip: the body of rolo_scan2map_optimize; feat_on_device: corner / surf are device clouds that are complete once feat_ready (may be null) has passed ----
int s2m_optimize_core(rolo_ctx* c, const float* corner, int n_corner, const float* surf, int n_surf, bool feat_on_device, hipEvent_t feat_ready, const float* map_corner,
                      int m_corner, const float* map_surf, int m_surf, float* transformTobeMapped, int edge_min, int surf_min, rolo_scan2map_stats* stats,
                      unsigned char* selected_out, float* coeff_out);
// ---- posegraph.hip: device room for more_poses poses, more_factors factors and more_chords chords beyond what the graph holds: the next optimise allocates nothing ----
int pgo_reserve(rolo_pgo* g, int more_poses, int more_factors, int more_chords);
}  // namespace rolo

extern "C" {   // called by rolo_ctx_destroy / rolo_ctx_release (api.hip); no part of include/rolo_hip.h
void rolo_front_destroy(rolo_ctx* c);     // front.hip
void rolo_s2m_destroy(rolo_ctx* c);       // scan2map.hip
void rolo_s2m_forget(rolo_ctx* c);        // scan2map.hip: a context going back to the pool forgets its resident sub-map and gives its helper context back
void rolo_loopicp_destroy(rolo_ctx* c);   // loopicp.hip
}

#pragma GCC visibility push(hidden)
namespace rolo {

inline int fail_hip(hipError_t e, const char* what) {
  ctx_set_error((std::string(what) + ": " + hipGetErrorString(e)).c_str());
  return ROLO_EHIP;
}
#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) return rolo::fail_hip(_e, #x); } while (0)

// Device (and pinned host) buffers, counted in elements: the ones that only grow, and the fixed-size ones an owner creates once (alloc). The store remembers every
// allocation it makes and release() frees them all, the live ones and the outgrown ones: an owner keeps no list of its own. An outgrown buffer stays allocated
// until then: a hipFree is a device-wide synchronisation that would stall the frames other contexts have in flight, and work queued on the owner's stream may
// still read the old buffer. Sizes grow by half, so the outgrown buffers together stay below twice the live one. The owner drains its stream, then calls release().
struct DevStore {
  hipStream_t stream = nullptr;   // carries the copy of the `keep` elements
  const char* who = "";           // names the unit in the allocation's error message
  size_t slack = 256;             // elements a buffer gets beyond one and a half times the need
  std::atomic<unsigned long long>* epoch = nullptr;   // counts the device allocations, where captured frames are keyed on them (a context's buffers)
  std::vector<void*> dev, pinned; // everything allocated since the last release()

  // exactly n elements of device memory; with p set before, the first `keep` of the old buffer copied over on the stream
  template <typename T>
  int alloc(T*& p, size_t n, size_t keep = 0) {
    T* q = nullptr;
    if (hipMalloc((void**)&q, n * sizeof(T)) != hipSuccess) { ctx_set_error((std::string("hipMalloc failed (") + who + ")").c_str()); return ROLO_EHIP; }
    dev.push_back(q);
    if (epoch) ++*epoch;
    if (p && keep) HIPCHK(hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, stream));
    p = q;
    return ROLO_OK;
  }
  template <typename T>
  int alloc_pinned(T*& p, size_t n) {
    T* q = nullptr;
    if (hipHostMalloc((void**)&q, n * sizeof(T)) != hipSuccess) { ctx_set_error((std::string("hipHostMalloc failed (") + who + ")").c_str()); return ROLO_EHIP; }
    pinned.push_back(q);
    p = q;
    return ROLO_OK;
  }
  template <typename T>
  int grow(T*& p, size_t& cap, size_t need, size_t keep = 0) {
    if (need <= cap && p) return ROLO_OK;
    const size_t want = need + need / 2 + slack;
    const int rc = alloc(p, want, keep);
    if (rc == ROLO_OK) cap = want;
    return rc;
  }
  template <typename T>
  int grow_pinned(T*& p, size_t& cap, size_t need, size_t pinned_slack) {
    if (need <= cap && p) return ROLO_OK;
    const size_t want = need + need / 2 + pinned_slack;
    const int rc = alloc_pinned(p, want);
    if (rc == ROLO_OK) cap = want;
    return rc;
  }
  void release() {   // (the owner's pointers dangle from here on)
    for (void* p : dev) (void)hipFree(p);
    for (void* p : pinned) (void)hipHostFree(p);
    dev.clear(); pinned.clear();
  }
};

}  // namespace rolo
#pragma GCC visibility pop
