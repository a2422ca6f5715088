// Multi-GPU: the peer exchange kernels below, and behind them the host side of everything a context shares with other ranks (shards, RCCL, rolo_peer_*).
// Peer exchange kernels that are not part of the LM controller (passes.hip calls peer_allreduce_block from ctrl_kernel itself):
//   * peer_allreduce_kernel — the 32 fp64 sums of a stage-level evaluation (rolo_so3_linearize, rolo_compute_error, rolo_t3_linearize ...)
//     summed over the ranks in rank order;
//   * peer_cov_push_kernel / peer_cov_wait_kernel — K5's covariance exchange ("K5 shards by query point ... all-gather of
//     <= 4 MB per cloud"): every rank computed the 48-byte covariances of ITS slice of the curve-sorted queries into segment `rank` of its
//     exchange area; the push kernel copies that segment into the same segment of every peer's area (plain 16-byte stores over xGMI /
//     the fabric; two areas alternate by the parity of the exchange's number, taken from the epoch word on the device), each workgroup fences at system scope and takes a ticket, and the LAST workgroup raises this rank's flag (the epoch) in
//     every mailbox; the wait kernel (one wavefront) polls the own mailbox for every rank's flag of this epoch. The scatter kernel that
//     follows in stream order (knn_unstage_kernel) then reads complete segments. Replaces ncclAllGather on the sharded path: no
//     library call, graph-capturable, and testable with two processes on ONE device (which RCCL refuses).
#include "peer_dev.hpp"
#include "ctx.hpp"
#include <dlfcn.h>
#include <map>
#include <mutex>

namespace rolo {

namespace {

__global__ __launch_bounds__(256) void peer_allreduce_kernel(double* __restrict__ sums_io, PeerArgs pa, int* __restrict__ err_flag) {
  __shared__ double sums[NV_MAX];
  __shared__ unsigned xw[PEER_MAX * PEER_SLOT_WORDS];
  __shared__ int bad;
  if (threadIdx.x < NV_MAX) sums[threadIdx.x] = sums_io[threadIdx.x];
  __syncthreads();
  const bool ok = peer_allreduce_block<256>(sums, xw, &bad, pa);
  if (threadIdx.x < NV_MAX) sums_io[threadIdx.x] = sums[threadIdx.x];
  if (!ok && threadIdx.x == 0 && err_flag) *err_flag = ROLO_ECOMM;
}

// grid-stride copy of the own segment into every peer's area; flag by the last workgroup to arrive
__global__ __launch_bounds__(256) void peer_cov_push_kernel(PeerArgs pa, size_t area_bytes /* of ONE exchange area */, size_t seg_doubles) {
  const int W = pa.world, rank = pa.rank;
  unsigned long long* own = pa.box[rank];
  // the area of exchange number e = (own epoch + 1) is e & 1 — on every rank, in every launch of a replayed hipGraph (the wait kernel behind this one bumps the epoch)
  const size_t area_off = PEER_STAGE_OFFSET + (size_t)((peer_load(own + PEER_W_COV_EPOCH) + 1ull) & 1ull) * area_bytes;
  const size_t n2 = seg_doubles / 2;   // 16-byte units (seg_doubles is a multiple of 6 * 256)
  const double2* __restrict__ src = reinterpret_cast<const double2*>(reinterpret_cast<const char*>(own) + area_off) + (size_t)rank * n2;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (size_t)gridDim.x * blockDim.x) {
    const double2 v = src[i];
    for (int p = 1; p < W; p++) {   // start with the next rank: the ranks' bursts fan out over different links
      const int dst = (rank + p) % W;
      reinterpret_cast<double2*>(reinterpret_cast<char*>(pa.box[dst]) + area_off)[(size_t)rank * n2 + i] = v;
    }
  }
  __threadfence_system();   // this thread's stores are visible system-wide before its workgroup takes the ticket
  __syncthreads();
  __shared__ int last;
  if (threadIdx.x == 0) {
    const unsigned long long t = __hip_atomic_fetch_add(own + PEER_W_TICKET, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    last = t == gridDim.x - 1 ? 1 : 0;   // (the last workgroup resets the ticket below: every launch starts at 0)
  }
  __syncthreads();
  if (!last) return;
  __threadfence_system();
  const unsigned long long e = peer_load(own + PEER_W_COV_EPOCH) + 1ull;
  if ((int)threadIdx.x < W) __hip_atomic_store(pa.box[threadIdx.x] + PEER_W_COV_FLAG + rank, e, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  if (threadIdx.x == 0) __hip_atomic_store(own + PEER_W_TICKET, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // every workgroup has arrived: reset for the next frame
}

__global__ __launch_bounds__(64) void peer_cov_wait_kernel(PeerArgs pa, int* __restrict__ err_flag) {
  unsigned long long* own = pa.box[pa.rank];
  const unsigned long long e = peer_load(own + PEER_W_COV_EPOCH) + 1ull;
  const long long t0 = wall_clock64();
  bool ok = true;
  if ((int)threadIdx.x < pa.world) {
    const unsigned long long* p = own + PEER_W_COV_FLAG + threadIdx.x;
    while (__hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < e) {
      if ((unsigned long long)(wall_clock64() - t0) > pa.timeout_ticks) { ok = false; break; }
      __builtin_amdgcn_s_sleep(2);
    }
  }
  const bool all_ok = __all(ok);
  if (threadIdx.x == 0) {
    peer_store(own + PEER_W_COV_EPOCH, e);
    if (!all_ok && err_flag) *err_flag = ROLO_ECOMM;
  }
}

// rolo_peer_selftest: known words into the own segment of the area the NEXT exchange uses (word i of rank r = r * 2^32 + i, exact in fp64)
__global__ __launch_bounds__(256) void peer_selftest_fill_kernel(PeerArgs pa, size_t area_bytes, size_t seg_doubles) {
  unsigned long long* own = pa.box[pa.rank];
  const size_t area_off = PEER_STAGE_OFFSET + (size_t)((peer_load(own + PEER_W_COV_EPOCH) + 1ull) & 1ull) * area_bytes;
  double* seg = reinterpret_cast<double*>(reinterpret_cast<char*>(own) + area_off) + (size_t)pa.rank * seg_doubles;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < seg_doubles; i += (size_t)gridDim.x * blockDim.x)
    seg[i] = (double)pa.rank * 4294967296.0 + (double)i;
}
// ... and after the exchange: every rank's segment of the area the LAST exchange used, checked against the same pattern; bad[r] = words of rank r that differ
__global__ __launch_bounds__(256) void peer_selftest_check_kernel(PeerArgs pa, size_t area_bytes, size_t seg_doubles, unsigned* __restrict__ bad) {
  unsigned long long* own = pa.box[pa.rank];
  const size_t area_off = PEER_STAGE_OFFSET + (size_t)(peer_load(own + PEER_W_COV_EPOCH) & 1ull) * area_bytes;
  const double* area = reinterpret_cast<const double*>(reinterpret_cast<const char*>(own) + area_off);
  for (int r = 0; r < pa.world; r++) {
    unsigned n = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < seg_doubles; i += (size_t)gridDim.x * blockDim.x)
      if (area[(size_t)r * seg_doubles + i] != (double)r * 4294967296.0 + (double)i) n++;
    if (n) atomicAdd(bad + r, n);
  }
}

}  // namespace

hipError_t launch_peer_selftest_fill(const PeerArgs& peer, size_t area_bytes, size_t seg_doubles, hipStream_t s) {
  peer_selftest_fill_kernel<<<64, 256, 0, s>>>(peer, area_bytes, seg_doubles);
  return hipGetLastError();
}
hipError_t launch_peer_selftest_check(const PeerArgs& peer, size_t area_bytes, size_t seg_doubles, unsigned* bad, hipStream_t s) {
  peer_selftest_check_kernel<<<64, 256, 0, s>>>(peer, area_bytes, seg_doubles, bad);
  return hipGetLastError();
}

hipError_t launch_peer_allreduce(double* sums, const PeerArgs& peer, int* err_flag, hipStream_t s) {
  peer_allreduce_kernel<<<1, 256, 0, s>>>(sums, peer, err_flag);
  return hipGetLastError();
}

hipError_t launch_peer_cov_exchange(const PeerArgs& peer, size_t area_bytes, size_t seg_doubles, int* err_flag, hipStream_t s) {
  const size_t n2 = seg_doubles / 2;
  const int grid = (int)std::min<size_t>(std::max<size_t>((n2 + 255) / 256, 1), 1024);
  peer_cov_push_kernel<<<grid, 256, 0, s>>>(peer, area_bytes, seg_doubles);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  peer_cov_wait_kernel<<<1, 64, 0, s>>>(peer, err_flag);
  return hipGetLastError();
}

}  // namespace rolo

// ================================================================ host side =================================================================
// rolo_shard_range / rolo_set_shard*, RCCL through dlopen (rolo_comm_*), and the peer exchange without a collective library (rolo_peer_*)
using namespace rolo;

namespace rolo {

Rccl g_rccl;

static int load_rccl() {
  if (g_rccl.lib) return ROLO_OK;
  void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!h) { g_err = std::string("dlopen librccl: ") + dlerror(); return ROLO_ECOMM; }
  g_rccl.lib = h;
  g_rccl.GetUniqueId = (int (*)(void*))dlsym(h, "ncclGetUniqueId");
  g_rccl.CommInitRank = (int (*)(void**, int, Uid, int))dlsym(h, "ncclCommInitRank");
  g_rccl.AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclAllReduce");
  g_rccl.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(h, "ncclAllGather");
  g_rccl.CommDestroy = (int (*)(void*))dlsym(h, "ncclCommDestroy");
  g_rccl.GetErrorString = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
  g_rccl.CommCount = (int (*)(void*, int*))dlsym(h, "ncclCommCount");
  g_rccl.CommUserRank = (int (*)(void*, int*))dlsym(h, "ncclCommUserRank");
  if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.AllGather || !g_rccl.CommDestroy) { g_err = "librccl: missing symbols"; return ROLO_ECOMM; }
  return ROLO_OK;
}

}  // namespace rolo

extern "C" void rolo_shard_range(int n, int rank, int world, int* begin, int* end) {
  const long long N = n;
  if (begin) *begin = (int)(N * rank / world);
  if (end) *end = (int)(N * (rank + 1) / world);
}

// ---- peer exchange: process-local registry of exported mailboxes (two contexts of ONE process must not go through hipIpcOpenMemHandle:
// a handle cannot be opened by the process that exported it) ----
namespace {
struct PeerExport { void* base; int device; };
std::mutex g_peer_mu;
std::map<std::array<char, ROLO_PEER_HANDLE_BYTES>, PeerExport> g_peer_exports;
}  // namespace

namespace rolo {

// both captured frames of a context (the one in use and the other load regime's) hold what is about to change
static void drop_captured_frames(rolo_ctx* c) {
  c->sched.invalidate();
  if (c->galt.exec) { (void)hipGraphExecDestroy(c->galt.exec); c->galt.exec = nullptr; }
}

// unmap the peers' mailboxes, free the own one
void peer_disconnect_impl(rolo_ctx* c) {
  rolo_peer_state& P = c->peer;
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (int r = 0; r < PEER_MAX; r++) {
    if (P.ipc_opened[r] && P.mapped[r]) (void)hipIpcCloseMemHandle(P.mapped[r]);
    P.mapped[r] = nullptr; P.ipc_opened[r] = false;
  }
  if (P.connected) { c->rank = 0; c->world = 1; c->have_corr = false; c->src.have_cov = false; c->tgt.have_cov = false; c->have_map = false; }
  P.connected = false; P.args = PeerArgs{};
  drop_captured_frames(c);   // a captured schedule holds the peers' pointers
}
void peer_release(rolo_ctx* c) {
  rolo_peer_state& P = c->peer;
  peer_disconnect_impl(c);
  if (P.base) {
    { std::lock_guard<std::mutex> lk(g_peer_mu); g_peer_exports.erase(P.handle); }
    (void)hipFree(P.base); P.base = nullptr; P.bytes = 0;
  }
  if (P.h_err) { (void)hipHostFree(P.h_err); P.h_err = nullptr; }
}

}  // namespace rolo

extern "C" {

int rolo_set_shard(rolo_ctx* c, int rank, int world) {
  if (!c || world < 1 || rank < 0 || rank >= world) return ROLO_EINVAL;
  c->rank = rank; c->world = world; c->have_corr = false;
  if (c->shard_knn) { c->src.have_cov = false; c->tgt.have_cov = false; c->have_map = false; }
  drop_captured_frames(c);   // the captured schedule bakes the shard range in
  return ROLO_OK;
}

int rolo_set_shard_knn(rolo_ctx* c, int on) {
  if (!c) return ROLO_EINVAL;
  c->shard_knn = on != 0;
  c->src.have_cov = false; c->tgt.have_cov = false; c->have_map = false; c->have_corr = false;
  return ROLO_OK;
}

int rolo_comm_unique_id(void* uid128) {
  if (!uid128) return ROLO_EINVAL;
  int rc = load_rccl(); if (rc) return rc;
  int e = g_rccl.GetUniqueId(uid128);
  if (e != 0) { g_err = "ncclGetUniqueId failed"; return ROLO_ECOMM; }
  return ROLO_OK;
}

int rolo_comm_init(rolo_ctx* c, const void* uid128, int rank, int world) {
  if (!c || !uid128 || world < 1 || rank < 0 || rank >= world) return ROLO_EINVAL;
  if (c->peer.connected) { g_err = "context is connected to peers (rolo_peer_connect): disconnect first"; return ROLO_ESTATE; }
  int rc = set_device(c); if (rc) return rc;
  // world == 1 is a real (loopback) communicator too: the single-GPU test drives the whole collective path with it
  if ((rc = load_rccl())) return rc;
  Uid id; memcpy(&id, uid128, sizeof(id));
  int e = g_rccl.CommInitRank(&c->comm, world, id, rank);
  if (e != 0) { g_err = std::string("ncclCommInitRank: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(e) : "?"); return ROLO_ECOMM; }
  c->rank = rank; c->world = world;
  c->have_corr = false; c->src.have_cov = false; c->tgt.have_cov = false; c->have_map = false;
  return ROLO_OK;
}

int rolo_comm_info(rolo_ctx* c, int* rank, int* world) {
  if (!c) return ROLO_EINVAL;
  if (!c->comm) { if (rank) *rank = 0; if (world) *world = 0; return ROLO_OK; }   // world 0: no communicator
  int r = -1, w = -1;
  if (!g_rccl.CommCount || !g_rccl.CommUserRank || g_rccl.CommCount(c->comm, &w) != 0 || g_rccl.CommUserRank(c->comm, &r) != 0) { g_err = "ncclCommCount / ncclCommUserRank failed"; return ROLO_ECOMM; }
  if (rank) *rank = r;
  if (world) *world = w;
  return ROLO_OK;
}

int rolo_comm_destroy(rolo_ctx* c) {
  if (!c) return ROLO_EINVAL;
  if (c->comm && g_rccl.CommDestroy) { (void)hipStreamSynchronize(c->stream); g_rccl.CommDestroy(c->comm); }
  c->comm = nullptr; c->rank = 0; c->world = 1;
  c->have_corr = false; c->src.have_cov = false; c->tgt.have_cov = false; c->have_map = false;
  return ROLO_OK;
}

// ---- peer exchange without a collective library -------------------------------------------------------------------
int rolo_peer_export(rolo_ctx* c, int world, int max_points, void* handle64) {
  if (!c || !handle64 || world < 1 || world > PEER_MAX || max_points < 0) { g_err = "rolo_peer_export: bad arguments (1 <= world <= 8)"; return ROLO_EINVAL; }
  if (c->comm) { g_err = "context already holds an RCCL communicator"; return ROLO_ESTATE; }
  if (c->async_pending) { g_err = "a registration is in flight on this context"; return ROLO_ESTATE; }
  int rc = set_device(c); if (rc) return rc;
  peer_release(c);
  rolo_peer_state& P = c->peer;
  // per area: one segment per rank, a segment = the rank's share of whole 256-query workgroups of both clouds, 6 doubles per position
  P.area_bytes = ((size_t)max_points + (size_t)(2 * 256 + 2 * KNN_LEAF) * world + 512) * 6 * sizeof(double);
  P.area_bytes = (P.area_bytes + 4095) & ~(size_t)4095;
  P.bytes = PEER_STAGE_OFFSET + 2 * P.area_bytes;
  // Fine-grained device memory: what the peers write here while a kernel of this rank polls must not be served from a stale L2 line — the
  // memory type RCCL keeps its flags in; the words of the LM exchange are read with system-scope atomics either way. Ordinary (coarse)
  // device memory is the fall-back when the allocation or its export fails (ROLO_PEER_MEM = finegrained | coarse forces one).
  // NOT hipDeviceMallocUncached: measured on MI355X / ROCm 7.2 — after such an allocation is freed, later ordinary hipMalloc blocks of the
  // same process that land on its pages lose kernel writes (an unrelated context created afterwards read back covariances that were partly
  // zero, differently every run); fine-grained and coarse allocations do not leave that behind.
  const char* want = peer_mem_now();
  hipError_t e = hipErrorUnknown;
  if (!want || !strcmp(want, "finegrained")) { e = hipExtMallocWithFlags(&P.base, P.bytes, hipDeviceMallocFinegrained); P.mem_kind = "finegrained"; }
  if (e != hipSuccess && (!want || !strcmp(want, "coarse"))) { (void)hipGetLastError(); e = hipMalloc(&P.base, P.bytes); P.mem_kind = "coarse"; }
  if (e != hipSuccess) { P.base = nullptr; return fail_hip(e, "peer mailbox allocation"); }
  hipIpcMemHandle_t h;
  static_assert(sizeof(hipIpcMemHandle_t) == ROLO_PEER_HANDLE_BYTES, "hipIpcMemHandle_t is 64 bytes");
  e = hipIpcGetMemHandle(&h, P.base);
  if (e != hipSuccess && strcmp(P.mem_kind, "coarse") != 0 && !want) {   // this allocation kind cannot be exported here: ordinary device memory can
    (void)hipGetLastError(); (void)hipFree(P.base); P.base = nullptr;
    e = hipMalloc(&P.base, P.bytes); P.mem_kind = "coarse";
    if (e == hipSuccess) e = hipIpcGetMemHandle(&h, P.base);
  }
  if (e != hipSuccess) { if (P.base) { (void)hipFree(P.base); P.base = nullptr; } return fail_hip(e, "hipIpcGetMemHandle (HSA_ENABLE_IPC_MODE_LEGACY=0 set?)"); }
  HIPCHK(hipMemsetAsync(P.base, 0, PEER_STAGE_OFFSET, c->stream));
  {  // what the peers check before they push anything here (rolo_peer_connect)
    const unsigned long long hdr[2] = {(unsigned long long)P.area_bytes, (unsigned long long)world};
    HIPCHK(hipMemcpyAsync(static_cast<unsigned long long*>(P.base) + PEER_W_AREA_BYTES, hdr, sizeof(hdr), hipMemcpyHostToDevice, c->stream));
  }
  if (!P.h_err) HIPCHK(hipHostMalloc((void**)&P.h_err, sizeof(int)));
  *P.h_err = 0;
  HIPCHK(hipStreamSynchronize(c->stream));
  memcpy(P.handle.data(), &h, ROLO_PEER_HANDLE_BYTES);
  { std::lock_guard<std::mutex> lk(g_peer_mu); g_peer_exports[P.handle] = PeerExport{P.base, c->device}; }
  P.export_world = world;
  memcpy(handle64, &h, ROLO_PEER_HANDLE_BYTES);
  return ROLO_OK;
}

int rolo_peer_connect(rolo_ctx* c, const void* handles, int rank, int world) {
  if (!c || !handles || world < 1 || world > PEER_MAX || rank < 0 || rank >= world) return ROLO_EINVAL;
  rolo_peer_state& P = c->peer;
  if (!P.base || P.export_world != world) { g_err = "rolo_peer_connect: call rolo_peer_export with the same world first"; return ROLO_ESTATE; }
  if (c->async_pending) { g_err = "a registration is in flight on this context"; return ROLO_ESTATE; }
  int rc = set_device(c); if (rc) return rc;
  peer_disconnect_impl(c);
  const char* hb = static_cast<const char*>(handles);
  if (memcmp(hb + (size_t)rank * ROLO_PEER_HANDLE_BYTES, P.handle.data(), ROLO_PEER_HANDLE_BYTES) != 0) { g_err = "rolo_peer_connect: handles[rank] is not this context's export"; return ROLO_EINVAL; }
  for (int r = 0; r < world; r++) {
    std::array<char, ROLO_PEER_HANDLE_BYTES> key; memcpy(key.data(), hb + (size_t)r * ROLO_PEER_HANDLE_BYTES, ROLO_PEER_HANDLE_BYTES);
    if (r == rank) { P.mapped[r] = P.base; continue; }
    PeerExport local{nullptr, -1};
    { std::lock_guard<std::mutex> lk(g_peer_mu); auto it = g_peer_exports.find(key); if (it != g_peer_exports.end()) local = it->second; }
    if (local.base) {   // a context of this process (one process driving several GPUs, or the in-process test)
      if (local.device != c->device) {
        hipError_t e = hipDeviceEnablePeerAccess(local.device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { peer_disconnect_impl(c); return fail_hip(e, "hipDeviceEnablePeerAccess"); }
        (void)hipGetLastError();
      }
      P.mapped[r] = local.base;
    } else {
      hipIpcMemHandle_t h; memcpy(&h, key.data(), ROLO_PEER_HANDLE_BYTES);
      void* ptr = nullptr;
      hipError_t e = hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess);
      if (e != hipSuccess) { peer_disconnect_impl(c); return fail_hip(e, "hipIpcOpenMemHandle"); }
      P.mapped[r] = ptr; P.ipc_opened[r] = true;
    }
  }
  // every rank pushes its covariance segments into every peer's exchange area and its LM sums into every peer's slots: a peer that exported a
  // smaller mailbox (another max_points, another world) would be written out of bounds — refuse before the first frame
  for (int r = 0; r < world; r++) {
    if (r == rank) continue;
    unsigned long long hdr[2] = {0, 0};
    hipError_t e = hipMemcpy(hdr, static_cast<const unsigned long long*>(P.mapped[r]) + PEER_W_AREA_BYTES, sizeof(hdr), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { peer_disconnect_impl(c); return fail_hip(e, "reading a peer's mailbox header"); }
    if (hdr[0] != (unsigned long long)P.area_bytes || hdr[1] != (unsigned long long)world) {
      peer_disconnect_impl(c);
      g_err = "rolo_peer_connect: rank " + std::to_string(r) + " exported a mailbox for another max_points / world (every rank must call rolo_peer_export with the same arguments)";
      return ROLO_EINVAL;
    }
  }
  P.args = PeerArgs{};
  P.args.rank = rank; P.args.world = world;
  for (int r = 0; r < world; r++) P.args.box[r] = static_cast<unsigned long long*>(P.mapped[r]);
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) != hipSuccess || khz <= 0) khz = 100000;   // 100 MHz
  const double ms = peer_timeout_ms_now();
  P.args.timeout_ticks = (unsigned long long)(std::max(ms, 1.0) * (double)khz);
  P.connected = true;
  c->rank = rank; c->world = world;
  c->have_corr = false; c->src.have_cov = false; c->tgt.have_cov = false; c->have_map = false;
  return ROLO_OK;
}

// Collective self-test of a connected group, meant to run before the first frame (bench.py's sharded leg, a deployment's start-up): the two
// exchanges of the sharded path with KNOWN words — `reps` all-reduces of 32 fp64 through the LM mailboxes (peer_allreduce_kernel: the block the
// controller runs per trial) and one covariance-segment push into every peer's exchange area — verified on every rank. The first time the
// ranks' mailboxes are written across devices (hipIpc mapping, peer access, fine-grained memory over xGMI) fails HERE, with a named error,
// instead of as a wrong pose or a time-out inside a frame. Every rank must call it with the same reps (it advances both exchange epochs).
int rolo_peer_selftest(rolo_ctx* c, int reps, double* us2) {
  if (!c || reps < 1 || reps > 1000) return ROLO_EINVAL;
  if (!peers(c)) { g_err = "rolo_peer_selftest: context is not connected to peers"; return ROLO_ESTATE; }
  if (c->async_pending) { g_err = "a registration is in flight on this context"; return ROLO_ESTATE; }
  int rc = set_device(c); if (rc) return rc;
  const int W = c->peer.args.world, rank = c->peer.args.rank;
  hipEvent_t ea = nullptr, eb = nullptr;
  HIPCHK(hipEventCreate(&ea)); HIPCHK(hipEventCreate(&eb));
  struct EvGuard { hipEvent_t a, b; ~EvGuard() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } guard{ea, eb};
  // (1) the LM exchange: rank r contributes (r + 1)(i + 1) + rep in value i; every rank must read W (W + 1) / 2 (i + 1) + W rep
  double lm_us = 0.0; int timed = 0;
  for (int rep = 0; rep < reps; rep++) {
    for (int i = 0; i < NV_MAX; i++) c->h_sums[i] = (double)(rank + 1) * (i + 1) + rep;
    HIPCHK(hipMemcpyAsync(c->sums, c->h_sums, sizeof(double) * NV_MAX, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(ea, c->stream));
    HIPCHK(launch_peer_allreduce(c->sums, c->peer.args, c->peer.h_err, c->stream));
    HIPCHK(hipEventRecord(eb, c->stream));
    HIPCHK(hipMemcpyAsync(c->h_sums, c->sums, sizeof(double) * NV_MAX, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (*c->peer.h_err != 0) { g_err = "rolo_peer_selftest: LM exchange " + std::to_string(rep) + " timed out on rank " + std::to_string(rank) + " (a peer's words never arrived in this rank's mailbox)"; return ROLO_ECOMM; }
    for (int i = 0; i < NV_MAX; i++) {
      const double want = 0.5 * W * (W + 1) * (i + 1) + (double)W * rep;
      if (c->h_sums[i] != want) { g_err = "rolo_peer_selftest: LM exchange " + std::to_string(rep) + " on rank " + std::to_string(rank) + ": value " + std::to_string(i) + " = " + std::to_string(c->h_sums[i]) + ", expected " + std::to_string(want); return ROLO_ECOMM; }
    }
    if (rep > 0 || reps == 1) { float ms = 0.f; (void)hipEventElapsedTime(&ms, ea, eb); lm_us += 1e3 * ms; timed++; }   // the first one carries every rank's start-up skew
  }
  // (2) the covariance exchange: 4 workgroups' worth of words per rank
  const size_t seg = (size_t)6 * 256 * 4;
  if (seg * (size_t)W * sizeof(double) > c->peer.area_bytes) { g_err = "rolo_peer_selftest: exchange area smaller than the test segment"; return ROLO_EINVAL; }
  unsigned* bad = reinterpret_cast<unsigned*>(c->sums);   // NV_MAX doubles of scratch: PEER_MAX counters fit
  static_assert(PEER_MAX * sizeof(unsigned) <= NV_MAX * sizeof(double), "selftest counters");
  HIPCHK(hipMemsetAsync(bad, 0, PEER_MAX * sizeof(unsigned), c->stream));
  HIPCHK(launch_peer_selftest_fill(c->peer.args, c->peer.area_bytes, seg, c->stream));
  HIPCHK(hipEventRecord(ea, c->stream));
  HIPCHK(launch_peer_cov_exchange(c->peer.args, c->peer.area_bytes, seg, c->peer.h_err, c->stream));
  HIPCHK(hipEventRecord(eb, c->stream));
  HIPCHK(launch_peer_selftest_check(c->peer.args, c->peer.area_bytes, seg, bad, c->stream));
  unsigned h_bad[PEER_MAX] = {};
  HIPCHK(hipMemcpyAsync(h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (*c->peer.h_err != 0) { g_err = "rolo_peer_selftest: covariance exchange timed out on rank " + std::to_string(rank) + " (a peer's flag never arrived)"; return ROLO_ECOMM; }
  for (int r = 0; r < W; r++)
    if (h_bad[r]) { g_err = "rolo_peer_selftest: rank " + std::to_string(rank) + " read " + std::to_string(h_bad[r]) + " wrong words in the segment rank " + std::to_string(r) + " pushed"; return ROLO_ECOMM; }
  float ms = 0.f; (void)hipEventElapsedTime(&ms, ea, eb);
  if (us2) { us2[0] = timed ? lm_us / timed : 0.0; us2[1] = 1e3 * ms; }
  return ROLO_OK;
}

int rolo_peer_disconnect(rolo_ctx* c) {
  if (!c) return ROLO_EINVAL;
  int rc = set_device(c); if (rc) return rc;
  peer_release(c);
  return ROLO_OK;
}

int rolo_peer_info(rolo_ctx* c, int* rank, int* world, char* mem_kind16) {
  if (!c) return ROLO_EINVAL;
  if (rank) *rank = c->peer.connected ? c->peer.args.rank : 0;
  if (world) *world = c->peer.connected ? c->peer.args.world : 0;
  if (mem_kind16) { strncpy(mem_kind16, c->peer.base ? c->peer.mem_kind : "", 15); mem_kind16[15] = 0; }
  return ROLO_OK;
}

}  // extern "C"
