// flame_ros_amd/csrc/graph_handle.h -- the definition of the handle behind the C ABI (struct flame_hip_graph) and the
// helpers its translation units share: flame_hip.cpp (the driver of every stage) and resident.cpp (the resident-tile
// solve, g->res).  Private to csrc/, not installed.
#pragma once
#include "../../include/flame_hip.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "delaunay_dev.h"
#include "kernels.h"
#include "plan.h"
#include "plan_dev.h"
#include "resident.h"
#include "sync.h"

#define HIPCHK(expr)                                             \
  do {                                                           \
    hipError_t e__ = (expr);                                     \
    if (e__ != hipSuccess) return FLAME_HIP_ERR_HIP - (int)e__;  \
  } while (0)

namespace flamehip {

struct GraphExecEntry {
  int32_t iters;
  int cur;
  SolveParams p;
  hipGraphExec_t exec;
  int launches;
};

// Device buffers are owned by the handle and keep their capacity across uploads (a frame stream
// re-uploads a similar graph every frame: no hipMalloc/hipFree after the first few frames).
// `caps` maps the address of the pointer member to its capacity in bytes.
typedef std::unordered_map<void*, size_t> CapMap;

template <class T>
int dev_alloc(CapMap& caps, T** p, size_t n) {
  n += 1;  // one pad element: kernels clamp indices of empty lists to element 0
  const size_t bytes = n * sizeof(T);
  auto it = caps.find((void*)p);
  if (*p && it != caps.end() && it->second >= bytes) return 0;
  if (*p && it != caps.end()) (void)hipFree(*p);  // (no entry: the pointer lives inside the upload arena)
  *p = nullptr;
  const size_t want = bytes + bytes / 4;  // slack for the next, slightly larger frame
  hipError_t e = hipMalloc(reinterpret_cast<void**>(p), want);
  if (e == hipErrorOutOfMemory) return FLAME_HIP_ERR_ALLOC;
  if (e != hipSuccess) return FLAME_HIP_ERR_HIP - (int)e;
  const int fill = flamehip::test_alloc_fill();  // (-1 in the product library)
  if (fill >= 0) (void)hipMemset(*p, fill, want);
  caps[(void*)p] = want;
  return 0;
}

// All copies go through the handle's own non-blocking stream (hipMemcpyAsync + stream sync),
// never the legacy stream: a legacy-stream copy in one host thread collides with a stream capture
// running in another thread (hipErrorStreamCaptureImplicit), and distinct handles must be usable
// from distinct threads.
inline hipError_t memcpy_sync(hipStream_t s, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, s);
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(s);
}

// Page-locked staging area of a handle: host arrays are copied into it once and leave through
// truly asynchronous DMAs (a hipMemcpyAsync from pageable memory is staged and waited for by the
// runtime, call by call -- ~10 us each, the larger part of a small frame's upload).
struct PinnedArena {
  char* base = nullptr;
  size_t cap = 0, used = 0;
  // room for `bytes` more (only ever grows between uploads: call with nothing in flight)
  hipError_t reserve(size_t bytes) {
    used = 0;
    if (bytes <= cap) return hipSuccess;
    if (base) (void)hipHostFree(base);
    base = nullptr; cap = 0;
    const size_t want = bytes + bytes / 2 + 4096;
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&base), want, hipHostMallocDefault);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void* put(const void* src, size_t bytes) {
    used = (used + 63) & ~(size_t)63;
    if (used + bytes > cap) return nullptr;
    void* p = base + used;
    std::memcpy(p, src, bytes);
    used += bytes;
    return p;
  }
  void release() { if (base) (void)hipHostFree(base); base = nullptr; cap = used = 0; }
};

// The solver state of V vertices and E edges copied aside, or back (device to device, on s)
struct StateTriple { float4 *A, *B, *q; };
inline int copy_state(hipStream_t s, StateTriple dst, StateTriple src, int32_t V, int32_t E) {
  HIPCHK(hipMemcpyAsync(dst.A, src.A, sizeof(float4) * (size_t)V, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(dst.B, src.B, sizeof(float4) * (size_t)V, hipMemcpyDeviceToDevice, s));
  if (E > 0) HIPCHK(hipMemcpyAsync(dst.q, src.q, sizeof(float4) * (size_t)E, hipMemcpyDeviceToDevice, s));
  return 0;
}

// flame_hip.cpp: what the hooks library's flame_hip_test_hook() set ("persist_fail", "persist_stall_us"), else 0
bool test_persist_fail();
int test_persist_stall_us();

}  // namespace flamehip

struct flame_hip_graph {
  int device = -1;
  int32_t V = 0, E = 0, T = 0;
  bool uploaded = false;
  flamehip::PlanOptions opt;
  int num_cus = 0;
  int use_graph = 1;
  flamehip::Plan plan;
  flamehip::SyncOut sync;          // inputs derived by flame_hip_graph_sync (kept for flame_hip_graph_edges)
  bool synced = false;   // the current graph came from flame_hip_graph_sync
  int path = 0;  // resolved path after upload

  hipStream_t stream = nullptr;
  hipStream_t stream_in = nullptr;  // input staging (H2D of a frame overlaps the partition kernels)
  flamehip::DelaunayScratch dt;               // flame_hip_delaunay: arenas kept between frames
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_in = nullptr;
  hipEvent_t ev_state = nullptr;  // last state-writing work on `stream` (upload, scale, filter, results)
  bool state_pending = false;     // ev_state was recorded since the last full synchronisation
  float state_scale = 1.0f;       // factor applied to the resident state since its upload (rescale_data epilogue)
  bool timed = false;
  int last_launches = 0;

  float4* A[2] = {nullptr, nullptr};
  float4* B[2] = {nullptr, nullptr};
  float4* q[2] = {nullptr, nullptr};
  int cur = 0;
  int2* eij = nullptr;
  float4* ew = nullptr;
  int32_t* grow = nullptr;
  int32_t* ginc = nullptr;
  float2* pos = nullptr;
  // tiles
  flamehip::TileDesc* tiles = nullptr;
  int32_t* t_vmap = nullptr;
  int32_t* t_emap = nullptr;
  uint2* t_eij = nullptr;
  float4* t_ew = nullptr;
  uint32_t* t_srow = nullptr;
  // triangles
  int32_t* tris = nullptr;
  int32_t* trow = nullptr;
  int32_t* tinc = nullptr;
  float4* tri_normals = nullptr;
  float4* vtx_normals = nullptr;
  uint8_t* tri_valid = nullptr;
  // dense maps (row f2), allocated on first use for the requested image size
  int64_t map_pixels = 0;
  uint32_t* map_owner = nullptr;
  float* map_idm = nullptr;
  float* map_dm = nullptr;
  float* map_cloud = nullptr;
  uint32_t* map_cov = nullptr;   // per-block covered-pixel counts of the last raster (stat key coverage)
  char* fr_dev = nullptr;        // output arena of flame_hip_frame_results (one D2H per frame)
  uint32_t* dbg_key = nullptr;   // debug images: winning-primitive key map, BGR8 output, staged features
  uint8_t* dbg_bgr = nullptr;
  float* dbg_feat = nullptr;
  // which raster the map buffers hold: the solver state it was made from (state_serial), the
  // filter parameters, filtered or not -- dense maps, coverage and the debug images share it
  uint64_t state_serial = 1, raster_serial = 0;
  int raster_filtered = -1;
  flame_hip_tri_params raster_tp;
  float raster_kinv[9];
  // prediction stage (flame_hip_predict, predict.h): scratch sized like the dense raster's and kept across frames
  bool tri_stage_run = false;    // a triangle stage has written tri_valid since the last upload
  bool is_batch = false;         // the handle holds a batch of graphs (flame_hip_graph_upload_batch)
  int64_t pg_pixels = 0;         // W x H of the key map the last flame_hip_predict made (0 = none)
  unsigned long long* pg_key = nullptr;
  float4* pg_proj = nullptr;
  float2* pg_pix = nullptr;
  float* pg_pred = nullptr;
  float* pg_map = nullptr;
  hipEvent_t pg_ev0 = nullptr, pg_ev1 = nullptr;
  double predict_us = 0.0, predict_device_us = 0.0;
  // evaluate stage (flame_hip_photo_reference / _photo_error / _truth_stats, evaluate.h): two dense images -- ev_img[ev_cmp]
  // the comparison frame, the other one the current image of the last photo_error call (promoted without a second upload) --,
  // the uploaded map / depth, the error map, the words and the partials; kept across frames, re-allocated only when W x H grows
  uint8_t* ev_img[2] = {nullptr, nullptr};
  int ev_cmp = 0;
  bool ev_has_ref = false, ev_has_cur = false;
  int32_t ev_ref_W = 0, ev_ref_H = 0, ev_cur_W = 0, ev_cur_H = 0;
  double ev_ref_pose[12] = {0.0}, ev_cur_pose[12] = {0.0};
  float* ev_map = nullptr;
  float* ev_depth = nullptr;
  float* ev_err = nullptr;
  unsigned long long* ev_words = nullptr;
  double* ev_partial = nullptr;
  hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;
  double photo_us = 0.0, photo_device_us = 0.0, truth_us = 0.0;
  // graph filter scratch (row a9)
  float* filter_tmp = nullptr;
  // mesh output (row f1)
  float4* mesh_pts = nullptr;
  // permutations on the device (results leave in the caller's order without a host pass)
  int32_t* v_i2o_dev = nullptr;
  int32_t* v_o2i_dev = nullptr;
  int32_t* e_i2o_dev = nullptr;
  int32_t* e_o2i_dev = nullptr;
  float* dl_v = nullptr;  // download staging: 3V floats
  float* dl_q = nullptr;  // 3E floats
  float* dl_n = nullptr;  // 3V floats (vertex normals of flame_hip_frame_results)
  // device plan builder (row f3) and the staged inputs it reads (caller's order)
  int plan_device = 1;
  int plan_reuse = 1;          // frame streams: partition from the previous frame's tile map
  int plan_mini = 1;           // option "plan_mini": small frames of a graph sync planned by one launch (k_mini_plan)
  bool plan_mini_used = false; // ... the current plan was
  flamehip::ResidentSolve res;  // option "persist": solves by ONE launch of resident tiles, and what recovers them (resident.h)
  float4 *snapA = nullptr, *snapB = nullptr, *snapq = nullptr;  // flame_hip_state_snapshot / _rollback
  bool snap_valid = false;
  int32_t snap_V = 0, snap_E = 0;
  hipStream_t last_stream = nullptr;  // the stream the last solve went to
  bool init_have_x0 = false;        // the device-built plan's initial state came with an x0 array
  int stream_depth = 0;        // option "stream_depth": halo depth of small graphs (<= 64 tiles) instead of the
                               // auto depth 8, which is tuned for a RESIDENT graph (fewest launches); a graph
                               // that is solved once pays for its plan, and that is cheapest at depth 4-5
  int tile_imbalance_pct = 100; // info "tile_imbalance_pct": 100 x max / mean of the tiles' cost (e_loc + 2 n_ext)
  int single_cap = 1 << 30;    // an isolated tile did not fit a graph of this many vertices + 1 on this handle
  bool plan_reused = false;    // the current plan's partition came from the map
  int reuse_tile_own_opt = 0;  // the "tile_own" option the map was made with
  int reuse_backoff = 0, reuse_skip = 0;  // frames to sit out after a rejected reuse (doubles, <= 16)
  // graph sync without waiting for the edge count: E is predicted (V + T + euler_off, -1 for a
  // triangulated disk) and checked at the plan builder's first synchronisation
  bool spec_edges = false;     // the current upload_device_plan() runs on a predicted count
  int32_t true_edges = 0;      // ... and this is what the device counted when the prediction failed
  int32_t euler_off = -1;      // E - V - T of the last frame
  int euler_skip = 0, euler_backoff = 0;
  flamehip::DevPlanner planner;
  float2* in_pos = nullptr;
  int2* in_edges = nullptr;
  float* in_alpha = nullptr;
  float* in_beta = nullptr;
  float* in_z = nullptr;
  float* in_wgt = nullptr;
  float* in_x0 = nullptr;
  int32_t* in_tris = nullptr;
  float* in_mu = nullptr;    // graph sync on the device: measured idepths, variances, predictions
  float* in_var = nullptr;
  float* in_pred = nullptr;
  bool sync_on_device = false;  // the derived edge list lives in in_edges (sync.edges is stale)
  bool beta_is_alpha = false;   // staged graph sync: beta = alpha, one buffer
  int32_t* dflags = nullptr;
  bool host_perms = true;  // plan.v_i2o / v_o2i / e_i2o / e_o2i / tris are valid on the host
  // costs
  double* partials = nullptr;
  uint8_t* cost_mask = nullptr;  // flame_hip_costs_masked: V vertex flags then E edge flags, internal order
  // halo exchange lists (internal ids), see flame_hip_halo_register
  int32_t n_send_v = 0, n_send_e = 0, n_recv_v = 0, n_recv_e = 0;
  int32_t* halo_send_v = nullptr;
  int32_t* halo_send_e = nullptr;
  int32_t* halo_recv_v = nullptr;
  int32_t* halo_recv_e = nullptr;
  // debug timeline of the tile kernel
  int profile = 0;
  unsigned long long* prof = nullptr;

  std::vector<flamehip::GraphExecEntry> execs;
  flamehip::CapMap caps;
  int solves_since_upload = 0;
  flamehip::PinnedArena pin;             // page-locked staging of the host arrays of an upload
  flamehip::PinnedArena pin_in;          // ... of the inputs of a small graph sync (one DMA; k_mini_plan reads the device copy)
  char* in_stage = nullptr;
  flamehip::PinnedArena pout;            // page-locked landing area of the results (frame_results, download)
  char* harena = nullptr;      // device arena the host-built plan of the current upload lives in
  bool lanes_applied = false;  // lane_order = 1: the conflict-avoiding lane order is in the device arrays

  void drop_execs() {
    for (auto& e : execs) (void)hipGraphExecDestroy(e.exec);
    execs.clear();
  }

  void free_device() {
    if (device < 0) return;
    (void)hipSetDevice(device);
    drop_execs();
    // every device buffer of the handle is registered in `caps` (key = address of the member)
    for (auto& kv : caps) {
      void** pp = reinterpret_cast<void**>(kv.first);
      if (*pp) (void)hipFree(*pp);
      *pp = nullptr;
    }
    caps.clear();
    pin.release();
    pin_in.release();
    pout.release();
    map_pixels = 0;
    ev_has_ref = ev_has_cur = false;
    n_send_v = n_send_e = n_recv_v = n_recv_e = 0;
  }
};

namespace flamehip {

// flame_hip.cpp: the arguments every tile launch of a solve shares, and -- for the resident unit's repeat of a solve that
// gave up -- `iters` PD iterations by ordinary launches on s, starting from buffer `cur` (tile path: one launch per
// `depth` iterations; global path: two per iteration).  *cur_out: the buffer that holds the result.
TileArgs tile_args(const flame_hip_graph* g, const SolveParams& sp);
int enqueue_by_launches(flame_hip_graph* g, const SolveParams& sp, int32_t iters, hipStream_t s, int cur, int* cur_out, int* launches);

}  // namespace flamehip
