// flame_ros_amd/csrc/resident.cpp -- the host side of the resident-tile solve (resident.h): the device's lease, the pool of
// uncached memory behind the hand-off buffers, the poll lists, one launch of k_tile_persist for a whole solve, and what a
// launch that gave up leaves behind -- the record of how far its tiles got, the lease's back-off, the repeat of the solve
// (or of the whole queue of solves) by ordinary launches through flame_hip.cpp's enqueue_by_launches().
#include "resident.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "graph_handle.h"

namespace flamehip {
namespace {

constexpr int kPollDelayDefault = 2;  // x 256 clocks.  r05, address-sorted poll: a pass is short enough to sample memory before the neighbours' stores have landed (passes per round 1.35 at 0, 1.10 at 2, 1.01 at 3; 50 k 1.316 / 1.319 / 1.304 / 1.303 / 1.357 us per iteration at 0 / 1 / 2 / 3 / 4, profiles/r05_sorted_poll_delay.txt; swept again in r06 behind the one-block poll: 1.313 / 1.334 / 1.309 / 1.329 / 1.350); option "poll_delay" overrides

// Hand-off buffers live in UNCACHED device memory (hipDeviceMallocUncached: no L2 holds it, so stores and loads of different
// XCDs meet in memory while a kernel runs -- the hand-off copies of the resident tiles, kernels.hip PersistArgs).  Uncached
// blocks are never handed back to the runtime: on this stack (ROCm 7.2) a later ordinary hipMalloc that recycles such a
// block misbehaves (tools/exp/fault_repro.py: the plan builder's kernels fault on it), so freed blocks wait in a
// process-wide pool, per device, for the next uncached request (bounded by the largest graph the process has seen).
struct UncachedPool {
  std::mutex m;
  struct Block { void* p; size_t bytes; int device; };
  std::vector<Block> free_blocks;
  void* take(int device, size_t bytes, size_t* got) {
    std::lock_guard<std::mutex> lk(m);
    size_t best = free_blocks.size();
    for (size_t i = 0; i < free_blocks.size(); ++i)
      if (free_blocks[i].device == device && free_blocks[i].bytes >= bytes &&
          (best == free_blocks.size() || free_blocks[i].bytes < free_blocks[best].bytes))
        best = i;
    if (best == free_blocks.size()) return nullptr;
    void* p = free_blocks[best].p;
    *got = free_blocks[best].bytes;
    free_blocks.erase(free_blocks.begin() + (long)best);
    return p;
  }
  void give(int device, void* p, size_t bytes) {
    std::lock_guard<std::mutex> lk(m);
    free_blocks.push_back({p, bytes, device});
  }
};
UncachedPool& uncached_pool() {
  static UncachedPool* pool = new UncachedPool();  // (never destroyed: handles may outlive static destruction order)
  return *pool;
}
// (the blocks are NOT registered in the handle's CapMap: free_device() must not hipFree them; *cap = bytes of *p)
template <class T>
int dev_alloc_uncached(int device, T** p, size_t* cap, size_t n, bool* fresh) {
  n += 1;
  const size_t bytes = n * sizeof(T);
  *fresh = false;
  if (*p && *cap >= bytes) return 0;
  if (*p) uncached_pool().give(device, *p, *cap);
  *p = nullptr; *cap = 0;
  *fresh = true;  // (contents unknown: the caller zeroes it)
  size_t got = 0;
  if (void* q = uncached_pool().take(device, bytes, &got)) {
    *p = static_cast<T*>(q); *cap = got;
    return 0;
  }
  const size_t want = bytes + bytes / 4;
  hipError_t e = hipExtMallocWithFlags(reinterpret_cast<void**>(p), want, hipDeviceMallocUncached);
  if (e == hipErrorOutOfMemory) return FLAME_HIP_ERR_ALLOC;
  if (e != hipSuccess) return FLAME_HIP_ERR_HIP - (int)e;
  *cap = want;
  return 0;
}

// The six hand-off buffers of a launch -- both round parities of the copies of A, B and q -- with their index 3 * b + k and
// their element counts; f(index, &pointer, elements) returns 0 to go on.
template <class F>
int for_handoff(float4* (&hA)[2], float4* (&hB)[2], float4* (&hq)[2], int32_t V, int32_t E, F f) {
  const size_t nn[3] = {(size_t)V, (size_t)V, (size_t)std::max(E, 1)};
  for (int b = 0; b < 2; ++b) {
    float4** pp[3] = {&hA[b], &hB[b], &hq[b]};
    for (int k = 0; k < 3; ++k)
      if (int rc = f(3 * b + k, pp[k], nn[k])) return rc;
  }
  return 0;
}

// Resident tiles need every workgroup of their launch on the chip at once.  Two such launches from two handles of one
// process can each get part of the CUs and starve each other until both time out, so a device has ONE lease: a handle
// takes it for a solve and holds it until that solve's end event has fired; a handle that finds it taken solves by
// ordinary launches.  After a launch gave up for any other reason (a foreign kernel holding CUs, another process) the
// whole process stays off resident tiles for a while: 16 solves, doubling up to 4096 with every further give-up.
struct PersistLease {
  std::mutex m;
  const flame_hip_graph* holder = nullptr;
  hipEvent_t holder_done = nullptr;  // (the holder's ev1)
  hipStream_t holder_stream = nullptr;  // the stream its launch went to: a launch queued BEHIND it on the same stream can
                                     // never be co-resident with it (the partition mode's parts of one rank)
  bool recorded = false;             // the holder's end event has been recorded behind its launch (until then: busy)
  bool one_xcd_broken = false;       // a one-XCD launch gave up on this device: the mode is off for the rest of the process
  int backoff = 0;                   // solves (of any handle) to sit out
  int backoff_next = 16;
  int gave_up = 0;                   // give-ups seen on this device (info "persist_gave_up")
};
PersistLease& persist_lease(int device) {
  static PersistLease leases[64];
  return leases[(unsigned)device & 63];
}
// wait_for_holder: a FAT plan -- halo depth 1 or 2, sized for ONE resident launch -- that finds the lease taken
// would otherwise run as one 256-workgroup launch per 1-2 iterations, several times slower than waiting for the other
// handle's solve to end; so it waits for the holder's end event (host side, bounded by that solve) and takes the lease then
bool persist_lease_take(const flame_hip_graph* g, hipStream_t s, bool wait_for_holder = false) {
  PersistLease& L = persist_lease(g->device);
  std::unique_lock<std::mutex> lk(L.m);
  if (L.backoff > 0) { --L.backoff; return false; }
  if (L.holder && L.holder != g && (!L.recorded || (L.holder_stream != s && hipEventQuery(L.holder_done) != hipSuccess))) {
    if (!wait_for_holder || !L.recorded || !L.holder_done) return false;
    hipEvent_t ev = L.holder_done;
    lk.unlock();
    const hipError_t e = hipEventSynchronize(ev);  // (the event belongs to a live handle of this process: handles outlive their solves)
    lk.lock();
    if (e != hipSuccess || (L.holder && L.holder != g && hipEventQuery(L.holder_done) != hipSuccess)) return false;
  }
  L.holder = g;
  L.holder_done = g->ev1;
  L.holder_stream = s;
  L.recorded = false;  // (flame_hip_solve records ev1 behind the launch, then ResidentSolve::end_recorded())
  return true;
}
void persist_lease_recorded(const flame_hip_graph* g) {
  PersistLease& L = persist_lease(g->device);
  std::lock_guard<std::mutex> lk(L.m);
  if (L.holder == g) L.recorded = true;
}
int persist_gave_up_count(int device) {
  PersistLease& L = persist_lease(device);
  std::lock_guard<std::mutex> lk(L.m);
  return L.gave_up;
}
int persist_backoff(int device) {
  PersistLease& L = persist_lease(device);
  std::lock_guard<std::mutex> lk(L.m);
  return L.backoff;
}
bool one_xcd_allowed(int device) {
  if (device < 0) return true;  // (a host-only plan: sized as the MI355X would)
  PersistLease& L = persist_lease(device);
  std::lock_guard<std::mutex> lk(L.m);
  return !L.one_xcd_broken;
}
void persist_lease_drop(const flame_hip_graph* g, bool gave_up, bool one_xcd_used) {
  PersistLease& L = persist_lease(g->device);
  std::lock_guard<std::mutex> lk(L.m);
  if (L.holder == g) { L.holder = nullptr; L.holder_done = nullptr; L.holder_stream = nullptr; }
  if (gave_up && one_xcd_used) L.one_xcd_broken = true;
  if (gave_up) {
    ++L.gave_up;
    L.backoff = L.backoff_next;
    L.backoff_next = std::min(L.backoff_next * 2, 4096);
  }
}

}  // namespace

size_t ResidentSolve::stage_bytes(const std::vector<TileDesc>& tiles) {
  int64_t stage = 0;
  for (const TileDesc& D : tiles) stage = std::max(stage, persist_stage_bytes(D));  // (plan.h)
  return (size_t)stage;
}

bool ResidentSolve::set_option(const std::string& k, int32_t value, int* rc) {
  *rc = 0;
  if (k == "persist") {
    persist_ = value != 0;  // (2 was r03's "also size small frames for it": the automatic tiles do as well now)
  } else if (k == "persist_prof") {
    if (value < 0) *rc = FLAME_HIP_ERR_ARG;
    else prof_want_ = value;
  } else if (k == "one_xcd") {
    one_xcd_opt_ = value != 0;
  } else if (k == "poll_delay") {  // x 256 clocks between a round's stores and its first poll pass; -1 = automatic
    if (value < -1 || value > 255) *rc = FLAME_HIP_ERR_ARG;
    else poll_delay_opt_ = value;
  } else if (k == "persist_timeout_us") {  // what a poll may wait before the launch gives up; 0 = automatic
    if (value < 0) *rc = FLAME_HIP_ERR_ARG;
    else timeout_opt_ = value;
  } else if (k == "need_marks") {  // fat tiles hand over only what somebody polls (default 1)
    need_marks_ = value != 0;
  } else {
    return false;
  }
  return true;
}

bool ResidentSolve::info(const flame_hip_graph* g, const std::string& k, int64_t* value, int* rc) const {
  *rc = 0;
  if (k == "persist") *value = persist_ ? 1 : 0;
  else if (k == "persist_used") *value = used_ ? 1 : 0;
  else if (k == "one_xcd_used") *value = (used_ && one_xcd_used_) ? 1 : 0;
  else if (k == "one_xcd") *value = one_xcd_opt_ ? 1 : 0;
  else if (k == "persist_recovered") *value = recovered_;
  else if (k == "persist_launches") *value = launches_;
  else if (k == "persist_timeout_us") *value = timeout_us_;
  else if (k == "persist_torn") {  // torn hand-off entries seen so far (only a FLAME_TORN_CHECK build counts; synchronise first)
    int32_t v = 0;
    if (xp_.prof && hipMemcpy(&v, xp_.prof + 8, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) *rc = FLAME_HIP_ERR_HIP;
    else *value = v;
  }
  else if (k == "persist_round_ns") *value = (int64_t)(round_us_ * 1e3f);
  else if (k == "persist_wait_us_max") {  // the longest a poll of any wave waited since the last look (read and cleared; synchronise first)
    int32_t v = 0;
    if (!xp_.prof) *value = 0;
    else if (hipMemcpy(&v, xp_.prof + 7, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess ||
             hipMemset(xp_.prof + 7, 0, sizeof(v)) != hipSuccess) *rc = FLAME_HIP_ERR_HIP;
    else *value = v / 100;
  }
  else if (k == "persist_gave_up") *value = persist_gave_up_count(g->device);  // (give-ups of any handle on this device)
  else if (k == "persist_backoff") *value = g->device >= 0 ? persist_backoff(g->device) : 0;  // solves the device's lease still sits out (plans uploaded meanwhile are sized for launches)
  else if (k == "one_xcd_allowed") *value = one_xcd_allowed(g->device) ? 1 : 0;  // 0: a one-XCD launch gave up in this process, the mode is off
  else if (k == "persist_gave_up_tile") *value = give_up_.tile;        // (this handle's last give-up, see GiveUp)
  else if (k == "persist_gave_up_round") *value = give_up_.round;
  else if (k == "persist_gave_up_front_round") *value = give_up_.front_round;
  else if (k == "persist_gave_up_not_started") *value = give_up_.not_started;
  else if (k == "persist_gave_up_rounds") *value = give_up_.rounds;
  else if (k == "persist_gave_up_tiles") *value = give_up_.tiles;
  else if (k == "persist_gave_up_one_xcd") *value = give_up_.one_xcd;
  else if (k == "persist_gave_up_timeout_us") *value = give_up_.timeout_us;
  else if (k.rfind("persist_prof_", 0) == 0) {  // dev aid (option "persist_prof" = <tile + 1>): 10 ns ticks of that tile, summed over rounds
    const int i = std::atoi(k.c_str() + 13);
    int32_t v = 0;
    if (i < 0 || i > 4 || !xp_.prof) *rc = FLAME_HIP_ERR_ARG;
    else if (hipMemcpy(&v, xp_.prof + 2 + i, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) *rc = FLAME_HIP_ERR_HIP;
    else *value = v;
  }
  else return false;
  return true;
}

// (plan-only handles size their tiles the same way: they are the device plans' reference.  ADVICE r4: the depth follows
// whether resident tiles can actually be taken -- not while the device's lease sits out a back-off after a give-up, not
// under the in-kernel timeline -- because depth 5 by ordinary launches is the slower configuration)
void ResidentSolve::sizing(const flame_hip_graph* g, bool* resident, bool* one_xcd) const {
  *resident = persist_ && !g->prof && (g->device < 0 || persist_backoff(g->device) == 0);
  *one_xcd = *resident && one_xcd_opt_ && g->opt.num_cus >= 256 && one_xcd_allowed(g->device);
}

bool ResidentSolve::applies(const flame_hip_graph* g, int32_t num_iters) const {
  const Plan& P = g->plan;
  if (!persist_ || g->path != FLAME_HIP_PATH_TILE || g->prof || P.tile_depth <= 0 || num_iters <= P.tile_depth) return false;
  const size_t nt = P.tiles.size();
  if (nt < 2 || nt > (size_t)kPersistMaxTiles || (int)nt > g->num_cus) return false;  // (one workgroup per CU is always resident)
  for (const TileDesc& D : P.tiles)
    if (D.n_ext <= 0) return false;  // (an empty tile has nothing to hand over, but its neighbours would not know)
  // (r05: what a tile polls is delivered through an LDS staging area behind its incidence slots)
  return resident_fits(P.tile_lds_bytes, (int64_t)stage_bytes(P.tiles), P.tile_slot12, P.tile_threads, P.tile_ept, P.tile_vpt,
                       g->opt.lds_bytes);
}

void ResidentSolve::plan_changed(int32_t V) {
  poll_valid_ = false;  // (new tile arrays: the poll lists are rebuilt at the next launch)
  // (the round time the resident launches' time-out follows was measured on ANOTHER graph -- a frame stream's
  // next frame is about as large and keeps it, a graph of another size starts again from the 4 ms of a first launch)
  if (round_V_ > 0 && (V > 2 * round_V_ || 2 * V < round_V_)) { round_us_ = 0.f; round_V_ = 0; }
}

void ResidentSolve::release(flame_hip_graph* g) {
  persist_lease_drop(g, false, one_xcd_used_);
  for_handoff(xp_.hA, xp_.hB, xp_.hq, 0, 0, [&](int i, float4** p, size_t) {  // (uncached blocks go back to the pool, never to the runtime)
    if (*p) uncached_pool().give(g->device, *p, xp_cap_[i]);
    *p = nullptr; xp_cap_[i] = 0;
    return 0;
  });
  if (err_) (void)hipHostFree(err_);
  err_ = nullptr;
}

// The tiles' poll lists: in local order for the FIRST solve of a plan (a frame of a stream is solved once and would not
// earn the sorts back), address-sorted from the second solve on (a resident graph; the lane order, applied then,
// invalidates them anyway)
int ResidentSolve::poll_lists(flame_hip_graph* g, hipStream_t s) {
  const Plan& P = g->plan;
  PersistBufs& x = xp_;
  const bool want_sorted = g->solves_since_upload > 0;
  if (poll_valid_ && (!want_sorted || poll_sorted_)) return 0;
  int rc;
  size_t nv_loc = 0, ne_loc = 0;
  for (const TileDesc& D : P.tiles) { nv_loc += (size_t)D.n_ext; ne_loc += (size_t)D.e_loc; }
  // (+ 1: a tile without local edges still reads the list's entry at its own offset -- the last tile's is one past the end)
  if ((rc = dev_alloc(g->caps, &x.poll_v, nv_loc + 1)) || (rc = dev_alloc(g->caps, &x.poll_e, ne_loc + 1)) ||
      (rc = dev_alloc(g->caps, &x.poll_ne, P.tiles.size())))
    return rc;
  // (r05: the sorted lists' kernel also marks what anybody polls; the rest of a tile's own entries is not handed over.
  // A plan's first solve -- a frame of a stream -- stores everything and pays neither the marks nor their memsets)
  x.need_valid = false;
  if (want_sorted && need_marks_ && P.tile_fat) {  // (the FAT kernel variants read the marks)
    if ((rc = dev_alloc(g->caps, &x.need_v, std::max<size_t>((size_t)g->V, 1))) || (rc = dev_alloc(g->caps, &x.need_e, std::max<size_t>((size_t)g->E, 1))))
      return rc;
    HIPCHK(hipMemsetAsync(x.need_v, 0, sizeof(int32_t) * std::max<size_t>((size_t)g->V, 1), s));
    HIPCHK(hipMemsetAsync(x.need_e, 0, sizeof(int32_t) * std::max<size_t>((size_t)g->E, 1), s));
    x.need_valid = true;
  }
  HIPCHK(launch_poll_lists(s, (int32_t)P.tiles.size(), g->tiles, g->t_vmap, g->t_emap, g->t_eij, x.poll_v, x.poll_e, x.poll_ne, want_sorted,
                           x.need_valid ? x.need_v : nullptr, x.need_valid ? x.need_e : nullptr));
  poll_sorted_ = want_sorted;
  x.stage_bytes = stage_bytes(P.tiles);
  poll_valid_ = true;
  return 0;
}

// The hand-off buffers of this launch, in *xl: the uncached ones, or -- a graph of up to kOneXcdTiles tiles kept on ONE XCD --
// copies in ordinary memory.  A new, recycled or re-grown buffer is zeroed: tag 0 is never a round's, garbage could pass for one.
int ResidentSolve::handoff_buffers(flame_hip_graph* g, hipStream_t s, bool rezero, PersistBufs* xl) {
  int rc = for_handoff(xp_.hA, xp_.hB, xp_.hq, g->V, g->E, [&](int i, float4** p, size_t n) {
    bool fresh = false;
    if (int r = dev_alloc_uncached(g->device, p, &xp_cap_[i], n, &fresh)) return r;
    if (fresh || rezero) HIPCHK(hipMemsetAsync(*p, 0, xp_cap_[i], s));
    return 0;
  });
  if (rc) return rc;
  *xl = xp_;  // (what this launch gets)
  one_xcd_used_ = false;
  if (!(one_xcd_opt_ && g->plan.tiles.size() <= (size_t)kOneXcdTiles && g->num_cus >= 256 && one_xcd_allowed(g->device))) return 0;
  rc = for_handoff(cA_, cB_, cq_, g->V, g->E, [&](int i, float4** p, size_t n) {
    if (int r = dev_alloc(g->caps, p, n)) return r;
    const size_t cap_now = g->caps[(void*)p];
    if (c_zeroed_[i] != (void*)*p || c_zeroed_cap_[i] != cap_now || rezero) {  // (address AND capacity: no reallocation since)
      HIPCHK(hipMemsetAsync(*p, 0, cap_now, s));
      c_zeroed_[i] = (void*)*p;
      c_zeroed_cap_[i] = cap_now;
    }
    return 0;
  });
  if (rc) return rc;
  for (int b = 0; b < 2; ++b) { xl->hA[b] = cA_[b]; xl->hB[b] = cB_[b]; xl->hq[b] = cq_[b]; }
  xl->one_xcd = 1;
  one_xcd_used_ = true;
  return 0;
}

int ResidentSolve::launch(flame_hip_graph* g, const SolveParams& sp, int32_t num_iters, hipStream_t s, int cur, bool* taken) {
  const Plan& P = g->plan;
  *taken = false;
  used_ = false;
  if (!applies(g, num_iters) || !persist_lease_take(g, s, P.tile_fat && P.tile_depth <= 2)) return 0;
  PersistBufs& x = xp_;
  int rc;
  if (!err_) {
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&err_), 64, hipHostMallocDefault));
    *err_ = 0;
  }
  if (!x.prof || prof_set_ != prof_want_) {  // dev aid: which tile (if any) splits its rounds' time
    if ((rc = dev_alloc(g->caps, &x.prof, 16))) return rc;
    int32_t w[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int want = prof_want_;
    if (want > 0) { w[0] = 1; w[1] = want - 1; }
    HIPCHK(memcpy_sync(s, x.prof, w, sizeof(w), hipMemcpyHostToDevice));
    prof_set_ = prof_want_;
  }
  const int rounds = (num_iters + P.tile_depth - 1) / P.tile_depth;
  bool rezero = base_ > (1 << 23);  // (the tags only grow; 2^23: the torn-read debug build compares 24 bits)
  if (rezero) base_ = 0;
  if ((rc = poll_lists(g, s))) return rc;
  PersistBufs xl;
  if ((rc = handoff_buffers(g, s, rezero, &xl))) return rc;
  TileArgs a = tile_args(g, sp);
  a.A_src = g->A[cur]; a.B_src = g->B[cur]; a.q_src = g->q[cur];
  a.A_dst = g->A[cur ^ 1]; a.B_dst = g->B[cur ^ 1]; a.q_dst = g->q[cur ^ 1];
  a.iters = num_iters;
  {
    // (the lists in local order: a pass is long enough, 0; fat tiles with a 1- or 2-iteration round: the hand-off is the
    // larger part of the round and the first pass should not wait -- 200 k 3.02 / 3.05 / 3.13 / 3.15 / 3.23 us per
    // iteration at 0 .. 4, 160 k and 100 k (depth 3) flat: profiles/r05_fat_poll_delay.txt)
    const bool short_fat_round = g->V > 256 * 196 && P.tile_depth <= 2;
    x.poll_delay = poll_delay_opt_ >= 0 ? poll_delay_opt_ : ((poll_sorted_ && !short_fat_round) ? kPollDelayDefault : 0);
    // A poll waits at most max(0.5 ms, 8 x the handle's last measured round) -- r04's flat 4 ms was 5.5 headline
    // solves; 4 ms while nothing has been measured.  Option "persist_timeout_us" overrides.
    const float us = timeout_opt_ > 0 ? (float)timeout_opt_ : (round_us_ > 0.f ? std::max(500.f, 8.f * round_us_) : 4000.f);
    timeout_us_ = (int32_t)std::min(us, 1.0e6f);
    x.timeout_ticks = timeout_us_ * 100;
    const int stall_us = test_persist_stall_us();  // (hooks library: a REAL late tile, tests/test_gpu_persist.py)
    if (stall_us > 0 && tile_stall_hook_build()) x.poll_delay = (x.poll_delay & 0xff) | (stall_us << 8);  // (microseconds, bits 8.. of poll_delay; debug kernels only)
  }
  last_rounds_ = rounds;
  // (one XCD: a pass through the L2 is short and cheap -- no pause in front of the first one, profiles/r06_one_xcd_ab.txt)
  xl.poll_delay = (xl.one_xcd && poll_delay_opt_ < 0) ? 0 : x.poll_delay;
  xl.timeout_ticks = x.timeout_ticks;
  HIPCHK(launch_tile_persist(s, P.tile_threads, P.tile_ept, P.tile_vpt, (size_t)P.tile_lds_bytes, a, xl, err_, base_));
  give_up_base_ = base_;
  base_ += rounds - 1;
  used_ = true;
  unchecked_ = true;
  ++unchecked_n_;
  ++launches_;
  last_src_ = cur;
  *taken = true;  // (the result is in buffer cur ^ 1: written once, by the last round; the source buffers are only read)
  return 0;
}

// r05: a solve queued behind an unchecked resident one -- before it overwrites that one's source, the source is set aside
int ResidentSolve::before_solve(flame_hip_graph* g, hipStream_t s, const SolveParams& sp, int32_t num_iters) {
  if (unchecked_n_ == 0) forget_queue();
  if (queued_.size() == 1 && !qsnap_valid_ && g->state_serial == queued_serial_ + 1 && num_iters > 0) {
    int rc;
    if ((rc = dev_alloc(g->caps, &qsnapA_, (size_t)g->V)) || (rc = dev_alloc(g->caps, &qsnapB_, (size_t)g->V)) ||
        (rc = dev_alloc(g->caps, &qsnapq_, (size_t)std::max(g->E, 1))))
      return rc;
    const int src = queued_src_;
    if ((rc = copy_state(s, {qsnapA_, qsnapB_, qsnapq_}, {g->A[src], g->B[src], g->q[src]}, g->V, g->E))) return rc;
    qsnap_valid_ = true;
  }
  last_sp_ = sp; last_iters_ = num_iters;
  // (a hipGraph replay or a solve of 0 iterations does not pass through launch(); without this a stale
  // `used_` made check() repeat the SHORT solve from buffers the replay had already overwritten)
  used_ = false;
  return 0;
}

void ResidentSolve::after_solve(flame_hip_graph* g, const SolveParams& sp, int32_t num_iters, int cur_before, uint64_t serial_before) {
  solve_serial_ = g->state_serial;
  if (num_iters <= 0 || g->V <= 0) return;
  // the log of what a give-up would have to repeat (behind the first entry every solve is logged, copy or not: without
  // one something else wrote the state in between, and the check refuses)
  if (!queued_.empty()) queued_.push_back({sp, num_iters});
  else if (used_) { queued_.push_back({sp, num_iters}); queued_src_ = cur_before; queued_serial_ = serial_before; }
}

void ResidentSolve::end_recorded(flame_hip_graph* g) {
  if (used_) persist_lease_recorded(g);
}

// A launch of resident tiles gave up: say how far its tiles got (cold path, nothing in the kernel -- a per-tile record written at
// the time-out cost every size 3-5 % through the poll loop's registers and code layout, profiles/r06_giveup_record_ab.txt).
// The x_bar hand-off copies of both parities still hold what the LAST launch's tiles stored: a tile's highest tag above the
// launch's base is the last round it handed over.  The tile with the lowest one is the late one (0 rounds: it never started) or,
// when the late one caught up after its neighbours had stopped, stood next to it.  analyse = false: the plan is no longer the
// launch's (a new upload), only the launch's own numbers are kept.
void ResidentSolve::note_give_up(const flame_hip_graph* g, bool analyse) {
  GiveUp u;
  u.tiles = (int32_t)g->plan.tiles.size();
  u.one_xcd = one_xcd_used_ ? 1 : 0;
  u.timeout_us = timeout_us_;
  u.rounds = last_rounds_;
  const int32_t V = g->V, base = give_up_base_;
  float4* const* hB = one_xcd_used_ ? cB_ : xp_.hB;
  if (analyse && V > 0 && hB[0] && hB[1] && used_ && *err_ == 1) {  // (a forced failure of the hooks library: nothing to look at)
    std::vector<float4> e0((size_t)V), e1((size_t)V);
    if (hipMemcpy(e0.data(), hB[0], sizeof(float4) * (size_t)V, hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(e1.data(), hB[1], sizeof(float4) * (size_t)V, hipMemcpyDeviceToHost) == hipSuccess) {
      for (int t = 0; t < u.tiles; ++t) {
        const TileDesc& T = g->plan.tiles[t];
        int32_t last = 0;
        for (int32_t v = T.vstart; v < T.vstart + T.n_own && v < V; ++v)
          for (const float4* e : {&e0[(size_t)v], &e1[(size_t)v]}) {
            int32_t tag;
            std::memcpy(&tag, &e->w, sizeof(tag));
            if (tag > base && tag - base <= u.rounds) last = std::max(last, tag - base);
          }
        if (last == 0) ++u.not_started;
        if (u.tile < 0 || last < u.round) { u.tile = t; u.round = last; }
        u.front_round = std::max(u.front_round, last);
      }
    } else (void)hipGetLastError();
  }
  give_up_ = u;
}

// (Called behind the upload's own wait for the solves before it.)
void ResidentSolve::discard(flame_hip_graph* g) {
  forget_queue();
  if (!unchecked_) return;
  unchecked_ = false;
  unchecked_n_ = 0;
  if (test_persist_fail() && used_ && err_) *err_ = 3;  // (hooks library only, as in check())
  if (err_ && *err_ != 0) {
    note_give_up(g, false);
    *err_ = 0;
    persist_lease_drop(g, true, one_xcd_used_);
  }
}

// The launch only reads its source buffers, so it can be repeated whenever nothing else wrote the state since; anything
// but the caller's own_marks that wrote it (a graph filter, new data terms) cannot be replayed here.
int ResidentSolve::check(flame_hip_graph* g, int own_marks) {
  if (test_persist_fail() && used_ && err_) *err_ = 3;  // (hooks library only: the recovery path)
  unchecked_ = false;  // (every caller has synchronised the solve's stream)
  const int unchecked = unchecked_n_;
  unchecked_n_ = 0;
  if (!err_ || *err_ == 0) {
    if (used_ && last_rounds_ > 0 && unchecked == 1) {  // the round time the next launch's time-out follows
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, g->ev0, g->ev1) == hipSuccess && ms > 0.f) { round_us_ = ms * 1e3f / (float)last_rounds_; round_V_ = g->V; }
      else (void)hipGetLastError();
    }
    forget_queue();
    return 0;
  }
  note_give_up(g);
  *err_ = 0;
  persist_lease_drop(g, true, one_xcd_used_);
  // r05: a queue of solves is repeated as a whole from the state copied aside in front of its second member; one solve
  // from its own untouched source.  (Several solves queued WITHOUT that copy: an earlier one may have been the one that gave
  // up, and the later ones started from its unfinished result -- nothing to repeat from.)
  std::vector<QueuedSolve> q;
  q.swap(queued_);
  const bool whole_queue = q.size() > 1;
  const bool can = whole_queue ? qsnap_valid_ && g->state_serial == queued_serial_ + (uint64_t)q.size() + (uint64_t)own_marks
                               : used_ && unchecked <= 1 && g->state_serial == solve_serial_ + (uint64_t)own_marks && last_iters_ > 0;
  qsnap_valid_ = false;
  used_ = false;
  if (!can) {
    g->uploaded = false;  // the state is that of an unfinished solve
    return FLAME_HIP_ERR_STATE;
  }
  hipStream_t s = g->last_stream ? g->last_stream : g->stream;
  int cur = last_src_, total_launches = 0;
  if (whole_queue) {
    cur = queued_src_;
    if (int rc = copy_state(s, {g->A[cur], g->B[cur], g->q[cur]}, {qsnapA_, qsnapB_, qsnapq_}, g->V, g->E)) return rc;
  } else {
    q.assign(1, {last_sp_, last_iters_});
  }
  HIPCHK(hipEventRecord(g->ev0, s));
  for (const QueuedSolve& e : q) {
    int launches = 0;
    if (int rc = enqueue_by_launches(g, e.sp, e.iters, s, cur, &cur, &launches)) return rc;
    total_launches += launches;
  }
  g->cur = cur;
  g->state_serial++;
  g->last_launches = total_launches;
  HIPCHK(hipEventRecord(g->ev1, s));
  ++recovered_;
  return 1;
}

void ResidentSolve::take_error(flame_hip_graph* g, int32_t* gave_up) {
  *gave_up = 0;
  const bool had = unchecked_;
  unchecked_ = false;
  unchecked_n_ = 0;
  forget_queue();  // (the caller -- the partition mode -- keeps snapshots of its own)
  if (had && err_ && (*err_ != 0 || test_persist_fail())) {
    note_give_up(g);
    *err_ = 0;
    persist_lease_drop(g, true, one_xcd_used_);
    used_ = false;
    *gave_up = 1;
  }
}

}  // namespace flamehip
