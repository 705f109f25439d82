// flame_ros_amd/csrc/resident.h -- the host side of the resident-tile solve (option "persist", kernels.hip k_tile_persist):
// one member of the handle (graph_handle.h, g->res).  The handle's driver (flame_hip.cpp) asks it whether a solve can go by
// ONE launch of resident tiles, lets it try, and tells it about the calls around a solve; everything else -- the device's
// lease, the hand-off buffers and their pool of uncached memory, the poll lists, the time-out, what a give-up leaves behind
// and how the solve is repeated by launches -- is private to resident.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "kernels.h"

struct flame_hip_graph;

namespace flamehip {

class ResidentSolve {
 public:
  // LDS the poll delivery of a partition's resident launch needs behind a tile's incidence slots (max over the tiles)
  static size_t stage_bytes(const std::vector<TileDesc>& tiles);

  // options / info keys of the resident solve: true when the key was theirs (*rc = the call's return code)
  bool set_option(const std::string& key, int32_t value, int* rc);
  bool info(const flame_hip_graph* g, const std::string& key, int64_t* value, int* rc) const;
  // PlanOptions::resident / ::one_xcd of the next plan: what the tiles are sized for
  void sizing(const flame_hip_graph* g, bool* resident, bool* one_xcd) const;

  // one launch of resident tiles instead of ceil(iters / depth) launches?
  bool applies(const flame_hip_graph* g, int32_t iters) const;
  // ... enqueued on s, from buffer cur into cur ^ 1.  *taken = false: the device's lease is busy or sits out a back-off,
  // nothing was enqueued and the caller goes by launches.
  int launch(flame_hip_graph* g, const SolveParams& sp, int32_t iters, hipStream_t s, int cur, bool* taken);
  bool used() const { return used_; }        // the last solve went by a launch of resident tiles (info "persist_used")
  bool pending() const { return unchecked_; }  // a resident launch is in flight / finished and nobody has looked at its error word

  // flame_hip_solve, in front of the solve's start event / behind its bookkeeping / behind its end event
  int before_solve(flame_hip_graph* g, hipStream_t s, const SolveParams& sp, int32_t iters);
  void after_solve(flame_hip_graph* g, const SolveParams& sp, int32_t iters, int cur_before, uint64_t serial_before);
  void end_recorded(flame_hip_graph* g);

  // After a synchronisation: did a launch give up?  0 = no, 1 = the solve (or the queue of solves) was REPEATED by
  // launches -- enqueued, not waited for --, else an error code.  own_marks: state-writing steps the caller queued behind
  // the solve and will redo.
  int check(flame_hip_graph* g, int own_marks = 0);
  // A new upload throws the state of the solves before it away: a give-up only matters for the lease and the back-off.
  void discard(flame_hip_graph* g);
  // flame_hip_persist_take_error: the caller owns the recovery
  void take_error(flame_hip_graph* g, int32_t* gave_up);

  void plan_changed(int32_t V);               // new tile arrays (an upload)
  void lanes_changed() { poll_valid_ = false; }  // edges moved inside their 64-blocks: a poll record names a position
  void release(flame_hip_graph* g);           // the handle is destroyed (its streams are idle)

 private:
  struct GiveUp { int32_t tile = -1, round = -1, front_round = 0, not_started = 0, rounds = 0, tiles = 0, one_xcd = 0, timeout_us = 0; };
  struct QueuedSolve { SolveParams sp; int32_t iters; };

  void note_give_up(const flame_hip_graph* g, bool analyse = true);
  int poll_lists(flame_hip_graph* g, hipStream_t s);
  int handoff_buffers(flame_hip_graph* g, hipStream_t s, bool rezero, PersistBufs* xl);
  void forget_queue() { queued_.clear(); qsnap_valid_ = false; }

  // option "persist" (default 1): graphs of 2 .. min(kPersistMaxTiles, CUs) halo tiles are solved by ONE launch of
  // RESIDENT tiles (kernels.hip k_tile_persist: round-tagged hand-offs through uncached memory instead of a kernel
  // boundary per `depth` iterations); 0: launches
  bool persist_ = true, used_ = false;
  int64_t launches_ = 0;        // launches of resident tiles so far (info "persist_launches")
  float round_us_ = 0.f;        // device time of a round of the last resident solve that was looked at (0 = none yet)
  int32_t round_V_ = 0;         // ... and the size of the graph it was measured on
  int32_t last_rounds_ = 0;     // rounds of the last resident launch
  int32_t timeout_us_ = 0;      // what the last resident launch was given (info "persist_timeout_us")
  PersistBufs xp_;              // hand-off buffers (uncached, from the process-wide pool: NOT in caps) + dev-aid words
  size_t xp_cap_[6] = {0, 0, 0, 0, 0, 0};
  // r06, option "one_xcd" (default 1): a graph of up to 32 resident tiles keeps them on ONE XCD -- the launch has 8 x ntiles
  // workgroups of which every 8th carries a tile -- and hands over through ORDINARY memory, i.e. that XCD's L2 (0.5 us per
  // load instead of 0.9 through uncached memory: 1.2 k vertices 0.89 -> 0.81 us per iteration).  Which XCD a workgroup lands on
  // is the dispatcher's habit, not a guarantee: tiles on different XCDs would never see each other's tags, time out, and the
  // solve is repeated by launches like any give-up -- after which the device's lease never tries the mode again.
  bool one_xcd_opt_ = true, one_xcd_used_ = false;
  float4* cA_[2] = {nullptr, nullptr};  // the hand-off copies in ordinary memory
  float4* cB_[2] = {nullptr, nullptr};
  float4* cq_[2] = {nullptr, nullptr};
  void* c_zeroed_[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // the allocations that have been zeroed (tag 0 is never a
  size_t c_zeroed_cap_[6] = {0, 0, 0, 0, 0, 0};                                 // round's): address AND capacity, i.e. no reallocation since
  int poll_delay_opt_ = -1;     // option "poll_delay" (-1 = automatic)
  int timeout_opt_ = 0;         // option "persist_timeout_us" (0 = automatic)
  bool need_marks_ = true;      // option "need_marks"
  int prof_want_ = 0, prof_set_ = 0;  // option "persist_prof": tile + 1 that records its round split (0 = none)
  bool poll_valid_ = false;     // the poll lists (xp_.poll_*) belong to the current tile arrays
  bool poll_sorted_ = false;    // ... and are the address-sorted ones (from a plan's second solve on)
  bool unchecked_ = false;      // a resident launch is in flight / finished and nobody has looked at err_ yet
  int unchecked_n_ = 0;         // ... how many of them (the error word does not say WHICH launch gave up: only when it
                                // can only have been the last solve is that solve repeated)
  int last_src_ = 0;            // the buffer the last solve started from
  int32_t* err_ = nullptr;      // page-locked: raised by a launch whose wait timed out
  int32_t base_ = 0;            // the hand-off tags used so far (they only grow)
  SolveParams last_sp_{};       // the last solve (a resident launch that gave up is repeated by launches)
  int32_t last_iters_ = 0;
  int recovered_ = 0;           // how many solves were repeated that way (info "persist_recovered")
  // the last give-up of this handle, for whoever has to find out why (info "persist_gave_up_tile" / _round / _front_round /
  // _not_started / _rounds / _tiles / _one_xcd / _timeout_us, note_give_up()): the tile that had handed over the fewest
  // rounds and how many, the most any tile had, the tiles that had handed over none, the launch's rounds
  GiveUp give_up_;
  int32_t give_up_base_ = 0;    // base_ of the last resident launch (its tags are give_up_base_ + 1 ..)
  uint64_t solve_serial_ = 0;   // state_serial right behind the last solve: later state-writing calls move on from it
  // r05: SEVERAL solves queued behind each other without a synchronising call are repeatable too (a bench window, a caller
  // that pipelines solves): every solve from the first unchecked resident one on is logged, and when a second one is queued
  // the source buffers of the first -- which it would overwrite -- are copied aside first (device to device, once per
  // synchronising call).  A give-up then restores that state and repeats the whole queue by launches.
  std::vector<QueuedSolve> queued_;  // since the last look, the first unchecked resident solve first
  int queued_src_ = 0;               // the buffer that solve started from
  uint64_t queued_serial_ = 0;       // state_serial in front of it
  float4 *qsnapA_ = nullptr, *qsnapB_ = nullptr, *qsnapq_ = nullptr;
  bool qsnap_valid_ = false;
};

}  // namespace flamehip
