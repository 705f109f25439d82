// flame_ros_amd/csrc/common.h -- structures shared by the host plan builder and the HIP kernels.
//
// Device data layout (all "internal" order = tile-major: the own vertices / own edges of tile t
// are contiguous, tiles follow a recursive-coordinate-bisection order so neighbours in the image
// are neighbours in memory):
//   vtxA[V] float4 {x, w1, w2, z}        primal state + data term      (ping-pong x2)
//   vtxB[V] float4 {xb, w1b, w2b, wgt}   extrapolated state + weight   (ping-pong x2)
//   q[E]    float4 {q1, q2, q3, 0}       dual state                    (ping-pong x2)
//   eij[E]  int2   {i, j}                internal endpoints, i = source (global path)
//   ew[E]   float4 {alpha, beta, dx, dy} d = pos_i - pos_j
//   grow[V+1], ginc[2E]                  vertex -> incident edges, ascending ORIGINAL edge id,
//                                        bit 31 set when the vertex is the edge's target
// Tile plan (tile path): per tile a TileDesc + slices of the flat arrays t_vmap / t_eij /
// t_ew / t_emap / t_srow (see TileDesc).
#pragma once
#include <math.h>
#include <stdint.h>

namespace flamehip {

constexpr int kMaxDepth = 16;    // max halo depth (iterations per tile launch)
constexpr int kProfWords = 2 * kMaxDepth + 4;  // debug timeline words per tile
#ifndef FLAME_SLOT_ROUND
#define FLAME_SLOT_ROUND 6
#endif
constexpr int kSlotRound = FLAME_SLOT_ROUND;    // incidence slots summed per round of phase P
constexpr int kDummySlots = 64;  // per-lane trash slots behind the incidence slots (inert writes);
                                 // one more, always +0, follows them (reads past a vertex's degree)

struct SolveParams {
  float lambda, tau, sigma, theta, x_min, x_max;
  float tl;  // tau * lambda, rounded once on the host exactly like the oracle does
};

// One LDS-resident subdomain.  Local vertices are ordered by ring (graph distance from the own
// set): ring 0 = own = internal ids [vstart, vstart+n_own); t_vmap lists all n_ext ids.  Local
// edges are ordered by level = max(ring_i, ring_j); the first e_own of them are owned
// (source vertex is own) = internal edge ids [estart, estart+e_own); t_emap lists all e_loc ids.
struct TileDesc {
  int32_t vstart, n_own, n_ext;
  int32_t estart, e_own, e_loc;
  int32_t n_upd;      // local vertices that are ever updated (ring <= depth-1, or all if depth 0)
  int32_t depth;      // halo depth D (0: isolated tile, any number of iterations per launch)
  int32_t vmap_off;   // into t_vmap: n_ext internal vertex ids (gather list, own first)
  int32_t emap_off;   // into t_emap: e_loc internal edge ids (gather list of q, owned first)
  int32_t erec_off;   // into t_eij / t_ew: e_loc records
  int32_t srow_off;   // into t_srow: n_upd packed {slot of incidence 0 | degree << 16}
  int32_t nslots;     // incidence slots (one row per vertex, odd pitch per 64-vertex group)
  int32_t ring_end[kMaxDepth + 1];   // ring_end[r] = #local vertices with ring <= r
  int32_t level_end[kMaxDepth + 1];  // level_end[l] = #local edges with level <= l
};

// LDS of a tile's workgroup: bar[n_ext] (16 B) + the incidence slots, 16 B each -- or, slot12 (fat tiles), 12 B each as a
// 4-byte and an 8-byte array, the slot count rounded up to 4 (kernels.hip SlotMem).  Resident tiles add their staging area.
constexpr int64_t kTileLdsReserve = 64;  // the tile kernels' static LDS (two words) + alignment: a dynamic request of exactly
                                         // the CU's 160 KiB does not launch (found by the fat-size frame soak, r05)
// fat tiles keep a margin to the CU's LDS, and 16-byte slots at depth 1 -- the last configuration tried before the 12-byte
// layout, i.e. the one that ends up closest to 160 KiB -- a larger one: in frame streams of 185-200 k-vertex frames four
// solves in ~1 900 on such plans (156-160 KiB per tile) took 11-27 ms instead of 0.3 (correct bits, no give-up: some tile
// started that late; not reproduced on a resident graph, nor with 12-byte slots at 146-150 KiB).  Cause not found; avoided.
constexpr int64_t kFatLdsMargin = 4096;
constexpr int64_t kFatLdsMarginDepth1 = 12288;
inline int64_t tile_lds_bytes(int32_t n_ext, int32_t nslots, bool slot12) {
  const int64_t n = (int64_t)nslots + kDummySlots + 1;
  return slot12 ? (int64_t)n_ext * 16 + ((n + 3) & ~(int64_t)3) * 12 : (int64_t)n_ext * 16 + n * 16;
}

// ---- incidence-slot layout of a tile: ONE statement for every plan builder (plan.cpp on the host; plan_dev.hip's fused tile pass,
// pass 2 and the one-launch mini plan on the device) and for what the kernels assume (kernels.hip phase P).  One row per
// UPDATED local vertex; the 64 vertices a wavefront updates together (local ids 64 g .. 64 g + 63) share one pitch = their
// largest degree made ODD, so that a column read -- lane l reads row_l[j] -- touches 64 different 16-byte slots, a multiple of
// an odd number apart: conflict-free for ds_read_b128 (and for the split 12-byte layout's b64 / b32 reads); rows are
// zero-padded up to the pitch (phase P sums the wave's longest row from every row: fmaf(-tau, +0, x) == x).  A group takes 64
// pitches even when it holds fewer vertices (the last group of a tile).  Slot numbers are 16 bits (edge records pack two).
#ifdef __HIPCC__
#define FLAME_HD __host__ __device__
#else
#define FLAME_HD
#endif
FLAME_HD inline int32_t slot_group_pitch(int32_t max_degree_of_group) { return (max_degree_of_group < 1 ? 1 : max_degree_of_group) | 1; }
FLAME_HD inline int32_t slot_group_span(int32_t pitch) { return 64 * pitch; }
FLAME_HD inline bool slot_group_fits(int32_t base, int32_t pitch) { return base + slot_group_span(pitch) + kDummySlots <= 65535; }
FLAME_HD inline int32_t slot_row_start(int32_t group_base, int32_t lv, int32_t pitch) { return group_base + (lv & 63) * pitch; }
FLAME_HD inline uint32_t slot_row_word(int32_t row_start, int32_t degree) { return (uint32_t)row_start | ((uint32_t)degree << 16); }  // t_srow

// Cost model of a tile for the balance of the partition (both plan builders, integer): a launch / a round lasts as long as its
// slowest tile -- local edges + 2 x local vertices (r02).  (r05 tried local edges + 2 x UPDATED vertices, what a resident tile's
// iterate time correlates with best at 50 k: -1 % there, +6...18 % at 20 k / 100 k / 200 k, profiles/r05_cost_model_ab.txt.)
FLAME_HD inline long long tile_cost(const TileDesc& D) { return (long long)D.e_loc + 2 * (long long)D.n_ext; }
// Integer cost density of a tile (x 1024): what one own vertex of the tile "costs" a launch.  Integer so that sums of it are
// exact whatever the summation order (a host loop, device atomics).
FLAME_HD inline int32_t tile_weight(const TileDesc& D) {
  const long long w = tile_cost(D) * 1024 / (D.n_own > 1 ? D.n_own : 1);
  return (int32_t)(w > 1 ? w : 1);
}
// Cell of a position in the kCostGrid x kCostGrid cost-density field over the bounding box [mn, mx] of a frame's positions
// (Plan::wgrid: the next frame's balance weights).  Float arithmetic, so every builder evaluates this one expression.
constexpr int kCostGrid = 32;
FLAME_HD inline int cost_grid_cell(const float* mn, const float* mx, float x, float y) {
  const float fx = (x - mn[0]) / fmaxf(mx[0] - mn[0], 1e-20f);
  const float fy = (y - mn[1]) / fmaxf(mx[1] - mn[1], 1e-20f);
  const int ix = (int)(fx * kCostGrid), iy = (int)(fy * kCostGrid);
  const int cx = ix < 0 ? 0 : (ix > kCostGrid - 1 ? kCostGrid - 1 : ix);
  const int cy = iy < 0 ? 0 : (iy > kCostGrid - 1 ? kCostGrid - 1 : iy);
  return cy * kCostGrid + cx;
}
// Bits of a 16-bit coordinate spread to the even positions: Morton code = spread(qx) | spread(qy) << 1 (the spatial vertex
// order inside a tile).
FLAME_HD inline uint32_t morton_spread16(uint32_t x) {
  x &= 0xffff; x = (x | (x << 8)) & 0x00ff00ff; x = (x | (x << 4)) & 0x0f0f0f0f;
  x = (x | (x << 2)) & 0x33333333; x = (x | (x << 1)) & 0x55555555;
  return x;
}

// ---- per-element rules of the graph sync and the plan: ONE statement each for the host builder (plan.cpp, sync.cpp), the
// staged device kernels and the one-launch plan (plan_dev.hip); DESIGN.md lists who calls what.  They take values, not
// arrays: the callers keep their operands in registers, LDS or vectors as suits them. ----
// Morton code of a position inside the box [mn, mx]: quantise to 16 bits per axis, spread.  The clamp is the identity for a box
// that is the frame's own (the host builder, a bisected device plan); a reused partition keeps the box of the frame it was made from.
FLAME_HD inline uint32_t morton_quant16(float x, float mn, float mx) { return (uint32_t)(65535.0f * (fminf(fmaxf(x, mn), mx) - mn) / fmaxf(mx - mn, 1e-20f)); }
FLAME_HD inline uint32_t morton_code(float x, float y, float mnx, float mny, float mxx, float mxy) {
  return morton_spread16(morton_quant16(x, mnx, mxx)) | (morton_spread16(morton_quant16(y, mny, mxy)) << 1);
}
// ... and the sort key of vertex v inside its tile: (code, id)
FLAME_HD inline uint64_t morton_key(uint32_t code, int32_t v) { return ((uint64_t)code << 32) | (uint32_t)v; }
// Side (u, w) of a triangle as the half edge (min, max); false: an index out of range or a degenerate side
FLAME_HD inline bool tri_side(int32_t u, int32_t w, int32_t V, int32_t* lo, int32_t* hi) {
  *lo = u < w ? u : w; *hi = u < w ? w : u;
  return !(u < 0 || w < 0 || u >= V || w >= V || u == w);
}
// Edge weight of the graph sync: 1 / length, dx * dx + dy * dy in two roundings (-ffp-contract=off), as the oracle states it
FLAME_HD inline float edge_alpha(float dx, float dy) { return 1.0f / sqrtf(dx * dx + dy * dy); }
// Data terms of the graph sync; pred: the prediction, or any non-finite value where there is none (or it is not used)
struct DataTerm { float z, wgt, x0; };
FLAME_HD inline DataTerm data_term(float mu, float var, float pred, float scale, bool adaptive) {
  DataTerm d;
  d.z = mu / scale;
  d.wgt = adaptive ? 1.0f / var : 1.0f;
  d.x0 = isfinite(pred) ? pred / scale : d.z;
  return d;
}
FLAME_HD inline bool data_term_finite(const DataTerm& d) { return isfinite(d.z) && isfinite(d.wgt) && isfinite(d.x0); }
// Edge record {alpha, beta, d}: d = d_sign * (pos_i - pos_j) (a multiplication by +-1 is exact)
FLAME_HD inline float edge_dsign(int d_sign) { return d_sign < 0 ? -1.0f : 1.0f; }
template <class F4>
FLAME_HD inline F4 edge_record(float alpha, float beta, float dsign, float xi, float yi, float xj, float yj) {
  return F4{alpha, beta, dsign * (xi - xj), dsign * (yi - yj)};
}
// Incidence entry of a vertex's row: while the row is sorted, (ORIGINAL edge id << 1 | role) -- ascending entry = ascending
// original id, the summation order of the arithmetic contract; role 1: the vertex is the edge's target.  In the finished plan
// (ginc) the INTERNAL edge id, the role in bit 31.
FLAME_HD inline uint32_t inc_entry(int32_t e_orig, int role) { return ((uint32_t)e_orig << 1) | (uint32_t)role; }
FLAME_HD inline int32_t inc_entry_edge(uint32_t x) { return (int32_t)(x >> 1); }
FLAME_HD inline int inc_entry_role(uint32_t x) { return (int)(x & 1u); }
FLAME_HD inline uint32_t inc_word(int32_t e_int, int role) { return (uint32_t)e_int | ((uint32_t)role << 31); }

// ---- phase D of the tile kernels, as the lane order of a 64-edge block prices it (plan.cpp assign_lanes(), plan_dev.hip
// assign_lanes_block()) ----
// ds_read_b128 is served in 4 groups of 16 lanes: {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, and the same of lanes 32-63.
FLAME_HD inline int lane_read_group(int lane) {
  const int l = lane & 31;
  return ((l < 4 || (l >= 12 && l < 16) || (l >= 20 && l < 28)) ? 0 : 1) + 2 * (lane >> 5);
}
// An edge end without an incidence slot (0xffff: its vertex is never updated) stores into the lane's own trash slot.  (The
// resident tiles' poll lists stage a halo edge through the source's slot, else the target's, else that trash slot: kernels.hip
// k_poll_lists.)
FLAME_HD inline uint32_t edge_store_slot(uint32_t slot, int32_t nslots, int lane) { return slot != 0xffffu ? slot : (uint32_t)(nslots + lane); }

// Local edge record halves.
//   t_eij[e] = {li | lj << 16, slot_src | slot_dst << 16}   (local vertex ids / incidence slots)
//   t_ew[e]  = {alpha, beta, dx, dy}

}  // namespace flamehip
