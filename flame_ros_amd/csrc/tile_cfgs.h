// flame_ros_amd/csrc/tile_cfgs.h -- the tile kernels' configurations {threads, edges per thread, vertices per thread}: ONE
// statement for the kernels that get instantiated (kernels.hip) and for the plan builders' choice among them (plan.cpp).
// Plain C++, no HIP.  The order of a list is the tie-break of the builders' choice (plan.cpp pick_cfg: first fit wins).
#pragma once

#define FLAME_TILE_CFGS(X)                                                             \
  X(256, 2, 1) X(256, 3, 1) X(256, 4, 1) X(256, 6, 1) X(256, 4, 2) X(256, 6, 2)         \
  X(512, 2, 1) X(512, 3, 1) X(512, 4, 1) X(512, 6, 1) X(512, 4, 2) X(512, 6, 2)         \
  X(1024, 2, 1) X(1024, 3, 1) X(1024, 4, 1) X(1024, 6, 1) X(1024, 4, 2) X(1024, 6, 2)

// resident tiles (ONE launch for the whole solve): the configurations small graphs get
#define FLAME_PERSIST_CFGS(X) X(256, 2, 1) X(256, 3, 1) X(512, 2, 1) X(512, 3, 1) X(1024, 2, 1) X(1024, 3, 1)

// 12-byte incidence slots (fat tiles, SlotMem<true>), resident or by launches, and the FAT resident variants on either slot
// layout: the configurations a one-tile-per-CU partition of a graph beyond 256 x 196 vertices gets
#define FLAME_S12_CFGS(X) X(1024, 2, 1) X(1024, 3, 1)

namespace flamehip {

struct TileCfg { int nt, ept, vpt; };

#define FLAME_CFG_ENTRY(N, Ep, Vp) {N, Ep, Vp},
constexpr TileCfg kTileCfgs[] = {FLAME_TILE_CFGS(FLAME_CFG_ENTRY)};
constexpr TileCfg kPersistCfgs[] = {FLAME_PERSIST_CFGS(FLAME_CFG_ENTRY)};
constexpr TileCfg kSlot12Cfgs[] = {FLAME_S12_CFGS(FLAME_CFG_ENTRY)};
#undef FLAME_CFG_ENTRY

template <int N>
inline bool tile_cfg_in(const TileCfg (&list)[N], int nt, int ept, int vpt) {
  for (const TileCfg& c : list)
    if (c.nt == nt && c.ept == ept && c.vpt == vpt) return true;
  return false;
}
inline bool tile_config_exists(int nt, int ept, int vpt) { return tile_cfg_in(kTileCfgs, nt, ept, vpt); }
inline bool tile_persist_exists(int nt, int ept, int vpt) { return tile_cfg_in(kPersistCfgs, nt, ept, vpt); }
inline bool tile_slot12_exists(int nt, int ept, int vpt) { return tile_cfg_in(kSlot12Cfgs, nt, ept, vpt); }

}  // namespace flamehip
