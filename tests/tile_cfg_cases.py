"""One small case per instantiated tile-kernel configuration (flame_ros_amd/csrc/tile_cfgs.h): the table behind
tests/test_tile_cfg_cases.py (CPU: every case lands on its target on a plan-only handle) and tests/test_gpu_tile_cfgs.py
(GPU: the kernel that configuration names, against the float64 step and the C oracle's bits).

A case is a tests/solver_corpus.py mk() case -- free beta, wide data weights with zeros, a random start state -- plus
  tile    the plan options that make plan.cpp pick_cfg() / tile_fit() choose the configuration,
  target  (nt, ept, vpt, slot12, fat, kind): kind "launches" (k_tile, persist = 0), "resident" (k_tile_persist, several
          tiles, ONE launch per solve) or "fat" (the FAT resident variants, one tile per CU beyond 256 x 196 vertices),
  uses    what its tiles are there to fill (test_tile_cfg_cases.py checks each against the plan's TileDesc):
          "last_e"  some tile has e_loc > nt (ept - 1): the last edge register slot is in use,
          "last_v"  some tile has n_ext > nt (vpt 2): the second vertex register slot is in use,
          "upd_v"   some tile has n_upd > nt (vpt 2): a vertex in the second slot is updated and written back,
          "full_e"  some tile has e_loc == nt ept, "full_v" some tile has n_ext == nt vpt: exactly full,
          "tiles"   more than one tile.

How a graph lands where it does (pick_cfg: pass 0 takes one vertex and <= 3 edges per thread, pass 1 <= 4 edges, pass 2
anything; within a pass the first entry of FLAME_TILE_CFGS with nt ept >= e_loc and nt vpt >= n_ext wins; tile_threads
fixes nt): a Delaunay graph has E ~ 3 V, so a tile of it that needs four or six edges per thread also needs more vertices
than threads and gets vpt 2; jittered lattices with 4 .. 20 neighbour offsets (E = 4 V .. 16 V) reach vpt 1 with ept >= 4.
An edge list cut to nt ept edges on a lattice of nt vpt vertices fills a single tile exactly.  Beyond 4 096 local edges no
isolated tile fits 160 KiB (two 16-byte incidence slots per edge): the last edge slot of (1024, 6, .) is reached by depth-1
tiles whose halo ring has no slots (_two_sides; one iteration per launch, so what a tile keeps in LDS between iterations
is not at stake there), and (1024, 6, 2) with iterations that stay in LDS by a one-tile partition of two regular graphs
(_two_regular).

Checked against deliberately wrong kernels (scratch builds, tests/test_gpu_tile_cfgs.py on the device): with the dual
update of the sixth edge slot dropped when EPT == 6, exactly the cases of (., 6, .) that use "last_e" fail; with the
second vertex slot's write-back to LDS dropped when VPT == 2, exactly the cases of (., ., 2) with more than one iteration
per launch fail (every such configuration has one); no case of another configuration fails either time.
"""
import numpy as np

from flame_ros_amd import graphgen
from oracle import COracle
from oracle.cbind import OracleParams
from tests.solver_corpus import free_beta, inv_len, mk, state, wide_wgt

LAUNCH = dict(path=2, persist=0)
OFF2 = [(1, 0), (0, 1)]
OFF4 = OFF2 + [(1, 1), (-1, 1)]
OFF6 = OFF4 + [(2, 0), (0, 2)]
OFF8 = OFF6 + [(2, 1), (1, 2)]
OFF20 = [(dx, dy) for dy in range(0, 4) for dx in range(-3, 4) if (dy, dx) > (0, 0)][:20]

# Configurations no input reaches: {(list, nt, ept, vpt): the arithmetic that excludes it}.  (None today.)
UNREACHABLE = {}


def lattice(w, h, offsets, seed, cut=None, pitch=9.0):
    """A jittered w x h lattice with an edge from every vertex to its neighbour at each offset; cut: the first
    `cut` edges only."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(w), np.arange(h))
    pos = np.c_[gx.ravel(), gy.ravel()] * pitch + 20.0 + rng.uniform(-2.0, 2.0, (w * h, 2))
    e = []
    for dx, dy in offsets:
        i, j = gx.ravel() + dx, gy.ravel() + dy
        ok = (i >= 0) & (i < w) & (j >= 0) & (j < h)
        e.append(np.c_[(gy.ravel() * w + gx.ravel())[ok], (j * w + i)[ok]])
    e = np.concatenate(e).astype(np.int32)
    return pos.astype(np.float32), (e if cut is None else e[:cut])


def _case(name, target, pos, edges, z, seed, tile, uses=()):
    rng = np.random.default_rng(seed)
    alpha = inv_len(pos, edges)
    c = mk(name, pos, edges, alpha, free_beta(alpha, rng), z, wide_wgt(len(z), rng), state(z, len(edges), rng), tile=tile)
    c["target"], c["uses"] = tuple(target), tuple(uses)
    return c


def _lat(name, target, w, h, offsets, seed, tile, uses=(), **kw):
    pos, edges = lattice(w, h, offsets, seed, **kw)
    rng = np.random.default_rng(seed + 1000)
    z = 0.5 + 0.2 * np.sin(pos[:, 0] / 40.0) * np.cos(pos[:, 1] / 55.0) + rng.normal(0, 0.02, len(pos))
    return _case(name, target, pos, edges, z, seed, tile, uses)


def _syn(name, target, V, tile, uses=()):
    g = graphgen.synthetic(V, seed=V)
    return _case(name, target, g.pos, g.edges, g.z, V, tile, uses)


def _two_sides(name, target, n, k, seed, tile, uses=(), m=None):
    """Two clouds of n vertices, left and right, a ring through each, and k edges from each of the first m (default: all)
    left vertices to the first m right ones (vertex i to i + 97 j mod m, j < k: each of the 2 m has k of them; every other
    one points right to left).  As two depth-1 tiles -- one per side -- each holds its own n vertices, the other side's m
    as its halo ring and n + m k local edges, but incidence slots for its own vertices only: the way to more than 4 096
    local edges beside more than 1 024 local vertices inside 160 KiB (16 B per local vertex + 16 B per incidence slot; an
    isolated tile of that many edges has two slots per edge, and plan.cpp single_fits prices it out at 38 B per edge).
    The first m of a side lie in the lower half of the image, the others in the upper half, so that a tile's Morton order
    keeps the rows of k + 2 incidences apart from the rows of 2 (a 64-vertex group pays its longest row 64 times)."""
    m = n if m is None else m
    rng = np.random.default_rng(seed)
    half = lambda x0, cnt, y0: rng.uniform([x0, y0], [x0 + 200, y0 + 216], (cnt, 2))  # noqa: E731
    pos = np.concatenate([half(20, m, 20), half(20, n - m, 244), half(420, m, 20), half(420, n - m, 244)])
    i, im = np.arange(n), np.arange(m)
    e = [np.c_[i, (i + 1) % n], np.c_[n + i, n + (i + 1) % n]]
    for j in range(k):
        a, b = im, n + (im + 97 * j) % m
        e.append(np.c_[b, a] if j % 2 else np.c_[a, b])
    z = 0.5 + 0.2 * np.sin(pos[:, 0] / 40.0) * np.cos(pos[:, 1] / 55.0) + rng.normal(0, 0.02, 2 * n)
    return _case(name, target, pos.astype(np.float32), np.concatenate(e).astype(np.int32), z, seed, tile, uses)


def _two_regular(name, target, seed, tile, uses=()):
    """1 088 vertices in ONE tile with a halo depth (all of them updated, the iterations of a launch stay in LDS) and 4 384
    edges: (1024, 6, 2) with updated vertices in the second slot.  An isolated tile of more than 3 853 edges is priced out
    (plan.cpp single_fits, 38 B per edge), so this is a one-tile partition, whose rows lie in Morton order at an odd pitch
    per 64-vertex group: 576 vertices of degree 9 in the lower half of the image (a circulant: i +- 1 .. 4 and i + 288)
    and 512 of degree 7 in the upper half (i +- 1 .. 3 and i + 256) are 9 groups at pitch 9 and 8 at pitch 7 -- 8 768 slots,
    16 (1 088 + 8 768 + 65) = 158 736 bytes of LDS."""
    rng = np.random.default_rng(seed)
    pos = np.concatenate([rng.uniform([20, 20], [620, 236], (576, 2)), rng.uniform([20, 244], [620, 460], (512, 2))])
    e = []
    for base, n, r in ((0, 576, 4), (576, 512, 3)):
        i = np.arange(n)
        e += [np.c_[base + i, base + (i + d) % n] for d in range(1, r + 1)] + [np.c_[base + i[:n // 2], base + i[:n // 2] + n // 2]]
    z = 0.5 + 0.2 * np.sin(pos[:, 0] / 40.0) * np.cos(pos[:, 1] / 55.0) + rng.normal(0, 0.02, len(pos))
    return _case(name, target, pos.astype(np.float32), np.concatenate(e).astype(np.int32), z, seed, tile, uses)


def _single(nt=0):
    """One isolated tile (tile_own = V is filled in by config_cases) by launches, on nt threads (0: the planner's)."""
    return dict(LAUNCH, tile_own=-1, **({"tile_threads": nt} if nt else {}))


def config_cases(with_fat=True):
    L, R = "launches", "resident"
    c = [
        # ---- k_tile<nt, ept, vpt>: the 18 launch configurations ----
        _syn("l256x2x1", (256, 2, 1, 0, 0, L), 150, _single(256), ("last_e",)),
        _syn("l256x3x1", (256, 3, 1, 0, 0, L), 220, _single(256), ("last_e",)),
        _lat("l256x4x1", (256, 4, 1, 0, 0, L), 16, 16, OFF4, 1, _single(256), ("last_e", "full_v")),
        _lat("l256x4x1_full", (256, 4, 1, 0, 0, L), 16, 16, OFF6, 2, _single(256), ("last_e", "full_e", "full_v"), cut=1024),
        _lat("l256x6x1", (256, 6, 1, 0, 0, L), 16, 16, OFF4 + [(2, 0)], 3, _single(256)),
        _lat("l256x6x1_full", (256, 6, 1, 0, 0, L), 16, 16, OFF8, 4, _single(256), ("last_e", "full_e", "full_v"), cut=1536),
        _syn("l256x4x2", (256, 4, 2, 0, 0, L), 300, _single(256), ("last_e", "last_v")),
        _lat("l256x4x2_fullv", (256, 4, 2, 0, 0, L), 32, 16, OFF2, 5, _single(256), ("last_e", "last_v", "full_v")),
        _syn("l256x4x2_tiles", (256, 4, 2, 0, 0, L), 2000, dict(LAUNCH, tile_own=150, tile_depth=3, tile_threads=256),
             ("last_e", "last_v", "tiles")),
        _syn("l256x6x2", (256, 6, 2, 0, 0, L), 450, _single(256), ("last_e", "last_v")),
        _lat("l256x6x2_full", (256, 6, 2, 0, 0, L), 32, 16, OFF4, 6, _single(256), ("last_e", "last_v", "full_e", "full_v"),
             cut=1536),
        _syn("l512x2x1", (512, 2, 1, 0, 0, L), 320, _single(512), ("last_e",)),
        _syn("l512x3x1", (512, 3, 1, 0, 0, L), 450, _single(512), ("last_e",)),
        _lat("l512x4x1", (512, 4, 1, 0, 0, L), 32, 16, OFF4, 7, _single(512), ("last_e", "full_v")),
        _lat("l512x6x1", (512, 6, 1, 0, 0, L), 32, 16, OFF6, 8, _single(512), ("last_e", "full_v")),
        _syn("l512x4x2", (512, 4, 2, 0, 0, L), 600, _single(512), ("last_e", "last_v")),
        _syn("l512x6x2", (512, 6, 2, 0, 0, L), 900, _single(512), ("last_e", "last_v")),
        _syn("l512x6x2_tiles", (512, 6, 2, 0, 0, L), 2000, dict(LAUNCH, tile_own=400, tile_depth=4, tile_threads=512),
             ("last_v", "tiles")),
        _syn("l1024x2x1", (1024, 2, 1, 0, 0, L), 650, _single(1024), ("last_e",)),
        _syn("l1024x3x1", (1024, 3, 1, 0, 0, L), 900, _single(1024), ("last_e",)),
        _lat("l1024x4x1", (1024, 4, 1, 0, 0, L), 30, 30, OFF4, 9, _single(), ("last_e",)),
        _lat("l1024x6x1", (1024, 6, 1, 0, 0, L), 16, 16, OFF20, 10, _single()),
        _two_sides("l1024x6x1_last", (1024, 6, 1, 0, 0, L), 500, 10, 13, dict(LAUNCH, tile_own=500, tile_depth=1),
                   ("last_e", "tiles")),
        _lat("l1024x4x2", (1024, 4, 2, 0, 0, L), 34, 33, OFF4[:3], 11, _single(), ("last_e", "last_v")),
        # (both vertex slots UPDATED needs more than 1 024 own vertices a tile: 2 x 1 030 vertices, the one case beyond 2 k)
        _two_sides("l1024x6x2", (1024, 6, 2, 0, 0, L), 1030, 9, 12, dict(LAUNCH, tile_own=1030, tile_depth=1),
                   ("last_e", "last_v", "tiles"), m=500),
        _two_regular("l1024x6x2_lds", (1024, 6, 2, 0, 0, L), 14, dict(LAUNCH, tile_own=1088, tile_depth=2), ("last_v",)),
        # ---- k_tile_persist<nt, ept, vpt>: the 6 resident configurations, several tiles, one launch per solve ----
        _syn("r256x2x1", (256, 2, 1, 0, 0, R), 600, dict(path=2, tile_own=60, tile_depth=3, tile_threads=256), ("last_e", "tiles")),
        _syn("r256x3x1", (256, 3, 1, 0, 0, R), 600, dict(path=2, tile_own=90, tile_depth=3, tile_threads=256), ("last_e", "tiles")),
        _syn("r512x2x1", (512, 2, 1, 0, 0, R), 900, dict(path=2, tile_own=150, tile_depth=3, tile_threads=512), ("last_e", "tiles")),
        _syn("r512x3x1", (512, 3, 1, 0, 0, R), 1200, dict(path=2, tile_own=240, tile_depth=3, tile_threads=512), ("last_e", "tiles")),
        _syn("r1024x2x1", (1024, 2, 1, 0, 0, R), 1500, dict(path=2, tile_own=375, tile_depth=3, tile_threads=1024), ("last_e", "tiles")),
        _syn("r1024x3x1", (1024, 3, 1, 0, 0, R), 2000, dict(path=2, tile_own=500, tile_depth=4, tile_threads=1024), ("last_e", "tiles")),
    ]
    for x in c:
        if x["tile"].get("tile_own") == -1:
            x["tile"]["tile_own"] = len(x["z"])
        if "last_v" in x["uses"]:  # (in every case here the second slot also holds updated vertices)
            x["uses"] += ("upd_v",)
    if with_fat:
        c += fat_cases()
    assert len({x["name"] for x in c}) == len(c)
    return c


# Fat tiles need V > 256 x 196 (tests/solver_corpus.py FAT_V); 256 x 197 gives every tile 197 vertices of its own.  At the
# automatic depth (4) its tiles stay below 2 048 local edges: two edges per thread on 16-byte slots.  The other three
# variants, by public options only, as small as a plan-only scan over graphgen.synthetic(V, seed=V) found them:
#   V = 51 456 is the first size (in steps of 512) whose largest tile, on the image border, has more than 2 048 local
#   edges at depth 4: three edges per thread, still on 16-byte slots;
#   a smaller lds_bytes prices the 16-byte layout out (plan.cpp tile_fit: lds16 + stage + 4 096 > lds_bytes) and, the
#   depth being fixed by tile_depth, the attempt policy (PlanAttempts::fat_next) goes to 12-byte slots at the same depth.
#   lds_bytes is the middle of [lds12, lds16) + stage + 4 096 of the partition at the default 160 KiB.
FAT_SMALL, FAT_EPT3 = 256 * 197, 51456


def fat_cases():
    F = "fat"
    return [
        _syn("f1024x2x1_s16", (1024, 2, 1, 0, 1, F), FAT_SMALL, {}, ("last_e", "tiles")),
        _syn("f1024x2x1_s12", (1024, 2, 1, 1, 1, F), FAT_SMALL, dict(tile_depth=4, lds_bytes=106000), ("last_e", "tiles")),
        _syn("f1024x3x1_s16", (1024, 3, 1, 0, 1, F), FAT_EPT3, {}, ("last_e", "tiles")),
        _syn("f1024x3x1_s12", (1024, 3, 1, 1, 1, F), FAT_EPT3, dict(tile_depth=4, lds_bytes=136000), ("last_e", "tiles")),
    ]


def oracle_of(c):
    """(the C oracle at the case's start state, its parameters), as tests/test_solver_f64_oracle.py oracle_of."""
    o = COracle(c["pos"] * np.float32(c["d_sign"]), c["edges"], c["alpha"], c["beta"], c["z"], c["wgt"])
    o.set_state(**c["st"])
    p = c["p"]
    return o, OracleParams(p["lam"], p["tau"], p["sigma"], p["theta"], p["x_min"], p["x_max"])


def targets(cases):
    """{(list, nt, ept, vpt[, slot12]): [case names]}: list is "tile" (FLAME_TILE_CFGS, k_tile), "persist"
    (FLAME_PERSIST_CFGS, k_tile_persist) or "fat" (FLAME_S12_CFGS as k_tile_persist<.., S12, FAT = true>, per slot layout)."""
    out = {}
    for c in cases:
        nt, ept, vpt, s12, fat, kind = c["target"]
        key = {"launches": ("tile", nt, ept, vpt), "resident": ("persist", nt, ept, vpt), "fat": ("fat", nt, ept, vpt, s12)}[kind]
        out.setdefault(key, []).append(c["name"])
    return out
