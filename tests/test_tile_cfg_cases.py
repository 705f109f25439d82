"""CPU: the table of tests/tile_cfg_cases.py covers every tile-kernel configuration flame_ros_amd/csrc/tile_cfgs.h states --
18 by launches (k_tile), 6 resident (k_tile_persist), 2 x 2 fat resident (k_tile_persist<.., S12, FAT = true> on either slot
layout) -- each case lands on its target with the host plan builder on a plan-only handle (device = -1: sized as the MI355X
would), fills the register slots it says it fills, and the C oracle's steps on it lie inside the float64 bands (every GPU
test of these cases compares bits with the oracle: tests/test_gpu_tile_cfgs.py).  (k_tile<.., S12 = true> runs only behind
a resident launch that gave up -- the hooks library's tests, tests/test_gpu_fat_tiles.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from flame_ros_amd import lib
from flame_ros_amd.regularizer import GraphRegularizer
from tests.solver_corpus import FAT_V, STATE, check_step, state_of, step_f64
from tests.tile_cfg_cases import UNREACHABLE, config_cases, oracle_of, targets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in config_cases()}
SMALL_V = 2 * 1030  # no launch / resident case is larger (l1024x6x2: two tiles of more than 1 024 own vertices each)
ORACLE_STEPS = 10  # the GPU test compares up to 2 D + 2 iterations, D <= 4 in this table


def header_lists():
    """{macro name: [(nt, ept, vpt), ...]} of tile_cfgs.h, the one statement of the configurations."""
    text = open(os.path.join(ROOT, "flame_ros_amd", "csrc", "tile_cfgs.h")).read()
    out = {}
    for m in re.finditer(r"^#define (FLAME_\w+_CFGS)\(X\)((?:.*\\\n)*.*)$", text, re.M):
        out[m.group(1)] = [tuple(int(v) for v in x) for x in re.findall(r"X\((\d+),\s*(\d+),\s*(\d+)\)", m.group(2))]
    return out


def instantiations():
    h = header_lists()
    assert set(h) == {"FLAME_TILE_CFGS", "FLAME_PERSIST_CFGS", "FLAME_S12_CFGS"}, sorted(h)
    return ({("tile",) + c for c in h["FLAME_TILE_CFGS"]} | {("persist",) + c for c in h["FLAME_PERSIST_CFGS"]} |
            {("fat",) + c + (s12,) for c in h["FLAME_S12_CFGS"] for s12 in (0, 1)})


def plan_of(c):
    """(info dict, TileDesc list) of the case's plan on a plan-only handle."""
    with GraphRegularizer(c["pos"], c["edges"], c["alpha"], c["beta"], c["z"], c["wgt"], device=-1, d_sign=c["d_sign"],
                          **c["tile"]) as r:
        info = {k: r.info(k) for k in ("path", "num_tiles", "tile_threads", "tile_ept", "tile_vpt", "tile_slot12", "tile_fat",
                                       "tile_depth", "tile_lds_bytes", "lds_bytes")}
        raw = r.plan_array("tiles", np.dtype((np.void, C.sizeof(lib.TileDesc))))
        return info, list((lib.TileDesc * len(raw)).from_buffer_copy(raw.tobytes()))


def test_header_lists_are_what_the_table_was_made_for():
    h = header_lists()
    assert (len(h["FLAME_TILE_CFGS"]), len(h["FLAME_PERSIST_CFGS"]), len(h["FLAME_S12_CFGS"])) == (18, 6, 2), h
    assert len(instantiations()) == 28


def test_every_instantiation_has_a_case(capsys):
    reach = targets(CASES.values())
    want = instantiations()
    assert not (set(reach) & set(UNREACHABLE)), "a configuration with a case is no unreachable one"
    missing = want - set(reach) - set(UNREACHABLE)
    assert not missing, "tile_cfgs.h configurations without a case: %s" % sorted(missing)
    extra = (set(reach) | set(UNREACHABLE)) - want
    assert not extra, "cases for configurations tile_cfgs.h does not state: %s" % sorted(extra)
    kernel = {"tile": "k_tile<%d, %d, %d>", "persist": "k_tile_persist<%d, %d, %d>",
              "fat": "k_tile_persist<%d, %d, %d, S12 = %d, FAT = 1>"}
    with capsys.disabled():
        print()
        for key in sorted(want, key=lambda k: (("tile", "persist", "fat").index(k[0]),) + k[1:]):
            print("  %-46s %s" % (kernel[key[0]] % key[1:], ", ".join(reach[key]) if key in reach else
                                  "UNREACHABLE: " + UNREACHABLE[key]))


def test_every_register_slot_and_the_exactly_full_tile_have_a_case():
    """Every configuration has a case that uses its last edge slot and, with two vertices per thread, its second vertex
    slot for an updated vertex; and some tile is exactly full of edges, some exactly full of vertices
    (test_case_lands_on_its_target holds each case to its `uses`)."""
    by_name = {c["name"]: c for c in CASES.values()}
    for key, names in targets(CASES.values()).items():
        uses = set().union(*(by_name[n]["uses"] for n in names))
        assert "last_e" in uses, key
        assert key[3] == 1 or {"last_v", "upd_v"} <= uses, key
    every = set().union(*(c["uses"] for c in CASES.values()))
    assert {"full_e", "full_v", "tiles"} <= every
    assert any({"full_v", "last_v"} <= set(c["uses"]) for c in CASES.values())  # full with both vertex slots in use
    for kind in ("resident", "fat"):
        assert all("tiles" in c["uses"] for c in CASES.values() if c["target"][5] == kind)


@pytest.mark.parametrize("name", list(CASES))
def test_case_lands_on_its_target(name):
    c = CASES[name]
    nt, ept, vpt, s12, fat, kind = c["target"]
    info, tiles = plan_of(c)
    got = tuple(info[k] for k in ("tile_threads", "tile_ept", "tile_vpt", "tile_slot12", "tile_fat"))
    assert info["path"] == 2 and got == (nt, ept, vpt, s12, fat), (info, c["tile"])
    V = len(c["z"])
    assert all(t.e_loc <= nt * ept for t in tiles)
    assert info["tile_lds_bytes"] + 64 <= min(info["lds_bytes"], 160 * 1024)  # (what the device can launch)
    if kind == "launches":
        assert c["tile"].get("persist") == 0 and V <= SMALL_V
        assert all(t.n_ext <= nt * vpt for t in tiles)
    elif kind == "resident":
        assert "persist" not in c["tile"] and 2 <= len(tiles) <= 256 and V <= SMALL_V and info["tile_depth"] >= 1
        assert all(t.n_ext <= nt * vpt for t in tiles)
    else:  # fat: one tile per CU, only the updated vertices and the halo need a lane
        assert "persist" not in c["tile"] and len(tiles) == 256 and V > FAT_V and info["tile_depth"] >= 1
        assert all(max(t.n_upd, t.n_ext - t.n_own) <= nt * vpt for t in tiles)
    e_max, v_max = max(t.e_loc for t in tiles), max(t.n_ext for t in tiles)
    facts = dict(last_e=e_max > nt * (ept - 1), last_v=vpt == 2 and v_max > nt,
                 upd_v=vpt == 2 and max(t.n_upd for t in tiles) > nt,
                 full_e=e_max == nt * ept, full_v=v_max == nt * vpt, tiles=len(tiles) > 1)
    for u in c["uses"]:
        assert facts[u], (u, e_max, v_max, len(tiles))


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_steps_on_the_case_against_f64(oracle_built, name):
    c = CASES[name]
    nxt, band, _ = step_f64(c, c["st"])
    for k in STATE:
        assert np.isfinite(nxt[k]).all() and np.isfinite(band[k]).all(), k
    o, p = oracle_of(c)
    for n in range(ORACLE_STEPS):
        prev = state_of(o)
        o.solve(p, 1)
        check_step(c, prev, state_of(o), "%s step %d" % (name, n + 1))
