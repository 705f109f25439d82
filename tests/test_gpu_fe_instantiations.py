"""GPU: every instantiation of k_fe_track<COST, RG, WARP> (csrc/frontend.hip) against the restatement tests/frontend_ref.py: the
three costs x the gradient gate off / on x the warped window off / on, the letterbox and the height band set in every case, compared
through tests/fe_pair.py after EVERY frame.  The scene is fe_warp_scenes.small(): 48 x 36 under a roll of 45 degrees, 4 frames, 32
slots, a ring of two pose frames (frames 0 and 2), win 7 -- a few hundred milliseconds a case.  That a case exercises its switches
is decided from the restatement alone, on the CPU, before the device is asked anything."""
import functools

import pytest

from tests import fe_rg_ref as RG
from tests import fe_warp_scenes as WS
from tests import frontend_ref as R
from tests.fe_pair import K_4836, pair  # noqa: F401  (pair: the fixture)

pytestmark = pytest.mark.gpu
# At 48 x 36 with win 7 the 32 slots hold about a dozen features.  min_grad 8 refuses 4 of the frames' 22 gradient tests and passes
# 18; the band of +-0.1 around the camera's height holds 3 to 10 projections and the letterbox (rows 12 ... 23) refuses 9.
MIN_GRAD = 8.0
GATES = dict(letterbox=True, min_height=-0.1, max_height=0.1, up=(0, 1, 0))
POSEFRAMES = (0, 2)
SIZES = dict(max_features=32, max_poseframes=2, K=K_4836, win_size=7)


def configure(fe, cost, rg, warp):
    """`fe`: a FrontEndRef or a Pair -- the same setters."""
    fe.set_cost(cost == "zssd")
    fe.set_gain_invariant(cost == "gi")
    fe.set_ref_grad(MIN_GRAD if rg else 0.0)
    fe.set_warp(warp)
    fe.set_gates(**GATES)


@functools.lru_cache(maxsize=None)
def restatement_alone(cost, rg, warp):
    """What the case exercises: OK features, REF_GRAD refusals, passed gradient tests, invalid and valid warped samples."""
    fe = R.FrontEndRef(WS.SMALL_W, WS.SMALL_H, SIZES["K"], SIZES["max_features"], SIZES["max_poseframes"])
    configure(fe, cost, rg, warp)
    samples = []
    cost_of = fe._cost
    fe._cost = lambda *a: samples.append((cost_of(*a), fe._Jq)) or samples[-1][0]
    seen = dict(ok=0, ref_grad=0, passed=0)
    for k, (img, T) in enumerate(WS.small()):
        fe.track(R.params(win_size=SIZES["win_size"]), img, k, T, k in POSEFRAMES)
        seen["ok"] += fe.counts.get(R.OK, 0)
        seen["ref_grad"] += fe.counts.get(RG.REF_GRAD, 0)
        seen["passed"] += sum(d[-1] for d in fe.decisions)
    warped = [c for c, Jq in samples if Jq is not None]
    assert (len(warped) == len(samples)) if warp else not warped
    seen["invalid"], seen["valid"] = sum(c is None for c in warped), sum(c is not None for c in warped)
    return seen


@pytest.mark.parametrize("warp", [False, True], ids=["upright", "warp"])
@pytest.mark.parametrize("rg", [False, True], ids=["norg", "rg"])
@pytest.mark.parametrize("cost", ["ssd", "zssd", "gi"])
def test_every_instantiation_equals_the_restatement(pair, cost, rg, warp):
    seen = restatement_alone(cost, rg, warp)
    print(cost, rg, warp, seen)
    assert seen["ok"] >= 1
    if rg:
        assert seen["ref_grad"] >= 1 and seen["passed"] >= 1
    if warp:
        assert seen["invalid"] >= 1 and seen["valid"] >= 1
    p = pair(WS.SMALL_W, WS.SMALL_H, **SIZES)
    configure(p, cost, rg, warp)
    for k, (img, T) in enumerate(WS.small()):
        p.track(img, T, k in POSEFRAMES)
    assert p.total["ok"] == seen["ok"] and p.total["ref_grad"] == seen["ref_grad"]
    assert p.total["held"] >= 1 and p.total["refused"] >= 1  # (both gates acted)
