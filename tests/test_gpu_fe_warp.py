"""GPU: the warped matching window (flame_hip_frontend_set_warp: k_fe_track<., ., true>, csrc/frontend.hip) against the restatement
tests/fe_warp_ref.py (pinned by tests/test_fe_warp_ref.py): after EVERY frame the emitted features, `state()`, `searches()`, every
count and the info keys bit for bit.  The shapes are the smallest at which the rule still bites: the 160 x 120 roll scenes of the
ground-truth test, 48 x 36 images under a roll of 45 degrees, where most turned windows touch a border, and feature tables of 5
and 8 slots (one slot past a block of four wavefronts, and two whole blocks)."""
import numpy as np
import pytest

from tests import fe_debug_ref as D
from tests import fe_warp_ref as WR
from tests import fe_warp_scenes as WS
from tests import frontend_scenes as SC
from tests.fe_pair import K_4836, pair  # noqa: F401  (pair: the fixture)

pytestmark = pytest.mark.gpu
COSTS = ("ssd", "zssd", "gi")


def spy_costs(p):
    """Records every cost the restatement forms from now on, with whether a map was in force."""
    seen = []
    cost = p.ref._cost

    def spy(*a):
        c = cost(*a)
        seen.append((c, p.ref._Jq))
        return c
    p.ref._cost = spy
    return seen


@pytest.mark.parametrize("name,cost,win", [("roll30", "ssd", 5), ("roll30", "zssd", 7), ("roll30", "gi", 7), ("roll30_closer", "ssd", 5),
                                           ("roll30_closer", "zssd", 7)])
def test_roll_scenes(pair, name, cost, win):
    """The scenes of the CPU ground-truth test: the device tracks through the roll what the restatement tracks."""
    p = pair(WS.W, WS.H, K=WS.K, win_size=win)
    p.set_warp()
    p.set_cost_name(cost)
    for k, (img, T) in enumerate(WS.scene(name)):
        out = p.track(img, T, k == 0)
    err, emitted = WS.ZS.relative_errors(out, T)
    assert len(err) >= 25 and (err > 0.10).sum() == 0 and p.total["ok"] >= 200 and p.total["warp_refused"] == 0


@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("win", [5, 7, 9])
def test_48x36_under_45_degrees(pair, win, cost):
    """Most windows touch a border: samples the upright window would accept are invalid for the turned one, and features whose
    every sample is invalid end OUTSIDE after a search that has a record."""
    p = pair(WS.SMALL_W, WS.SMALL_H, max_features=32, max_poseframes=2, K=K_4836, win_size=win)
    p.set_warp()
    p.set_cost_name(cost)
    seen = spy_costs(p)
    for k, (img, T) in enumerate(WS.small()):
        p.track(img, T, k == 0)
    turned = [c for c, Jq in seen if Jq is not None]
    assert all(Jq is not None and Jq != WR.IDENTITY for _, Jq in seen)
    assert sum(c is None for c in turned) >= 10 and sum(c is not None for c in turned) >= 10
    assert p.total["ok"] + p.total["bad_match"] + p.total["ambiguous"] + p.total["outside"] >= 6


def test_with_the_gradient_gate_and_both_gates(pair):
    p = pair(WS.W, WS.H, K=WS.K, win_size=7)
    p.set_warp()
    p.set_cost()
    p.set_gates(letterbox=True, max_height=0.05, up=(0, 1, 0))
    p.set_ref_grad(12.0)
    assert p.gpu.info("gates") == 3 and p.gpu.info("warp") == 1 and p.gpu.info("ref_grad") == 1
    for k, (img, T) in enumerate(WS.scene("roll30")):
        o = p.track(img, T, k in (0, 4))
        assert (o["vtx"][:, 1] >= 40).all() and (o["vtx"][:, 1] <= 79).all()
    assert p.total["ok"] >= 30 and p.total["ref_grad"] >= 10 and p.total["held"] + p.total["refused"] >= 10, p.total


def test_with_the_gradient_gate_alone(pair):
    p = pair(WS.W, WS.H, K=WS.K, win_size=5)
    p.set_warp()
    p.set_ref_grad(12.0)
    for k, (img, T) in enumerate(WS.scene("roll30")[:5]):
        p.track(img, T, k == 0)
    assert p.total["ok"] >= 50 and p.total["ref_grad"] >= 20, p.total


@pytest.mark.parametrize("first", [False, True])
def test_switch_flipped_between_frames(pair, first):
    """The state holds nothing of the switch: every frame is the current setting's on the state it finds.  Under the roll an
    upright frame loses most searches, a warped one finds them again."""
    p = pair(WS.W, WS.H, K=WS.K, win_size=5)
    ok = []
    for k, (img, T) in enumerate(WS.scene("roll30")):
        on = first if k % 2 == 1 else not first
        p.set_warp(on)
        before = p.total["ok"]
        p.track(img, T, k == 0)
        ok.append((on, p.total["ok"] - before))
    warped = [n for on, n in ok[1:] if on]
    upright = [n for on, n in ok[1:] if not on]
    assert min(warped) > max(upright), ok


def test_two_pose_frames_with_different_maps(pair):
    """Pose frames 0 (upright) and 3 (rolled): the features of ring slot 0 are tracked through the roll, those of slot 1 through
    nearly the identity, in one launch."""
    p = pair(WS.W, WS.H, K=WS.K, win_size=5)
    p.set_warp()
    for k, (img, T) in enumerate(WS.scene("roll30")):
        p.ref.maps = []
        p.track(img, T, k in (0, 3))
    pf = p.ref.pf
    by_slot = {0: set(), 1: set()}
    for m in p.ref.maps:
        by_slot[int(pf[m[0]])].add(m[-1])
    assert len(by_slot[0]) >= 1 and len(by_slot[1]) >= 1 and not (by_slot[0] & by_slot[1])
    assert all(abs(Jq[1]) >= 100 for Jq in by_slot[0]) and all(abs(Jq[1]) <= 8 for Jq in by_slot[1])
    assert p.total["ok"] >= 250


@pytest.mark.parametrize("kind", ["closer", "grazing"])
def test_refusal(pair, kind):
    """Refused maps on the device: OUTSIDE, counted, no search record, and the Matches picture draws nothing for them."""
    img, T0 = WS.scene("roll30")[0]
    p = pair(WS.W, WS.H, K=WS.K, win_size=5, max_dropouts=1, **WS.REFUSAL_PRIOR)
    p.set_warp()
    p.track(img, T0, True)
    p.track(img, WS.refusal(kind), False)
    n = p.total["warp_refused"]
    assert n >= 40 and p.gpu.info("outside") >= n
    got = p.gpu.debug_image(D.IMG_MATCHES)
    assert np.array_equal(got, p.ref.debug_image(D.IMG_MATCHES))
    if kind == "closer":  # (every feature is refused: the picture is the grey image)
        assert np.array_equal(got, D.background(img))
        p.track(img, WS.refusal(kind), False)  # the second dropout: they die
        assert p.gpu.info("died") == n and p.gpu.info("live") == 0


@pytest.mark.parametrize("how", ["never_set", "set_and_cleared"])
def test_switch_off_changes_nothing(pair, how):
    """The no-behaviour-change proof: against frontend_ref.FrontEndRef with every switch off on "diagonal_roll"."""
    p = pair(SC.W, SC.H, K=SC.K)
    if how == "set_and_cleared":
        p.gpu.set_warp()
        assert p.gpu.info("warp") == 1
        p.gpu.set_warp(False)
    assert p.gpu.info("warp") == 0
    for k, (img, T) in enumerate(SC.scene("diagonal_roll", 1)):
        p.track(img, T, k in (0, 3))
    assert p.total["emitted"] >= 300 and p.total["ok"] >= 100


def test_pure_translation_changes_no_bit_on_the_device(pair):
    """Jq = (256, 0, 0, 256) for every feature: the warped kernel gives what the restatement WITHOUT the switch gives."""
    p = pair(WS.W, WS.H, K=WS.K, win_size=5)
    p.gpu.set_warp()
    p.expect["warp"] = 1  # (the restatement runs without the switch)
    for k, (img, T) in enumerate(WS.translation()):
        p.track(img, T, k == 0)
    assert p.total["ok"] >= 200


def test_debug_images_of_a_warped_frame(pair):
    p = pair(WS.W, WS.H, K=WS.K, win_size=5)
    p.set_warp()
    frames = WS.scene("roll30")
    for k, (img, T) in enumerate(frames[:3]):
        p.track(img, T, k == 0)
    got = p.gpu.debug_image(D.IMG_MATCHES)
    want = D.draw_matches(frames[2][0], p.ref.status, p.ref.kstar, p.ref.seg, p.ref.steps)  # fe_debug_ref fed this frame's record
    assert np.array_equal(got, want) and np.array_equal(want, p.ref.debug_image(D.IMG_MATCHES))
    colour = lambda im, c: (im == np.array(c, np.uint8)).all(axis=2)  # noqa: E731
    assert colour(got, D.YELLOW).sum() >= 30 and colour(got, D.GREEN).sum() >= 100
    assert np.array_equal(p.gpu.debug_image(D.IMG_DETECTIONS), p.ref.debug_image(D.IMG_DETECTIONS))
    # the upright tracker's picture of the same frames is another one
    q = pair(WS.W, WS.H, K=WS.K, win_size=5)
    for k, (img, T) in enumerate(frames[:3]):
        q.track(img, T, k == 0)
    assert not np.array_equal(q.gpu.debug_image(D.IMG_MATCHES), got)


@pytest.mark.parametrize("max_features", [5, 8])
def test_small_feature_tables(pair, max_features):
    """One slot past a block of four wavefronts, and two whole blocks: the detections that find no slot are dropped."""
    p = pair(WS.W, WS.H, max_features=max_features, K=WS.K, win_size=5)
    p.set_warp()
    for k, (img, T) in enumerate(WS.scene("roll30")[:4]):
        p.track(img, T, k == 0)
        assert p.gpu.info("live") <= max_features
    assert p.total["ok"] >= 2 * max_features
