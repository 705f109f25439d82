"""GPU: the zero-mean matching cost (flame_hip_frontend_set_cost: k_fe_track<true>, csrc/frontend.hip) against the restatement
tests/fe_zm_ref.py (pinned by tests/test_fe_zm_ref.py): after EVERY frame the emitted features, `state()`, `searches()` and the counts
bit for bit.  The shapes are the smallest at which the rule still bites: 48 x 36 images for the window sizes and the extremes, the
160 x 120 plane scenes of the invariance test, one 160 x 120 pair for the searches of 256 steps."""
import numpy as np
import pytest

from tests import fe_debug_ref as D
from tests import fe_zm_scenes as ZS
from tests import frontend_ref as R
from tests import frontend_scenes as SC
from tests.fe_pair import compare, pair  # noqa: F401  (pair: the fixture)

pytestmark = pytest.mark.gpu
K_4836 = np.array([140, 0, 23.5, 0, 140, 17.5, 0, 0, 1], np.float32)
STATUS_KEYS = ("ok", "no_parallax", "outside", "bad_match", "ambiguous", "new", "died")


OFFSETS = ZS.random_offsets(7)


@pytest.mark.parametrize("win", [5, 7])
@pytest.mark.parametrize("name", ["sideways", "diagonal_roll"])
def test_invariance_scenes_and_offset_invariance_on_the_device(pair, name, win):
    """The CPU test's scenes (frames 0 and 4 are pose frames): the plain and the offset run each equal the restatement, and the
    device's own two runs equal each other bit for bit."""
    plain, shifted = pair(ZS.W, ZS.H, K=ZS.K, win_size=win), pair(ZS.W, ZS.H, K=ZS.K, win_size=win)
    for p, offsets in ((plain, None), (shifted, OFFSETS)):
        p.set_cost()
        for k, (img, T) in enumerate(ZS.scene(name, 1, offsets)):
            p.track(img, T, k in (0, 4))
            assert (p.ref.steps[p.ref.alive > 0] < 64).all()  # (every search of these scenes fits the first pass)
    assert plain.total["ok"] >= 150 and plain.total["emitted"] >= 240
    for k, (a, b) in enumerate(zip(plain.record, shifted.record)):
        for i, what in enumerate(("features", "state", "searches")):
            compare("frame %d %s, plain against offset" % (k, what), a[i], b[i])
    assert plain.total == shifted.total


def test_ssd_on_the_device_is_moved_by_the_offsets(pair):
    """... so the invariance above is the cost's and not the scene's."""
    plain, shifted = pair(ZS.W, ZS.H, K=ZS.K, win_size=7), pair(ZS.W, ZS.H, K=ZS.K, win_size=7)
    for p, offsets in ((plain, None), (shifted, OFFSETS)):
        for k, (img, T) in enumerate(ZS.scene("sideways", 1, offsets)[:3]):
            p.track(img, T, k == 0)
    assert shifted.total["bad_match"] > plain.total["bad_match"] and shifted.total["ok"] < plain.total["ok"]


@pytest.mark.parametrize("win", [3, 5, 9])
def test_48x36(pair, win):
    """Two pose frames, searches along rows and along a slanted line, windows that leave the small image."""
    W, H = 48, 36
    p = pair(W, H, max_features=32, max_poseframes=2, K=K_4836, win_size=win)
    p.set_cost()
    a, b = R.shift_scene(3, 4, W=W, H=H)
    o = p.track(a[0], a[1], True)
    assert len(o["slot"]) >= 4
    p.track(b[0], b[1], False)
    p.track(b[0], R.pose((3 * 2.0 / R.SCENE_F, 0.03, 0.0)), True)
    p.track(a[0], R.pose((0.0, -0.03, 0.02), 0.004), False)
    p.track(a[0], R.pose((0.08, 0.0, 0.0)), False)
    assert p.total["ok"] >= 4 and p.total["ok"] + p.total["bad_match"] + p.total["ambiguous"] + p.total["outside"] >= 12


def test_extremes_windows(pair):
    """A one-pixel chessboard of 0 / 255 with one flipped pixel per cell (the only gradients there are), tracked against its inverse
    at win = 9 under the largest threshold: where the inverse lines up, D alternates +-65 280 over the whole window and C comes
    within a pixel's worth of (81^2 - 1) 65 280^2 = 2^44.7; a sample one pixel on costs next to nothing.  A 32-bit S1^2 or n S2 would
    wrap the large costs below the small ones and move k*."""
    W, H = 48, 36
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.where((yy + xx) % 2 == 0, 255, 0).astype(np.uint8)
    for y in (8, 24):
        for x in (8, 24, 40):
            img[y, x] = 255 - img[y, x]
    p = pair(W, H, max_features=32, max_poseframes=2, K=K_4836, win_size=9, max_match_error=65025.0)
    p.set_cost()
    o = p.track(img, R.pose(), True)
    assert len(o["slot"]) >= 6
    seen = []
    cost = p.ref._cost
    p.ref._cost = lambda *a: seen.append(cost(*a)) or seen[-1]
    p.track(255 - img, R.pose((0.03, 0.0, 0.0)), False)
    costs = [c for c in seen if c is not None]
    assert max(costs) >= 2 ** 44 and min(costs) < 2 ** 41 and max(costs) < 2 ** 45
    assert p.total["ok"] + p.total["ambiguous"] >= 6 and p.total["bad_match"] == 0


@pytest.mark.parametrize("tx,steps", [(0.1, 140), (1.0, 256)])
def test_long_search(pair, tx, steps):
    """A prior as wide as the clamp makes the search 140 tx x 9.99 px long: 140 steps (three passes of the 64 lanes) and the cap of
    256 (all five passes live: the last one holds sample 256 alone)."""
    p = pair(ZS.W, ZS.H, K=R.SCENE_K, var_init=25.0, win_size=7)
    p.set_cost()
    (a, _), = ZS.scene("sideways", 1, [OFFSETS[0]], frames=1)
    p.track(a, R.pose(), True)
    p.track(np.ascontiguousarray(a[:, ::-1]) + np.uint8(9), R.pose((tx, 0.004, 0.0)), False)
    live = p.ref.alive > 0
    assert live.sum() >= 40 and (p.ref.steps[live] == steps).all()
    if steps < 256:
        assert (p.ref.kstar[live] > 64).any()


def test_mode_switched_in_mid_sequence(pair):
    """SSD -> ZSSD -> SSD on the offset scene: the state holds no cost, every frame is the current mode's on the state it finds."""
    p = pair(ZS.W, ZS.H, K=ZS.K, win_size=7)
    frames = ZS.scene("sideways", 1, OFFSETS)
    bad = []
    for k, (img, T) in enumerate(frames):
        if k in (2, 4):
            p.set_cost(zero_mean=(k == 2))
        before = p.total["bad_match"]
        p.track(img, T, k == 0)
        bad.append(p.total["bad_match"] - before)
    assert p.gpu.info("cost_mode") == 0
    assert bad[1] >= 10 and bad[2] <= 5 and bad[3] <= 5 and bad[5] >= 10, bad  # (SSD refuses what the offsets moved, ZSSD does not)


def test_zssd_with_both_gates(pair):
    p = pair(ZS.W, ZS.H, K=ZS.K, win_size=7)
    p.set_cost()
    p.set_gates(letterbox=True, max_height=0.05, up=(0, 1, 0))
    assert p.gpu.info("gates") == 3 and p.gpu.info("cost_mode") == 1
    for k, (img, T) in enumerate(ZS.scene("sideways", 1, OFFSETS)):
        o = p.track(img, T, k in (0, 4))
        assert (o["vtx"][:, 1] >= 40).all() and (o["vtx"][:, 1] <= 79).all()
    assert p.total["held"] >= 10 and p.total["ok"] >= 50, p.total


def test_matches_image_of_a_zssd_frame(pair):
    p = pair(ZS.W, ZS.H, K=ZS.K, win_size=7)
    p.set_cost()
    frames = ZS.scene("sideways", 1, OFFSETS)
    for k, (img, T) in enumerate(frames[:3]):
        p.track(img, T, k == 0)
    got = p.gpu.debug_image(D.IMG_MATCHES)
    want = D.draw_matches(frames[2][0], p.ref.status, p.ref.kstar, p.ref.seg, p.ref.steps)  # fe_debug_ref fed the ZSSD record
    assert np.array_equal(got, want) and np.array_equal(want, p.ref.debug_image(D.IMG_MATCHES))
    colour = lambda im, c: (im == np.array(c, np.uint8)).all(axis=2)  # noqa: E731
    assert colour(got, D.YELLOW).sum() >= 30 and colour(got, D.GREEN).sum() >= 100
    # the SSD tracker's picture of the same frames is another one: the offsets move its matches
    q = pair(ZS.W, ZS.H, K=ZS.K, win_size=7)
    for k, (img, T) in enumerate(frames[:3]):
        q.track(img, T, k == 0)
    assert not np.array_equal(q.gpu.debug_image(D.IMG_MATCHES), got)


@pytest.mark.parametrize("how", ["never_set", "set_to_ssd", "zssd_and_back"])
def test_ssd_mode_changes_nothing(pair, how):
    """The no-behaviour-change proof: against frontend_ref.FrontEndRef with every switch off on "diagonal_roll"."""
    p = pair(SC.W, SC.H, K=SC.K)
    if how == "set_to_ssd":
        p.gpu.set_cost(zero_mean=False)
    elif how == "zssd_and_back":
        p.gpu.set_cost()
        assert p.gpu.info("cost_mode") == 1
        p.gpu.set_cost(zero_mean=False)
    assert p.gpu.info("cost_mode") == 0
    for k, (img, T) in enumerate(SC.scene("diagonal_roll", 1)):
        p.track(img, T, k in (0, 3))
    assert p.total["emitted"] >= 300 and p.total["ok"] >= 100
