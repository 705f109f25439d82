"""GPU: the gain-invariant matching cost (flame_hip_frontend_set_gain_invariant: k_fe_track<kFeCostGi, .>, csrc/frontend.hip)
against the restatement tests/fe_gi_ref.py (pinned by tests/test_fe_gi_ref.py): after EVERY frame the emitted features, `state()`,
`searches()` and the counts bit for bit.  The shapes are the smallest at which the rule still bites: 48 x 36 images for the window
sizes and the branches, the 160 x 120 plane scenes of the ground-truth and the invariance tests, one 160 x 120 pair for the searches
of 256 steps."""
import numpy as np
import pytest

from tests import fe_debug_ref as D
from tests import fe_gi_ref as GI
from tests import fe_gi_scenes as GS
from tests import fe_zm_ref as Z
from tests import fe_zm_scenes as ZS
from tests import frontend_ref as R
from tests import frontend_scenes as SC
from tests.fe_pair import compare, pair  # noqa: F401  (pair: the fixture)

pytestmark = pytest.mark.gpu
K_4836 = np.array([140, 0, 23.5, 0, 140, 17.5, 0, 0, 1], np.float32)
STATUS_KEYS = ("ok", "no_parallax", "outside", "bad_match", "ambiguous", "new", "died")


def spy_costs(p):
    """Records every cost the restatement forms from now on."""
    seen = []
    cost = p.ref._cost
    p.ref._cost = lambda *a: seen.append(cost(*a)) or seen[-1]
    return seen


@pytest.mark.parametrize("gain", [1.0, 0.8])
@pytest.mark.parametrize("name", ["sideways", "diagonal_roll", "refpose_nonidentity"])
def test_plane_scenes_under_gain(pair, name, gain):
    """The scenes of the CPU ground-truth test (win 7, pose frame 0, frames 1 ... 5 = floor(gain v + 0.5))."""
    p = pair(ZS.W, ZS.H, K=ZS.K, win_size=7)
    p.set_gain_invariant()
    for k, (img, T) in enumerate(ZS.scene(name, 1, gain=None if gain == 1.0 else gain)):
        out = p.track(img, T, k == 0)
        assert (p.ref.steps[p.ref.alive > 0] < 64).all()  # (every search of these scenes fits the first pass)
    err, emitted = ZS.relative_errors(out, T)
    assert emitted >= 40 and len(err) >= 0.8 * emitted and p.total["ok"] >= 100


@pytest.mark.parametrize("win", [5, 7])
@pytest.mark.parametrize("name", ["sideways", "diagonal_roll"])
def test_halved_scenes_and_gain_invariance_on_the_device(pair, name, win):
    """The CPU invariance test's scenes (frames 0 and 4 are pose frames): the plain and the gained run each equal the restatement,
    and the device's own two runs equal each other bit for bit."""
    plain, gained = pair(ZS.W, ZS.H, K=ZS.K, win_size=win), pair(ZS.W, ZS.H, K=ZS.K, win_size=win)
    for p, frames in ((plain, GS.halved(name)), (gained, GS.gained(name)[0])):
        p.set_gain_invariant()
        for k, (img, T) in enumerate(frames):
            p.track(img, T, k in GS.POSEFRAMES)
    assert plain.total["ok"] >= 100 and plain.total["emitted"] >= 180
    for k, (a, b) in enumerate(zip(plain.record, gained.record)):
        for i, what in enumerate(("features", "state", "searches")):
            compare("frame %d %s, plain against gained" % (k, what), a[i], b[i])
    assert plain.total == gained.total


def test_zssd_on_the_device_is_moved_by_the_gain(pair):
    """... so the invariance above is the cost's and not the scene's."""
    plain, gained = pair(ZS.W, ZS.H, K=ZS.K, win_size=7), pair(ZS.W, ZS.H, K=ZS.K, win_size=7)
    for p, frames in ((plain, GS.halved("sideways")), (gained, GS.gained("sideways")[0])):
        p.set_cost()
        for k, (img, T) in enumerate(frames[:3]):
            p.track(img, T, k == 0)
    assert gained.total["bad_match"] > plain.total["bad_match"] and gained.total["ok"] < plain.total["ok"]


@pytest.mark.parametrize("win", [3, 5, 9])
def test_48x36(pair, win):
    """Two pose frames, searches along rows and along a slanted line, windows that leave the small image."""
    W, H = 48, 36
    p = pair(W, H, max_features=32, max_poseframes=2, K=K_4836, win_size=win)
    p.set_gain_invariant()
    a, b = R.shift_scene(3, 4, W=W, H=H)
    o = p.track(a[0], a[1], True)
    assert len(o["slot"]) >= 4
    p.track(b[0], b[1], False)
    p.track(b[0], R.pose((3 * 2.0 / R.SCENE_F, 0.03, 0.0)), True)
    p.track(a[0], R.pose((0.0, -0.03, 0.02), 0.004), False)
    p.track(a[0], R.pose((0.08, 0.0, 0.0)), False)
    assert p.total["ok"] >= 4 and p.total["ok"] + p.total["bad_match"] + p.total["ambiguous"] + p.total["outside"] >= 12


def chessboard(W=48, H=36):
    """A one-pixel chessboard of 0 / 255 with one flipped pixel per cell (the only gradients there are)."""
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.where((yy + xx) % 2 == 0, 255, 0).astype(np.uint8)
    for y in (8, 24):
        for x in (8, 24, 40):
            img[y, x] = 255 - img[y, x]
    return img


def test_near_extreme_windows_and_anti_correlation(pair):
    """The chessboard tracked against its inverse at win = 9 under the largest threshold: where the inverse lines up ZIR < 0 with
    n SII, SI^2 and SI SR near 2^43.7 and C = ZR near 2^42.7 -- the anti-correlated fit is refused --, a sample one pixel on
    correlates and costs a sixteenth of that.  Sums held in 32 bits or in float would move k*."""
    W, H = 48, 36
    img = chessboard(W, H)
    p = pair(W, H, max_features=32, max_poseframes=2, K=K_4836, win_size=9, max_match_error=65025.0)
    p.set_gain_invariant()
    o = p.track(img, R.pose(), True)
    assert len(o["slot"]) >= 6
    seen = spy_costs(p)
    p.track(255 - img, R.pose((0.03, 0.0, 0.0)), False)
    costs = [c for c in seen if c is not None]
    assert max(costs) >= 2 ** 42 and min(costs) < 2 ** 39 and max(costs) < 2 ** 45
    assert p.total["ok"] + p.total["ambiguous"] >= 6 and p.total["bad_match"] == 0


def test_identical_and_flat_current_windows(pair):
    """Two branches on the device.  (1) Every row of the image one grey, the camera moved along x: every sample's window IS the
    reference window (ZI = ZR = ZIR, the quotient is exact) and C = 0.  (2) The next frame is flat: ZI == 0 at every sample, C = ZR
    of a textured window, far above the threshold: BAD_MATCH."""
    W, H = 48, 36
    rows = np.random.default_rng(2).integers(30, 226, H).astype(np.uint8)
    img = np.ascontiguousarray(np.repeat(rows[:, None], W, axis=1))
    p = pair(W, H, max_features=32, max_poseframes=2, K=K_4836, win_size=5)
    p.set_gain_invariant()
    o = p.track(img, R.pose(), True)
    assert len(o["slot"]) >= 4
    seen = spy_costs(p)
    p.track(img, R.pose((0.03, 0.0, 0.0)), False)
    costs = [c for c in seen if c is not None]
    assert len(costs) >= 12 and max(costs) == 0 and p.total["ok"] >= 4
    del seen[:]
    before = p.total["bad_match"]
    p.track(np.full((H, W), 77, np.uint8), R.pose((0.03, 0.0, 0.0)), False)
    costs = [c for c in seen if c is not None]
    assert costs and min(costs) > Z.bad_threshold(100.0, 5, Z.COST_ZSSD)
    assert p.total["bad_match"] - before >= 4


def test_flat_reference_window(pair):
    """ZR == 0 on the device.  A detection sits on a gradient maximum, so no window of 3 x 3 or more around it is flat; the 1 x 1
    window the ABI admits always is (n = 1: ZR = ZI = ZIR = 0): every cost is 0 and every search ends in BAD_MATCH, where ZSSD, whose
    costs are 0 as well, matches."""
    W, H = 48, 36
    a, b = R.shift_scene(3, 4, W=W, H=H)
    p = pair(W, H, max_features=32, max_poseframes=2, K=K_4836, win_size=1)
    p.set_gain_invariant()
    o = p.track(a[0], a[1], True)
    assert len(o["slot"]) >= 4
    seen = spy_costs(p)
    p.track(b[0], b[1], False)
    costs = [c for c in seen if c is not None]
    assert costs and max(costs) == 0
    assert p.total["bad_match"] >= 4 and p.total["ok"] == 0
    q = pair(W, H, max_features=32, max_poseframes=2, K=K_4836, win_size=1)
    q.set_cost()
    q.track(a[0], a[1], True)
    q.track(b[0], b[1], False)
    assert q.total["ok"] >= 4 and q.total["bad_match"] == 0


@pytest.mark.parametrize("tx,steps", [(0.1, 140), (1.0, 256)])
def test_long_search(pair, tx, steps):
    """A prior as wide as the clamp makes the search 140 tx x 9.99 px long: 140 steps (three passes of the 64 lanes) and the cap of
    256 (all five passes live: the last one holds sample 256 alone)."""
    p = pair(ZS.W, ZS.H, K=R.SCENE_K, var_init=25.0, win_size=7)
    p.set_gain_invariant()
    (a, _), = ZS.scene("sideways", 1, frames=1)
    p.track(a, R.pose(), True)
    dark = np.floor(0.7 * np.ascontiguousarray(a[:, ::-1]) + 0.5).astype(np.uint8)
    p.track(dark, R.pose((tx, 0.004, 0.0)), False)
    live = p.ref.alive > 0
    assert live.sum() >= 40 and (p.ref.steps[live] == steps).all()
    if steps < 256:
        assert (p.ref.kstar[live] > 64).any()


@pytest.mark.parametrize("zero_mean", [False, True])
def test_switched_on_off_and_on_in_mid_sequence(pair, zero_mean):
    """On the scene at gain 0.6: the state holds no cost, every frame is the current cost's on the state it finds, and switching
    off returns to what set_cost chose."""
    p = pair(ZS.W, ZS.H, K=ZS.K, win_size=7)
    p.set_cost(zero_mean)
    frames = ZS.scene("sideways", 1, gain=0.6)
    bad = []
    for k, (img, T) in enumerate(frames):
        if k in (1, 3, 5):
            p.set_gain_invariant(k != 3)
        before = p.total["bad_match"]
        p.track(img, T, k == 0)
        bad.append(p.total["bad_match"] - before)
    assert p.gpu.info("gain_invariant") == 1 and p.gpu.info("cost_mode") == int(zero_mean)
    assert bad[1] <= 8 and bad[2] <= 8 and bad[3] >= 20 and bad[4] >= 20 and bad[5] <= 8, bad  # (SSD and ZSSD refuse what the gain moved)


def test_with_both_gates_and_the_gradient_gate(pair):
    p = pair(ZS.W, ZS.H, K=ZS.K, win_size=7)
    p.set_gain_invariant()
    p.set_gates(letterbox=True, max_height=0.05, up=(0, 1, 0))
    p.set_ref_grad(12.0)
    assert p.gpu.info("gates") == 3 and p.gpu.info("gain_invariant") == 1 and p.gpu.info("ref_grad") == 1
    for k, (img, T) in enumerate(ZS.scene("sideways", 1, gain=0.8)):
        o = p.track(img, T, k in (0, 4))
        assert (o["vtx"][:, 1] >= 40).all() and (o["vtx"][:, 1] <= 79).all()
    assert p.total["held"] >= 10 and p.total["ok"] >= 50 and p.total["ref_grad"] >= 20, p.total


def test_matches_image_of_a_gain_invariant_frame(pair):
    p = pair(ZS.W, ZS.H, K=ZS.K, win_size=7)
    p.set_gain_invariant()
    frames = ZS.scene("sideways", 1, gain=0.6)
    for k, (img, T) in enumerate(frames[:3]):
        p.track(img, T, k == 0)
    got = p.gpu.debug_image(D.IMG_MATCHES)
    want = D.draw_matches(frames[2][0], p.ref.status, p.ref.kstar, p.ref.seg, p.ref.steps)  # fe_debug_ref fed this cost's record
    assert np.array_equal(got, want) and np.array_equal(want, p.ref.debug_image(D.IMG_MATCHES))
    colour = lambda im, c: (im == np.array(c, np.uint8)).all(axis=2)  # noqa: E731
    assert colour(got, D.YELLOW).sum() >= 30 and colour(got, D.GREEN).sum() >= 100
    # the ZSSD tracker's picture of the same frames is another one: the gain moves its matches
    q = pair(ZS.W, ZS.H, K=ZS.K, win_size=7)
    q.set_cost()
    for k, (img, T) in enumerate(frames[:3]):
        q.track(img, T, k == 0)
    assert not np.array_equal(q.gpu.debug_image(D.IMG_MATCHES), got)


@pytest.mark.parametrize("how", ["never_set", "set_and_cleared"])
def test_switch_off_changes_nothing(pair, how):
    """The no-behaviour-change proof: against frontend_ref.FrontEndRef with every switch off on "diagonal_roll"."""
    p = pair(SC.W, SC.H, K=SC.K)
    if how == "set_and_cleared":
        p.gpu.set_gain_invariant()
        assert p.gpu.info("gain_invariant") == 1
        p.gpu.set_gain_invariant(False)
    assert p.gpu.info("gain_invariant") == 0 and p.gpu.info("cost_mode") == 0
    for k, (img, T) in enumerate(SC.scene("diagonal_roll", 1)):
        p.track(img, T, k in (0, 3))
    assert p.total["emitted"] >= 300 and p.total["ok"] >= 100
