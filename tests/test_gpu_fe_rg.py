"""GPU: the reference-patch gradient gate (flame_hip_frontend_set_ref_grad: the RG instantiations of k_fe_track, csrc/frontend.hip)
against the restatement tests/fe_rg_ref.py (pinned by tests/test_fe_rg_ref.py): after EVERY frame the emitted features, `state()`,
`searches()` and the counts bit for bit.  The shapes are the smallest at which the rule still bites: the 160 x 120 plane scenes
(80 cells, six frames at the most) and 48 x 36 images for the window sizes."""
import numpy as np
import pytest

from tests import fe_debug_ref as D
from tests import fe_rg_ref as RG
from tests import fe_zm_scenes as ZS
from tests import frontend_ref as R
from tests import frontend_scenes as SC
from tests.fe_pair import pair  # noqa: F401  (pair: the fixture)

pytestmark = pytest.mark.gpu
K_4836 = np.array([140, 0, 23.5, 0, 140, 17.5, 0, 0, 1], np.float32)
STATUS_KEYS = ("ok", "no_parallax", "outside", "bad_match", "ambiguous", "new", "died")
G0 = 5.0


@pytest.mark.parametrize("name", ["sideways", "vertical"])
def test_half_striped_scenes(pair, name):
    """The ground-truth test's scenes: the striped half is refused, the isotropic half is tracked; a refused feature keeps its
    prior, takes its dropouts and dies with the sixth."""
    p = pair(ZS.W, ZS.H, K=ZS.K, win_size=7)
    p.set_ref_grad(G0)
    for k, (img, T) in enumerate(RG.half_striped(name)):
        p.track(img, T, k == 0)
        refused = p.ref.status == RG.REF_GRAD
        assert (p.ref.kstar[refused] == -1).all() and (p.ref.steps[refused] == 0).all() and (p.ref.drop[refused] == k).all()
        assert (p.ref.mu[refused] == np.float32(0.5)).all() and (p.ref.var[refused] == np.float32(0.25)).all()
    assert p.ref_grad[0] == 0 and min(p.ref_grad[1:]) >= 25 and p.total["ok"] >= 150, (p.ref_grad, p.total)
    q = pair(ZS.W, ZS.H, K=ZS.K, win_size=7, max_dropouts=3)  # ... and death: the refused features die in the fourth tracking frame
    q.set_ref_grad(G0)
    for k, (img, T) in enumerate(RG.half_striped(name)[:5]):
        before = q.total["died"]
        q.track(img, T, k == 0)
        if k == 4:
            assert q.total["died"] - before >= 25 and q.ref_grad[4] == q.ref_grad[3]  # (counted as REF_GRAD and as DIED)
    assert q.gpu.info("live") == int(q.ref.alive.sum()) <= 55


@pytest.mark.parametrize("name", ["diagonal_roll", "forward"])
def test_general_motion(pair, name):
    """Epipolar lines that are neither rows nor columns (a roll; an epipole inside the image), frames 0 and 3 pose frames: two ring
    slots with an epipole each."""
    p = pair(SC.W, SC.H, K=SC.K)
    p.set_ref_grad(6.0)  # (on this smooth texture, 15 px per texel, a part of the windows lies below it: both outcomes in every frame)
    for k, (img, T) in enumerate(SC.scene(name, 1)):
        p.track(img, T, k in (0, 3))
    assert p.total["ref_grad"] >= 20 and p.total["ok"] >= 60, p.total
    assert len({int(f) for f in p.ref.pf[p.ref.alive > 0]}) == 2


@pytest.mark.parametrize("along", ["x", "y"])
def test_direction_comes_from_the_reference_image(pair, along):
    """Rolled by pi / 2: the line runs along x in the reference image and along y in the current one."""
    p = pair(ZS.W, ZS.H, K=ZS.K, win_size=7)
    p.set_ref_grad(G0)
    for k, (img, T) in enumerate(RG.rolled(along)):
        p.track(img, T, k == 0)
    tested = p.total["ref_grad"] + p.total["ok"] + p.total["bad_match"] + p.total["ambiguous"]
    assert tested >= 100
    if along == "x":
        assert p.total["ref_grad"] == tested
    else:
        assert p.total["ref_grad"] <= tested // 10


@pytest.mark.parametrize("win", [3, 5, 9])
def test_48x36(pair, win):
    """One and two passes of the lanes over the window (9, 25, 81 pixels), two pose frames, windows at the image's edge."""
    W, H = 48, 36
    p = pair(W, H, max_features=32, max_poseframes=2, K=K_4836, win_size=win)
    p.set_ref_grad(8.0)
    a, b = R.shift_scene(3, 4, W=W, H=H)
    o = p.track(a[0], a[1], True)
    assert len(o["slot"]) >= 4
    p.track(b[0], b[1], False)
    p.track(b[0], R.pose((3 * 2.0 / R.SCENE_F, 0.03, 0.0)), True)
    p.track(a[0], R.pose((0.0, -0.03, 0.02), 0.004), False)
    p.track(a[0], R.pose((0.08, 0.0, 0.0)), False)
    assert p.total["ref_grad"] >= 2 and p.total["ok"] + p.total["bad_match"] + p.total["ambiguous"] + p.total["outside"] >= 4, p.total


def test_ring_leaves_the_image_when_the_window_grew(pair):
    """Detected at win 3 on the detector's margin, tracked at win 5: the ring of that window leaves the image -> OUTSIDE, no read
    (tests/test_fe_rg_ref.py shows that the ungated tracker searches this feature)."""
    MW, MH, MK, margin_scene = RG.MARGIN_W, RG.MARGIN_H, RG.MARGIN_K, RG.margin_scene
    img, second, T0, T1 = margin_scene()
    p = pair(MW, MH, max_features=32, max_poseframes=2, K=MK, win_size=3)
    p.set_ref_grad(G0)
    p.track(img, T0, True)
    s, = np.flatnonzero((p.ref.alive > 0) & (p.ref.u == MW - 3) & (p.ref.v == 18))
    p.pr = R.params(win_size=5)
    p.pg.win_size = 5
    p.track(second, T1, False)
    assert p.ref.status[s] == R.OUTSIDE and p.ref.steps[s] == 0 and p.ref.drop[s] == 1
    assert p.total["ok"] + p.total["ref_grad"] >= 4  # (the others were tested)


def test_gate_switched_in_mid_sequence(pair):
    """Off -> on -> off: the state holds no gate, every frame is the current setting's on the state it finds."""
    p = pair(ZS.W, ZS.H, K=ZS.K, win_size=7)
    for k, (img, T) in enumerate(RG.half_striped("sideways")):
        if k in (2, 4):
            p.set_ref_grad(G0 if k == 2 else 0.0)
        p.track(img, T, k == 0)
    assert p.gpu.info("ref_grad") == 0
    assert p.ref_grad[:2] == [0, 0] and min(p.ref_grad[2:4]) >= 25 and p.ref_grad[4:] == [0, 0], p.ref_grad


def test_with_zssd(pair):
    p = pair(ZS.W, ZS.H, K=ZS.K, win_size=7)
    p.set_cost()
    p.set_ref_grad(G0)
    assert p.gpu.info("cost_mode") == 1 and p.gpu.info("ref_grad") == 1
    for k, (img, T) in enumerate(RG.half_striped("vertical")):
        p.track(img, T, k in (0, 4))
    assert p.total["ref_grad"] >= 100 and p.total["ok"] >= 100, p.total


def test_with_both_gates(pair):
    """The letterbox refuses projections of REF_GRAD features too: still one dropout per frame."""
    p = pair(ZS.W, ZS.H, K=ZS.K, win_size=7)
    p.set_gates(letterbox=True, max_height=0.05, up=(0, 1, 0))
    p.set_ref_grad(G0)
    assert p.gpu.info("gates") == 3
    for k, (img, T) in enumerate(RG.half_striped("sideways")):
        o = p.track(img, T, k in (0, 4))
        assert (o["vtx"][:, 1] >= 40).all() and (o["vtx"][:, 1] <= 79).all()
    assert p.total["ref_grad"] >= 30 and p.total["held"] >= 5 and p.total["ok"] >= 30, p.total


def test_with_zssd_and_both_gates(pair):
    p = pair(ZS.W, ZS.H, K=ZS.K, win_size=7)
    p.set_cost()
    p.set_gates(letterbox=True, max_height=0.05, up=(0, 1, 0))
    p.set_ref_grad(G0)
    for k, (img, T) in enumerate(RG.half_striped("sideways")[:4]):
        p.track(img, T, k == 0)
    assert p.total["ref_grad"] >= 20 and p.total["ok"] >= 20, p.total


def test_matches_image_of_a_frame_with_refused_slots(pair):
    p = pair(ZS.W, ZS.H, K=ZS.K, win_size=7)
    p.set_ref_grad(G0)
    frames = RG.half_striped("sideways")
    for k, (img, T) in enumerate(frames[:3]):
        p.track(img, T, k == 0)
    assert (p.ref.status == RG.REF_GRAD).sum() >= 25
    got = p.gpu.debug_image(D.IMG_MATCHES)
    want = D.draw_matches(frames[2][0], p.ref.status, p.ref.kstar, p.ref.seg, p.ref.steps)
    assert np.array_equal(got, want) and np.array_equal(want, p.ref.debug_image(D.IMG_MATCHES))
    colour = lambda im, c: (im == np.array(c, np.uint8)).all(axis=2)  # noqa: E731
    assert colour(got, D.YELLOW).sum() >= 20
    # ... and the refused slots draw nothing: the ungated tracker's picture has searches in the striped half, this one has none
    q = pair(ZS.W, ZS.H, K=ZS.K, win_size=7)
    for k, (img, T) in enumerate(frames[:3]):
        q.track(img, T, k == 0)
    ungated = q.gpu.debug_image(D.IMG_MATCHES)
    drawn = lambda im: ~colour(im, (0, 0, 0)) & (im[..., 0] != im[..., 1])  # noqa: E731
    refused = p.ref.status == RG.REF_GRAD
    box = np.zeros((ZS.H, ZS.W), bool)
    for u, v in zip(p.ref.u[refused], p.ref.v[refused]):
        box[max(v - 8, 0):v + 9, max(u - 8, 0):u + 9] = True
    assert (drawn(ungated) & box).sum() > (drawn(got) & box).sum()


@pytest.mark.parametrize("how", ["never_set", "set_to_zero", "set_and_cleared"])
def test_gate_off_changes_nothing(pair, how):
    """The no-behaviour-change proof: against frontend_ref.FrontEndRef with every switch off on "diagonal_roll"."""
    p = pair(SC.W, SC.H, K=SC.K)
    if how == "set_to_zero":
        p.gpu.set_ref_grad(0.0)
    elif how == "set_and_cleared":
        p.gpu.set_ref_grad(G0)
        assert p.gpu.info("ref_grad") == 1
        p.gpu.set_ref_grad(0.0)
    assert p.gpu.info("ref_grad") == 0
    for k, (img, T) in enumerate(SC.scene("diagonal_roll", 1)):
        p.track(img, T, k in (0, 3))
    assert p.total["emitted"] >= 300 and p.total["ok"] >= 100 and p.total["ref_grad"] == 0
