"""GPU: the front end's gates (flame_hip_frontend_set_gates: letterbox and height band, csrc/frontend.hip) against the restatement
tests/fe_gates_ref.py (pinned by tests/test_fe_gates_ref.py): after EVERY frame the emitted features, `state()`, `searches()` and
the counts -- the two gate counters included -- bit for bit.  The shapes are the smallest at which the rules still bite: the
48 x 37 image of the band arithmetic, the 160 x 120 plane scenes of the ground-truth test."""
import ctypes as C

import numpy as np
import pytest

from tests import fe_debug_ref as D
from tests import fe_gates_ref as G
from tests import frontend_corpus as FC
from tests import frontend_ref as R
from tests import frontend_scenes as SC
from tests.fe_pair import pair  # noqa: F401  (pair: the fixture)

pytestmark = pytest.mark.gpu
K_4837 = np.array([140, 0, 23.5, 0, 140, 18, 0, 0, 1], np.float32)


def test_letterbox_48x37(pair):
    """H = 37: band rows 12...24, cells of 16 (cell row 0 clipped to 12...15, row 2 = rows 32...36 outside).  Two pose frames; the
    camera steps down and up so that projections cross both edges of the band."""
    W, H = 48, 37
    p = pair(W, H, max_features=32, max_poseframes=2, K=K_4837, max_dropouts=1)
    p.set_gates(letterbox=True)
    assert p.gpu.info("gates") == 1
    a, b = R.shift_scene(3, 4, W=W, H=H)
    o = p.track(a[0], a[1], True)
    assert len(o["slot"]) >= 4 and (o["vtx"][:, 1] >= 12).all() and (o["vtx"][:, 1] <= 24).all()
    p.track(b[0], b[1], False)
    p.track(b[0], R.pose((3 * 2.0 / R.SCENE_F, 0.06, 0.0)), False)
    p.track(b[0], R.pose((3 * 2.0 / R.SCENE_F, -0.06, 0.0)), True)
    p.track(a[0], R.pose((0.0, -0.08, 0.0)), False)
    p.track(a[0], R.pose((0.0, 0.08, 0.0)), False)
    assert p.total["refused"] >= 4 and p.total["died"] >= 1 and p.total["new"] >= 6


def test_letterbox_vertical_scene_features_leave_the_band_and_die(pair):
    """max_dropouts = 0: the first refused projection kills.  (A match that succeeds clears the counter before the refusal adds its
    one dropout, so with max_dropouts >= 1 a feature that leaves the band but still matches lives on at one dropout, exactly like
    one that leaves the image.)"""
    p = pair(SC.W, SC.H, K=SC.K, max_dropouts=0)
    p.set_gates(letterbox=True)
    for k, (img, T) in enumerate(SC.scene("vertical", 1)):
        o = p.track(img, T, k == 0)
        assert (o["vtx"][:, 1] >= 40).all() and (o["vtx"][:, 1] <= 79).all()
    assert p.total["refused"] >= 4 and p.total["died"] >= p.total["refused"]


@pytest.mark.parametrize("name", list(G.BANDS))
def test_height_band_on_the_ground_truth_scenes(pair, name):
    """The bands of the ground-truth test; frame 4 is a second pose frame, so held cells block detections."""
    lo, hi = G.BANDS[name]
    p = pair(SC.W, SC.H, K=SC.K)
    p.set_gates(min_height=lo, max_height=hi, up=(0, 1, 0))
    assert p.gpu.info("gates") == 2
    for k, (img, T) in enumerate(SC.scene(name, 1)):
        p.track(img, T, k in (0, 4))
    assert p.total["held"] >= 80 and p.total["emitted"] >= 200 and p.total["refused"] == 0


def test_height_band_colliding_pair(pair):
    """The holder with the smallest variance of its cell leaves the emission to the other feature; min_height == max_height."""
    c, pr, plain, out_plain, (cell, win, lose), h = G.colliding_runs()
    p = pair(FC.W, FC.H, FC.SLOTS, FC.RING, K=c.K, **c.kw)
    for call in c.calls[:2]:
        p.track(call[1], call[2], call[3], call[4])
    p.set_gates(min_height=h[lose], max_height=h[lose], up=(0, 1, 0))
    o = p.track(c.calls[2][1], c.calls[2][2], c.calls[2][3], c.calls[2][4])
    assert win in p.ref.held_slots and lose in o["slot"] and win not in o["slot"]
    before = p.total["new"]
    p.track(c.calls[3][1], c.calls[3][2], c.calls[3][3], c.calls[3][4])  # the pose frame: no detection in a held cell
    assert p.total["held"] >= 60 and p.total["new"] == before + p.ref.counts[R.NEW]


def test_nan_height_is_held(pair):
    W, H = 48, 36
    K = np.array([50, 0, 24, 0, 50, 18, 0, 0, 1], np.float32)
    img = np.full((H, W), 100, np.uint8)
    img[19, 8] = 255
    p = pair(W, H, max_features=32, max_poseframes=2, K=K, idepth_init=0.0)
    p.set_gates(min_height=-G.BIG, max_height=G.BIG, up=(0, 1, 0))
    p.track(img, R.pose(), True)
    o = p.track(img, R.pose(), False)
    assert len(o["slot"]) == 0 and p.ref.held_slots == [0]


def test_both_gates_then_cleared_then_set_again(pair):
    """Letterbox and height band together on "sideways" with a second pose frame; cleared in mid-sequence (the next frames are the
    ungated tracker's on the state the gates left), then set again."""
    p = pair(SC.W, SC.H, K=SC.K)
    p.set_gates(letterbox=True, max_height=0.05, up=(0, 1, 0))
    assert p.gpu.info("gates") == 3
    frames = SC.scene("sideways", 1, frames=10)
    for k, (img, T) in enumerate(frames[:6]):
        o = p.track(img, T, k in (0, 4))
        assert (o["vtx"][:, 1] >= 40).all() and (o["vtx"][:, 1] <= 79).all()
    gated = dict(p.total)
    assert gated["held"] >= 20 and gated["refused"] >= 1
    p.set_gates()
    assert p.gpu.info("gates") == 0
    o = p.track(frames[6][0], frames[6][1], True)
    assert (o["vtx"][:, 1] < 40).any() and (o["vtx"][:, 1] > 79).any() and p.total["held"] == gated["held"]
    p.track(frames[7][0], frames[7][1], False)
    p.set_gates(letterbox=True, min_height=-0.3, max_height=0.05, up=(0, 1, 0))
    for k in (8, 9):
        p.track(frames[k][0], frames[k][1], k == 9)
    assert p.total["held"] > gated["held"] and p.total["refused"] > gated["refused"] + 20


@pytest.mark.parametrize("how", ["never_set", "switches_off", "set_and_cleared"])
def test_no_gate_changes_nothing(pair, how):
    """The no-behaviour-change proof: against frontend_ref.FrontEndRef with every switch off on "diagonal_roll"."""
    from flame_ros_amd import frontend as FE
    p = pair(SC.W, SC.H, K=SC.K)
    if how == "switches_off":
        g = FE.Gates(0, 0, 0.25, -0.25, (C.c_float * 3)(0.0, 0.0, 0.0))  # (the other fields are not read)
        assert p.gpu._lib.flame_hip_frontend_set_gates(p.gpu._h, C.byref(g)) == 0
    elif how == "set_and_cleared":
        p.gpu.set_gates(letterbox=True, min_height=-0.1, max_height=0.1)
        p.gpu.set_gates()
    assert p.gpu.info("gates") == 0
    for k, (img, T) in enumerate(SC.scene("diagonal_roll", 1)):
        p.track(img, T, k in (0, 3))
    assert p.total["emitted"] >= 300 and p.total["held"] == 0 and p.total["refused"] == 0


def test_detections_image_shows_the_gated_output(pair):
    p = pair(SC.W, SC.H, K=SC.K)
    p.set_gates(letterbox=True, max_height=0.05, up=(0, 1, 0))
    for k, (img, T) in enumerate(SC.scene("sideways", 1)[:5]):
        o = p.track(img, T, k in (0, 4))
    assert p.ref.held >= 10 and (o["status"] == R.NEW).any() and (o["status"] != R.NEW).any()
    got = p.gpu.debug_image(D.IMG_DETECTIONS)
    want = D.draw_detections(SC.scene("sideways", 1)[4][0], o["vtx"], o["status"])
    assert np.array_equal(got, want) and np.array_equal(want, p.ref.debug_image(D.IMG_DETECTIONS))
    assert np.array_equal(p.gpu.debug_image(D.IMG_MATCHES), p.ref.debug_image(D.IMG_MATCHES))  # held features' searches are drawn
    colour = lambda im, c: (im == np.array(c, np.uint8)).all(axis=2)  # noqa: E731
    assert not colour(got, D.GREEN)[:39].any() and not colour(got, D.BLUE)[:39].any() and not colour(got, D.GREEN)[81:].any()
