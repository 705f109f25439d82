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

pytestmark = pytest.mark.gpu
K_4837 = np.array([140, 0, 23.5, 0, 140, 18, 0, 0, 1], np.float32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def compare(tag, got, want):
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, "%s: %s has shape %s, restatement %s" % (tag, k, g.shape, w.shape)
        bad = np.flatnonzero((bits(g) != bits(w)).reshape(len(w), -1).any(axis=1)) if len(w) else []
        assert len(bad) == 0, "%s: %s differs at %s: gpu %s restatement %s" % (tag, k, bad[:5], g[bad[:5]], w[bad[:5]])


class Pair:
    """One GPU handle and one restatement fed the same calls."""

    def __init__(self, W, H, max_features=256, max_poseframes=4, K=R.SCENE_K, ref=None, **kw):
        from flame_ros_amd.frontend import GpuFrontEnd, default_frontend_params
        self.gpu = GpuFrontEnd(W, H, K, max_features, max_poseframes)
        self.ref = (ref or G.GatesDebugRef)(W, H, K, max_features, max_poseframes)
        self.pr, self.pg = R.params(**kw), default_frontend_params(**kw)
        self.frame = 0
        self.total = dict(held=0, refused=0, died=0, new=0, emitted=0)

    def close(self):
        self.gpu.close()

    def set_gates(self, **kw):
        self.gpu.set_gates(**kw)
        self.ref.set_gates(**kw)

    def track(self, img, T, is_pf, img_id=None):
        img_id = self.frame if img_id is None else img_id
        want = self.ref.track(self.pr, img, img_id, T, is_pf)
        got = self.gpu.track(self.pg, img, img_id, T, is_pf)
        tag = "frame %d" % self.frame
        compare(tag, got, want)
        compare(tag + " state", self.gpu.state(), self.ref.state())
        if hasattr(self.ref, "searches"):
            compare(tag + " searches", self.gpu.searches(), self.ref.searches())
        for st, key in enumerate(("ok", "no_parallax", "outside", "bad_match", "ambiguous", "new", "died")):
            assert self.gpu.info(key) == self.ref.counts.get(st, 0), (tag, key)
        assert self.gpu.info("emitted") == len(want["slot"]) and self.gpu.info("detections_dropped") == self.ref.dropped
        assert self.gpu.info("live") == int(self.ref.alive.sum())
        held, refused = getattr(self.ref, "held", 0), getattr(self.ref, "refused", 0)
        assert self.gpu.info("held_height") == held and self.gpu.info("refused_letterbox") == refused, tag
        for k, v in (("held", held), ("refused", refused), ("died", self.ref.counts.get(R.DIED, 0)), ("new", self.ref.counts.get(R.NEW, 0)),
                     ("emitted", len(want["slot"]))):
            self.total[k] += v
        self.frame += 1
        return want


@pytest.fixture
def pair(gpu):
    made = []

    def make(*a, **kw):
        made.append(Pair(*a, **kw))
        return made[-1]
    yield make
    for p in made:
        p.close()


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
    """The no-behaviour-change proof: against frontend_ref.FrontEndRef itself (which knows no gates) on "diagonal_roll"."""
    from flame_ros_amd import frontend as FE
    p = pair(SC.W, SC.H, K=SC.K, ref=R.FrontEndRef)
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
