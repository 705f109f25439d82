"""The GPU front-end tests' harness: one GPU handle (flame_hip_frontend_*) and one restatement (tests/frontend_ref.py) fed the same
calls, the switches included, and compared after EVERY frame -- the emitted features, `state()` and `searches()` bit for bit, both
debug images byte for byte, every count and the switches' read-backs.  A helper, not a test and not a conftest: the test modules
import the `pair` fixture by name."""
import numpy as np
import pytest

from tests import fe_debug_ref as D
from tests import fe_rg_ref as RG
from tests import frontend_ref as R

STATUS_KEYS = ("ok", "no_parallax", "outside", "bad_match", "ambiguous", "new", "died")
K_4836 = np.array([140, 0, 23.5, 0, 140, 17.5, 0, 0, 1], np.float32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def compare(tag, got, want):
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, "%s: %s has shape %s, restatement %s" % (tag, k, g.shape, w.shape)
        bad = np.flatnonzero((bits(g) != bits(w)).reshape(len(w), -1).any(axis=1)) if len(w) else []
        assert len(bad) == 0, "%s: %s differs at %s: gpu %s restatement %s" % (tag, k, bad[:5], g[bad[:5]], w[bad[:5]])


def same_picture(tag, got, want):
    assert got.shape == want.shape and got.dtype == np.uint8, tag
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, "%s: %d pixels differ, first (y, x) %s: gpu %s restatement %s" % (
        tag, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


class Pair:
    """One GPU handle and one restatement fed the same calls."""

    def __init__(self, W, H, max_features=256, max_poseframes=4, K=R.SCENE_K, pitch=None, out_pitch=None, **kw):
        from flame_ros_amd.frontend import GpuFrontEnd, default_frontend_params
        self.gpu = GpuFrontEnd(W, H, K, max_features, max_poseframes)
        self.ref = R.FrontEndRef(W, H, K, max_features, max_poseframes)
        self.pr, self.pg = R.params(**kw), default_frontend_params(**kw)
        self.W, self.H, self.pitch, self.out_pitch, self.frame = W, H, pitch, out_pitch, 0
        self.total = dict(held=0, refused=0, emitted=0, ref_grad=0, warp_refused=0)
        self.total.update({k: 0 for k in STATUS_KEYS})
        self.expect = {}    # read-backs a test sets on the device alone: key -> value, against the restatement's switch
        self.ref_grad = []  # REF_GRAD count per frame
        self.record = []    # per frame: what the GPU gave (features, state, searches)

    def close(self):
        self.gpu.close()

    # ---- the switches: set on both sides, every read-back checked ----
    def set_cost(self, zero_mean=True):
        self.gpu.set_cost(zero_mean)
        self.ref.set_cost(zero_mean)
        self.check_switches("set_cost")

    def set_gain_invariant(self, on=True):
        self.gpu.set_gain_invariant(on)
        self.ref.set_gain_invariant(on)
        assert self.ref.gain_invariant == bool(on)
        self.check_switches("set_gain_invariant")  # (cost_mode untouched)

    def set_cost_name(self, cost):
        if cost == "zssd":
            self.set_cost()
        if cost == "gi":
            self.set_gain_invariant()

    def set_warp(self, on=True):
        self.gpu.set_warp(on)
        self.ref.set_warp(on)
        assert self.ref.warp == bool(on)
        self.check_switches("set_warp")

    def set_ref_grad(self, g):
        self.gpu.set_ref_grad(g)
        self.ref.set_ref_grad(g)
        assert self.gpu.info("ref_grad") == int(g > 0)
        self.check_switches("set_ref_grad")

    def set_gates(self, **kw):
        self.gpu.set_gates(**kw)
        self.ref.set_gates(**kw)
        self.check_switches("set_gates")

    def check_switches(self, tag):
        ref, gates = self.ref, self.ref.gates or dict(letterbox=False, height=False)
        want = dict(cost_mode=ref.cost_mode, gain_invariant=int(ref.gain_invariant), ref_grad=int(ref.min_epi_grad > 0), warp=int(ref.warp),
                    gates=int(gates["letterbox"]) | 2 * int(gates["height"]))
        want.update(self.expect)
        for key, w in want.items():
            assert self.gpu.info(key) == w, (tag, key)

    def track(self, img, T, is_pf, img_id=None, raw=None):
        """`raw`: the GPU takes this raw image through track_raw, the restatement the rectified `img`."""
        img_id = self.frame if img_id is None else img_id
        gimg = img
        if self.pitch:  # rows `pitch` bytes apart, the image starting at an odd address
            buf = np.full(img.shape[0] * self.pitch + 1, 0xAB, np.uint8)
            gimg = np.lib.stride_tricks.as_strided(buf[1:], img.shape, (self.pitch, 1))
            gimg[...] = img
        want = self.ref.track(self.pr, img, img_id, T, is_pf)
        got = self.gpu.track_raw(self.pg, raw, img_id, T, is_pf) if raw is not None else self.gpu.track(self.pg, gimg, img_id, T, is_pf)
        tag = "frame %d" % self.frame
        compare(tag, got, want)
        state = self.check_state(tag)
        searches = self.gpu.searches()
        compare(tag + " searches", searches, self.ref.searches())
        self.pictures(tag)
        counts = self.ref.counts
        for st, key in enumerate(STATUS_KEYS):
            assert self.gpu.info(key) == counts.get(st, 0), (tag, key)
            self.total[key] += counts.get(st, 0)
        n_rg, n_wr = counts.get(RG.REF_GRAD, 0), counts.get("warp_refused", 0)
        assert self.gpu.info("fail_ref_grad") == n_rg and self.gpu.info("warp_refused") == n_wr, tag
        assert self.gpu.info("emitted") == len(want["slot"]) and self.gpu.info("detections_dropped") == self.ref.dropped, tag
        assert self.gpu.info("held_height") == self.ref.held and self.gpu.info("refused_letterbox") == self.ref.refused, tag
        self.check_switches(tag)
        for k, v in (("held", self.ref.held), ("refused", self.ref.refused), ("emitted", len(want["slot"])), ("ref_grad", n_rg),
                     ("warp_refused", n_wr)):
            self.total[k] += v
        self.ref_grad.append(n_rg)
        self.record.append((got, state, searches))
        self.frame += 1
        return want

    def check_state(self, tag):
        state = self.gpu.state()
        compare(tag + " state", state, self.ref.state())
        assert self.gpu.info("live") == int(self.ref.alive.sum()), tag
        assert self.gpu.info("poseframes") == sum(self.ref.pf_used), tag
        return state

    def check(self, tag):
        """Between frames: the record of the last tracked frame and both pictures outlive set_poses and prune (the restatement
        need not have followed them: status and k* alone are read of the state); returns the pictures."""
        st = self.gpu.state()
        assert np.array_equal(st["status"], self.ref.status) and np.array_equal(st["kstar"], self.ref.kstar), tag
        compare(tag + " searches", self.gpu.searches(), self.ref.searches())
        return self.pictures(tag)

    def pictures(self, tag):
        """Both debug images against the restatement's, byte for byte; returns them."""
        pics = {}
        for kind, name in ((D.IMG_MATCHES, "matches"), (D.IMG_DETECTIONS, "detections")):
            if self.out_pitch:  # the bytes between the rows stay what they were
                buf = np.full(self.H * self.out_pitch, 0xAB, np.uint8)
                pic = self.gpu.debug_image(kind, pitch=self.out_pitch, out=buf)
                rows = buf.reshape(self.H, self.out_pitch)
                assert (rows[:, 3 * self.W:] == 0xAB).all(), "%s %s: padding bytes written" % (tag, name)
            else:
                pic = self.gpu.debug_image(kind)
            same_picture("%s %s" % (tag, name), pic, self.ref.debug_image(kind))
            pics[name] = np.array(pic)
        return pics


@pytest.fixture
def pair(gpu):
    made = []

    def make(*a, **kw):
        made.append(Pair(*a, **kw))
        return made[-1]
    yield make
    for p in made:
        p.close()
