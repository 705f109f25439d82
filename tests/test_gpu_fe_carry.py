"""GPU: the hand-over of an evicted pose frame's features (flame_hip_frontend_set_carry: k_fe_carry behind k_fe_compact and the
evicting frame's other order, csrc/frontend.hip and frontend.cpp) against the restatement tests/fe_carry_ref.py (pinned by
tests/test_fe_carry_ref.py): after EVERY frame what fe_pair.Pair compares -- the emitted features, `state()`, `searches()`, both
debug images, every count and the info keys, bit for bit -- plus `carried` and `carry_lost`.  The shapes are the smallest at which
the rule still bites: the 160 x 120 hovering sequence of the ground-truth test at rings of 2 and 1, and 48 x 36 images, where
every cell touches a border or the letterbox band."""
import numpy as np
import pytest

from tests import fe_carry_ref as CR
from tests import frontend_ref as R
from tests.fe_pair import K_4836, Pair

pytestmark = pytest.mark.gpu
FAILED = (R.OUTSIDE, R.BAD_MATCH, R.AMBIGUOUS, 7)


class CarryPair(Pair):
    """fe_pair.Pair with the restatement of the hand-over in the restatement's place."""

    def __init__(self, W, H, max_features=256, max_poseframes=2, K=R.SCENE_K, **kw):
        super().__init__(W, H, max_features, max_poseframes, K, **kw)
        self.ref = CR.CarryRef(W, H, K, max_features, max_poseframes)
        self.expect["carry"] = 0
        self.total.update(carried=0, carry_lost=0)
        self.why = dict(failed=0, held=0, loser=0, border=0)  # why the restatement's old features were not carried
        self.evictions = 0

    def set_carry(self, on=True):
        self.gpu.set_carry(on)
        self.ref.set_carry(on)
        self.expect["carry"] = int(bool(on))
        self.check_switches("set_carry")

    def track(self, img, T, is_pf, **kw):
        want = super().track(img, T, is_pf, **kw)
        tag = "frame %d" % (self.frame - 1)
        assert self.gpu.info("carried") == self.ref.carried and self.gpu.info("carry_lost") == self.ref.carry_lost, tag
        self.total["carried"] += self.ref.carried
        self.total["carry_lost"] += self.ref.carry_lost
        self.evictions += self.ref.evicted is not None
        emitted = set(int(s) for s in want["slot"])
        for s in self.ref.lost_slots:
            st = self.ref.status[s]
            self.why["failed" if st in FAILED else "held" if s in self.ref.held_slots else "loser" if s not in emitted else "border"] += 1
        return want


@pytest.fixture
def cpair(gpu):
    made = []

    def make(*a, **kw):
        made.append(CarryPair(*a, **kw))
        return made[-1]
    yield make
    for p in made:
        p.close()


HOVER = CR.hover_scene(1, 14)
SMALL = CR.hover_small(14)


def feed(p, frames, every, between=None):
    for k, (img, T) in enumerate(frames):
        if between:
            between(k)
        p.track(img, T, k % every == 0)


@pytest.mark.parametrize("ring, every", [(2, 3), (1, 2)])
def test_hovering_sequence(cpair, ring, every):
    """The sequence of the CPU ground-truth test, 14 frames: the graph's vertices survive every eviction on the device."""
    p = cpair(R.SCENE_W, R.SCENE_H, max_poseframes=ring)
    p.set_carry()
    feed(p, HOVER, every)
    assert p.evictions == len([k for k in range(14) if k % every == 0 and k // every >= ring])
    assert p.total["carried"] >= 40 * p.evictions // 2 and p.total["carry_lost"] >= 1, p.total
    out, T = p.record[-1][0], HOVER[-1][1]
    n, err = CR.graph_vertices(out, T)
    assert n >= 0.8 * 44 and np.median(err) < 0.01


@pytest.mark.parametrize("cost, win", [("zssd", 5), ("gi", 7)])
def test_with_each_cost(cpair, cost, win):
    p = cpair(R.SCENE_W, R.SCENE_H, max_poseframes=2, win_size=win)
    p.set_carry()
    p.set_cost_name(cost)
    feed(p, HOVER[:10], 3)
    assert p.evictions == 2 and p.total["carried"] >= 40, p.total


def test_with_warp_and_the_gradient_gate(cpair):
    p = cpair(R.SCENE_W, R.SCENE_H, max_poseframes=2)
    p.set_carry()
    p.set_warp()
    p.set_ref_grad(5.0)
    feed(p, HOVER[:10], 3)
    assert p.evictions == 2 and p.total["carried"] >= 30, p.total


def test_with_a_letterbox_at_160x120(cpair):
    p = cpair(R.SCENE_W, R.SCENE_H, max_poseframes=2)
    p.set_carry()
    p.set_gates(letterbox=True)
    feed(p, HOVER[:10], 3)
    st = p.record[-1][1]
    live = st["alive"] != 0
    assert p.evictions == 2 and p.total["carried"] >= 10 and (st["v"][live] >= 40).all() and (st["v"][live] < 80).all(), p.total


@pytest.mark.parametrize("case", ["plain", "letterbox_ring1", "height_win7"])
def test_rule_cases_through_images_at_48x36(cpair, case):
    """Failed features, cell losers, features the height gate holds and pixels within m of the border
    all occur among the old features of these runs, and the device loses exactly the restatement's.  (A projection outside the
    letterbox band is refused by the tracker already: it is not emitted and counts as a loser here.)"""
    kw, gates, ring, every, reached = dict(
        plain=(dict(detection_win_size=8), None, 2, 3, ("failed", "loser", "border")),
        letterbox_ring1=(dict(detection_win_size=8), dict(letterbox=True), 1, 2, ("failed", "loser")),
        height_win7=(dict(detection_win_size=8, win_size=7), dict(max_height=0.05, up=(0, 1, 0)), 2, 2, ("failed", "held")))[case]
    p = cpair(48, 36, max_features=64, max_poseframes=ring, K=K_4836, **kw)
    p.set_carry()
    if gates:
        p.set_gates(**gates)
    feed(p, SMALL, every)
    assert p.total["carried"] >= 10 and all(p.why[r] >= 1 for r in reached), (p.total, p.why)


def test_a_full_table_takes_detections_into_slots_that_died(cpair):
    """Eight slots: old features die in tracking and at the hand-over, and detections take the free slots of the same frame."""
    p = cpair(48, 36, max_features=8, max_poseframes=1, K=K_4836, detection_win_size=8, max_dropouts=0)
    p.set_carry()
    feed(p, SMALL, 2)
    assert p.total["carried"] >= 4 and p.total["died"] >= 1 and p.total["new"] >= 10, p.total


def test_ring_slot_image_after_the_copy(cpair):
    """Rows 171 bytes apart from an odd address: after an evicting frame `image()` reads the ring slot's copy, which is the frame."""
    p = cpair(R.SCENE_W, R.SCENE_H, max_poseframes=1, pitch=171)
    p.set_carry()
    for k, (img, T) in enumerate(HOVER[:5]):
        p.track(img, T, k % 2 == 0)
        assert np.array_equal(p.gpu.image(), img), k
    assert p.evictions == 2 and p.total["carried"] >= 40
    # the next frame is tracked against that copy: Pair.track has compared it bit for bit
    p.track(*HOVER[5], False)
    assert p.total["ok"] >= 100


def test_toggling_between_frames(cpair):
    """Ring 2, a pose frame every 3rd frame: frames 6, 9 and 12 evict; the switch is on for 6 and 12."""
    p = cpair(R.SCENE_W, R.SCENE_H, max_poseframes=2)
    toggles = {4: True, 7: False, 11: True}
    seen = []

    def between(k):
        if k in toggles:
            p.set_carry(toggles[k])
    for k, (img, T) in enumerate(HOVER):
        between(k)
        p.track(img, T, k % 3 == 0)
        seen.append((p.ref.evicted is not None, p.gpu.info("carried")))
    assert [k for k, (e, _) in enumerate(seen) if e] == [6, 12] and seen[9][1] == 0 and seen[6][1] > 0 and seen[12][1] > 0


def test_prune_and_set_poses_between_frames(cpair):
    """`prune` kills as before, carried features included; `set_poses` moves the new pose frame's pose, which the carried features
    follow like its detections."""
    p = cpair(R.SCENE_W, R.SCENE_H, max_poseframes=2)
    p.set_carry()
    for k, (img, T) in enumerate(HOVER[:8]):
        p.track(img, T, k % 3 == 0)
    assert p.evictions == 1 and p.total["carried"] >= 20  # frame 6 took ring slot 0 from frame 0
    T6 = HOVER[6][1].copy()
    T6[0, 3] += 0.002
    p.gpu.set_poses([6], [T6])
    p.ref.set_poses([6], [T6])
    p.track(*HOVER[8], False)
    p.gpu.prune([6])  # pose frame 3 goes: its features die, the carried ones of pose frame 6 stay
    p.ref.prune([6])
    p.check_state("after prune")
    assert p.gpu.info("poseframes") == 1 and p.gpu.info("live") >= 20
    p.track(*HOVER[9], True)  # takes ring slot 1, which prune has freed: not an evicting frame
    assert p.ref.evicted is None and p.gpu.info("carried") == 0
    p.gpu.prune([])
    p.ref.prune([])
    p.check_state("after prune of everything")
    assert p.gpu.info("live") == 0


@pytest.mark.parametrize("how", ["never_set", "set_and_cleared"])
def test_switch_off_equals_frontend_ref(pair_off, how):
    """The no-behaviour-change proof: fe_pair.Pair itself, frontend_ref.FrontEndRef on the other side, through evictions."""
    p = pair_off
    if how == "set_and_cleared":
        p.gpu.set_carry()
        assert p.gpu.info("carry") == 1
        p.gpu.set_carry(False)
    assert p.gpu.info("carry") == 0
    for k, (img, T) in enumerate(HOVER[:10]):
        p.track(img, T, k % 3 == 0)
        assert p.gpu.info("carried") == 0 and p.gpu.info("carry_lost") == 0
    assert type(p.ref) is R.FrontEndRef and p.total["ok"] >= 200


@pytest.fixture
def pair_off(gpu):
    p = Pair(R.SCENE_W, R.SCENE_H, max_poseframes=2)
    yield p
    p.close()
