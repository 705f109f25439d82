"""CPU: the hand-over of an evicted pose frame's features (DESIGN.md 5.3 "Hand-over") -- the restatement tests/fe_carry_ref.py,
which the GPU has to equal bit for bit (tests/test_gpu_fe_carry.py), pinned independently of any kernel:
  1. the ABI surface on a handle without a device;
  2. the rule on hand-built states at 48 x 36, one case each;
  3. no evicting frame, or the switch off: no bit of output, state or searches changes against frontend_ref.FrontEndRef;
  4. after every evicting frame every live slot of the ring slot is NEW or carried, and the counts add up;
  5. toggling the switch between frames;
  6. ground truth on the hovering sequence."""
import ctypes as C

import numpy as np
import pytest

from flame_ros_amd import lib
from tests import fe_carry_ref as CR
from tests import frontend_ref as R
from tests.fe_pair import K_4836

F = np.float32
W, H = 48, 36


# ---- 1. the ABI surface, on a handle without a device ----

def test_abi_surface_without_a_device():
    L = lib.load()
    assert hasattr(L, "flame_hip_frontend_set_carry")
    assert L.flame_hip_version() >= 413
    from flame_ros_amd import frontend as FE
    assert callable(FE.GpuFrontEnd.set_carry)
    assert C.sizeof(FE.FrontEndParams) == 40  # (the parameter record keeps its size: the switch is the handle's)
    h = C.c_void_p()
    assert L.flame_hip_frontend_create(C.byref(h), -1, W, H, K_4836.ctypes.data_as(C.c_void_p), 64, 2) == 0
    try:
        def info(key):
            v = C.c_int64(-7)
            assert L.flame_hip_frontend_info(h, key, C.byref(v)) == 0
            return v.value
        sc = L.flame_hip_frontend_set_carry
        assert info(b"carry") == 0 and info(b"carried") == 0 and info(b"carry_lost") == 0
        assert sc(None, 1) == lib.ERR_ARG and sc(None, 0) == lib.ERR_ARG
        assert sc(h, 1) == 0 and info(b"carry") == 1
        for bad in (2, -1, 256, -2 ** 31):
            assert sc(h, bad) == lib.ERR_ARG and info(b"carry") == 1  # a refused value leaves the switch as it was
        assert sc(h, 0) == 0 and info(b"carry") == 0
        assert sc(h, 7) == lib.ERR_ARG and info(b"carry") == 0
        assert sc(h, 1) == 0
        p = FE.default_frontend_params()
        img, T, n = np.zeros((H, W), np.uint8), np.ascontiguousarray(R.pose().reshape(-1)), C.c_int32()
        assert L.flame_hip_frontend_track(h, C.byref(p), img.ctypes.data_as(C.c_void_p), W, 0, T.ctypes.data_as(C.c_void_p), 1,
                                          C.byref(n)) == lib.ERR_NODEVICE
        assert info(b"carry") == 1 and info(b"warp") == 0 and info(b"cost_mode") == 0 and info(b"gain_invariant") == 0
    finally:
        L.flame_hip_frontend_destroy(h)
    with FE.GpuFrontEnd(W, H, K_4836, 64, 2, device=-1) as fe:
        assert fe.info("carry") == 0
        fe.set_carry()
        assert fe.info("carry") == 1
        fe.set_carry(False)
        assert fe.info("carry") == 0 and fe.info("carried") == 0 and fe.info("carry_lost") == 0


# ---- 2. the rule on hand-built states ----

WIN, DWS, NCX = 5, 16, 3  # m = 3: detections sit in 3 <= x < 45, 3 <= y < 33


def one(status=R.OK, px=20.25, py=10.75, xc=0.41, vc=0.003, pf=1, a=1, wins=True, cell=None, alive=1, y_lo=0, y_hi=None, P=2):
    """One old feature in slot 2 beside a NEW detection of ring slot `a` in slot 0 and a feature of another pose frame in slot 1."""
    cell = (int(py) // DWS) * NCX + int(px) // DWS if cell is None else cell
    alive_ = np.array([1, 1, alive], np.uint8)
    pf_ = np.array([a, (a + 1) % max(P, 2), pf], np.int32)
    status_ = np.array([R.NEW, R.OK, status], np.int32)
    cell_of = np.array([5, 4, cell], np.int32)
    winner = {5: 0, 4: 1}
    if cell >= 0:
        winner[cell] = 2 if wins else 1
    proj = {0: (F(40), F(20), F(0.5), F(0.25)), 1: (F(30.5), F(20.5), F(0.3), F(0.002)), 2: (F(px), F(py), F(xc), F(vc))}
    return CR.carry_rule(a, alive_, pf_, status_, cell_of, winner, proj, W, H, WIN, y_lo, y_hi)


def test_rule_a_winner_is_carried_with_the_emitted_bits():
    carried, lost = one()
    assert lost == [] and list(carried) == [2]
    ur, vr, mu, var = carried[2]
    assert (ur, vr) == (20, 11)
    assert F(mu).view(np.uint32) == F(0.41).view(np.uint32) and F(var).view(np.uint32) == F(0.003).view(np.uint32)


def test_rule_no_parallax_is_carried():
    carried, lost = one(status=R.NO_PARALLAX)
    assert list(carried) == [2] and lost == []


@pytest.mark.parametrize("status", [R.BAD_MATCH, R.AMBIGUOUS, R.OUTSIDE, 7])
def test_rule_a_failed_feature_dies(status):
    assert one(status=status) == ({}, [2])


def test_rule_a_cell_loser_dies():
    assert one(wins=False) == ({}, [2])


def test_rule_a_held_feature_dies():
    """The height gate leaves cell_of = -1."""
    assert one(cell=-1) == ({}, [2])


@pytest.mark.parametrize("px, py, kept", [
    (2.49, 10.0, False), (2.5, 10.0, True),      # ur = m - 1 | m
    (44.49, 10.0, True), (44.5, 10.0, False),    # ur = W - m - 1 | W - m
    (20.0, 2.49, False), (20.0, 2.5, True),      # vr = m - 1 | m
    (20.0, 32.49, True), (20.0, 32.5, False),    # vr = H - m - 1 | H - m
])
def test_rule_image_border(px, py, kept):
    carried, lost = one(px=px, py=py)
    assert (list(carried), lost) == (([2], []) if kept else ([], [2]))


@pytest.mark.parametrize("py, kept", [(11.49, False), (11.5, True), (23.49, True), (23.5, False)])
def test_rule_letterbox_band(py, kept):
    """H = 36: the band is the rows 12 <= y < 24."""
    carried, lost = one(py=py, y_lo=12, y_hi=24)
    assert (list(carried), lost) == (([2], []) if kept else ([], [2]))


def test_rule_a_half_rounds_up():
    carried, _ = one(px=20.5, py=10.5)
    assert carried[2][:2] == (21, 11)
    carried, _ = one(px=float(np.nextafter(F(20.5), F(0))), py=10.5)
    assert carried[2][:2] == (20, 11)


def test_rule_leaves_new_dead_and_other_pose_frames_alone():
    """Slot 0 is a NEW detection of ring slot a (it may have died in this frame and been taken again), slot 1 another pose frame's."""
    carried, lost = one(status=R.BAD_MATCH)
    assert 0 not in carried and 1 not in carried and lost == [2]
    assert one(alive=0) == ({}, [])
    assert one(pf=0, a=1) == ({}, [])
    assert one(status=R.NEW) == ({}, [])


def test_rule_ring_of_one():
    carried, lost = one(pf=0, a=0, P=1)
    assert list(carried) == [2] and lost == []


# ---- the sequences ----

def hover(frames):
    return CR.hover_scene(1, frames)


FRAMES = hover(26)


def run(fe, frames, every, toggles=None, check=None):
    p, outs = R.params(), []
    for k, (img, T) in enumerate(frames):
        if toggles and k in toggles:
            fe.set_carry(toggles[k])
        before = fe.state()
        out = fe.track(p, img, k, T, k % every == 0)
        if check:
            check(k, fe, before, out)
        outs.append((out, fe.state(), fe.searches()))
    return outs


def same_runs(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        for dx, dy in zip(x, y):
            assert dx.keys() == dy.keys()
            for key in dx:
                g, w = np.ascontiguousarray(dx[key]), np.ascontiguousarray(dy[key])
                assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (k, key)


# ---- 3. nothing changes without an evicting frame, or with the switch off ----

def test_no_evicting_frame_changes_no_bit():
    base = run(R.FrontEndRef(R.SCENE_W, R.SCENE_H, R.SCENE_K, 256, 4), FRAMES[:12], 3)
    fe = CR.CarryRef(R.SCENE_W, R.SCENE_H, R.SCENE_K, 256, 4)
    fe.set_carry()
    same_runs(run(fe, FRAMES[:12], 3), base)
    assert fe.carried == 0 and fe.carry_lost == 0 and sum(fe.pf_used) == 4


@pytest.mark.parametrize("ring, every", [(2, 3), (1, 2)])
def test_switch_off_changes_no_bit(ring, every):
    base = R.FrontEndRef(R.SCENE_W, R.SCENE_H, R.SCENE_K, 256, ring)
    fe = CR.CarryRef(R.SCENE_W, R.SCENE_H, R.SCENE_K, 256, ring)
    same_runs(run(fe, FRAMES[:14], every), run(base, FRAMES[:14], every))
    assert sum(fe.pf_used) == sum(base.pf_used) == ring and fe.pf_id[:ring] == base.pf_id


# ---- 4. the invariants of an evicting frame ----

def invariants(seen):
    def check(k, fe, before, out):
        a = fe.evicted
        if a is None:
            assert fe.carried == 0 and fe.carry_lost == 0
            return
        st = fe.state()
        old = np.flatnonzero((before["alive"] != 0) & (before["pf"] == a))
        # the old features that were live when step 3 ran: they did not die in tracking (a slot that did may be NEW now)
        live_old = [s for s in old if st["status"][s] not in (R.DIED, R.NEW, R.FREE)]
        assert fe.carried + fe.carry_lost == len(live_old), k
        assert sorted(fe.carried_slots + fe.lost_slots) == live_old, k
        em = {int(s): i for i, s in enumerate(out["slot"])}
        for s in np.flatnonzero((st["alive"] != 0) & (st["pf"] == a)):
            if st["status"][s] == R.NEW:
                continue
            assert s in fe.carried_slots and st["status"][s] in (R.OK, R.NO_PARALLAX), (k, s)
            i = em[int(s)]  # carried: the frame emitted it, and its state is the emitted record at the rounded pixel
            assert st["mu"][s].view(np.uint32) == out["idepth_mu"][i].view(np.uint32), (k, s)
            assert st["var"][s].view(np.uint32) == out["idepth_var"][i].view(np.uint32), (k, s)
            assert (st["u"][s], st["v"][s]) == tuple(int(np.floor(c + F(0.5))) for c in out["vtx"][i]), (k, s)
            assert st["drop"][s] == before["drop"][s] * (st["status"][s] != R.OK), (k, s)
        for s in fe.lost_slots:
            assert not st["alive"][s] and st["status"][s] not in (R.NEW, R.FREE, R.DIED), (k, s)
        assert not fe.pf_used[fe.ring] and fe.pf_img[fe.ring] is None and not (st["pf"][st["alive"] != 0] == fe.ring).any()
        assert fe.pf_id[a] == k and sum(fe.pf_used) == fe.ring
        seen.append((k, fe.carried, fe.carry_lost))
    return check


@pytest.mark.parametrize("ring, every", [(2, 3), (1, 2)])
def test_evicting_frames_account_for_every_old_feature(ring, every):
    fe, seen = CR.CarryRef(R.SCENE_W, R.SCENE_H, R.SCENE_K, 256, ring), []
    fe.set_carry()
    run(fe, FRAMES[:20], every, check=invariants(seen))
    assert [k for k, _, _ in seen] == [k for k in range(20) if k % every == 0 and k // every >= ring]
    assert all(c > 0 for _, c, _ in seen) and any(lost > 0 for _, _, lost in seen)


# ---- 5. toggling between frames ----

def test_toggling_between_frames():
    """Ring 2, a pose frame every 3rd frame: the evicting frames are 6, 9, 12, 15, 18; the switch is on for 6, 12 and 15."""
    fe, seen = CR.CarryRef(R.SCENE_W, R.SCENE_H, R.SCENE_K, 256, 2), []
    toggles = {4: True, 7: False, 11: True, 17: False}
    outs = run(fe, FRAMES[:20], 3, toggles, invariants(seen))
    assert [k for k, _, _ in seen] == [6, 12, 15]
    # up to the first evicting frame the run is the plain one; frame 9 evicts as ever: no old feature of its slot survives it
    base = run(R.FrontEndRef(R.SCENE_W, R.SCENE_H, R.SCENE_K, 256, 2), FRAMES[:6], 3)
    same_runs(outs[:6], base)
    st8, st9 = outs[8][1], outs[9][1]
    old = (st8["alive"] != 0) & (st8["pf"] == 1)
    assert old.any() and not ((st9["alive"] != 0) & old & (st9["status"] != R.NEW)).any()


# ---- 6. ground truth on the hovering sequence ----

# The camera swings sideways and back with period 8 in front of frontend_ref's slanted plane (160 x 120, texture seed 1):
# x = 0.06 (0, 1, 2, 3, 4, 3, 2, 1, ...) m, yaw = 0.004 (the same numbers) rad; ring of 2, a pose frame every 3rd frame, 26 frames,
# default parameters.  Graph vertices = emitted features with idepth_var < 0.01.  The restatement gives at least 44 of them in every
# frame >= 3 with the switch on; the bound is 0.8 of that, the margin being for other seeds of the same scene.
MEASURED_FLOOR = 44


def test_hovering_ground_truth():
    """Measured on the restatement: vertices with the switch off 0, 0, 20, 45, 46, 45, 0, 24, 42, 42, 49, 42, 26, 25, 41, 41, 42, 41,
    0, 27, 36, 37, 49, 44, 32, 34; on, from frame 6: 44, 53, 53, 59, 65, 59, 55, 54, 59, 68, 58, 68, 62, 60, 58, 63, 68, 62, 56, 56;
    median relative error in the last 10 frames 0.57 ... 2.19 % off, 0.25 ... 0.33 % on."""
    assert [CR.SWING[k % 8] for k in range(9)] == [0, 1, 2, 3, 4, 3, 2, 1, 0]
    T5 = CR.hover_pose(5)
    assert abs(T5[0, 3] - 0.18) < 1e-12 and abs(np.arcsin(T5[0, 2]) - 0.012) < 1e-12
    rows = {}
    for on in (False, True):
        fe = CR.CarryRef(R.SCENE_W, R.SCENE_H, R.SCENE_K, 256, 2)
        fe.set_carry(on)
        rows[on] = CR.hover_run(fe, R.params(), FRAMES, 3)
    n_off, n_on = [r[0] for r in rows[False]], [r[0] for r in rows[True]]
    print("vertices off", n_off, "\nvertices on ", n_on)
    # off: the graph is empty whenever the well-populated pose frame is evicted (a fact of the parent's restatement)
    assert n_off[6] == 0 and n_off[18] == 0
    # on: never a collapse
    assert min(n_on[3:]) >= 0.8 * MEASURED_FLOOR, n_on
    # on: the vertices are no worse, frame by frame and pooled over the last 10 frames
    med = {on: [float(np.median(r[1])) if len(r[1]) else float("inf") for r in rows[on][-10:]] for on in rows}  # (no vertex: inf)
    pooled = {on: float(np.median(np.concatenate([r[1] for r in rows[on][-10:]]))) for on in rows}
    print("median relative error, last 10 frames: off", med[False], "on", med[True], "pooled", pooled)
    assert pooled[True] <= pooled[False]
    assert all(a <= b for a, b in zip(med[True], med[False]))
