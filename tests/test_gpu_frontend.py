"""GPU: the feature front end (flame_hip_frontend_*, csrc/frontend.hip) against its NumPy restatement
(tests/frontend_ref.py, itself pinned to ground truth by tests/test_frontend_ref.py): BIT FOR BIT -- the emitted features
(vtx, idepth_mu, idepth_var, slot, status) and every slot's state (alive, pixel, pose frame, mu, var, dropouts, status, k*)
after every frame, and the per-status counts.  No tolerance anywhere: the costs are integers and the float path uses only
correctly rounded operations in one order.  The shapes are the smallest at which the kernels can still go wrong."""
import numpy as np
import pytest

from tests import frontend_ref as R
from tests import frontend_scenes as SC
from tests.fe_pair import pair  # noqa: F401  (pair: the fixture)

pytestmark = pytest.mark.gpu


def test_odd_width_pitch_and_partial_cells(pair):
    """157x93: odd width, rows 173 bytes apart from an odd address, partial cells on the right and bottom edge."""
    W, H = 157, 93
    p = pair(W, H, pitch=173)
    a, b = R.shift_scene(6, 11, W=W, H=H)
    o = p.track(a[0], a[1], True)
    assert len(o["slot"]) >= 40 and (o["vtx"][:, 0] >= 144).any() and (o["vtx"][:, 1] >= 80).any()  # partial cells detect too
    p.track(b[0], b[1], False)
    assert p.ref.counts.get(R.OK, 0) >= 30
    p.track(a[0], R.pose((0.02, 0.01, 0.05), 0.003), True)  # a second pose frame, the search no longer along a row
    p.track(b[0], R.pose((0.1, -0.02, -0.04), -0.002), False)


@pytest.mark.parametrize("D", [5, 7])
def test_exact_shift_scene(pair, D):
    p = pair(R.SCENE_W, R.SCENE_H)
    for k, (img, T) in enumerate(R.shift_scene(D, 1)):
        p.track(img, T, k == 0)
    assert p.ref.counts.get(R.OK, 0) >= 60


def test_slanted_plane_six_frames(pair):
    p = pair(R.SCENE_W, R.SCENE_H)
    for k, (img, T) in enumerate(R.plane_scene(1)):
        o = p.track(img, T, k == 0)
    assert (o["idepth_var"] < 0.01).sum() >= 30


@pytest.mark.parametrize("name", SC.NAMES)
def test_general_motion_scenes(pair, name):
    """The six general-motion scenes (fx != fy, vertical / forward / backward motion, roll, a reference pose that is not the
    identity), six frames each: bit parity where the two image axes and all of R and t matter."""
    p = pair(SC.W, SC.H, K=SC.K)
    for k, (img, T) in enumerate(SC.scene(name, 1)):
        o = p.track(img, T, k == 0)
        assert k == 0 or p.ref.counts.get(R.OK, 0) >= 30
    assert (o["idepth_var"] < 0.01).sum() >= 15


@pytest.mark.parametrize("tx,steps", [(0.1, 140), (1.0, 256)])
def test_long_search(pair, tx, steps):
    """A prior as wide as the clamp (var 25: xi in [0.01, 10]) makes the search 140 tx x 9.99 px long: 140 steps at tx = 0.1
    (three passes of the 64 lanes, step <= 1 px), the cap of 256 at tx = 1 (five passes, step 5.5 px)."""
    p = pair(R.SCENE_W, R.SCENE_H, var_init=25.0)
    a, _ = R.shift_scene(7, 3)
    p.track(a[0], a[1], True)
    p.track(np.ascontiguousarray(a[0][:, ::-1]), R.pose((tx, 0.004, 0.0)), False)
    live = p.ref.alive > 0
    assert live.sum() >= 60 and (p.ref.steps[live] == steps).all()
    if steps < 256:  # (at the cap the samples are 5.5 px apart: only the first thirty can lie inside a 160 px image)
        assert (p.ref.kstar[live] > 64).any()


def test_edge_image_windows_touch_the_border(pair):
    """Features exactly at the margin m = win / 2 + 1 of all four borders; after a sideways jump the windows of the left ones
    leave the image for every sample (OUTSIDE), the others search along the border rows."""
    W, H, m = R.SCENE_W, R.SCENE_H, 3
    img = np.full((H, W), 100, np.uint8)
    for y in range(8, H - 8, 16):
        img[y, m - 1] = 255          # gradient maximum at (m, y)
        img[y, W - m] = 255          # ... at (W - m - 1, y)
    for x in range(24, W - 24, 16):
        img[m - 1, x] = 255          # (x, m)
        img[H - m, x] = 255          # (x, H - m - 1)
    p = pair(W, H)
    o = p.track(img, R.pose(), True)
    xs, ys = o["vtx"][:, 0], o["vtx"][:, 1]
    assert (xs == m).any() and (xs == W - m - 1).any() and (ys == m).any() and (ys == H - m - 1).any()
    p.track(img, R.pose((2.0, 0.0, 0.0)), False)
    assert p.ref.counts.get(R.OUTSIDE, 0) >= 5 and p.ref.counts.get(R.OUTSIDE, 0) < len(xs)
    p.track(img, R.pose((0.0, 0.3, 0.0)), False)
    p.track(img, R.pose((0.05, 0.0, 1.2)), False)   # the camera moves forward: projections leave the image


def test_constant_image(pair):
    p = pair(R.SCENE_W, R.SCENE_H)
    img = np.full((R.SCENE_H, R.SCENE_W), 77, np.uint8)
    for k in range(2):
        o = p.track(img, R.pose((0.05 * k, 0, 0)), True)
        assert len(o["slot"]) == 0 and p.gpu.info("live") == 0


def test_checkerboard_ties_and_ambiguous_matches(pair):
    """Squares of 4 px: dozens of pixels of a cell tie for the largest gradient; the pattern repeats every 8 px along the
    15 px search, and +-2 grey levels of noise keep the best cost off zero, so the repeats are within a factor 1.5 of it."""
    W, H = R.SCENE_W, R.SCENE_H
    yy, xx = np.mgrid[0:H, 0:W + 8]
    big = (((yy // 4) + (xx // 4)) % 2 * 40 + 100).astype(np.uint8)
    p = pair(W, H)
    a, b = R.shift_scene(5, 0, big=big)
    o = p.track(a[0], a[1], True)
    assert len(o["slot"]) == 80
    noisy = (b[0].astype(int) + np.random.default_rng(3).integers(-2, 3, b[0].shape)).astype(np.uint8)
    p.track(noisy, b[1], False)
    assert p.ref.counts.get(R.AMBIGUOUS, 0) >= 20


def test_colliding_tracks_one_feature_per_cell(pair):
    """The camera backs off: the features' projections shrink towards the centre, several per cell; the smallest variance is
    emitted, ties to the lower slot."""
    p = pair(R.SCENE_W, R.SCENE_H)
    a, b = R.shift_scene(5, 5)
    p.track(a[0], a[1], True)
    p.track(b[0], b[1], False)  # variances now differ
    o = p.track(b[0], R.pose((5 * 2.0 / R.SCENE_F, 0.0, -2.5)), False)
    live = int(p.ref.alive.sum())
    assert 4 <= len(o["slot"]) < live // 2
    o = p.track(b[0], R.pose((5 * 2.0 / R.SCENE_F, 0.0, -2.5)), True)  # a pose frame on top: detections only in the empty cells
    assert (o["status"] == R.NEW).any() and (o["status"] != R.NEW).any()


def test_small_ring_overwrites_kill_features(pair):
    p = pair(R.SCENE_W, R.SCENE_H, max_features=128, max_poseframes=2)
    big = R.upsampled_texture(R.SCENE_H, R.SCENE_W + 16, 9)
    lives = []
    for k, D in enumerate((0, 2, 4, 6)):
        img = np.ascontiguousarray(big[:, D:D + R.SCENE_W])
        p.track(img, R.pose((D * 2.0 / R.SCENE_F, 0.0, 0.0)), True, img_id=100 + k)
        lives.append((p.ref.pf[p.ref.alive > 0] == k % 2).sum())
        assert p.gpu.info("poseframes") == min(k + 1, 2)
    assert lives[0] >= 60 and lives[2] > 0  # frame 2 reuses ring slot 0: its features are all new, the old ones died
    assert (p.ref.status[(p.ref.alive > 0) & (p.ref.pf == 1)] == R.NEW).all()


def test_set_poses_and_prune(pair):
    p = pair(R.SCENE_W, R.SCENE_H, max_poseframes=3)
    fr = R.plane_scene(2)
    p.track(fr[0][0], fr[0][1], True, img_id=10)
    p.track(fr[1][0], fr[1][1], False, img_id=11)
    p.track(fr[2][0], fr[2][1], True, img_id=12)
    moved = [R.pose((0.001, -0.002, 0.0005), 0.0002), R.pose((0.061, 0.0, 0.001), 0.0081)]
    for o in (p.gpu, p.ref):
        o.set_poses([10, 12, 999], moved + [R.pose()])  # an id the ring does not hold is ignored
    p.track(fr[3][0], fr[3][1], False, img_id=13)
    for o in (p.gpu, p.ref):
        o.prune([12, 555])
    p.check_state("after prune")
    assert p.gpu.info("poseframes") == 1 and 0 < p.gpu.info("live") < 80
    p.track(fr[4][0], fr[4][1], False, img_id=14)
    for o in (p.gpu, p.ref):
        o.prune([])
    p.check_state("after prune of everything")
    assert p.gpu.info("live") == 0
    o = p.track(fr[5][0], fr[5][1], False, img_id=15)
    assert len(o["slot"]) == 0


def test_slot_boundaries_and_exhaustion(pair):
    """640x480, 2 048 slots, cells of 12 (2 160 cells): more than one workgroup of features, more than one pass of the
    compaction's 1 024 threads, and more detections than free slots."""
    W, H = 640, 480
    K = np.array([525, 0, 319.5, 0, 525, 239.5, 0, 0, 1], np.float32)
    p = pair(W, H, max_features=2048, max_poseframes=2, K=K, detection_win_size=12)
    big = R.upsampled_texture(H, W + 8, 21)
    o = p.track(np.ascontiguousarray(big[:, :W]), R.pose(), True)
    assert len(o["slot"]) == 2048 and p.ref.dropped > 0
    o = p.track(np.ascontiguousarray(big[:, 6:6 + W]), R.pose((6 * 2.0 / 525, 0.0, 0.0)), False)
    assert p.ref.counts.get(R.OK, 0) >= 1500


def test_argument_errors(gpu):
    from flame_ros_amd import lib
    from flame_ros_amd.frontend import FlameHipError, GpuFrontEnd, default_frontend_params
    img = np.zeros((R.SCENE_H, R.SCENE_W), np.uint8)
    with GpuFrontEnd(R.SCENE_W, R.SCENE_H, R.SCENE_K, 64, 2) as fe:
        for kw, code in ((dict(win_size=4), lib.ERR_ARG), (dict(win_size=11), lib.ERR_ARG), (dict(detection_win_size=0), lib.ERR_ARG),
                         (dict(min_grad_mag=float("nan")), lib.ERR_NAN), (dict(var_init=0.0), lib.ERR_ARG)):
            with pytest.raises(FlameHipError) as e:
                fe.track(default_frontend_params(**kw), img, 0, R.pose(), True)
            assert e.value.code == code, kw
        T = R.pose()
        T[1, 3] = np.inf
        with pytest.raises(FlameHipError) as e:
            fe.track(default_frontend_params(), img, 0, T, True)
        assert e.value.code == lib.ERR_NAN
        assert fe.info("live") == 0
    with pytest.raises(FlameHipError):
        GpuFrontEnd(R.SCENE_W, R.SCENE_H, R.SCENE_K, 64, 65)
