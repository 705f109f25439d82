"""GPU: the front end's search record and its two debug images (flame_hip_frontend_searches / _debug_image,
csrc/frontend_debug.hip) against the restatement tests/fe_debug_ref.py (pinned by tests/test_fe_debug_ref.py): after EVERY frame
`seg` (as uint32), `steps` and both pictures, byte for byte -- the pictures are integers and the sample positions the tracker's
own float32 expression, so there is no tolerance.  The situations are the ones tests/test_gpu_frontend.py builds, at the smallest
shapes at which the kernels can still go wrong."""
import numpy as np
import pytest

from tests import fe_debug_ref as D
from tests import frontend_ref as R
from tests import frontend_scenes as SC
from tests import ingest_ref as IR
from tests.fe_pair import pair  # noqa: F401  (pair: the fixture)

pytestmark = pytest.mark.gpu


def count(im, colour):
    return int((im == np.array(colour, np.uint8)).all(axis=2).sum())


def test_odd_width_odd_pitches(pair):
    """157x93, input rows 173 bytes apart from an odd address; the picture asked for with rows 3 W + 5 bytes apart."""
    W, H = 157, 93
    p = pair(W, H, pitch=173, out_pitch=3 * W + 5)
    a, b = R.shift_scene(6, 11, W=W, H=H)
    p.track(a[0], a[1], True)
    p.track(b[0], b[1], False)
    assert p.ref.counts.get(R.OK, 0) >= 30
    p.track(a[0], R.pose((0.02, 0.01, 0.05), 0.003), True)
    p.track(b[0], R.pose((0.1, -0.02, -0.04), -0.002), False)


def test_sideways_ten_frames_all_layers(pair):
    p = pair(SC.W, SC.H, K=SC.K)
    seen = set()
    for k, (img, T) in enumerate(SC.scene("sideways", 1, frames=10)):
        p.track(img, T, k == 0)
        seen |= set(int(s) for s in p.ref.status[p.ref.steps > 0])
    assert {R.OK, R.BAD_MATCH, R.OUTSIDE, R.DIED} <= seen
    m = p.ref.debug_image(D.IMG_MATCHES)
    assert count(m, D.GREEN) >= 150 and count(m, D.RED) >= 10 and count(m, D.YELLOW) >= 40


def test_diagonal_roll(pair):
    """Segments that are neither axis-aligned nor x-dominant."""
    p = pair(SC.W, SC.H, K=SC.K)
    for k, (img, T) in enumerate(SC.scene("diagonal_roll", 1)):
        p.track(img, T, k == 0)
    ran = p.ref.steps > 0
    ex, ey = np.abs(p.ref.seg[ran, 2]), np.abs(p.ref.seg[ran, 3])
    assert ran.sum() >= 30 and ((ey > ex) & (ex > 0.05)).sum() >= 10


@pytest.mark.parametrize("tx,steps", [(0.1, 140), (1.0, 256)])
def test_long_search(pair, tx, steps):
    """var_init = 25: 140 steps (three passes of the lanes) at tx = 0.1, the cap of 256 (five passes, samples 5.5 px apart and
    mostly outside the image: a dotted line) at tx = 1."""
    p = pair(R.SCENE_W, R.SCENE_H, var_init=25.0)
    a, _ = R.shift_scene(7, 3)
    p.track(a[0], a[1], True)
    p.track(np.ascontiguousarray(a[0][:, ::-1]), R.pose((tx, 0.004, 0.0)), False)
    live = p.ref.alive > 0
    assert live.sum() >= 60 and (p.ref.steps[live] == steps).all()


def test_border_features_and_searches_outside_the_image(pair):
    W, H, m = R.SCENE_W, R.SCENE_H, 3
    img = np.full((H, W), 100, np.uint8)
    for y in range(8, H - 8, 16):
        img[y, m - 1] = 255
        img[y, W - m] = 255
    for x in range(24, W - 24, 16):
        img[m - 1, x] = 255
        img[H - m, x] = 255
    p = pair(W, H)
    o = p.track(img, R.pose(), True)
    xs, ys = o["vtx"][:, 0], o["vtx"][:, 1]
    assert (xs == m).any() and (xs == W - m - 1).any() and (ys == m).any() and (ys == H - m - 1).any()  # squares touch the border
    p.track(img, R.pose((2.0, 0.0, 0.0)), False)
    outside = (p.ref.status == R.OUTSIDE) & (p.ref.steps > 0)
    assert outside.sum() >= 5  # searched, every sample outside
    p.track(img, R.pose((0.0, 0.3, 0.0)), False)
    p.track(img, R.pose((0.05, 0.0, 1.2)), False)


def test_small_ring_slots_die_and_are_detected_again_in_one_frame(pair):
    p = pair(R.SCENE_W, R.SCENE_H, max_features=128, max_poseframes=2)
    big = R.upsampled_texture(R.SCENE_H, R.SCENE_W + 16, 9)
    reused = 0
    for k, D_ in enumerate((0, 2, 4, 6)):
        before = p.ref.alive.copy()
        img = np.ascontiguousarray(big[:, D_:D_ + R.SCENE_W])
        p.track(img, R.pose((D_ * 2.0 / R.SCENE_F, 0.0, 0.0)), True, img_id=100 + k)
        reused += int(((before > 0) & (p.ref.status == R.NEW)).sum())
    assert reused > 0 and not p.ref.steps[p.ref.status == R.NEW].any()


def test_prune_without_a_new_frame_leaves_the_pictures(pair):
    p = pair(R.SCENE_W, R.SCENE_H, max_poseframes=3)
    fr = R.plane_scene(2)
    p.track(fr[0][0], fr[0][1], True, img_id=10)
    p.track(fr[1][0], fr[1][1], False, img_id=11)
    p.track(fr[2][0], fr[2][1], True, img_id=12)
    before = p.check("before prune")
    live = p.gpu.info("live")
    p.gpu.set_poses([10], [R.pose((0.001, -0.002, 0.0005), 0.0002)])
    p.gpu.prune([12])
    assert 0 < p.gpu.info("live") < live
    after = p.check("after prune")  # (the restatement was not pruned: the picture is the tracked frame's)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    assert count(after["matches"], D.GREEN) > 0


def test_many_workgroups_of_detections(pair):
    """640x480, 2 048 slots, cells of 12: the pose frame only."""
    W, H = 640, 480
    K = np.array([525, 0, 319.5, 0, 525, 239.5, 0, 0, 1], np.float32)
    p = pair(W, H, max_features=2048, max_poseframes=2, K=K, detection_win_size=12)
    big = R.upsampled_texture(H, W + 8, 21)
    o = p.track(np.ascontiguousarray(big[:, :W]), R.pose(), True)
    assert len(o["slot"]) == 2048
    assert count(p.ref.debug_image(D.IMG_DETECTIONS), D.GREEN) > 9 * 1500


def test_background_is_the_ingest_stages_output(pair):
    """track_raw, BGR8 at resize factor 2."""
    W, H = SC.W, SC.H
    Dc = (-0.28, 0.07, 0.0002, 0.00002, 0.0)
    p = pair(W, H, K=SC.K, max_poseframes=2)
    p.gpu.set_camera(2 * W + 1, 2 * H + 1, Dc, format=IR.BGR8, resize_factor=2)
    for k, (img, T) in enumerate(SC.scene("sideways", 1)[:3]):
        big = np.zeros((2 * H + 1, 2 * W + 1, 3), np.uint8)
        big[:2 * H, :2 * W] = np.repeat(np.repeat(img, 2, axis=0), 2, axis=1)[..., None]
        big[..., 0] //= 2
        rect = IR.ingest(big, IR.BGR8, 2, SC.K4, Dc)
        assert (rect != img).mean() > 0.3
        p.track(rect, T, k == 0, raw=big)
        assert np.array_equal(p.gpu.image(), rect)


def test_errors(gpu):
    from flame_ros_amd import lib
    from flame_ros_amd.frontend import IMG_MATCHES, FlameHipError, GpuFrontEnd, default_frontend_params
    W, H = R.SCENE_W, R.SCENE_H
    with GpuFrontEnd(W, H, R.SCENE_K, 64, 2) as fe:
        for call in (lambda: fe.debug_image(IMG_MATCHES), fe.searches):  # a fresh handle
            with pytest.raises(FlameHipError) as e:
                call()
            assert e.value.code == lib.ERR_STATE
        fe.track(default_frontend_params(), np.zeros((H, W), np.uint8), 0, R.pose(), True)
        for kw in (dict(kind=IMG_MATCHES, pitch=3 * W - 1), dict(kind=2), dict(kind=-1)):
            with pytest.raises(FlameHipError) as e:
                fe.debug_image(**kw)
            assert e.value.code == lib.ERR_ARG, kw
        assert not fe.debug_image(IMG_MATCHES).any()  # a black frame, nothing tracked


def test_slot_dies_of_its_search_and_is_taken_by_a_detection_in_the_same_frame(pair):
    """max_dropouts = 0 on a pose frame: a feature whose search fails dies in the tracker (its record holds that search) and the
    detection of the same frame takes its slot -- the record of a NEW slot is zero again and the slot draws nothing."""
    W, H, m = R.SCENE_W, R.SCENE_H, 3
    img = np.full((H, W), 100, np.uint8)
    for y in range(8, H - 8, 16):
        img[y, m - 1] = 255
        img[y, W - m] = 255
    p = pair(W, H, max_dropouts=0)
    p.track(img, R.pose(), True)
    before = p.ref.alive.copy()
    p.track(img, R.pose((2.0, 0.0, 0.0)), True)
    assert p.ref.counts.get(R.DIED, 0) >= 5
    retaken = (before > 0) & (p.ref.status == R.NEW)
    assert retaken.sum() >= 5 and not p.ref.steps[retaken].any()
