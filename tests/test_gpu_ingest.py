"""GPU: the ingest stage (flame_hip_frontend_set_camera / _track_raw / _rectify / _image, csrc/ingest.hip) against its NumPy
restatement (tests/ingest_ref.py, itself pinned to include/flame_ros/image_io.h and to ground truth by
tests/test_ingest_ref.py): BIT FOR BIT, no tolerance -- the grey and box steps are integers and the remap uses only correctly
rounded float32 operations in one order.  Shapes: 188 x 120 and 157 x 93 (odd width, no multiple of the 64 x 4 pixel workgroup,
several workgroups in both directions), raw sizes that the resize factor does not divide."""
import numpy as np
import pytest

from tests import frontend_ref as R
from tests import frontend_scenes as SC
from tests import ingest_ref as IR
from tests.fe_pair import compare, pair  # noqa: F401  (pair: the fixture)

pytestmark = pytest.mark.gpu


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d pixels differ, first at (y, x) = %s: gpu %d restatement %d" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.fixture
def frontend(gpu):
    from flame_ros_amd.frontend import GpuFrontEnd
    made = []

    def make(W, H, K4, max_features=256, max_poseframes=4):
        made.append(GpuFrontEnd(W, H, IR.K9(K4), max_features, max_poseframes))
        return made[-1]
    yield make
    for fe in made:
        fe.close()


@pytest.mark.parametrize("name", list(IR.CAMERAS))
def test_rectify_three_cameras(frontend, name):
    W, H, K4, D = IR.CAMERAS[name]
    fe = frontend(W, H, K4)
    fe.set_camera(W, H, D)
    for tag, raw in (("noise", IR.noise(H, W, 5)), ("smooth", IR.smooth(H, W))):
        same(fe.rectify(raw), IR.ingest(raw, IR.GRAY8, 1, K4, D), "%s %s" % (name, tag))
        assert fe.info("ingest_raw_bytes") == W * H and fe.info("ingest_device_us") >= 0


def test_odd_pitch_from_an_odd_address(frontend):
    W, H, K4, D = IR.CAMERAS["pincushion"]
    fe = frontend(W, H, K4)
    want = {}
    for fmt, ch in ((IR.GRAY8, 1), (IR.BGR8, 3)):
        raw = IR.noise(H, W, 6 + fmt, ch)
        pitch = W * ch + 11 + (W * ch) % 2  # odd
        assert pitch % 2 == 1
        buf = np.full(H * pitch + 1, 0xAB, np.uint8)
        shape, strides = ((H, W), (pitch, 1)) if ch == 1 else ((H, W, ch), (pitch, ch, 1))
        strided = np.lib.stride_tricks.as_strided(buf[1:], shape, strides)
        strided[...] = raw
        assert strided.ctypes.data % 2 == 1
        fe.set_camera(W, H, D, format=fmt)
        want[fmt] = IR.ingest(raw, fmt, 1, K4, D)
        same(fe.rectify(strided), want[fmt], "format %d on pitch %d" % (fmt, pitch))


@pytest.mark.parametrize("fmt", [IR.GRAY8, IR.BGR8, IR.RGB8, IR.BGRA8, IR.RGBA8])
@pytest.mark.parametrize("name", ["pincushion", "zero"])
def test_every_format(frontend, fmt, name):
    W, H, K4, D = IR.CAMERAS[name]
    fe = frontend(W, H, K4)
    fe.set_camera(W, H, D, format=fmt)
    raw = IR.noise(H, W, 30 + fmt, IR.CHANNELS[fmt])
    same(fe.rectify(raw), IR.ingest(raw, fmt, 1, K4, D), "format %d, camera %s" % (fmt, name))
    assert fe.info("ingest_raw_bytes") == W * H * IR.CHANNELS[fmt]


@pytest.mark.parametrize("f,raw_w,raw_h", [(2, 315, 187), (3, 473, 280)])
@pytest.mark.parametrize("fmt", [IR.GRAY8, IR.RGBA8])
@pytest.mark.parametrize("name", ["pincushion", "zero"])
def test_resize_factors(frontend, f, raw_w, raw_h, fmt, name):
    W, H, K4, D = IR.CAMERAS[name]
    assert (raw_w // f, raw_h // f) == (W, H) and raw_w % f and raw_h % f
    fe = frontend(W, H, K4)
    fe.set_camera(raw_w, raw_h, D, format=fmt, resize_factor=f)
    raw = IR.noise(raw_h, raw_w, 60 + f + fmt, IR.CHANNELS[fmt])
    same(fe.rectify(raw), IR.ingest(raw, fmt, f, K4, D), "f = %d, format %d, camera %s" % (f, fmt, name))


@pytest.mark.parametrize("D", [(1e30, 0, 0, 0, 0), (3e38, 3e38, 0, 0, 0)])
def test_overflowing_positions_give_zero(frontend, D):
    W, H, K4, _ = IR.CAMERAS["pincushion"]
    fe = frontend(W, H, K4)
    fe.set_camera(W, H, D)
    raw = np.full((H, W), 200, np.uint8)
    got = fe.rectify(raw)
    same(got, IR.ingest(raw, IR.GRAY8, 1, K4, D), "D = %s" % (D,))
    assert (got == 0).all()


def test_argument_errors(frontend):
    from flame_ros_amd import lib
    from flame_ros_amd.frontend import FlameHipError, default_frontend_params
    W, H, K4, D = IR.CAMERAS["pincushion"]
    fe = frontend(W, H, K4)
    raw = np.zeros((H, W), np.uint8)
    with pytest.raises(FlameHipError) as e:
        fe.track_raw(default_frontend_params(), raw, 0, R.pose(), True)
    assert e.value.code == lib.ERR_STATE
    for kw, code in ((dict(raw_width=W + 1), lib.ERR_ARG), (dict(resize_factor=9), lib.ERR_ARG), (dict(format=7), lib.ERR_ARG),
                     (dict(D=(0, float("nan"), 0, 0, 0)), lib.ERR_NAN)):
        with pytest.raises(FlameHipError) as e:
            fe.set_camera(**{**dict(raw_width=W, raw_height=H, D=D), **kw})
        assert e.value.code == code, kw
    assert fe.info("camera") == 0 and fe.info("live") == 0


def test_rectify_leaves_state_and_tracking_untouched(pair):
    """A rectify call between two frames: every slot's state is what it was, and the next frame (rectified input, compared
    with the restatement inside Pair.track) is what it would have been."""
    W, H = R.SCENE_W, R.SCENE_H
    p = pair(W, H)
    a, b = R.shift_scene(6, 11)
    p.track(a[0], a[1], True)
    p.gpu.set_camera(W, H, IR.CAMERAS["barrel"][3])
    before = p.gpu.image()
    same(before, a[0], "image() after a track call")
    K4 = (R.SCENE_K[0], R.SCENE_K[4], R.SCENE_K[2], R.SCENE_K[5])
    raw = IR.noise(H, W, 8)
    same(p.gpu.rectify(raw), IR.ingest(raw, IR.GRAY8, 1, K4, IR.CAMERAS["barrel"][3]), "rectify between frames")
    p.check_state("after rectify")
    same(p.gpu.image(), before, "image() after rectify")
    p.track(b[0], b[1], False)
    assert p.ref.counts.get(R.OK, 0) >= 30


TRACK_D = (-0.28, 0.07, 0.0002, 0.00002, 0.0)


def track_raw_frame(p, raw, rect, T, is_pf):
    """Pair.track with the raw image on the GPU side and the restated rectified image on the restatement's side."""
    want = p.ref.track(p.pr, rect, p.frame, T, is_pf)
    got = p.gpu.track_raw(p.pg, raw, p.frame, T, is_pf)
    tag = "frame %d" % p.frame
    compare(tag, got, want)
    p.check_state(tag)
    for st, key in enumerate(("ok", "no_parallax", "outside", "bad_match", "ambiguous", "new", "died")):
        assert p.gpu.info(key) == p.ref.counts.get(st, 0), (tag, key)
    assert p.gpu.info("emitted") == len(want["slot"]) and p.gpu.info("detections_dropped") == p.ref.dropped
    same(p.gpu.image(), rect, tag + " image()")
    assert p.gpu.info("ingest_raw_bytes") == raw.size
    p.frame += 1
    return want


def test_track_raw_six_frames(pair):
    """The six frames of the sideways scene taken as raw (distorted) images of a barrel camera with the scene's K."""
    p = pair(SC.W, SC.H, K=SC.K)
    p.gpu.set_camera(SC.W, SC.H, TRACK_D)
    for k, (raw, T) in enumerate(SC.scene("sideways", 1)):
        rect = IR.ingest(raw, IR.GRAY8, 1, SC.K4, TRACK_D)
        assert (rect != raw).mean() > 0.3
        track_raw_frame(p, raw, rect, T, k == 0)
    assert p.ref.counts.get(R.OK, 0) >= 30  # (not vacuous: the restatement alone tracks the rectified frames)


def test_track_raw_colour_resized_poseframes(pair):
    """BGR8 at resize factor 2 through track_raw, every other frame a pose frame (the stage writes into ring slots and into the
    extra slot), on a ring of two."""
    W, H = SC.W, SC.H
    p = pair(W, H, K=SC.K, max_poseframes=2)
    p.gpu.set_camera(2 * W + 1, 2 * H + 1, TRACK_D, format=IR.BGR8, resize_factor=2)
    for k, (img, T) in enumerate(SC.scene("sideways", 1)):
        big = np.zeros((2 * H + 1, 2 * W + 1, 3), np.uint8)
        big[:2 * H, :2 * W] = np.repeat(np.repeat(img, 2, axis=0), 2, axis=1)[..., None]
        big[..., 0] //= 2  # (the channels differ, so their order matters)
        rect = IR.ingest(big, IR.BGR8, 2, SC.K4, TRACK_D)
        track_raw_frame(p, big, rect, T, k % 2 == 0)


def test_set_camera_none_restores_the_rectified_path(pair):
    from flame_ros_amd import lib
    from flame_ros_amd.frontend import FlameHipError
    p = pair(SC.W, SC.H, K=SC.K)
    frames = SC.scene("sideways", 1)
    p.gpu.set_camera(SC.W, SC.H, TRACK_D)
    raw, T = frames[0]
    track_raw_frame(p, raw, IR.ingest(raw, IR.GRAY8, 1, SC.K4, TRACK_D), T, True)
    p.gpu.set_camera(None)
    assert p.gpu.info("camera") == 0
    with pytest.raises(FlameHipError) as e:
        p.gpu.track_raw(p.pg, raw, 1, T, False)
    assert e.value.code == lib.ERR_STATE
    p.check_state("after the refused call")
    # the rectified path again: the image goes in as it is (Pair.track compares with the restatement)
    rect = IR.ingest(frames[1][0], IR.GRAY8, 1, SC.K4, TRACK_D)
    p.track(rect, frames[1][1], False)
    same(p.gpu.image(), rect, "image() on the rectified path")
    assert p.gpu.info("ingest_raw_bytes") == 0 and p.gpu.info("ingest_device_us") == 0
