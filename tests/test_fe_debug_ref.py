"""CPU: the restatement of the front end's debug images (tests/fe_debug_ref.py), so that "GPU equals restatement"
(tests/test_gpu_fe_debug.py) is not circular: the two drawing functions on hand-built records against bytes written out by
hand, the recomputed search record against the base restatement, non-vacuity on the ten-frame scene, and the ABI surface on a
handle without a device."""
import ctypes as C

import numpy as np
import pytest

from flame_ros_amd import lib
from tests import fe_debug_ref as D
from tests import frontend_ref as R
from tests import frontend_scenes as SC

COLOURS = {"G": D.GREEN, "R": D.RED, "Y": D.YELLOW, "B": D.BLUE}


def grey(W, H):
    return ((np.arange(W * H).reshape(H, W) * 7 + 3) % 251).astype(np.uint8)


def picture(img, rows):
    """The expected bytes, written as one character per pixel: '.' = the grey background, G R Y B = the layer colours."""
    assert len(rows) == img.shape[0] and all(len(r) == img.shape[1] for r in rows)
    out = np.zeros(img.shape + (3,), np.uint8)
    for y, row in enumerate(rows):
        for x, ch in enumerate(row):
            out[y, x] = (img[y, x],) * 3 if ch == "." else COLOURS[ch]
    return out


def record(n):
    return np.full(n, R.FREE, np.int32), np.full(n, -1, np.int32), np.zeros((n, 4), np.float32), np.zeros(n, np.int32)


# ---- 1. the drawing functions, by hand ----

def test_background_is_the_grey_image_in_all_three_channels():
    img = grey(8, 5)
    st, ks, seg, steps = record(3)
    got = D.draw_matches(img, st, ks, seg, steps)
    assert got.dtype == np.uint8 and got.shape == (5, 8, 3)
    for c in range(3):
        assert np.array_equal(got[:, :, c], img)
    assert np.array_equal(D.draw_detections(img, np.zeros((0, 2), np.float32), np.zeros(0, np.int32)), got)


def test_one_horizontal_ok_segment():
    img = grey(8, 5)
    st, ks, seg, steps = record(2)
    st[1], ks[1], seg[1], steps[1] = R.OK, 2, (1.0, 2.0, 1.0, 0.0), 4  # samples at x = 1 .. 5 of row 2, the best one at x = 3
    want = picture(img, ["........",
                         "........",
                         ".GGYGG..",
                         "........",
                         "........"])
    assert np.array_equal(D.draw_matches(img, st, ks, seg, steps), want)


def test_failed_segments_cross_an_ok_one_red_over_green_yellow_over_both():
    img = grey(8, 5)
    st, ks, seg, steps = record(4)
    st[0], ks[0], seg[0], steps[0] = R.BAD_MATCH, 1, (3.0, 0.0, 0.0, 1.0), 4   # column 3, through the OK slot's best sample
    st[1], ks[1], seg[1], steps[1] = R.OK, 2, (1.0, 2.0, 1.0, 0.0), 4
    st[2], ks[2], seg[2], steps[2] = R.AMBIGUOUS, 0, (5.0, 1.0, 0.0, 1.0), 2   # column 5, rows 1 .. 3, through a green pixel
    st[3], ks[3], seg[3], steps[3] = R.DIED, -1, (7.0, 3.0, 0.0, 1.0), 1       # a slot that died draws its last search
    want = picture(img, ["...R....",
                         "...R.R..",
                         ".GGYGR..",
                         "...R.R.R",
                         "...R...R"])
    got = D.draw_matches(img, st, ks, seg, steps)
    assert np.array_equal(got, want)
    for order in ([3, 2, 1, 0], [1, 0, 3, 2]):  # the order of the slots does not matter
        assert np.array_equal(D.draw_matches(img, st[order], ks[order], seg[order], steps[order]), want)
    st[3] = R.OUTSIDE
    assert np.array_equal(D.draw_matches(img, st, ks, seg, steps), want)


def test_clipping_tests_the_float_position():
    """Samples at x = -1.5, -0.5, 0.5, ..., 8.5 of an 8 pixel wide image: -0.5 rounds to pixel 0 and is drawn, W - 0.5 = 7.5 rounds
    to pixel 8 and is not; the best sample (k* = 0) lies outside and leaves no marker.  The same for rows, on the diagonal."""
    img = grey(8, 5)
    st, ks, seg, steps = record(1)
    st[0], ks[0], seg[0], steps[0] = R.OK, 0, (-1.5, 1.0, 1.0, 0.0), 10
    want = picture(img, ["........",
                         "GGGGGGGG",
                         "........",
                         "........",
                         "........"])
    assert np.array_equal(D.draw_matches(img, st, ks, seg, steps), want)
    # y = -1.5, -0.5, ..., 5.5 with x = y + 2: rows -1 .. 5 round to pixels -1 (out), 0 .. 4, 5 and 6 (out)
    st[0], ks[0], seg[0], steps[0] = R.BAD_MATCH, 3, (0.5, -1.5, 1.0, 1.0), 7
    want = picture(img, ["..R.....",
                         "...R....",
                         "....R...",
                         ".....R..",
                         "......R."])
    assert np.array_equal(D.draw_matches(img, st, ks, seg, steps), want)


def test_non_finite_positions_draw_nothing():
    img = grey(8, 5)
    st, ks, seg, steps = record(4)
    st[:] = R.OK
    ks[:] = 1
    seg[0], steps[0] = (np.nan, 1.0, 1.0, 0.0), 3
    seg[1], steps[1] = (0.0, 0.0, np.inf, 0.0), 2          # 0 x inf = NaN at k = 0, inf after it
    seg[2], steps[2] = (1.0, -np.inf, 0.0, 0.0), 2
    seg[3], steps[3] = (2.0, 3.0, 3e38, 0.0), 2            # sample 0 is drawn, 1 is far outside, 2 overflows to inf
    want = picture(img, ["........",
                         "........",
                         "........",
                         "..G.....",
                         "........"])
    assert np.array_equal(D.draw_matches(img, st, ks, seg, steps), want)


def test_slots_that_do_not_draw():
    img = grey(8, 5)
    st, ks, seg, steps = record(5)
    seg[:] = (1.0, 2.0, 1.0, 0.0)
    ks[:] = 1
    st[0], steps[0] = R.OK, 0            # steps = 0 with a drawing status
    st[1], steps[1] = R.OUTSIDE, 0
    st[2], steps[2] = R.NEW, 4           # steps > 0 with a status that does not draw
    st[3], steps[3] = R.NO_PARALLAX, 4
    st[4], steps[4] = R.FREE, 4
    assert np.array_equal(D.draw_matches(img, st, ks, seg, steps), D.background(img))


def test_detection_squares_clip_at_the_corners_and_new_lies_over_tracked():
    img = grey(8, 6)
    vtx = np.array([[0, 0], [7, 0], [0, 5], [6.6, 4.5], [3, 2], [4.4, 2.6]], np.float32)  # (6.6, 4.5) rounds to the corner (7, 5)
    st = np.array([R.NEW, R.OK, R.AMBIGUOUS, R.NEW, R.NO_PARALLAX, R.NEW], np.int32)
    want = picture(img, ["GG....BB",
                         "GGBBB.BB",
                         "..BGGG..",
                         "..BGGG..",
                         "BB.GGGGG",
                         "BB....GG"])
    assert np.array_equal(D.draw_detections(img, vtx, st), want)
    order = [5, 4, 3, 2, 1, 0]
    assert np.array_equal(D.draw_detections(img, vtx[order], st[order]), want)
    assert np.array_equal(D.draw_detections(img, np.array([[np.nan, 2.0], [30.0, 2.0]], np.float32), st[:2]), D.background(img))


# ---- 2. the record of the subclass against the base restatement; non-vacuity on the ten-frame scene ----

@pytest.fixture(scope="module")
def ten_frames():
    """frontend_scenes "sideways", ten frames, frame 0 the only pose frame, 256 slots, default parameters: per frame the emitted
    list, the state, the record and both pictures (computed once, read-only)."""
    ref = R.FrontEndRef(SC.W, SC.H, SC.K, 256, 4)
    base = R.FrontEndRef(SC.W, SC.H, SC.K, 256, 4)
    p, out = R.params(), []
    for k, (img, T) in enumerate(SC.scene("sideways", 1, frames=10)):
        o = ref.track(p, img, k, T, k == 0)
        ob = base.track(p, img, k, T, k == 0)
        assert all(np.array_equal(o[key], ob[key]) for key in ob)  # (the subclass changes nothing the base class computes)
        assert all(np.array_equal(a, b) for a, b in zip(ref.state().values(), base.state().values()))
        out.append(dict(img=img, out=o, state=ref.state(), pstar=ref.pstar.copy(), base_steps=base.steps.copy(), **ref.searches(),
                        matches=ref.debug_image(D.IMG_MATCHES), detections=ref.debug_image(D.IMG_DETECTIONS)))
    return out


def test_recomputed_record_is_consistent_with_the_base_class(ten_frames):
    n_ok = 0
    for k, fr in enumerate(ten_frames):
        st, ks, seg, steps = fr["state"]["status"], fr["state"]["kstar"], fr["seg"], fr["steps"]
        ran = steps > 0
        assert np.array_equal(steps[ran], fr["base_steps"][ran])
        assert not seg[~ran].any() and not ran[(st == R.FREE) | (st == R.NO_PARALLAX) | (st == R.NEW)].any()
        for s in np.flatnonzero(st == R.OK):
            assert ran[s] and 0 <= ks[s] <= steps[s]
            x0, y0, ex, ey = seg[s]
            at = np.array([x0 + np.float32(ks[s]) * ex, y0 + np.float32(ks[s]) * ey])
            # the matched position is sample k* moved by the sub-sample offset, |delta| <= 1/2 step (and a step is <= 1 px here)
            assert np.hypot(*(at - fr["pstar"][s])) <= np.hypot(ex, ey) <= 1.0 + 1e-6, (k, s)
            n_ok += 1
    assert n_ok >= 500


def count(im, colour):
    return int((im == np.array(colour, np.uint8)).all(axis=2).sum())


def test_ten_frame_scene_is_not_vacuous(ten_frames):
    f0, f8 = ten_frames[0], ten_frames[8]
    assert np.array_equal(f0["matches"], D.background(f0["img"]))  # the pose frame searched nothing
    n_new = int((f0["out"]["status"] == R.NEW).sum())
    assert n_new >= 60 and n_new == len(f0["out"]["status"])
    g = count(f0["detections"], D.GREEN)
    v = f0["out"]["vtx"]
    apart = all(max(abs(v[i, 0] - v[j, 0]), abs(v[i, 1] - v[j, 1])) >= 3 for i in range(len(v)) for j in range(i))
    inside = (v[:, 0] >= 1).all() and (v[:, 0] <= SC.W - 2).all() and (v[:, 1] >= 1).all() and (v[:, 1] <= SC.H - 2).all()
    assert g == 9 * n_new if (apart and inside) else 0 < g <= 9 * n_new
    assert count(f0["detections"], D.BLUE) == 0
    # frame 8: all three layers of Matches (the grey scene holds no saturated colour), tracked squares only in Detections
    assert count(D.background(f8["img"]), D.GREEN) == count(D.background(f8["img"]), D.RED) == 0
    assert count(f8["matches"], D.GREEN) >= 150 and count(f8["matches"], D.RED) >= 10 and 40 <= count(f8["matches"], D.YELLOW) <= 80
    assert count(f8["detections"], D.GREEN) == 0 and count(f8["detections"], D.BLUE) >= 9 * 30
    seen = set()
    for fr in ten_frames[7:]:
        seen |= set(int(s) for s in fr["state"]["status"][fr["steps"] > 0])
    assert {R.OK, R.BAD_MATCH, R.OUTSIDE, R.DIED} <= seen
    gated = [int((fr["out"]["idepth_var"] < 0.01).sum()) for fr in ten_frames]
    assert gated[:4] == [0, 0, 0, 0] and min(gated[4:]) >= 51


# ---- 3. the ABI surface, on a handle without a device ----

def test_abi_surface_without_a_device():
    L = lib.load()
    assert hasattr(L, "flame_hip_frontend_searches") and hasattr(L, "flame_hip_frontend_debug_image")
    assert L.flame_hip_version() >= 407
    from flame_ros_amd import frontend as FE
    assert (FE.IMG_DETECTIONS, FE.IMG_MATCHES) == (0, 1)
    assert callable(FE.GpuFrontEnd.debug_image) and callable(FE.GpuFrontEnd.searches)
    W, H = 40, 24
    K = np.array([50, 0, 20, 0, 50, 12, 0, 0, 1], np.float32)
    h = C.c_void_p()
    assert L.flame_hip_frontend_create(C.byref(h), -1, W, H, K.ctypes.data_as(C.c_void_p), 64, 2) == 0
    try:
        buf = np.zeros(H * (3 * W + 8), np.uint8)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        image = L.flame_hip_frontend_debug_image
        assert image(None, 0, vp(buf), 3 * W) == lib.ERR_ARG
        assert image(h, 0, None, 3 * W) == lib.ERR_ARG
        for kind in (-1, 2, 7):
            assert image(h, kind, vp(buf), 3 * W) == lib.ERR_ARG
        for kind in (0, 1):
            assert image(h, kind, vp(buf), 3 * W - 1) == lib.ERR_ARG
            assert image(h, kind, vp(buf), 0) == lib.ERR_ARG
            assert image(h, kind, vp(buf), 3 * W) == lib.ERR_NODEVICE
            assert image(h, kind, vp(buf), 3 * W + 8) == lib.ERR_NODEVICE
        assert not buf.any()
        seg, steps = np.zeros((64, 4), np.float32), np.zeros(64, np.int32)
        assert L.flame_hip_frontend_searches(None, vp(seg), vp(steps)) == lib.ERR_ARG
        assert L.flame_hip_frontend_searches(h, vp(seg), vp(steps)) == lib.ERR_NODEVICE
        assert L.flame_hip_frontend_searches(h, None, None) == lib.ERR_NODEVICE
    finally:
        L.flame_hip_frontend_destroy(h)
    with FE.GpuFrontEnd(W, H, K, 64, 2, device=-1) as fe:
        for call in (lambda: fe.debug_image(FE.IMG_MATCHES), fe.searches):
            with pytest.raises(FE.FlameHipError) as e:
                call()
            assert e.value.code == lib.ERR_NODEVICE
        with pytest.raises(FE.FlameHipError) as e:
            fe.debug_image(5)
        assert e.value.code == lib.ERR_ARG
