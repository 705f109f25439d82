"""CPU: the ingest stage's NumPy restatement (tests/ingest_ref.py) pinned from three sides, so that the GPU tests' "equals
the restatement bit for bit" is not circular:
  1. it equals include/flame_ros/image_io.h (toGray8, undistort<uint8_t>; tests/cpp/ingest_header.cc, g++ -O2
     -ffp-contract=off) bit for bit, on noise and on a smooth image, for the three cameras;
  2. ground truth: the rectified image of round(g), g(x, y) = 127.5 + 100 sin(2 pi x / 97) cos(2 pi y / 71), against g at the
     float64 source position.  The bound |out - g| <= 1.2 is derived: 0.5 input rounding (the convex bilinear weights cannot
     grow it) + 0.5 output rounding + (max|g_xx| + max|g_yy|) / 8 = 0.15 bilinear error + 0.05 for the float32 source
     position (<= 2.4e-5 px against a gradient <= 8.9 grey levels per px).  It applies to every pixel whose float64 source
     lies in [0, W - 1] x [0, H - 1];
  3. the two added rules (all-zero D, range) and the formats / resize factors, one test each;
  4. the ABI surface on a handle without a device."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from flame_ros_amd import lib
from tests import ingest_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1.2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ingest") / "ingest_header")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "ingest_header.cc"), "-o", out])
    return out


def header(exe, tmp_path, mode, img, K4=(1, 1, 0, 0), D=(0, 0, 0, 0, 0)):
    img = np.ascontiguousarray(img)
    H, W = img.shape[:2]
    ch = img.shape[2] if img.ndim == 3 else 1
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<4i", mode, W, H, ch))
        f.write(np.array(list(K4) + list(D), np.float32).tobytes())
        f.write(img.tobytes())
    p = subprocess.run([exe, inp, outp], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr)
    return np.fromfile(outp, np.uint8).reshape(H, W)


# ---- 1. the restatement equals the header ----

@pytest.mark.parametrize("image", ["noise", "smooth"])
@pytest.mark.parametrize("name", list(IR.CAMERAS))
def test_remap_equals_the_header(exe, tmp_path, name, image):
    W, H, K4, D = IR.CAMERAS[name]
    img = IR.noise(H, W, 11) if image == "noise" else IR.smooth(H, W)
    got, want = IR.remap(img, K4, D), header(exe, tmp_path, 1, img, K4, D)
    assert int((got != want).sum()) == 0
    if name != "zero":
        assert (got != img).mean() > 0.5  # the distortion really moved pixels


@pytest.mark.parametrize("fmt", [IR.GRAY8, IR.BGR8, IR.RGB8, IR.BGRA8, IR.RGBA8])
def test_each_format_agrees_with_toGray8(exe, tmp_path, fmt):
    ch = IR.CHANNELS[fmt]
    raw = IR.noise(37, 53, 20 + fmt, ch)
    if fmt == IR.GRAY8:
        as_rgb = raw
    else:  # the header reads R, G, B[, A]
        ri, gi, bi = IR.RGB_AT[fmt]
        as_rgb = np.stack([raw[..., ri], raw[..., gi], raw[..., bi]] + ([raw[..., 3]] if ch == 4 else []), -1)
    assert np.array_equal(IR.grey(raw, fmt), header(exe, tmp_path, 0, as_rgb))
    if ch >= 3:  # the channel order matters, alpha does not
        assert not np.array_equal(IR.grey(raw, fmt), IR.grey(raw, {IR.BGR8: IR.RGB8, IR.RGB8: IR.BGR8, IR.BGRA8: IR.RGBA8, IR.RGBA8: IR.BGRA8}[fmt]))
    if ch == 4:
        other = raw.copy()
        other[..., 3] ^= 0xFF
        assert np.array_equal(IR.grey(raw, fmt), IR.grey(other, fmt))


# ---- 2. ground truth ----

@pytest.mark.parametrize("name", ["barrel", "pincushion"])
def test_ground_truth(name):
    W, H, K4, D = IR.CAMERAS[name]
    out = IR.remap(IR.smooth(H, W), K4, D).astype(np.float64)
    su, sv = IR.source_position_f64(W, H, K4, D)
    inside = (su >= 0) & (su <= W - 1) & (sv >= 0) & (sv <= H - 1)
    err = np.abs(out - IR.wave(su, sv))[inside]
    su32, sv32 = IR.source_position(W, H, K4, D)
    pos_err = max(np.abs(su32 - su)[inside].max(), np.abs(sv32 - sv)[inside].max())
    print("%s: worst |out - g| %.3f over %d of %d pixels (%.1f %%), float32 source position off by <= %.2e px"
          % (name, err.max(), inside.sum(), W * H, 100.0 * inside.mean(), pos_err))
    assert inside.sum() > W * H // 2  # (not vacuous)
    assert pos_err <= 2.4e-5 * 2  # what the bound's 0.05 term assumes, with room: 8.9 grey levels per px x 4.8e-5 px << 0.05
    assert err.max() <= BOUND


# ---- 3. the rules ----

def test_zero_D_is_the_identity_on_noise():
    W, H, K4, D = IR.CAMERAS["zero"]
    img = IR.noise(H, W, 3)
    assert np.array_equal(IR.remap(img, K4, D), img)
    assert np.array_equal(IR.ingest(img, IR.GRAY8, 1, K4, D), img)
    # a single non-zero coefficient, however small, takes the remap (which blurs noise)
    assert not np.array_equal(IR.remap(img, K4, (1e-3, 0, 0, 0, 0)), img)


def test_zero_border():
    W, H, K4, D = IR.CAMERAS["pincushion"]
    img = np.full((H, W), 255, np.uint8)
    out = IR.remap(img, K4, D)
    su, sv = IR.source_position(W, H, K4, D)
    full = (su >= 0) & (su <= F32(W - 1)) & (sv >= 0) & (sv <= F32(H - 1))  # every tap inside the image
    su64, sv64 = IR.source_position_f64(W, H, K4, D)
    assert np.array_equal(full, (su64 >= 0) & (su64 <= W - 1) & (sv64 >= 0) & (sv64 <= H - 1))
    print("pincushion: %d pixels with outside sources" % (~full).sum())
    assert (~full).sum() == 1966
    assert (out[full] == 255).all()
    # beyond the one-pixel rim around the image the output is 0; inside the rim the zero border is blended in
    beyond = ~IR.in_range(su, sv, W, H)
    rim = ~full & ~beyond
    assert beyond.sum() > 1000 and (out[beyond] == 0).all()
    assert rim.sum() > 50 and (out[rim] < 255).all()


F32 = np.float32


def test_overflowing_positions_give_zero():
    """k1 = 1e30: every source position is finite but far beyond what an int holds (|su| >= 6e24 * fx); the range test runs in
    float, so none of them reaches the cast.  A second D makes infinite and NaN positions as well."""
    W, H, K4, _ = IR.CAMERAS["pincushion"]
    img = np.full((H, W), 200, np.uint8)
    for D, want_nonfinite in (((1e30, 0, 0, 0, 0), False), ((3e38, 3e38, 0, 0, 0), True)):
        out = IR.remap(img, K4, D)
        su, sv = IR.source_position(W, H, K4, D)
        finite = np.isfinite(su) & np.isfinite(sv)
        with np.errstate(all="ignore"):
            overflowing = ~finite | (np.abs(su) >= F32(2.0 ** 31)) | (np.abs(sv) >= F32(2.0 ** 31))
        assert overflowing.all() and (~finite).any() == want_nonfinite
        assert (out[overflowing] == 0).all()  # 0 at every overflowing pixel ...
        assert (out == 0).all()                # ... and the value at none


def test_nan_in_D_is_refused():
    W, H, K4, _ = IR.CAMERAS["zero"]
    for D in ((float("nan"), 0, 0, 0, 0), (0, 0, 0, float("inf"), 0), (0, 0, 0, 0, 1e39)):  # (1e39 is infinite in float32)
        with pytest.raises(ValueError):
            IR.remap(np.zeros((H, W), np.uint8), K4, D)


@pytest.mark.parametrize("f,raw_w,raw_h", [(2, 315, 187), (3, 473, 280)])
def test_resize_from_sizes_that_do_not_divide(f, raw_w, raw_h):
    raw = IR.noise(raw_h, raw_w, 40 + f)
    out = IR.box(raw, f)
    assert out.shape == (93, 157)
    # independently: the mean of the block rounded half up, in exact integers
    want = np.zeros((93, 157), np.int64)
    for dy in range(f):
        for dx in range(f):
            want += raw[dy:93 * f:f, dx:157 * f:f]
    assert np.array_equal(out, (2 * want + f * f) // (2 * f * f))
    if f == 2:  # = the bilinear value at the block centre, rounded half up
        r = raw.astype(np.float64)
        centre = 0.25 * (r[0:186:2, 0:314:2] + r[0:186:2, 1:314:2] + r[1:186:2, 0:314:2] + r[1:186:2, 1:314:2])
        assert np.array_equal(out, np.floor(centre + 0.5).astype(np.uint8))
    # trailing raw rows and columns are ignored
    other = raw.copy()
    other[93 * f:, :] ^= 0xFF
    other[:, 157 * f:] ^= 0xFF
    assert np.array_equal(IR.box(other, f), out)
    # the whole stage on a colour image: grey first, then the box, then the remap with the OUTPUT image's K
    W, H, K4, D = IR.CAMERAS["pincushion"]
    rgb = IR.noise(raw_h, raw_w, 50 + f, 3)
    assert np.array_equal(IR.ingest(rgb, IR.RGB8, f, K4, D), IR.remap(IR.box(IR.grey(rgb, IR.RGB8), f), K4, D))


# ---- 4. the ABI surface, on a handle without a device ----

def test_abi_surface_without_a_device():
    L = lib.load()
    for name in ("flame_hip_frontend_set_camera", "flame_hip_frontend_track_raw", "flame_hip_frontend_rectify", "flame_hip_frontend_image"):
        assert hasattr(L, name)
    assert L.flame_hip_version() >= 406
    from flame_ros_amd.frontend import Camera, default_frontend_params
    W, H, K4, D = IR.CAMERAS["pincushion"]
    h = C.c_void_p()
    K = IR.K9(K4)
    assert L.flame_hip_frontend_create(C.byref(h), -1, W, H, K.ctypes.data_as(C.c_void_p), 64, 2) == 0
    try:
        def cam(raw_w=W, raw_h=H, fmt=IR.GRAY8, f=1, D=D):
            return Camera(raw_w, raw_h, fmt, f, (C.c_float * 5)(*D))
        params = default_frontend_params()
        T = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)
        raw = np.zeros((3 * H + 2, 4 * (3 * W + 2)), np.uint8)
        out = np.zeros((H, W), np.uint8)
        n = C.c_int32(7)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        track_raw = lambda pitch, p=params, T=T: L.flame_hip_frontend_track_raw(h, C.byref(p), vp(raw), pitch, 1, vp(T), 1, C.byref(n))  # noqa: E731
        info = C.c_int64(-1)
        assert L.flame_hip_frontend_info(h, b"camera", C.byref(info)) == 0 and info.value == 0
        # without a camera: STATE
        assert track_raw(W) == lib.ERR_STATE and n.value == 0
        assert L.flame_hip_frontend_rectify(h, vp(raw), W, vp(out), W) == lib.ERR_STATE
        # set_camera: ARG / NAN before anything else
        for bad in (cam(raw_w=W + 1), cam(raw_h=H - 1), cam(f=0), cam(f=9), cam(fmt=5), cam(fmt=-1), cam(raw_w=2 * W, raw_h=2 * H, f=3)):
            assert L.flame_hip_frontend_set_camera(h, C.byref(bad)) == lib.ERR_ARG
        for bad in (cam(D=(float("nan"), 0, 0, 0, 0)), cam(D=(0, 0, 0, 0, float("inf")))):
            assert L.flame_hip_frontend_set_camera(h, C.byref(bad)) == lib.ERR_NAN
        assert L.flame_hip_frontend_info(h, b"camera", C.byref(info)) == 0 and info.value == 0  # (a refused camera is not set)
        # a valid camera (sizes that do not divide, a colour format): recorded; the calls then check against it
        assert L.flame_hip_frontend_set_camera(h, C.byref(cam(raw_w=3 * W + 2, raw_h=3 * H + 1, fmt=IR.BGRA8, f=3))) == 0
        assert L.flame_hip_frontend_info(h, b"camera", C.byref(info)) == 0 and info.value == 1
        need = 4 * (3 * W + 2)
        assert track_raw(need - 1) == lib.ERR_ARG
        assert L.flame_hip_frontend_rectify(h, vp(raw), need - 1, vp(out), W) == lib.ERR_ARG
        assert L.flame_hip_frontend_rectify(h, vp(raw), need, vp(out), W - 1) == lib.ERR_ARG
        assert L.flame_hip_frontend_rectify(h, None, need, vp(out), W) == lib.ERR_ARG
        assert track_raw(need, p=default_frontend_params(win_size=4)) == lib.ERR_ARG
        Tn = T.copy()
        Tn[3] = np.nan
        assert track_raw(need, T=Tn) == lib.ERR_NAN
        # everything valid: there is no CPU path
        assert track_raw(need) == lib.ERR_NODEVICE
        assert L.flame_hip_frontend_rectify(h, vp(raw), need, vp(out), W) == lib.ERR_NODEVICE
        assert L.flame_hip_frontend_image(h, vp(out), W) == lib.ERR_NODEVICE
        assert L.flame_hip_frontend_image(h, vp(out), W - 1) == lib.ERR_ARG
        img = np.zeros((H, W), np.uint8)
        assert L.flame_hip_frontend_track(h, C.byref(params), vp(img), W, 1, vp(T), 1, C.byref(n)) == lib.ERR_NODEVICE
        # NULL: back to rectified input
        assert L.flame_hip_frontend_set_camera(h, None) == 0
        assert track_raw(need) == lib.ERR_STATE
        for key in (b"ingest_device_us", b"ingest_raw_bytes"):
            assert L.flame_hip_frontend_info(h, key, C.byref(info)) == 0 and info.value == 0
    finally:
        L.flame_hip_frontend_destroy(h)
