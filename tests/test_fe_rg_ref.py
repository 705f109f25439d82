"""CPU: the restatement of the reference-patch gradient gate (tests/fe_rg_ref.py; DESIGN.md 5.3 "Reference-patch gradient") pinned
without a device, so that "GPU equals restatement" (tests/test_gpu_fe_rg.py) is not circular:
  1. rule by rule on hand-written windows: the tensor against hand-computed integers, the extreme 81 * 255^2, the boundary Q == thr N
     and one ulp below it, the ring leaving the image, a NaN;
  2. the direction comes from the REFERENCE image (a roll by pi / 2 between the pose frame and the tracked frames);
  3. the float32 decision against float64 geometry (the epipole from 4 x 4 poses, the quadratic form with exact integers) over the
     six scenes of tests/frontend_scenes.py;
  4. ground truth: on the half-striped scenes the ungated tracker emits converged features that are off by more than 10 %, the gated
     one emits none and keeps the isotropic half; on isotropic scenes the gate worsens nothing;
  5. the ABI surface on a handle without a device."""
import ctypes as C

import numpy as np
import pytest

from flame_ros_amd import lib
from tests import fe_rg_ref as RG
from tests import fe_zm_scenes as ZS
from tests import frontend_ref as R
from tests import frontend_scenes as SC

F = np.float32
G0 = 5.0


def same(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k in b)


MW, MH, MK, margin_scene = RG.MARGIN_W, RG.MARGIN_H, RG.MARGIN_K, RG.margin_scene


# ---- 1. rule by rule ----

def test_tensor_at_win_3_against_hand_computed_integers():
    """I(x, y) = x^2 + 2 y on 5 x 5: gx = (x + 1)^2 - (x - 1)^2 = 4 x, gy = 4.  The window at (2, 2) holds x = 1, 2, 3 in three rows:
    Sxx = 3 (16 + 64 + 144) = 672, Sxy = 3 (4 + 8 + 12) 4 = 288, Syy = 9 * 16 = 144."""
    yy, xx = np.mgrid[0:5, 0:5]
    img = xx * xx + 2 * yy
    assert RG.structure_tensor(img, 2, 2, 3) == (672, 288, 144)
    # a mixed sign: I = x y, gx = 2 y, gy = 2 x: Sxy = 4 sum x y over the window at (2, 2) = 4 * 6 * 6 = 144; mirrored in x it is -144
    assert RG.structure_tensor(xx * yy, 2, 2, 3) == (4 * 3 * 14, 144, 4 * 3 * 14)
    assert RG.structure_tensor((4 - xx) * yy, 2, 2, 3) == (4 * 3 * 14, -144, 4 * 3 * 14)
    # ... and the decision on it: dx = 1, dy = 0 reads Sxx alone, 672 >= 36 g^2 iff g <= 4.32; dx = 0, dy = 1 reads Syy: 144 >= 36 g^2 iff g <= 2
    S = (672, 288, 144)
    assert RG.passes((3, 2, 1), 2, 2, S, 3, 4.25) and not RG.passes((3, 2, 1), 2, 2, S, 3, 4.5)
    assert RG.passes((2, 3, 1), 2, 2, S, 3, 2.0) and not RG.passes((2, 3, 1), 2, 2, S, 3, 2.0625)
    # the sign of the direction is irrelevant, its length too
    assert RG.passes((1, 2, 1), 2, 2, S, 3, 4.25) and RG.passes((-30, -30, -16), 2, 2, S, 3, 4.25) and not RG.passes((1, 2, 1), 2, 2, S, 3, 4.5)
    # the diagonal (1, 1): Q = 672 + 2 * 288 + 144 = 1392 against 36 g^2 * 2: g <= 4.39;  (1, -1): 672 - 576 + 144 = 240: g <= 1.82
    assert RG.passes((3, 3, 1), 2, 2, S, 3, 4.375) and not RG.passes((3, 3, 1), 2, 2, S, 3, 4.5)
    assert RG.passes((3, 1, 1), 2, 2, S, 3, 1.8125) and not RG.passes((3, 1, 1), 2, 2, S, 3, 1.875)


def test_the_extreme_81_times_255_squared():
    """Columns 0 0 255 255 ...: every central difference along x is +-255.  win = 9: Sxx = 81 * 255^2 = 5 267 025 < 2^24, exact in
    float32; the same image transposed gives Syy; blocks of 2 x 2 give both and |Sxy| <= that."""
    yy, xx = np.mgrid[0:11, 0:11]
    big = 81 * 255 * 255
    assert big == 5267025 < 2 ** 24 and int(F(big)) == big
    cols = 255 * ((xx // 2) % 2)
    assert RG.structure_tensor(cols, 5, 5, 9) == (big, 0, 0) and RG.structure_tensor(cols.T, 5, 5, 9) == (0, 0, big)
    Sxx, Sxy, Syy = RG.structure_tensor(255 * ((xx // 2 + yy // 2) % 2), 5, 5, 9)
    assert Sxx == Syy == big and abs(Sxy) <= big
    # thr = (4 * 81) (127.5 * 127.5) = 5 267 025 exactly: the largest gate any window can pass, and this one passes it
    Q, T = RG.quantities((1, 0, 0), 5, 5, (big, 0, 0), 9, 127.5)
    assert Q == T == F(big) and RG.passes((1, 0, 0), 5, 5, (big, 0, 0), 9, 127.5)
    assert not RG.passes((0, 1, 0), 5, 5, (big, 0, 0), 9, 0.0078125)  # (nothing along y)


def test_boundary_passes_and_one_ulp_below_refuses():
    E, S = (1, 0, 0), (5267025, 0, 0)
    Q, T = RG.quantities(E, 5, 5, S, 9, 127.5)
    assert Q == T and RG.passes(E, 5, 5, S, 9, 127.5)
    # dy^2 = one ulp of 1: N = 1 + 2^-23, thr N rounds to the float32 next above Q (Syy = 0 keeps Q where it was)
    E = (1, F(2.0 ** -11.5), 0)
    Q, T = RG.quantities(E, 5, 5, S, 9, 127.5)
    assert Q == F(5267025) and T == np.nextafter(Q, F(np.inf)) and not RG.passes(E, 5, 5, S, 9, 127.5)
    # the integer step at a small window: thr = 36 * 4 = 144
    assert RG.passes((3, 2, 1), 2, 2, (144, 0, 0), 3, 2.0) and not RG.passes((3, 2, 1), 2, 2, (143, 0, 0), 3, 2.0)
    # a gate of 0 passes everything, a flat window included (the handle never runs the test then)
    assert RG.passes((3, 2, 1), 2, 2, (0, 0, 0), 3, 0.0)


def test_ring_leaving_the_image():
    img = np.arange(7 * 9).reshape(7, 9)
    assert RG.structure_tensor(img, 2, 2, 3) is not None and RG.structure_tensor(img, 6, 4, 3) is not None
    for u, v in ((1, 2), (2, 1), (7, 2), (2, 5)):
        assert RG.structure_tensor(img, u, v, 3) is None
    assert RG.structure_tensor(img, 3, 3, 5) is not None and RG.structure_tensor(img, 2, 3, 5) is None and RG.structure_tensor(img, 4, 3, 7) is None
    # in the tracker: detected at win 3 on the right margin (W - 3, 18), tracked at win 5 -> OUTSIDE, one dropout, no search
    img, second, T0, T1 = margin_scene()
    fe = R.FrontEndRef(MW, MH, MK, 32, 2)
    fe.set_ref_grad(G0)
    fe.track(R.params(win_size=3), img, 0, T0, True)
    s, = np.flatnonzero((fe.alive > 0) & (fe.u == MW - 3) & (fe.v == 18))
    fe.track(R.params(win_size=5), second, 1, T1, False)
    assert fe.status[s] == R.OUTSIDE and fe.drop[s] == 1 and fe.kstar[s] == -1 and fe.steps[s] == 0
    plain = R.FrontEndRef(MW, MH, MK, 32, 2)  # (without the gate the same feature is searched: the OUTSIDE is the ring's)
    plain.track(R.params(win_size=3), img, 0, T0, True)
    plain.track(R.params(win_size=5), second, 1, T1, False)
    assert plain.status[s] != R.OUTSIDE and plain.steps[s] > 0 and (plain.u[s], plain.v[s]) == (MW - 3, 18)


def test_a_nan_refuses():
    S = (672, 288, 144)
    for E in ((np.nan, 2, 1), (3, np.nan, 1), (3, 2, np.nan), (np.inf, 2, 1)):  # (the last: dy = 0, 2 (inf 0) is a NaN in Q)
        assert not RG.passes(E, 2, 2, S, 3, 1.0), E
    assert not RG.passes((3, 2, 1), 2, 2, S, 3, np.nan)
    with pytest.raises(ValueError):
        R.FrontEndRef(48, 36, SC.K, 8, 1).set_ref_grad(float("nan"))
    with pytest.raises(ValueError):
        R.FrontEndRef(48, 36, SC.K, 8, 1).set_ref_grad(-1.0)


def test_gate_off_is_the_base_class():
    p = R.params(win_size=7)
    a, b = R.FrontEndRef(ZS.W, ZS.H, ZS.K, 256, 4), R.FrontEndRef(ZS.W, ZS.H, ZS.K, 256, 4)
    a.set_ref_grad(G0)
    a.set_ref_grad(0.0)
    for k, (img, T) in enumerate(RG.half_striped("sideways")[:3]):
        assert same(a.track(p, img, k, T, k == 0), b.track(p, img, k, T, k == 0)) and same(a.state(), b.state())
        assert a.decisions == [] and a.counts == b.counts


def test_a_refused_feature_is_a_failure_like_ambiguous():
    """Prior and k* untouched, no search, one dropout a frame, death past max_dropouts, counted under its own status."""
    fe, outs, dec = RG.run(RG.half_striped("sideways")[:4], min_grad=G0, win_size=7, max_dropouts=3)
    refused = fe.status == RG.REF_GRAD
    assert refused.sum() >= 25 and (fe.drop[refused] == 3).all() and (fe.kstar[refused] == -1).all()
    assert (fe.mu[refused] == F(0.5)).all() and (fe.var[refused] == F(0.25)).all()
    assert (fe.steps[refused] == 0).all() and (fe.seg[refused] == 0).all()
    assert fe.counts[RG.REF_GRAD] == refused.sum() == sum(1 for d in dec[-1] if not d[-1])
    img, T = RG.half_striped("sideways")[4]
    fe.track(R.params(win_size=7, max_dropouts=3), img, 4, T, False)
    assert (fe.status[refused] == R.DIED).all() and not fe.alive[refused].any() and fe.counts[R.DIED] >= refused.sum()


# ---- 2. the direction comes from the reference image ----

def test_direction_under_a_roll_of_a_quarter_turn():
    """The pose frame at the identity, the tracked frames rolled by pi / 2 and translated along world x: in the reference image the
    epipolar lines run along x, in the current image along y.  Stripes constant along reference x: every search is refused; constant
    along reference y: at most a handful (a twentieth) are.  A gate that took the direction from the current image -- the epipole of
    the REFERENCE view in the current one -- decides both the other way round, which the last lines show."""
    count = {}
    for along in ("x", "y"):
        fe, outs, dec = RG.run(RG.rolled(along), min_grad=G0, win_size=7)
        d = [x for frame in dec for x in frame]
        swapped = [RG.passes(RG.epipole_record(ZS.K4, Tr, T), u, v, S, 7, G0) for k, (_, T) in enumerate(RG.rolled(along))
                   for (_, u, v, Tr, _, S, _) in dec[k]]
        count[along] = (len(d), sum(1 for x in d if not x[-1]), sum(1 for ok in swapped if not ok))
    print("tested, refused, refused with the current image's direction:", count)
    n, refused, wrong = count["x"]
    assert n >= 100 and refused == n and wrong <= n // 20
    n, refused, wrong = count["y"]
    assert n >= 100 and refused <= n // 20 and wrong >= n - n // 20


# ---- 3. the float32 decision against float64 geometry ----

# Roundings along the longest path from the inputs to Q - thr N, each 2^-24 relative: behind (dx, dy) the product dx dx, the product
# with the (exact) integer, two sums on the Q side; g g, thr, dx dx, the sum N, thr N on the other: at most 5; one more for the
# comparison's operands being rounded values.  (dx, dy) themselves carry 3 roundings -- E rounded once, u E2, the difference -- of
# |E0| + |u E2|, not of |dx|: that error reaches Q - thr N through its derivative, which the band carries separately.
ROUNDINGS, DIR_ROUNDINGS, EPS = 6, 3, 2.0 ** -24


@pytest.mark.parametrize("name", SC.NAMES)
def test_decision_against_float64_geometry(name):
    fe = R.FrontEndRef(SC.W, SC.H, SC.K, 256, 4)
    fe.set_ref_grad(G0)
    p = R.params()
    n = inside = close = 0
    for k, (img, T) in enumerate(SC.scene(name, 1)):
        fe.track(p, img, k, T, k in (0, 3))
        for (_, u, v, Tr, E32, S, ok) in fe.decisions:
            E = RG.epipole64(SC.K4, T, Tr)
            Q, TN, mag = RG.quantities64(E, u, v, S, p["win_size"], G0)
            dx, dy = E[0] - u * E[2], E[1] - v * E[2]
            thr = 4.0 * p["win_size"] ** 2 * G0 ** 2
            ex = DIR_ROUNDINGS * EPS * (abs(E[0]) + abs(u * E[2]))
            ey = DIR_ROUNDINGS * EPS * (abs(E[1]) + abs(v * E[2]))
            sens = (2 * abs(dx) * S[0] + 2 * abs(dy) * abs(S[1]) + 2 * thr * abs(dx)) * ex + \
                (2 * abs(dy) * S[2] + 2 * abs(dx) * abs(S[1]) + 2 * thr * abs(dy)) * ey
            band = ROUNDINGS * EPS * mag + sens
            n += 1
            if abs(Q - TN) <= band:
                inside += 1
            else:
                assert ok == (Q >= TN), (name, k, u, v, Q, TN, band)
            close += abs(Q - TN) <= 1e-4 * mag
    print("%s: %d decisions, %d inside the rounding band, %d within 1e-4 relative of the threshold" % (name, n, inside, close))
    assert n >= 250 and inside <= 0.15 * n


def test_epipole_record_is_the_float64_epipole_rounded():
    for name in SC.NAMES:
        Tr = SC.scene_pose(name, 0)
        for k in range(1, SC.FRAMES):
            T = SC.scene_pose(name, k)
            E32, E64 = RG.epipole_record(SC.K4, T, Tr), RG.epipole64(SC.K4, T, Tr)
            assert np.allclose(np.array(E32, np.float64), E64, rtol=4 * EPS, atol=1e-12 * np.abs(E64).max())


# ---- 4. ground truth ----

# Measured with this restatement at win 7, min_grad 5.0, frame 0 the pose frame, converged = var < 0.01 in the last frame:
#   half-striped "sideways": ungated 55 converged, 5 above 10 % (worst 67 %); gated 32 of 78 refused, 30 converged, worst 1.6 %
#   half-striped "vertical": ungated 57 converged, 13 above 10 % (worst 51 %); gated 40 of 80 refused, 31 converged, worst 1.8 %
# 0.10 is the line between the two populations (<= 0.018 gated, >= 0.31 among the ungated outliers), not a tuned tolerance.
OFF = 0.10


@pytest.mark.parametrize("name", ["sideways", "vertical"])
def test_half_striped_ground_truth(name):
    frames = RG.half_striped(name)
    T = frames[-1][1]
    _, outs, _ = RG.run(frames, min_grad=0.0, win_size=7)
    err, _ = ZS.relative_errors(outs[-1], T)
    print("%s ungated: converged %d, above %.2f: %d, worst %.4f" % (name, len(err), OFF, (err > OFF).sum(), err.max()))
    assert (err > OFF).sum() >= 1
    fe, outs, dec = RG.run(frames, min_grad=G0, win_size=7)
    err, _ = ZS.relative_errors(outs[-1], T)
    print("%s gated: refused %d of %d, converged %d, worst %.4f" % (name, sum(1 for d in dec[-1] if not d[-1]), len(dec[-1]), len(err), err.max()))
    assert len(err) >= 25 and (err > OFF).sum() == 0


@pytest.mark.parametrize("name", ["sideways", "diagonal_roll", "refpose_nonidentity"])
def test_isotropic_scenes_are_not_worsened(name):
    frames = ZS.scene(name, 5)
    T = frames[-1][1]
    worst = []
    for g in (0.0, G0):
        _, outs, _ = RG.run(frames, min_grad=g, win_size=7)
        err, _ = ZS.relative_errors(outs[-1], T)
        assert len(err) >= 40
        worst.append(err.max())
    print("%s: worst ungated %.4f, gated %.4f" % (name, worst[0], worst[1]))
    assert worst[1] <= worst[0]


# ---- 5. the ABI surface, on a handle without a device ----

def test_abi_surface_without_a_device():
    L = lib.load()
    assert hasattr(L, "flame_hip_frontend_set_ref_grad")
    assert L.flame_hip_version() >= 410
    from flame_ros_amd import frontend as FE
    assert callable(FE.GpuFrontEnd.set_ref_grad) and FE.REF_GRAD == 7 == RG.REF_GRAD
    assert C.sizeof(FE.FrontEndParams) == 40  # (the parameter record keeps its size: the gate is the handle's)
    W, H = 48, 36
    K = np.array([140, 0, 23.5, 0, 140, 17.5, 0, 0, 1], np.float32)
    h = C.c_void_p()
    assert L.flame_hip_frontend_create(C.byref(h), -1, W, H, K.ctypes.data_as(C.c_void_p), 64, 2) == 0
    try:
        def info(key):
            v = C.c_int64(-7)
            assert L.flame_hip_frontend_info(h, key, C.byref(v)) == 0
            return v.value
        sg = L.flame_hip_frontend_set_ref_grad
        assert info(b"ref_grad") == 0 and info(b"fail_ref_grad") == 0
        assert sg(None, 5.0) == lib.ERR_ARG and sg(None, 0.0) == lib.ERR_ARG
        assert sg(h, 5.0) == 0 and info(b"ref_grad") == 1
        for bad, code in ((float("nan"), lib.ERR_NAN), (float("inf"), lib.ERR_NAN), (float("-inf"), lib.ERR_NAN), (-1.0, lib.ERR_ARG),
                          (-1e-30, lib.ERR_ARG)):
            assert sg(h, bad) == code and info(b"ref_grad") == 1  # a refused value leaves the gate as it was
        assert sg(h, 0.0) == 0 and info(b"ref_grad") == 0
        for bad, code in ((float("nan"), lib.ERR_NAN), (-2.0, lib.ERR_ARG)):
            assert sg(h, bad) == code and info(b"ref_grad") == 0
        assert sg(h, 2.5) == 0
        p = FE.default_frontend_params()
        img, T, n = np.zeros((H, W), np.uint8), np.ascontiguousarray(R.pose().reshape(-1)), C.c_int32()
        assert L.flame_hip_frontend_track(h, C.byref(p), img.ctypes.data_as(C.c_void_p), W, 0, T.ctypes.data_as(C.c_void_p), 1,
                                          C.byref(n)) == lib.ERR_NODEVICE
        assert info(b"ref_grad") == 1 and info(b"cost_mode") == 0 and info(b"gates") == 0
    finally:
        L.flame_hip_frontend_destroy(h)
    with FE.GpuFrontEnd(W, H, K, 64, 2, device=-1) as fe:
        assert fe.info("ref_grad") == 0
        fe.set_ref_grad(5.0)
        assert fe.info("ref_grad") == 1
        with pytest.raises(FE.FlameHipError):
            fe.set_ref_grad(-1.0)
        assert fe.info("ref_grad") == 1
        fe.set_ref_grad(0)
        assert fe.info("ref_grad") == 0 and fe.info("fail_ref_grad") == 0
