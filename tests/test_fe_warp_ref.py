"""CPU: the warped matching window (DESIGN.md 5.3 "Warped window") -- the restatement tests/fe_warp_ref.py, which the GPU has to
equal bit for bit (tests/test_gpu_fe_warp.py), pinned independently of any kernel:
  1. the ABI surface on a handle without a device;
  2. hand-written windows for the three costs: the identity map gives the base classes' cost, the quarter turn np.rot90 of the
     window, a half-scale map D values written out by hand, negative offsets floor, a turned window's corner leaves the image;
  3. the refusal: a pose five and a half times closer, a grazing view, and the exact edges of both tests;
  4. J against float64 central differences of the exact projection, within 1/256 plus a counted rounding band;
  5. a pure translation: the switch changes no bit, for the three costs;
  6. ground truth on the five scenes of tests/fe_warp_scenes.py."""
import ctypes as C

import numpy as np
import pytest

from flame_ros_amd import lib
from tests import fe_warp_ref as WR
from tests import fe_warp_scenes as WS
from tests import fe_zm_scenes as ZS
from tests import frontend_ref as R

F = np.float32
COSTS = ("ssd", "zssd", "gi")


# ---- 1. the ABI surface, on a handle without a device ----

def test_abi_surface_without_a_device():
    L = lib.load()
    assert hasattr(L, "flame_hip_frontend_set_warp")
    assert L.flame_hip_version() >= 412
    from flame_ros_amd import frontend as FE
    assert callable(FE.GpuFrontEnd.set_warp)
    assert C.sizeof(FE.FrontEndParams) == 40  # (the parameter record keeps its size: the switch is the handle's)
    W, H = 48, 36
    K = np.array([140, 0, 23.5, 0, 140, 17.5, 0, 0, 1], np.float32)
    h = C.c_void_p()
    assert L.flame_hip_frontend_create(C.byref(h), -1, W, H, K.ctypes.data_as(C.c_void_p), 64, 2) == 0
    try:
        def info(key):
            v = C.c_int64(-7)
            assert L.flame_hip_frontend_info(h, key, C.byref(v)) == 0
            return v.value
        sw = L.flame_hip_frontend_set_warp
        assert info(b"warp") == 0 and info(b"warp_refused") == 0
        assert sw(None, 1) == lib.ERR_ARG and sw(None, 0) == lib.ERR_ARG
        assert sw(h, 1) == 0 and info(b"warp") == 1
        for bad in (2, -1, 256, -2 ** 31):
            assert sw(h, bad) == lib.ERR_ARG and info(b"warp") == 1  # a refused value leaves the switch as it was
        assert sw(h, 0) == 0 and info(b"warp") == 0
        assert sw(h, 7) == lib.ERR_ARG and info(b"warp") == 0
        assert sw(h, 1) == 0
        p = FE.default_frontend_params()
        img, T, n = np.zeros((H, W), np.uint8), np.ascontiguousarray(R.pose().reshape(-1)), C.c_int32()
        assert L.flame_hip_frontend_track(h, C.byref(p), img.ctypes.data_as(C.c_void_p), W, 0, T.ctypes.data_as(C.c_void_p), 1,
                                          C.byref(n)) == lib.ERR_NODEVICE
        assert info(b"warp") == 1 and info(b"cost_mode") == 0 and info(b"gain_invariant") == 0 and info(b"ref_grad") == 0
    finally:
        L.flame_hip_frontend_destroy(h)
    with FE.GpuFrontEnd(W, H, K, 64, 2, device=-1) as fe:
        assert fe.info("warp") == 0
        fe.set_warp()
        assert fe.info("warp") == 1
        fe.set_warp(False)
        assert fe.info("warp") == 0 and fe.info("warp_refused") == 0


# ---- 2. hand-written windows ----

SW, SH = 24, 24


def small_images(seed=3):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (SH, SW)).astype(np.int64), rng.integers(0, 256, (SH, SW)).astype(np.int64)


def make(cost):
    fe = R.FrontEndRef(SW, SH, np.array([20, 0, 11.5, 0, 20, 11.5, 0, 0, 1], np.float32), 8, 2)
    fe.set_cost(cost == "zssd")
    fe.set_gain_invariant(cost == "gi")
    return fe


def cost_with(fe, Jq, cur, ref, u, v, px, py, win):
    fe._Jq = Jq
    try:
        return fe._cost(cur, ref, u, v, F(px), F(py), win)
    finally:
        fe._Jq = None


@pytest.mark.parametrize("win", [3, 5, 9])
@pytest.mark.parametrize("cost", COSTS)
def test_identity_map_is_the_base_cost(cost, win):
    """Jq = (256, 0, 0, 256): ox = qx + 16 i, the unwarped integers -- at fractional positions, at the last valid position and one
    sixteenth beyond it."""
    cur, ref = small_images()
    fe, r = make(cost), win // 2
    last = SW - 2 - r  # ix + r + 1 <= W - 1
    seen = set()
    for (px, py) in ((11.3, 12.7), (r + 0.0, r + 0.0), (last + 0.9375, 10.25), (last + 1.0, 10.25), (r - 0.04, 9.0), (7.5, last + 0.96),
                     (7.5, last + 0.97)):
        base = cost_with(fe, None, cur, ref, 12, 11, px, py, win)
        assert cost_with(fe, WR.IDENTITY, cur, ref, 12, 11, px, py, win) == base, (px, py)
        seen.add(base is None)
    assert seen == {True, False}


@pytest.mark.parametrize("cost", COSTS)
def test_quarter_turn_is_rot90(cost):
    """Jq = (0, -256, 256, 0) permutes the sampling positions with the same fractional weights: the window of bilinear sums is
    np.rot90 of the unwarped one, and at an integer sample the cost is the base cost on the image turned about the sample."""
    cur, ref = small_images(4)
    fe, win, r = make(cost), 5, 2
    for (px, py) in ((11.3, 12.7), (9.0, 14.0), (12.5, 8.0625)):
        Iw, Rw = WR.warped_windows(cur, ref, 12, 11, F(px), F(py), win, WR.QUARTER_TURN, SW, SH)
        base_I, base_R = fe._windows(cur, ref, 12, 11, F(px), F(py), win)
        assert np.array_equal(Iw, np.rot90(base_I)) and np.array_equal(Rw, base_R)
        assert cost_with(fe, WR.QUARTER_TURN, cur, ref, 12, 11, px, py, win) == WR.warped_cost(np.rot90(base_I), base_R, cost)
    turned = cur.copy()
    turned[14 - r:14 + r + 1, 9 - r:9 + r + 1] = np.rot90(cur[14 - r:14 + r + 1, 9 - r:9 + r + 1])
    want = cost_with(fe, None, turned, ref, 12, 11, 9.0, 14.0, win)
    assert want is not None and cost_with(fe, WR.QUARTER_TURN, cur, ref, 12, 11, 9.0, 14.0, win) == want
    # a reference window that IS the turned patch: the warped cost is 0, the upright one is not
    ref2 = ref.copy()
    ref2[11 - r:11 + r + 1, 12 - r:12 + r + 1] = np.rot90(cur[14 - r:14 + r + 1, 9 - r:9 + r + 1])
    assert cost_with(fe, WR.QUARTER_TURN, cur, ref2, 12, 11, 9.0, 14.0, win) == 0 < cost_with(fe, None, cur, ref2, 12, 11, 9.0, 14.0, win)


def test_half_scale_against_d_written_by_hand():
    """Jq = (128, 0, 0, 128) samples at half-pixel steps.  On the ramp cur(x, y) = 10 x + y the bilinear sum is exact,
    I = 256 (10 x + y), against a flat reference window of the centre's grey: D_ij = 1280 i + 128 j."""
    yy, xx = np.mgrid[0:SH, 0:SW]
    cur = (10 * xx + yy).astype(np.int64)
    ref = np.full((SH, SW), cur[7, 9], np.int64)
    Iw, Rw = WR.warped_windows(cur, ref, 12, 11, F(9.0), F(7.0), 3, (128, 0, 0, 128), SW, SH)
    Dm = Iw - Rw
    assert Dm.tolist() == [[-1408, -128, 1152], [-1280, 0, 1280], [-1152, 128, 1408]]
    S2 = 1408 ** 2 * 2 + 128 ** 2 * 2 + 1152 ** 2 * 2 + 1280 ** 2 * 2
    assert S2 == 9928704
    assert WR.warped_cost(Iw, Rw, "ssd") == S2 and WR.warped_cost(Iw, Rw, "zssd") == 9 * S2  # (sum D = 0)
    # the gain-invariant cost of a flat reference window: ZR = 0, ZIR = 0 <= 0, C = ZR
    assert WR.warped_cost(Iw, Rw, "gi") == 0
    for cost in COSTS:
        fe = make(cost)
        assert cost_with(fe, (128, 0, 0, 128), cur, ref, 12, 11, 9.0, 7.0, 3) == WR.warped_cost(Iw, Rw, cost)


def test_negative_offsets_floor():
    """(Jq (i, j) + 8) >> 4 is an arithmetic shift: written out by hand for Jq = (100, -37, 19, 250), where truncation towards
    zero gives eight other values; then through ox >> 4 and ox & 15 on a ramp, where I = 16 (3 ox + 5 oy) exactly."""
    dx, dy = WR.offsets((100, -37, 19, 250), 1)
    assert dx.tolist() == [[-4, 2, 9], [-6, 0, 6], [-9, -2, 4]]
    assert dy.tolist() == [[-17, -16, -14], [-1, 0, 1], [14, 16, 17]]
    yy, xx = np.mgrid[0:SH, 0:SW]
    cur = (3 * xx + 5 * yy).astype(np.int64)
    qx, qy = 83, 170  # (5 + 3/16, 10 + 10/16)
    Iw, _ = WR.warped_windows(cur, cur, 12, 11, F(qx / 16.0), F(qy / 16.0), 3, (100, -37, 19, 250), SW, SH)
    assert np.array_equal(Iw, 16 * (3 * (qx + dx) + 5 * (qy + dy)))
    assert Iw[1, 0] == 16 * (3 * 77 + 5 * 169)  # (ox = 77: pixel 4, weight 13 -- a truncated -5 gives 78)
    # a sample whose offsets reach below zero is invalid, not wrapped
    assert WR.warped_windows(cur, cur, 12, 11, F(0.25), F(10.0), 3, (100, -37, 19, 250), SW, SH) is None


@pytest.mark.parametrize("cost", COSTS)
def test_a_turned_windows_corner_leaves_the_image(cost):
    """45 degrees, win 5: the corner (2, -2) reaches (362 + 362 + 8) >> 4 = 45 sixteenths = 2.81 px along x where the upright window
    reaches 2.  At x = 20.5 of 24 columns the upright window is inside (20 + 2 + 1 <= 23), the turned one is not."""
    cur, ref = small_images(5)
    fe, Jq = make(cost), (181, -181, 181, 181)
    assert WR.offsets(Jq, 2)[0].max() == 45
    assert cost_with(fe, None, cur, ref, 12, 11, 20.5, 12.0, 5) is not None
    assert cost_with(fe, Jq, cur, ref, 12, 11, 20.5, 12.0, 5) is None
    assert cost_with(fe, Jq, cur, ref, 12, 11, 20.0, 12.0, 5) is not None  # (365 >> 4 = 22, its neighbour 23: the last valid one)
    assert cost_with(fe, Jq, cur, ref, 12, 11, 12.0, 12.0, 5) is not None


# ---- 3. the refusal ----

def test_the_edges_of_the_two_tests():
    q = WR.quantise
    assert q((4.0, 0.0, 0.0, 4.0)) == (1024, 0, 0, 1024) and q((-4.0, 0.0, 0.0, -4.0)) == (-1024, 0, 0, -1024)
    assert q((4.0, -4.0, 4.0, 4.0)) == (1024, -1024, 1024, 1024)
    assert q((4.001, 0.0, 0.0, 4.0)) == (1024, 0, 0, 1024)  # (1024.256 + 0.5 floors to 1024)
    assert q((4.002, 0.0, 0.0, 4.0)) is None and q((1.0, 0.0, -4.002, 1.0)) is None  # 1025
    assert q((0.25, 0.0, 0.0, 0.25)) == (64, 0, 0, 64)  # det 4096
    assert q((0.25, 0.0, 0.0, 0.2461)) is None  # (64, 0, 0, 63): det 4032
    assert q((0.0, -0.25, 0.25, 0.0)) == (0, -64, 64, 0)
    assert q((1.0, 0.0, 0.0, -1.0)) is None and q((0.0, 1.0, 1.0, 0.0)) is None  # mirrored
    assert q((1.0, 2.0, 0.5, 1.0)) is None  # collapsed: det 0
    for bad in (float("nan"), float("inf"), float("-inf"), 1e30):
        assert q((1.0, 0.0, bad, 1.0)) is None


@pytest.mark.parametrize("kind", ["closer", "grazing"])
def test_refused_features(kind):
    img, T0 = WS.scene("roll30")[0]
    fe = R.FrontEndRef(WS.W, WS.H, WS.K, 256, 4)
    fe.set_warp()
    p = R.params(**WS.REFUSAL_PRIOR)
    fe.track(p, img, 0, T0, True)
    before = fe.state()
    fe.maps = []
    fe.track(p, img, 1, WS.refusal(kind), False)
    refused = [m for m in fe.maps if m[-1] is None]
    print("%s: %d maps, %d refused, counts %s" % (kind, len(fe.maps), len(refused), fe.counts))
    assert len(refused) >= 40 and fe.warp_refused() == len(refused) and fe.counts[R.OUTSIDE] >= len(refused)
    for (s, u, v, _, _, J, _) in refused:
        fq = [np.floor(F(x) * F(256.0) + F(0.5)) for x in J]
        if kind == "closer":
            assert max(abs(x) for x in fq) > 1024  # the stretch
        else:
            assert max(abs(x) for x in fq) <= 1024 and fq[0] * fq[3] - fq[1] * fq[2] < 4096  # the area
        assert fe.status[s] == R.OUTSIDE and fe.drop[s] == before["drop"][s] + 1 == 1 and fe.kstar[s] == -1
        assert fe.mu[s].view(np.uint32) == before["mu"][s].view(np.uint32) and fe.var[s].view(np.uint32) == before["var"][s].view(np.uint32)
        assert fe.steps[s] == 0 and (fe.seg[s] == 0).all()
    # with the switch off the same frame searches every one of them
    off = R.FrontEndRef(WS.W, WS.H, WS.K, 256, 4)
    off.track(p, img, 0, T0, True)
    off.track(p, img, 1, WS.refusal(kind), False)
    assert all(off.steps[m[0]] > 0 for m in refused) and off.warp_refused() == 0


def test_refused_features_die_after_max_dropouts():
    img, T0 = WS.scene("roll30")[0]
    fe = R.FrontEndRef(WS.W, WS.H, WS.K, 256, 4)
    fe.set_warp()
    p = R.params(max_dropouts=1, **WS.REFUSAL_PRIOR)
    fe.track(p, img, 0, T0, True)
    fe.track(p, img, 1, WS.refusal("closer"), False)
    assert fe.alive.sum() == 80 and fe.counts.get(R.DIED, 0) == 0
    fe.track(p, img, 2, WS.refusal("closer"), False)
    assert fe.alive.sum() == 0 and fe.counts[R.DIED] == 80 == fe.warp_refused()


# ---- 4. J against float64 central differences ----

def _exact_record(T, Tr):
    fx, fy, cx, cy = (float(x) for x in WS.K4)
    M = lambda X: np.vstack([np.asarray(X, np.float64).reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])  # noqa: E731
    Tcr = np.linalg.inv(M(T)) @ M(Tr)
    Km = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    return Km @ Tcr[:3, :3], Km @ Tcr[:3, 3]


@pytest.mark.parametrize("name", WS.NAMES)
def test_j_against_float64_central_differences(name):
    """|Jq / 256 - J| <= 1 / 256 + band per entry, J the central difference of the exact projection at xi_J in float64.  The band is
    counted, not measured: fe_warp_ref.Err carries a first-order error bound through the operations of jacobian32, one rounding of
    2^-24 each, A and c rounded once (it comes to below 1e-6; rounding to the nearest 1/256 itself takes half of the 1/256)."""
    fe = R.FrontEndRef(WS.W, WS.H, WS.K, 256, 4)
    fe.set_warp()
    p = R.params()
    n, worst, widest = 0, 0.0, 0.0
    for k, (img, T) in enumerate(WS.scene(name)):
        fe.maps = []
        fe.track(p, img, k, T, k == 0)
        for (s, u, v, Tr, xj, J, Jq) in fe.maps:
            assert Jq is not None
            J64 = WR.jacobian64(WS.K4, T, Tr, u, v, float(xj))
            band = WR.jacobian_band(WS.K4, *_exact_record(T, Tr), u, v, float(xj)) * 1.001 + 1e-8  # (second order; the differences' own noise)
            assert (np.abs(np.array(J, np.float64) - J64) <= band).all(), (name, k, u, v, J, J64, band)
            err = np.abs(np.array(Jq, np.float64) / 256.0 - J64)
            assert (err <= 1.0 / 256.0 + band).all(), (name, k, u, v, Jq, J64)
            n, worst, widest = n + 1, max(worst, err.max()), max(widest, band.max())
    print("%s: %d maps, worst |Jq / 256 - J| %.6f, widest band %.2e" % (name, n, worst, widest))
    assert n >= 400 and widest < 1e-5


# ---- 5. a pure translation ----

@pytest.mark.parametrize("cost", COSTS)
def test_pure_translation_changes_no_bit(cost):
    frames = WS.translation()
    runs = []
    for warp in (False, True):
        fe = R.FrontEndRef(WS.W, WS.H, WS.K, 256, 4)
        fe.set_warp(warp)
        fe.set_cost(cost == "zssd")
        fe.set_gain_invariant(cost == "gi")
        p = R.params(win_size=5)
        rec = []
        for k, (img, T) in enumerate(frames):
            out = fe.track(p, img, k, T, k == 0)
            rec.append((out, fe.state(), fe.searches(), dict((a, b) for a, b in fe.counts.items() if a != "warp_refused")))
        runs.append((fe, rec))
    (off, a), (on, b) = runs
    assert len(on.maps) >= 300 and all(m[-1] == WR.IDENTITY for m in on.maps) and not off.maps
    bits = lambda x: x.view(np.uint32) if x.dtype == np.float32 else x  # noqa: E731
    for k, (x, y) in enumerate(zip(a, b)):
        for i in range(3):
            for key in x[i]:
                assert np.array_equal(bits(x[i][key]), bits(y[i][key])), (k, i, key)
        assert x[3] == y[3], k
    assert sum(r[3].get(R.OK, 0) for r in b) >= 200


# ---- 6. ground truth ----

# Measured with this restatement, frame 0 the pose frame, the last of eight frames, converged = var < 0.01:
#                  SSD 5 x 5 off          SSD 5 x 5 on             ZSSD 7 x 7 off         ZSSD 7 x 7 on
#   roll30         5 emitted, 4 off       45 conv, median 0.57 %   3 emitted, 3 off       45 conv, 0.54 %, worst 2.4 %
#   roll90         2 emitted, 2 off       41 conv, 0.65 %          2 emitted, 2 off       39 conv, 0.58 %
#   roll180        5 emitted, 3 off       46 conv, 0.61 %          2 emitted, 2 off       45 conv, 0.61 %
#   back           42 conv, 1.68 %        47 conv, 0.32 %          43 conv, 1.32 %        46 conv, 0.62 %
#   roll30_closer  9 conv, 17 %, 7 off    37 conv, 0.35 %          6 conv, 14 %, 6 off    34 conv, 0.38 %, worst 1.8 %
# The bounds: no feature off by more than 10 % (worst measured 3.8 %), median at most 1 % (worst 0.65 %), at most 15 emitted with the
# switch off under a roll (worst 5).  The number converged was asked as at least 30; the smallest measured is 34, which leaves less
# than a quarter of margin, so the bound is 25 = 3/4 of it rounded down (DESIGN.md 6 says so).
MIN_CONVERGED, MAX_MEDIAN, OFF, MAX_EMITTED_OFF = 25, 0.01, 0.10, 15


@pytest.mark.parametrize("cost,win", [("ssd", 5), ("zssd", 7)])
@pytest.mark.parametrize("name", WS.NAMES)
def test_ground_truth(name, cost, win):
    frames = WS.scene(name)
    T = frames[-1][1]
    _, outs = WR.run(frames, WS.W, WS.H, WS.K, warp=True, cost=cost, win_size=win)
    err, emitted = ZS.relative_errors(outs[-1], T)
    print("%s %s %d on: emitted %d, converged %d, median %.4f, worst %.4f" % (name, cost, win, emitted, len(err), np.median(err), err.max()))
    assert len(err) >= MIN_CONVERGED and (err > OFF).sum() == 0 and np.median(err) <= MAX_MEDIAN
    if name in WS.ROLL_ONLY:
        _, outs = WR.run(frames, WS.W, WS.H, WS.K, warp=False, cost=cost, win_size=win)
        err, emitted = ZS.relative_errors(outs[-1], T)
        print("%s %s %d off: emitted %d, converged %d, off by more than %.2f: %d" % (name, cost, win, emitted, len(err), OFF, (err > OFF).sum()))
        assert emitted <= MAX_EMITTED_OFF
