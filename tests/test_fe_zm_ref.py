"""CPU: the zero-mean matching cost's restatement tests/fe_zm_ref.py (DESIGN.md 5.3 "Matching cost"), so that "the GPU equals the
restatement" (tests/test_gpu_fe_zm.py) is not circular:
  1. hand-written windows: C against hand-computed integers, the extremes a 32-bit S1^2 or n S2 would wrap at, the BAD_MATCH
     boundary, the saturation of n bad, a tie, and three samples where SSD under a grey offset picks the neighbour and ZSSD the
     true sample;
  2. exact invariance: under random per-frame grey offsets (the pose frame's included) the restatement's features, state, searches
     and counts equal the b = 0 run's bit for bit; SSD's do not;
  3. ground truth at win = 7 on the plane scenes;
  4. the ABI surface on a handle without a device."""
import ctypes as C

import numpy as np
import pytest

from flame_ros_amd import lib
from tests import fe_zm_ref as Z
from tests import fe_zm_scenes as ZS
from tests import frontend_ref as R

F = np.float32
M = 65280  # the largest |D|: 255 * 256


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return all(np.asarray(a[k]).shape == np.asarray(b[k]).shape and np.array_equal(bits(a[k]), bits(b[k])) for k in a)


# ---- 1. hand-written windows ----

def window_cost(cur_win, ref_win, zero_mean, qx=0, qy=0):
    """The restatement's cost of one sample whose window is `cur_win` ((win + 1)^2: the bilinear neighbours included) against the
    reference window `ref_win` (win^2), at the sub-pixel position (qx, qy) / 16."""
    cur_win, ref_win = np.asarray(cur_win, np.int64), np.asarray(ref_win, np.int64)
    win = ref_win.shape[0]
    r, n = win // 2, 12
    cur, ref = np.zeros((n, n), np.int64), np.zeros((n, n), np.int64)
    cur[1:win + 2, 1:win + 2] = cur_win
    ref[1:win + 1, 1:win + 1] = ref_win
    z = R.FrontEndRef(n, n, np.array([10, 0, 6, 0, 10, 6, 0, 0, 1], np.float32), 4, 1)
    z.set_cost(zero_mean)
    return z._cost(cur, ref, 1 + r, 1 + r, F(1 + r) + F(qx) / F(16), F(1 + r) + F(qy) / F(16), win)


def pad(w):
    """A win^2 window at an integer position: the bilinear neighbours get weight 0."""
    w = np.asarray(w, np.int64)
    out = np.zeros((w.shape[0] + 1, w.shape[1] + 1), np.int64)
    out[:-1, :-1] = w
    return out


def test_cost_at_win_3_against_hand_computed_integers():
    ref = np.full((3, 3), 100)
    d = np.array([[1, -2, 3], [0, 4, -1], [2, 5, -3]])
    # D = 256 d: S1 = 256 * 9 = 2304, S2 = 65536 * 69 = 4521984, C = 9 * 4521984 - 2304^2 = 40697856 - 5308416
    assert window_cost(pad(ref + d), ref, True) == 35389440
    assert window_cost(pad(ref + d), ref, False) == 4521984
    # a quarter pixel to the right, columns 10 20 40 80, reference 0: D = 16 (12 t0 + 4 t1) = 3200 6400 12800 in each of three rows
    # S1 = 3 * 22400 = 67200, S2 = 3 * 215040000 = 645120000, C = 9 * 645120000 - 67200^2 = 5806080000 - 4515840000
    cur = np.tile(np.array([10, 20, 40, 80]), (4, 1))
    assert window_cost(cur, np.zeros((3, 3)), True, qx=4) == 1290240000
    assert window_cost(cur, np.zeros((3, 3)), False, qx=4) == 645120000
    # a constant difference costs nothing, whatever its size
    for b in (-100, -1, 0, 1, 155):
        assert window_cost(pad(ref + b), ref, True) == 0
        assert window_cost(np.full((4, 4), 100 + b), ref, True, qx=7, qy=13) == 0


@pytest.mark.parametrize("win", [3, 5, 7, 9])
def test_extremes(win):
    """D alternating +-65 280 (41 of +, 40 of - at win = 9): S1 = 65 280, S2 = n 65 280^2, C = (n^2 - 1) 65 280^2."""
    n = win * win
    chess = (np.add.outer(np.arange(win), np.arange(win)) % 2 == 0)
    cur, ref = np.where(chess, 255, 0), np.where(chess, 0, 255)
    want = (n * n - 1) * M * M
    assert window_cost(pad(cur), ref, True) == want and want < 2 ** 45
    assert window_cost(pad(cur), ref, False) == n * M * M
    if win == 9:  # what 32-bit arithmetic would have made of it
        assert M * M < 2 ** 32 <= 2 * M * M and (n * M) ** 2 >= 2 ** 32 and n * (n * M * M) >= 2 ** 44 and want == 27955298304000
        assert Z.zssd(np.where(chess, M, -M)) == want
    # every D = +65 280: the largest S1, and zero cost
    assert window_cost(pad(np.full((win, win), 255)), np.zeros((win, win)), True) == 0
    assert n * M <= 81 * 65280 < 2 ** 31


def test_saturation_of_the_threshold():
    top = Z.U64_MAX
    assert Z.sat_mul(81, top // 81) == 81 * (top // 81) <= top
    assert Z.sat_mul(81, top // 81 + 1) == top and Z.sat_mul(9, top) == top and Z.sat_mul(1, top) == top
    assert Z.sat_mul(49, 0) == 0
    # inside the range the C ABI accepts (max_match_error <= 65 025) the product never saturates: n bad <= 81^2 65 280^2
    assert Z.bad_threshold(65025.0, 9, Z.COST_ZSSD) == 81 * 81 * M * M < 2 ** 46
    assert Z.bad_threshold(100.0, 7, Z.COST_SSD) == 321126400 and Z.bad_threshold(100.0, 7, Z.COST_ZSSD) == 49 * 321126400
    # a restatement fed a parameter far outside it saturates instead of wrapping
    assert Z.bad_threshold(3.0e38, 9, Z.COST_ZSSD) == top


class Injected(R.FrontEndRef):
    """One live feature at (24, 18) of pose frame 0 whose search has exactly six samples; the costs are hand-written."""
    TX = 0.02  # L = 140 * 0.02 * (1.5 - 0.01) = 4.17: S = 5

    def __init__(self, costs, zero_mean=True, **kw):
        super().__init__(48, 36, np.array([140, 0, 23.5, 0, 140, 17.5, 0, 0, 1], np.float32), 4, 2)
        self.set_cost(zero_mean)
        self.alive[0], self.u[0], self.v[0], self.pf[0], self.mu[0], self.var[0] = 1, 24, 18, 0, F(0.5), F(0.25)
        self.pf_used[0], self.pf_T[0], self.pf_img[0], self.pf_added = True, R.pose(), np.zeros((36, 48), np.int64), 1
        self.injected, self.p = list(costs), R.params(**kw)

    def _cost(self, cur, ref, u, v, px, py, win):
        self._k += 1
        return self.injected[self._k - 1]

    def run(self):
        self._k = 0
        self.track(self.p, np.zeros((36, 48), np.uint8), 1, R.pose((self.TX, 0.0, 0.0)), False)
        assert self._k == len(self.injected) == self.steps[0] + 1 == 6
        return int(self.status[0]), int(self.kstar[0])


def test_bad_match_boundary():
    bad_zm = Z.bad_threshold(100.0, 7, Z.COST_ZSSD)
    assert bad_zm == 49 * int(100.0 * 49 * 65536.0) == 15735193600
    big = 4 * bad_zm
    assert Injected([big, big, bad_zm, big, big, big], win_size=7).run() == (R.OK, 2)          # C == bad_zm is kept
    assert Injected([big, big, bad_zm + 1, big, big, big], win_size=7).run() == (R.BAD_MATCH, 2)
    # the SSD threshold is the base class's, untouched
    bad = Z.bad_threshold(100.0, 7, Z.COST_SSD)
    assert Injected([big, big, bad, big, big, big], zero_mean=False, win_size=7).run() == (R.OK, 2)
    assert Injected([big, big, bad + 1, big, big, big], zero_mean=False, win_size=7).run() == (R.BAD_MATCH, 2)
    assert Injected([big, big, bad + 1, big, big, big], zero_mean=True, win_size=7).run() == (R.OK, 2)


def test_tie_goes_to_the_smaller_k_and_ambiguity_keeps_its_rule():
    assert Injected([9, 5, 7, 5, 9, 9]).run() == (R.OK, 1)
    assert Injected([9, 9, 9, 5, 7, 5]).run() == (R.OK, 3)
    assert Injected([0, 0, 0, 0, 0, 0]).run() == (R.OK, 0)         # 2 * 0 < 3 * 0 is false: nothing is ambiguous
    assert Injected([10, 30, 30, 14, 30, 30]).run() == (R.AMBIGUOUS, 0)  # 2 * 14 < 3 * 10, three steps away
    assert Injected([10, 30, 30, 15, 30, 30]).run() == (R.OK, 0)         # 2 * 15 < 3 * 10 is false
    assert Injected([10, 30, 14, 30, 30, 30]).run() == (R.OK, 0)         # two steps away: a neighbour of the minimum, not a rival
    assert Injected([None] * 6).run() == (R.OUTSIDE, -1)
    top = (81 * 81 - 1) * M * M  # the largest cost there is, under the largest threshold the ABI accepts
    assert Injected([None, None, top, None, None, None], max_match_error=65025.0, win_size=9).run() == (R.OK, 2)


def test_offset_moves_the_ssd_minimum_to_the_neighbour_and_not_the_zssd_minimum():
    """win = 3, b = +12.  Sample 1 is the true one (the reference window itself), sample 0 a neighbour that is 12 grey levels darker
    plus a small pattern: once the frame is 12 brighter the neighbour's SSD is only the pattern's, the true sample's is 9 * 12^2."""
    ref = np.array([[60, 90, 120], [80, 130, 100], [150, 70, 110]])
    pat = np.array([[3, -3, 3], [-3, 3, -3], [3, -3, 0]])  # sum 0, sum of squares 72
    far = ref[::-1, ::-1] + 40
    b = 12
    costs = {}
    for zm in (False, True):
        for off in (0, b):
            costs[zm, off] = [window_cost(pad(w + off), ref, zm) for w in (ref - b + pat, ref, far)] + [window_cost(pad(far + off), ref, zm)] * 3
    u = 65536
    assert costs[False, 0][:2] == [u * (72 + 9 * 144), 0] and costs[False, b][:2] == [u * 72, u * 9 * 144]
    assert costs[True, 0][:2] == costs[True, b][:2] == [u * 9 * 72, 0] and costs[True, 0] == costs[True, b]
    kw = dict(win_size=3, max_match_error=1000.0)
    assert Injected(costs[False, 0], zero_mean=False, **kw).run() == (R.OK, 1)
    assert Injected(costs[False, b], zero_mean=False, **kw).run() == (R.OK, 0)   # SSD: the neighbour
    assert Injected(costs[True, 0], zero_mean=True, **kw).run() == (R.OK, 1)
    assert Injected(costs[True, b], zero_mean=True, **kw).run() == (R.OK, 1)     # ZSSD: the true sample


# ---- 2. exact invariance ----

def run_scene(name, win, zero_mean, offsets=None, poseframes=(0, 4)):
    ref = R.FrontEndRef(ZS.W, ZS.H, ZS.K, 256, 4)
    ref.set_cost(zero_mean)
    p = R.params(win_size=win)
    rec, out = [], None
    for k, (img, T) in enumerate(ZS.scene(name, 1, offsets)):
        out = ref.track(p, img, k, T, k in poseframes)
        rec.append((out, ref.state(), ref.searches(), dict(ref.counts, dropped=ref.dropped)))
    return rec, out, T


_runs = {}


def plain_run(name, win, zero_mean):
    key = (name, win, zero_mean)
    if key not in _runs:
        _runs[key] = run_scene(name, win, zero_mean)
    return _runs[key]


@pytest.mark.parametrize("win", [5, 7])
@pytest.mark.parametrize("name", ["sideways", "diagonal_roll"])
def test_offsets_change_nothing_under_zssd_and_something_under_ssd(name, win):
    """Frames 0 and 4 are pose frames, so two reference images carry an offset of their own."""
    offsets = ZS.random_offsets(7)
    assert len(set(offsets)) == len(offsets) and 0 not in offsets
    for (img, _), (img0, _), b in zip(ZS.scene(name, 1, offsets), ZS.scene(name, 1), offsets):
        assert np.array_equal(img.astype(np.int64), img0.astype(np.int64) + b)
    plain, shifted = plain_run(name, win, True)[0], run_scene(name, win, True, offsets)[0]
    assert len(plain) == len(shifted) == 6
    for k, (a, b) in enumerate(zip(plain, shifted)):
        assert same(a[0], b[0]) and same(a[1], b[1]) and same(a[2], b[2]) and a[3] == b[3], (name, win, k)
    assert sum(r[3].get(R.OK, 0) for r in plain) >= 150 and len(plain[-1][0]["slot"]) >= 40
    ssd_plain, ssd_shifted = plain_run(name, win, False)[0], run_scene(name, win, False, offsets)[0]
    assert not all(same(a[0], b[0]) and same(a[1], b[1]) for a, b in zip(ssd_plain, ssd_shifted))
    assert sum(r[3].get(R.BAD_MATCH, 0) for r in ssd_shifted) > sum(r[3].get(R.BAD_MATCH, 0) for r in ssd_plain)


def test_ssd_mode_is_the_base_class():
    p = R.params()
    a, b = R.FrontEndRef(ZS.W, ZS.H, ZS.K, 256, 4), R.FrontEndRef(ZS.W, ZS.H, ZS.K, 256, 4)
    a.set_cost(True)
    a.set_cost(False)
    for k, (img, T) in enumerate(ZS.scene("sideways", 1)[:3]):
        assert same(a.track(p, img, k, T, k == 0), b.track(p, img, k, T, k == 0)) and same(a.state(), b.state())


# ---- 3. ground truth ----

# Worst relative inverse-depth error of a converged (var < 0.01) emitted feature of the last frame, measured with this restatement at
# win = 7 over the three scenes below: 0.0572 ("sideways"), 0.2104 ("diagonal_roll"), 0.0292 ("refpose_nonidentity"); medians 0.0090,
# 0.0121, 0.0082.  The bounds are 4 x the worst of each -- the margin DESIGN.md 5.3 uses for its constants.
WORST, WORST_MEDIAN = 0.2104, 0.0121
BOUND, BOUND_MEDIAN = 4 * WORST, 4 * WORST_MEDIAN


@pytest.mark.parametrize("name", ["sideways", "diagonal_roll", "refpose_nonidentity"])
def test_ground_truth_at_win_7(name):
    rec, out, T = run_scene(name, 7, True, poseframes=(0,))
    err, emitted = ZS.relative_errors(out, T)
    print("%s: emitted %d, converged %d, worst %.4f, median %.4f" % (name, emitted, len(err), err.max(), np.median(err)))
    assert emitted >= 40 and len(err) >= 0.8 * emitted
    assert err.max() <= BOUND and np.median(err) <= BOUND_MEDIAN


# ---- 4. the ABI surface, on a handle without a device ----

def test_abi_surface_without_a_device():
    L = lib.load()
    assert hasattr(L, "flame_hip_frontend_set_cost")
    assert L.flame_hip_version() >= 409
    from flame_ros_amd import frontend as FE
    assert callable(FE.GpuFrontEnd.set_cost) and (FE.COST_SSD, FE.COST_ZSSD) == (0, 1) == (Z.COST_SSD, Z.COST_ZSSD)
    assert C.sizeof(FE.FrontEndParams) == 40  # (the parameter record keeps its size: the cost is the handle's, like the gates)
    W, H = 48, 36
    K = np.array([140, 0, 23.5, 0, 140, 17.5, 0, 0, 1], np.float32)
    h = C.c_void_p()
    assert L.flame_hip_frontend_create(C.byref(h), -1, W, H, K.ctypes.data_as(C.c_void_p), 64, 2) == 0
    try:
        def info(key):
            v = C.c_int64(-7)
            assert L.flame_hip_frontend_info(h, key, C.byref(v)) == 0
            return v.value
        sc = L.flame_hip_frontend_set_cost
        assert info(b"cost_mode") == 0
        assert sc(None, 0) == lib.ERR_ARG and sc(None, 1) == lib.ERR_ARG
        assert sc(h, 1) == 0 and info(b"cost_mode") == 1
        for mode in (2, -1, 256, 2 ** 31 - 1):  # a refused mode leaves the cost as it was
            assert sc(h, mode) == lib.ERR_ARG and info(b"cost_mode") == 1
        assert sc(h, 0) == 0 and info(b"cost_mode") == 0
        assert sc(h, 1) == 0
        p = FE.default_frontend_params()
        img, T, n = np.zeros((H, W), np.uint8), np.ascontiguousarray(R.pose().reshape(-1)), C.c_int32()
        assert L.flame_hip_frontend_track(h, C.byref(p), img.ctypes.data_as(C.c_void_p), W, 0, T.ctypes.data_as(C.c_void_p), 1,
                                          C.byref(n)) == lib.ERR_NODEVICE
        assert info(b"cost_mode") == 1 and info(b"gates") == 0
    finally:
        L.flame_hip_frontend_destroy(h)
    with FE.GpuFrontEnd(W, H, K, 64, 2, device=-1) as fe:
        assert fe.info("cost_mode") == FE.COST_SSD
        fe.set_cost()
        assert fe.info("cost_mode") == FE.COST_ZSSD
        fe.set_cost(zero_mean=False)
        assert fe.info("cost_mode") == FE.COST_SSD
