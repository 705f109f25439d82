"""The feature front end's corpus for the float64 statement (oracle/frontend_f64.py): the six general-motion scenes
(tests/frontend_scenes.py) and the situations of tests/test_gpu_frontend.py, all 160x120 with 256 slots and a ring of four
pose frames that never wraps.  A case is a list of calls; `drive` feeds them to an implementation (the float32 restatement
on the CPU, a GPU handle on the device) and holds every frame -- from the implementation's OWN pre-state -- against the
statement, so nothing accumulates across frames."""
import numpy as np

from oracle import frontend_f64 as F64
from tests import frontend_ref as R
from tests import frontend_scenes as SC

W, H, SLOTS, RING = 160, 120, 256, 4
CAP = 0.15  # at most this share of a case's tracked features may be uncertain (a condition of the corpus, not a measurement)


class Case:
    def __init__(self, K, calls, **kw):
        self.K, self.calls, self.kw = K, calls, kw


def _tracks(frames, poseframes=(0,)):
    return [("track", img, T, k in poseframes, k) for k, (img, T) in enumerate(frames)]


def _scene(name):
    return lambda: Case(SC.K, _tracks(SC.scene(name, 1)))


def _long_search(tx):
    def make():
        a, _ = R.shift_scene(7, 3)
        return Case(R.SCENE_K, [("track", a[0], a[1], True, 0),
                                ("track", np.ascontiguousarray(a[0][:, ::-1]), R.pose((tx, 0.004, 0.0)), False, 1)], var_init=25.0)
    return make


def _border():
    m = 3
    img = np.full((H, W), 100, np.uint8)
    for y in range(8, H - 8, 16):
        img[y, m - 1] = 255
        img[y, W - m] = 255
    for x in range(24, W - 24, 16):
        img[m - 1, x] = 255
        img[H - m, x] = 255
    poses = [R.pose(), R.pose((2.0, 0.0, 0.0)), R.pose((0.0, 0.3, 0.0)), R.pose((0.05, 0.0, 1.2))]
    return Case(R.SCENE_K, [("track", img, T, k == 0, k) for k, T in enumerate(poses)])


def _checkerboard():
    yy, xx = np.mgrid[0:H, 0:W + 8]
    big = (((yy // 4) + (xx // 4)) % 2 * 40 + 100).astype(np.uint8)
    a, b = R.shift_scene(5, 0, big=big)
    noisy = (b[0].astype(int) + np.random.default_rng(3).integers(-2, 3, b[0].shape)).astype(np.uint8)
    return Case(R.SCENE_K, [("track", a[0], a[1], True, 0), ("track", noisy, b[1], False, 1)])


def _noisy_match():
    """Noise of +-40 grey levels under a permissive match threshold lifts every cost: the samples two steps from the best come
    within a factor 1.5 of it for some features and not for others, which is where the ambiguity rule's distance shows
    (unmutated restatement: 68 OK, 12 AMBIGUOUS; with |k - k*| > 1 for > 2, eight statuses change)."""
    a, b = R.shift_scene(5, 1)
    noisy = np.clip(b[0].astype(int) + np.random.default_rng(3).integers(-40, 41, b[0].shape), 0, 255).astype(np.uint8)
    return Case(R.SCENE_K, [("track", a[0], a[1], True, 0), ("track", noisy, b[1], False, 1)], max_match_error=10000.0)


def _colliding():
    a, b = R.shift_scene(5, 5)
    back = R.pose((5 * 2.0 / R.SCENE_F, 0.0, -2.5))
    return Case(R.SCENE_K, [("track", a[0], a[1], True, 0), ("track", b[0], b[1], False, 1), ("track", b[0], back, False, 2),
                            ("track", b[0], back, True, 3)])


def _set_poses():
    fr = R.plane_scene(2)
    moved = [R.pose((0.001, -0.002, 0.0005), 0.0002), R.pose((0.061, 0.0, 0.001), 0.0081)]
    return Case(R.SCENE_K, [("track", fr[0][0], fr[0][1], True, 10), ("track", fr[1][0], fr[1][1], False, 11),
                            ("track", fr[2][0], fr[2][1], True, 12), ("set_poses", [10, 12, 999], moved + [R.pose()]),
                            ("track", fr[3][0], fr[3][1], False, 13), ("prune", [12, 555]), ("track", fr[4][0], fr[4][1], False, 14)])


CASES = {("scene_" + n): _scene(n) for n in SC.NAMES}
CASES.update({
    "exact_shift_5": lambda: Case(R.SCENE_K, _tracks(R.shift_scene(5, 1))),
    "slanted_plane": lambda: Case(R.SCENE_K, _tracks(R.plane_scene(1))),
    "long_search_140": _long_search(0.1),
    "long_search_cap": _long_search(1.0),
    "border_windows": _border,
    "checkerboard_noise": _checkerboard,
    "noisy_match": _noisy_match,
    "colliding_then_poseframe": _colliding,
    "set_poses_and_prune": _set_poses,
    "two_poseframes": lambda: Case(SC.K, _tracks(SC.scene("forward", 1), poseframes=(0, 3))),
})
NAMES = tuple(CASES)
_made = {}


def case(name):
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]


def drive(c, impl, p_impl, info):
    """Feed case `c` to `impl` (track / set_poses / prune / state, as FrontEndRef and GpuFrontEnd have them), p_impl its
    parameter object, info(impl) -> the frame's counters {status: n, "dropped": n, "emitted": n}.  Returns the reports of
    the tracking frames; asserts the cap over the case."""
    st = F64.FrontEndF64(W, H, c.K, SLOTS, RING)
    p = R.params(**c.kw)
    reports = []
    for call in c.calls:
        if call[0] == "track":
            _, img, T, is_pf, img_id = call
            pre = impl.state()
            emitted = impl.track(p_impl, img, img_id, T, is_pf)
            rep = st.check_frame(p, img, img_id, T, is_pf, pre, impl.state(), emitted, info(impl))
            reports.append(rep)
        else:
            getattr(impl, call[0])(*call[1:])
            getattr(st, call[0])(*call[1:])
    unc, n = sum(r["uncertain"] for r in reports), sum(r["tracked"] for r in reports)
    assert unc <= CAP * n, "%d of the case's %d tracked features are uncertain: above the cap of %.2f" % (unc, n, CAP)
    return reports
