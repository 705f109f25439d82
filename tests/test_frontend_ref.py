"""CPU: the NumPy restatement of the feature front end (tests/frontend_ref.py) against ground truth -- what keeps
"the GPU equals the restatement bit for bit" (tests/test_gpu_frontend.py) from being circular.

(a) exact-shift scene: matched disparity against the true shift; (b) slanted plane over six frames: inverse depths against
the analytic plane, and the same plane under general motion (tests/frontend_scenes.py); (c) properties that need no reference.
The per-feature float64 statement with rounding bands is tests/test_frontend_f64.py."""
import numpy as np
import pytest

from tests import frontend_ref as R
from tests import frontend_scenes as SC


def run(frames, poseframes=(0,), max_features=256, max_poseframes=4, W=R.SCENE_W, H=R.SCENE_H, K=R.SCENE_K, **kw):
    fe = R.FrontEndRef(W, H, K, max_features, max_poseframes)
    p = R.params(**kw)
    outs, states = [], []
    for k, (img, T) in enumerate(frames):
        outs.append(fe.track(p, img, k, T, k in poseframes))
        states.append(fe.state())
    return fe, outs, states


@pytest.mark.parametrize("D", [5, 7])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_exact_shift_disparity(D, seed):
    """160x120, f = 140, an 8x bilinearly upsampled random texture cut at two offsets D px apart = a fronto-parallel plane at
    depth Z seen after a sideways translation D Z / f; win 5, cells of 16, prior mu 0.5 / var 0.25.

    Eligible features: those whose true match window (with its +1 bilinear neighbours) lies inside the second image TOGETHER
    WITH the windows one sampling step (<= 1 px) to either side of it along the search -- the bound below is "half a step",
    which presumes that the samples on both sides of the truth exist (a feature whose true match touches the image edge loses
    the nearer sample to the validity rule and is matched one step off: seen at u - D = r).  For every eligible feature with
    status OK the matched disparity is within 0.5 (half a sampling step) + 1/16 (the position quantum) of D; at least 90 % of
    the eligible features are OK.  Measured with this float32 restatement: >= 97 % OK, all within 0.16 px."""
    fe, outs, st = run(R.shift_scene(D, seed))
    assert (outs[0]["status"] == R.NEW).all() and len(outs[0]["slot"]) >= 60
    r, W = 2, R.SCENE_W
    s1 = st[1]
    elig = [s for s in outs[0]["slot"] if s1["u"][s] - D - 1 - r >= 0 and s1["u"][s] - D + 1 + r + 1 <= W - 1]
    ok = [s for s in elig if s1["status"][s] == R.OK]
    err = np.array([abs(float(s1["u"][s]) - float(fe.pstar[s][0]) - D) for s in ok])
    print("eligible %d ok %d share %.3f max |disparity - D| %.4f" % (len(elig), len(ok), len(ok) / len(elig), err.max()))
    assert len(elig) >= 50
    assert (np.abs(fe.pstar[ok][:, 1] - s1["v"][ok]) <= 1.0 / 16).all()
    assert err.max() <= 0.5 + 1.0 / 16
    assert len(ok) >= 0.9 * len(elig)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_slanted_plane_converges(seed):
    """Plane with normal (0.2, -0.1, 1) through depth 3, the texture at 3 texels per world unit, rendered analytically from
    six poses (0.03 sideways, 0.004 rad per frame), frame 0 the pose frame.  After frame 5 the float32 restatement measured,
    over seeds 1 / 2 / 3: median relative inverse-depth error 0.82 % / 0.96 % / 1.13 %, share of live features with
    var < idepth_var_max_graph (0.01) 0.961 / 0.961 / 0.911 (the float64 prototype: 1.2 %, 0.94).  Bounds: twice the worst
    measured error (2.3 %), the worst share - 0.1 (0.81)."""
    frames = R.plane_scene(seed)
    fe, outs, st = run(frames)
    s = st[5]
    al = np.flatnonzero(s["alive"])
    truth, _ = R.plane_idepth(frames[0][1], s["u"][al].astype(np.float64), s["v"][al].astype(np.float64))
    rel = np.abs(s["mu"][al] - truth) / truth
    share = float((s["var"][al] < 0.01).mean())
    print("live %d median rel error %.4f share %.3f" % (len(al), np.median(rel), share))
    assert len(al) >= 60
    assert np.median(rel) <= 0.023
    assert share >= 0.81
    # the emitted features carry the inverse depth of the CURRENT frame: compare with the plane seen from pose 5
    o = outs[5]
    gated = o["idepth_var"] < 0.01
    assert gated.sum() >= 3
    truth5, _ = R.plane_idepth(frames[5][1], o["vtx"][gated, 0].astype(np.float64), o["vtx"][gated, 1].astype(np.float64))
    assert np.median(np.abs(o["idepth_mu"][gated] - truth5) / truth5) <= 0.023


# scene -> (worst median relative error of the state, worst share of var < 0.01, worst median relative error of the emitted,
# gated features), each the worst over seeds 1 / 2 / 3 of the unmutated float32 restatement on the CPU
GENERAL_MOTION = {
    "sideways": (0.0098, 0.925, 0.0093),             # 0.93 / 0.98 / 0.80 %, 0.988 / 0.925 / 0.935, 0.80 / 0.93 / 0.74 %
    "vertical": (0.0093, 0.922, 0.0077),             # 0.93 / 0.81 / 0.83 %, 0.975 / 0.963 / 0.922, 0.73 / 0.77 / 0.66 %
    "diagonal_roll": (0.0098, 0.857, 0.0079),        # 0.94 / 0.71 / 0.98 %, 0.925 / 0.900 / 0.857, 0.79 / 0.61 / 0.70 %
    "forward": (0.0219, 0.649, 0.0077),              # 2.11 / 1.48 / 2.19 %, 0.738 / 0.750 / 0.649, 0.73 / 0.75 / 0.77 %
    "backward_side": (0.0168, 0.762, 0.0152),        # 1.68 / 1.29 / 1.59 %, 0.762 / 0.787 / 0.818, 1.52 / 0.94 / 1.18 %
    "refpose_nonidentity": (0.0084, 0.878, 0.0074),  # 0.72 / 0.75 / 0.84 %, 0.910 / 0.911 / 0.878, 0.73 / 0.74 / 0.58 %
}


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("name", SC.NAMES)
def test_general_motion_plane_converges(name, seed):
    """The slanted plane under general motion (tests/frontend_scenes.py: fx != fy, an off-centre principal point, vertical,
    forward and backward motion, roll, a reference pose that is not the identity), six frames, frame 0 the pose frame.
    After frame 5 the unmutated float32 restatement measured the figures beside GENERAL_MOTION (live features 74-80, gated
    emitted features 30-62).  Bounds, by this file's rule: median relative inverse-depth error <= twice the worst measured
    over the seeds, share of live features with var < 0.01 >= the worst measured - 0.1, live >= 60; the emitted, gated
    features against the plane seen from pose 5: <= twice their worst measured median, at least 15 of them (half the fewest
    measured)."""
    worst_err, worst_share, worst_emitted = GENERAL_MOTION[name]
    frames = SC.scene(name, seed)
    fe, outs, st = run(frames, K=SC.K)
    s = st[5]
    al = np.flatnonzero(s["alive"])
    truth, _ = SC.plane_idepth(SC.K4, frames[0][1], s["u"][al], s["v"][al])
    rel = np.abs(s["mu"][al] - truth) / truth
    share = float((s["var"][al] < 0.01).mean())
    o = outs[5]
    gated = o["idepth_var"] < 0.01
    truth5, _ = SC.plane_idepth(SC.K4, frames[5][1], o["vtx"][gated, 0], o["vtx"][gated, 1])
    rel5 = np.abs(o["idepth_mu"][gated] - truth5) / truth5
    print("%s seed %d: live %d median rel error %.4f share %.3f; emitted gated %d median rel error %.4f" % (
        name, seed, len(al), np.median(rel), share, gated.sum(), np.median(rel5)))
    assert len(al) >= 60
    assert np.median(rel) <= 2.0 * worst_err
    assert share >= worst_share - 0.1
    assert gated.sum() >= 15
    assert np.median(rel5) <= 2.0 * worst_emitted


def brute_detections(img, win, dws, min_grad_mag):
    """Per cell the pixel of the largest g2 (ties: smallest y, then smallest x) by plain loops."""
    H, W = img.shape
    I = img.astype(int)
    m, thr = win // 2 + 1, max(1, int(np.ceil(4.0 * min_grad_mag * min_grad_mag)))
    best = {}
    for y in range(m, H - m):
        for x in range(m, W - m):
            g2 = (I[y, x + 1] - I[y, x - 1]) ** 2 + (I[y + 1, x] - I[y - 1, x]) ** 2
            cell = (y // dws, x // dws)
            if g2 >= thr and (cell not in best or g2 > best[cell][0]):
                best[cell] = (g2, x, y)
    return best


@pytest.mark.parametrize("W,H,dws", [(157, 93, 16), (160, 120, 16), (157, 93, 7)])
def test_detection_properties(W, H, dws):
    """Every detection is its cell's maximum of g2 under the tie rule, at or above the threshold, outside the margin; at most
    one per cell (partial cells at the right / bottom edge included) -- on a texture and on a checkerboard full of exact ties."""
    yy, xx = np.mgrid[0:H, 0:W]
    checker = (((yy // 4) + (xx // 4)) % 2 * 200 + 20).astype(np.uint8)
    for img in (R.upsampled_texture(H, W, 4), checker):
        fe, outs, st = run([(img, R.pose())], W=W, H=H, max_features=4096, detection_win_size=dws)
        o = outs[0]
        want = brute_detections(img, 5, dws, 5.0)
        got = {(int(y) // dws, int(x) // dws): (int(x), int(y)) for x, y in o["vtx"]}
        assert len(got) == len(o["slot"]) == len(want)
        for cell, (g2, x, y) in want.items():
            assert got[cell] == (x, y), (cell, got[cell], (x, y))
            assert g2 >= 100 and 3 <= x < W - 3 and 3 <= y < H - 3
        assert (o["idepth_mu"] == np.float32(0.5)).all() and (o["idepth_var"] == np.float32(0.25)).all()
        # slots ascending, cells in row-major order
        ncx = (W + dws - 1) // dws
        cells = (o["vtx"][:, 1].astype(int) // dws) * ncx + o["vtx"][:, 0].astype(int) // dws
        assert (np.diff(cells) > 0).all() and (o["slot"] == np.arange(len(cells))).all()


def test_no_detection_in_an_occupied_cell_and_variance_never_increases():
    frames = R.plane_scene(2)
    fe, outs, st = run(frames, poseframes=(0, 3))
    o2, o3 = outs[2], outs[3]
    new = o3["status"] == R.NEW
    assert new.any() and (~new).any()
    dws, ncx = 16, 10
    cells = (o3["vtx"][:, 1].astype(int) // dws) * ncx + o3["vtx"][:, 0].astype(int) // dws
    assert len(set(cells.tolist())) == len(cells)  # one emitted feature per cell, old or new
    for k in range(1, 6):
        both = np.flatnonzero(st[k - 1]["alive"] & st[k]["alive"])
        okk = both[st[k]["status"][both] == R.OK]
        assert len(okk) and (st[k]["var"][okk] <= st[k - 1]["var"][okk]).all()
        same = both[st[k]["status"][both] != R.OK]
        assert (st[k]["var"][same] == st[k - 1]["var"][same]).all() and (st[k]["mu"][same] == st[k - 1]["mu"][same]).all()


@pytest.mark.parametrize("max_dropouts", [0, 2, 5])
def test_feature_dies_after_max_dropouts_plus_one_failures(max_dropouts):
    """Frames of unrelated noise after the pose frame: every match fails; a feature lives through max_dropouts failures in a
    row and dies with the next one.  An OK in between clears the counter."""
    rng = np.random.default_rng(7)
    a, b = R.shift_scene(5, 1)
    noise = [(rng.integers(0, 256, a[0].shape).astype(np.uint8), b[1]) for _ in range(max_dropouts + 2)]
    fe, outs, st = run([a, b] + noise, max_dropouts=max_dropouts)
    ok1 = np.flatnonzero((st[1]["status"] == R.OK) & (st[1]["drop"] == 0))
    fails = (R.OUTSIDE, R.BAD_MATCH, R.AMBIGUOUS)
    always = [s for s in ok1 if all(st[k]["status"][s] in fails + (R.DIED,) for k in range(2, 2 + max_dropouts + 1))]
    assert len(always) >= 30
    for s in always:
        for j in range(1, max_dropouts + 1):
            assert st[1 + j]["alive"][s] and st[1 + j]["drop"][s] == j
        assert not st[2 + max_dropouts]["alive"][s] and st[2 + max_dropouts]["status"][s] == R.DIED
        assert st[3 + max_dropouts]["status"][s] == R.FREE
