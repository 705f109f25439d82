"""The feature front end's reference-patch gradient gate (DESIGN.md 5.3 "Reference-patch gradient"; include/flame_hip.h,
flame_hip_frontend_set_ref_grad) restated in NumPy: the rules tests/frontend_ref.py's FrontEndRef applies after `set_ref_grad`.  A
helper, not a test: tests/test_fe_rg_ref.py checks it rule by rule on hand-written windows, against float64 geometry and against
ground truth, tests/test_gpu_fe_rg.py compares the library with it bit for bit.

With the gate on (min_grad > 0) a feature that has passed the NO_PARALLAX test forms
  * the epipole of the current view in the feature's pose frame, E = K R_ref^T (t_cur - t_ref), in double, rounded once to float32,
  * the integer structure tensor (Sxx, Sxy, Syy) of central differences over the win x win reference window,
  * Q = ((dx dx) Sxx + (2 (dx dy)) Sxy) + (dy dy) Syy, N = dx dx + dy dy, thr = (4 n) (g g) with (dx, dy) = (E0 - u E2, E1 - v E2),
and is searched iff Q >= thr N.  A refused feature fails with status REF_GRAD and no search; a window whose one-pixel ring leaves
the image fails with OUTSIDE.

Also the scenes of the gate: the plane and the poses of tests/frontend_scenes.py under tests/fe_zm_scenes.py's renderer, with a
texture whose right half (or all of it) is stripes -- a 1-D random line in [70, 185], constant along one texture axis; the
renderer's bilinear taps interpolate it linearly."""
import math

import numpy as np

from tests import fe_zm_scenes as ZS
from tests import frontend_ref as R
from tests import frontend_scenes as SC

F = np.float32
REF_GRAD = 7


def epipole_record(K4, Tc, Tr):
    """E = (fx o0 + cx o2, fy o1 + cy o2, o2), o = R_ref^T (t_cur - t_ref), in double (sums left to right), each entry rounded once
    to float32.  Tc / Tr: 3x4 [R|t] float64 of the current camera and of the pose frame."""
    fx, fy, cx, cy = (float(x) for x in K4)
    Tc = [[float(x) for x in row] for row in np.asarray(Tc, np.float64).reshape(3, 4)]
    Tr = [[float(x) for x in row] for row in np.asarray(Tr, np.float64).reshape(3, 4)]
    d = [Tc[k][3] - Tr[k][3] for k in range(3)]
    o = [(Tr[0][i] * d[0] + Tr[1][i] * d[1]) + Tr[2][i] * d[2] for i in range(3)]
    return F(fx * o[0] + cx * o[2]), F(fy * o[1] + cy * o[2]), F(o[2])


def structure_tensor(ref, u, v, win):
    """(Sxx, Sxy, Syy) of the win x win window at (u, v) of the integer image `ref` as Python integers, central differences; None
    when the window's one-pixel ring leaves the image."""
    H, W = ref.shape
    r = win // 2
    if u - r - 1 < 0 or v - r - 1 < 0 or u + r + 1 > W - 1 or v + r + 1 > H - 1:
        return None
    I = np.asarray(ref).astype(np.int64)
    gx = I[v - r:v + r + 1, u - r + 1:u + r + 2] - I[v - r:v + r + 1, u - r - 1:u + r]
    gy = I[v - r + 1:v + r + 2, u - r:u + r + 1] - I[v - r - 1:v + r, u - r:u + r + 1]
    return int((gx * gx).sum()), int((gx * gy).sum()), int((gy * gy).sum())


def quantities(E, u, v, S, win, min_grad):
    """(Q, thr N) of the decision: float32, every operation rounded on its own, in the kernel's order."""
    E0, E1, E2 = (F(x) for x in E)
    with np.errstate(all="ignore"):
        dx, dy = E0 - F(u) * E2, E1 - F(v) * E2
        Q = ((dx * dx) * F(S[0]) + (F(2.0) * (dx * dy)) * F(S[1])) + (dy * dy) * F(S[2])
        N = dx * dx + dy * dy
        g = F(min_grad)
        thr = (F(4.0) * F(win * win)) * (g * g)
        return Q, thr * N


def passes(E, u, v, S, win, min_grad):
    """The decision: Q >= thr N (a NaN on either side refuses)."""
    Q, T = quantities(E, u, v, S, win, min_grad)
    return bool(Q >= T)


# ---------------------------------------------------------------- float64 side ----

def epipole64(K4, Tc, Tr):
    """The epipole from 4x4 poses in float64: K [I|0] T_world_ref^-1 (centre of the current camera)."""
    fx, fy, cx, cy = (float(x) for x in K4)
    M = lambda T: np.vstack([np.asarray(T, np.float64).reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])  # noqa: E731
    o = (np.linalg.inv(M(Tr)) @ M(Tc))[:3, 3]
    return np.array([fx * o[0] + cx * o[2], fy * o[1] + cy * o[2], o[2]])


def quantities64(E, u, v, S, win, min_grad):
    """(Q, thr N, sum of the absolute terms of Q - thr N) in float64 with the exact integers."""
    dx, dy = E[0] - u * E[2], E[1] - v * E[2]
    terms = [dx * dx * S[0], 2.0 * dx * dy * S[1], dy * dy * S[2]]
    thr = 4.0 * win * win * float(min_grad) ** 2
    tn = [thr * dx * dx, thr * dy * dy]
    return sum(terms), sum(tn), sum(abs(t) for t in terms + tn)


# ---------------------------------------------------------------- scenes ----

STRIPE_LO, STRIPE_HI = 70, 185


def striped_texture(along, seed=5, line_seed=11, half=True):
    """fe_zm_scenes.texture(seed) with the columns of its right half (`half=False`: all of them) replaced by stripes constant along
    texture axis `along` ("x": every row one grey; "y": every column one grey) -- a 1-D random line in [STRIPE_LO, STRIPE_HI]."""
    tex = ZS.texture(seed).copy()
    line = np.random.default_rng(line_seed).integers(STRIPE_LO, STRIPE_HI + 1, ZS.TEX_SIZE).astype(np.float64)
    c0 = ZS.TEX_SIZE // 2 if half else 0
    if along == "x":
        tex[:, c0:] = line[:, None]
    else:
        tex[:, c0:] = line[None, c0:]
    return tex


_cache = {}


def _frames(key, tex, poses):
    if key not in _cache:
        out = []
        for T in poses:
            img = ZS.render(T, tex).astype(np.uint8)
            img.setflags(write=False)
            out.append((img, T))
        _cache[key] = out
    return _cache[key]


HALF_STRIPED = {"sideways": "x", "vertical": "y"}  # scene -> the texture axis its camera moves along


def half_striped(name, frames=SC.FRAMES):
    """[(image, T_world_cam)]: frontend_scenes' `name` on the texture whose right half is stripes along the camera's motion."""
    return _frames(("half", name, frames), striped_texture(HALF_STRIPED[name]), [SC.scene_pose(name, k) for k in range(frames)])


def rolled(along, frames=4):
    """The direction case: the pose frame at the identity, the later frames rolled by pi / 2 about the optical axis and translated
    along world x, on a texture that is ALL stripes constant along `along`.  The epipolar lines run along x in the reference image
    and along y in the current one."""
    poses = [np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)]
    for k in range(1, frames):
        poses.append(np.concatenate([SC.rotation(0.0, 0.0, math.pi / 2), np.array([[0.03 * k], [0.0], [0.0]])], axis=1))
    return _frames(("rolled", along, frames), striped_texture(along, half=False), poses)


MARGIN_W, MARGIN_H = 48, 36
MARGIN_K = np.array([140, 0, 23.5, 0, 140, 17.5, 0, 0, 1], np.float32)


def margin_scene():
    """frontend_ref.shift_scene at 48 x 36 with the largest gradient of its cell put at (W - 3, 18): the detector's margin at win 3,
    one pixel short of the ring at win 5.  Returns (pose-frame image, second image, the two poses)."""
    a, b = R.shift_scene(3, 4, W=MARGIN_W, H=MARGIN_H)
    img = a[0].copy()
    img[18, MARGIN_W - 4], img[18, MARGIN_W - 2] = 0, 255
    return img, b[0], a[1], b[1]


def run(frames, poseframes=(0,), min_grad=0.0, zero_mean=False, **kw):
    """The restatement over a scene; returns (ref, per-frame outputs, per-frame decisions)."""
    fe = R.FrontEndRef(ZS.W, ZS.H, ZS.K, 256, 4)
    fe.set_ref_grad(min_grad)
    if zero_mean:
        fe.set_cost(True)
    p = R.params(**kw)
    outs, dec = [], []
    for k, (img, T) in enumerate(frames):
        outs.append(fe.track(p, img, k, T, k in poseframes))
        dec.append(list(fe.decisions))
    return fe, outs, dec
