"""The feature front end's reference-patch gradient gate (DESIGN.md 5.3 "Reference-patch gradient"; include/flame_hip.h,
flame_hip_frontend_set_ref_grad) restated in NumPy on top of tests/frontend_ref.py.  A helper, not a test: tests/test_fe_rg_ref.py
checks it rule by rule on hand-written windows, against float64 geometry and against ground truth, tests/test_gpu_fe_rg.py compares
the library with it bit for bit.

`RgRef` is FrontEndRef plus `set_ref_grad`.  With the gate off (min_grad 0) every call goes to the base class untouched.  With it on
`_track_one` repeats the base class's tests up to NO_PARALLAX -- the same float32 operations in the same order -- and, for a
feature that would now be searched, forms
  * the epipole of the current view in the feature's pose frame, E = K R_ref^T (t_cur - t_ref), in double, rounded once to float32,
  * the integer structure tensor (Sxx, Sxy, Syy) of central differences over the win x win reference window,
  * Q = ((dx dx) Sxx + (2 (dx dy)) Sxy) + (dy dy) Syy, N = dx dx + dy dy, thr = (4 n) (g g) with (dx, dy) = (E0 - u E2, E1 - v E2),
and lets the base class (or whichever class follows in the MRO: the ZSSD search) run the search iff Q >= thr N.  A refused feature
takes the failure path of the base class with status REF_GRAD and no search; a window whose one-pixel ring leaves the image takes
it with OUTSIDE.  `RgDebugRef` / `RgZmDebugRef` / `RgGatesDebugRef` / `RgZmGatesDebugRef` add fe_debug_ref.DebugRef's search record
and pictures, fe_zm_ref.ZmRef's cost and fe_gates_ref.GatesRef's gates for the GPU comparison.

Also the scenes of the gate: the plane and the poses of tests/frontend_scenes.py under tests/fe_zm_scenes.py's renderer, with a
texture whose right half (or all of it) is stripes -- a 1-D random line in [70, 185], constant along one texture axis; the
renderer's bilinear taps interpolate it linearly."""
import math

import numpy as np

from tests import fe_debug_ref as D
from tests import fe_gates_ref as G
from tests import fe_zm_ref as Z
from tests import fe_zm_scenes as ZS
from tests import frontend_ref as R
from tests import frontend_scenes as SC

F = np.float32
REF_GRAD = 7
FAILED = G.FAILED + (REF_GRAD,)


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


class RgRef(R.FrontEndRef):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.min_epi_grad = F(0.0)
        self._T_cur = None
        self._epi = {}
        self.decisions = []  # (slot, u, v, pose frame's T_world_ref, E, S, passed) of every test of the frame, for the tests

    def set_ref_grad(self, min_grad):
        g = F(min_grad)
        if not np.isfinite(g):
            raise ValueError("non-finite min_grad")
        if g < 0:
            raise ValueError("negative min_grad")
        self.min_epi_grad = g

    def _rg_begin(self, T_world_cam):
        self._T_cur = np.asarray(T_world_cam, np.float64).reshape(3, 4).copy()
        self._epi = {}
        self.decisions = []

    def track(self, p, img, img_id, T_world_cam, is_poseframe):
        self._rg_begin(T_world_cam)
        return super().track(p, img, img_id, T_world_cam, is_poseframe)

    def _epipole(self, f):
        if f not in self._epi:
            self._epi[f] = epipole_record(self.K4, self._T_cur, self.pf_T[f])
        return self._epi[f]

    def _warp(self, s, poses):
        fx, fy, cx, cy = self.K4
        u, v, f = int(self.u[s]), int(self.v[s]), int(self.pf[s])
        A, c = poses[f]
        b0, b1 = (F(u) - cx) / fx, (F(v) - cy) / fy
        a0 = (A[0][0] * b0 + A[0][1] * b1) + A[0][2]
        a1 = (A[1][0] * b0 + A[1][1] * b1) + A[1][2]
        a2 = (A[2][0] * b0 + A[2][1] * b1) + A[2][2]
        return a0, a1, a2, c[0], c[1], c[2]

    def _reaches_search(self, s, p, poses):
        """FrontEndRef._track_one's tests before the search: neither OUTSIDE nor NO_PARALLAX."""
        W, H, win = self.W, self.H, p["win_size"]
        u, v = int(self.u[s]), int(self.v[s])
        mu, var = self.mu[s], self.var[s]
        a0, a1, a2, c0, c1, c2 = self._warp(s, poses)
        two = F(2.0) * np.sqrt(var)
        lo, hi = mu - two, mu + two
        idmin, idmax = F(p["idepth_min"]), F(p["idepth_max"])
        xi0 = lo if lo > idmin else idmin
        xi1 = hi if hi < idmax else idmax
        d0, d1 = a2 + xi0 * c2, a2 + xi1 * c2
        r = win // 2
        ref_in = u - r >= 0 and v - r >= 0 and u + r <= W - 1 and v + r <= H - 1
        if not (d0 > 0 and d1 > 0) or not ref_in:
            return False
        x0, y0 = (a0 + xi0 * c0) / d0, (a1 + xi0 * c1) / d0
        x1, y1 = (a0 + xi1 * c0) / d1, (a1 + xi1 * c1) / d1
        dx, dy = x1 - x0, y1 - y0
        L = np.sqrt(dx * dx + dy * dy)
        return bool(L >= F(2.0))

    def _fail(self, s, p, poses, status):
        """FrontEndRef._track_one behind a failed status that ran no search: prior and k* = -1 untouched, the projection of the
        prior, one dropout, death past max_dropouts."""
        W, H = self.W, self.H
        mu, var, drop = self.mu[s], self.var[s], int(self.drop[s])
        a0, a1, a2, c0, c1, c2 = self._warp(s, poses)
        w0, w1, w2 = a0 + mu * c0, a1 + mu * c1, a2 + mu * c2
        pok, proj = False, None
        if w2 > 0:
            px, py, xc = w0 / w2, w1 / w2, mu / w2
            g = a2 / (w2 * w2)
            vc = var * (g * g)
            pok = bool(px >= 0 and px <= F(W - 1) and py >= 0 and py <= F(H - 1) and np.isfinite(xc) and np.isfinite(vc) and vc >= 0)
            proj = (px, py, xc, vc)
        drop += 1
        self.drop[s], self.kstar[s] = drop, -1
        self.counts[status] = self.counts.get(status, 0) + 1
        if drop > p["max_dropouts"]:
            self.alive[s], self.status[s] = 0, R.DIED
            self.counts[R.DIED] = self.counts.get(R.DIED, 0) + 1
            return None
        self.status[s] = status
        if not pok:
            return None
        dws = p["detection_win_size"]
        ncx = (W + dws - 1) // dws
        return (int(py) // dws) * ncx + int(px) // dws, proj

    def _track_one(self, s, p, cur, poses):
        if not self.min_epi_grad > 0 or not self._reaches_search(s, p, poses):
            return super()._track_one(s, p, cur, poses)
        u, v, f = int(self.u[s]), int(self.v[s]), int(self.pf[s])
        S = structure_tensor(self.pf_img[f], u, v, p["win_size"])
        if S is None:
            return self._fail(s, p, poses, R.OUTSIDE)
        E = self._epipole(f)
        ok = passes(E, u, v, S, p["win_size"], self.min_epi_grad)
        self.decisions.append((s, u, v, self.pf_T[f], E, S, ok))
        if ok:
            return super()._track_one(s, p, cur, poses)
        return self._fail(s, p, poses, REF_GRAD)


class RgGatesRef(G.GatesRef, RgRef):
    """GatesRef over RgRef.  GatesRef's own frame (a gate set) does not pass through RgRef.track, and its letterbox rule reads
    "failed" from the three statuses it knows: both are restated here with REF_GRAD among the failures."""

    def track(self, p, img, img_id, T_world_cam, is_poseframe):
        self._rg_begin(T_world_cam)
        return super().track(p, img, img_id, T_world_cam, is_poseframe)

    def _track_one(self, s, p, cur, poses):
        g = self._g
        res = super(G.GatesRef, self)._track_one(s, p, cur, poses)  # (the class behind GatesRef: RgRef, then the search)
        if g is None:
            return res
        pok, px, py, xc, vc = self._projection(s, poses)
        if res is not None:
            want = np.array([px, py, xc, vc], np.float32).view(np.uint32)
            assert pok and np.array_equal(np.array(res[1], np.float32).view(np.uint32), want)
        if not pok:
            return None
        self.proj_all[s] = (px, py, xc, vc)
        if not (py >= F(g["y_lo"]) and py <= F(g["y_hi"] - 1)):
            self.refused += 1
            if res is None:
                return None
            if int(self.status[s]) not in FAILED:
                self.drop[s] += 1
                if self.drop[s] > p["max_dropouts"]:
                    self.alive[s], self.status[s] = 0, R.DIED
                    self.counts[R.DIED] = self.counts.get(R.DIED, 0) + 1
            return None
        if res is None:
            return None
        if g["height"]:
            h = G.height32(self.K4, g["hr"], g["h0"], px, py, xc)
            if not (h >= g["min_height"] and h <= g["max_height"]):
                self.held += 1
                self.held_slots.append(s)
                self._held_cells.add(res[0])
                return None
        return res


class RgDebugRef(D.DebugRef, RgRef):
    """RgRef with DebugRef's search record and pictures (a refused slot leaves steps = 0 and draws nothing)."""


class RgZmDebugRef(D.DebugRef, RgRef, Z.ZmRef):
    """... over the ZSSD search: the gate does not look at the cost."""


class RgGatesDebugRef(D.DebugRef, RgGatesRef):
    """... with both gates behind it."""


class RgZmGatesDebugRef(D.DebugRef, RgGatesRef, Z.ZmRef):
    """... and all three."""


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


def run(frames, poseframes=(0,), min_grad=0.0, ref=None, zero_mean=False, **kw):
    """The restatement over a scene; returns (ref, per-frame outputs, per-frame decisions)."""
    fe = (ref or RgRef)(ZS.W, ZS.H, ZS.K, 256, 4)
    fe.set_ref_grad(min_grad)
    if zero_mean:
        fe.set_cost(True)
    p = R.params(**kw)
    outs, dec = [], []
    for k, (img, T) in enumerate(frames):
        outs.append(fe.track(p, img, k, T, k in poseframes))
        dec.append(list(fe.decisions))
    return fe, outs, dec
