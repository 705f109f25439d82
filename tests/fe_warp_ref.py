"""The feature front end's warped matching window (DESIGN.md 5.3 "Warped window"; include/flame_hip.h, flame_hip_frontend_set_warp)
restated in NumPy: the rules tests/frontend_ref.py's FrontEndRef applies after `set_warp`.  A helper, not a test:
tests/test_fe_warp_ref.py checks it on hand-written windows, rule by rule, against float64 geometry and against ground truth,
tests/test_gpu_fe_warp.py compares the library with it bit for bit.

With the switch on a feature that has passed the NO_PARALLAX test (and the gradient gate, which is tested first) forms
  * xi_J = the prior clamped into the searched interval, w = a + xi_J c, (px, py) = (w0, w1) / w2,
  * J = ((gx0 - px gx2, gy0 - px gy2), (gx1 - py gx2, gy1 - py gy2)) / w2 with gx_r = A[r][0] / fx, gy_r = A[r][1] / fy,
  * Jq = floor(256 J + 0.5) per entry, refused unless that float is finite and at most 1024 in magnitude, and unless
    det Jq >= 4096.
A refused feature fails with status OUTSIDE and no search, and is counted in counts["warp_refused"].  Otherwise the search runs and
every cost it asks for is `warped_windows` under the cost's own integer rule (`warped_cost`)."""
import numpy as np

from tests import fe_gi_ref as GI
from tests import fe_zm_ref as Z
from tests import frontend_ref as R

F = np.float32
IDENTITY = (256, 0, 0, 256)
QUARTER_TURN = (0, -256, 256, 0)
JQ_MAX, DET_MIN = 1024, 4096


def jacobian32(K4, A, c, a, mu, xi0, xi1):
    """(J00, J01, J10, J11, xi_J) in float32, every operation rounded on its own, in the kernel's order."""
    fx, fy = K4[0], K4[1]
    a0, a1, a2 = a
    with np.errstate(all="ignore"):
        t = mu if mu > xi0 else xi0
        xj = t if t < xi1 else xi1
        w0, w1, w2 = a0 + xj * c[0], a1 + xj * c[1], a2 + xj * c[2]
        px, py = w0 / w2, w1 / w2
        gx0, gx1, gx2 = A[0][0] / fx, A[1][0] / fx, A[2][0] / fx
        gy0, gy1, gy2 = A[0][1] / fy, A[1][1] / fy, A[2][1] / fy
        return ((gx0 - px * gx2) / w2, (gy0 - px * gy2) / w2, (gx1 - py * gx2) / w2, (gy1 - py * gy2) / w2, xj)


def quantise(J):
    """Jq of four float32 entries, or None when the map is refused."""
    q = []
    with np.errstate(all="ignore"):
        for x in J:
            fq = np.floor(F(x) * F(256.0) + F(0.5))
            if not abs(fq) <= F(JQ_MAX):  # (a NaN fails, an infinity fails)
                return None
            q.append(int(fq))
    if q[0] * q[3] - q[1] * q[2] < DET_MIN:
        return None
    return tuple(q)


def offsets(Jq, r):
    """(dx, dy): the offsets in sixteenths of a pixel of the window positions, arrays [j + r, i + r] (i along x, j along y)."""
    j, i = np.mgrid[-r:r + 1, -r:r + 1].astype(np.int64)
    return (Jq[0] * i + Jq[1] * j + 8) >> 4, (Jq[2] * i + Jq[3] * j + 8) >> 4  # (NumPy's >> on signed integers floors)


def warped_windows(cur, ref, u, v, px, py, win, Jq, W, H):
    """(I, R) of the sample at (px, py) under Jq -- I the 256-scaled bilinear sums of `cur` at the warped positions, R = 256 x the
    reference window, both [j + r, i + r] -- or None when the sample is invalid."""
    r = win // 2
    with np.errstate(all="ignore"):
        fqx, fqy = np.floor(px * F(16.0) + F(0.5)), np.floor(py * F(16.0) + F(0.5))
    if not (fqx >= 0 and fqx <= F(16 * W) and fqy >= 0 and fqy <= F(16 * H)):
        return None
    dx, dy = offsets(Jq, r)
    ox, oy = int(fqx) + dx, int(fqy) + dy
    X, Y = ox >> 4, oy >> 4
    if X.min() < 0 or Y.min() < 0 or X.max() + 1 > W - 1 or Y.max() + 1 > H - 1:  # every window pixel and its +1 neighbours
        return None
    wx1, wy1 = ox & 15, oy & 15
    wx0, wy0 = 16 - wx1, 16 - wy1
    c = np.asarray(cur).astype(np.int64)
    Iw = (wx0 * wy0) * c[Y, X] + (wx1 * wy0) * c[Y, X + 1] + (wx0 * wy1) * c[Y + 1, X] + (wx1 * wy1) * c[Y + 1, X + 1]
    return Iw, 256 * np.asarray(ref)[v - r:v + r + 1, u - r:u + r + 1].astype(np.int64)


def warped_cost(Iw, Rw, cost):
    """The three costs on a window (warped or upright): "ssd", "zssd", "gi"."""
    if cost == "gi":
        return GI.gi_cost(Iw, Rw)[0]
    Dm = Iw - Rw
    return Z.zssd(Dm) if cost == "zssd" else int(sum(int(x) * int(x) for x in Dm.reshape(-1)))


def run(frames, W, H, K, warp=True, cost="ssd", poseframes=(0,), **kw):
    """The restatement over a scene; returns (ref, per-frame outputs)."""
    fe = R.FrontEndRef(W, H, K, 256, 4)
    fe.set_warp(warp)
    fe.set_cost(cost == "zssd")
    fe.set_gain_invariant(cost == "gi")
    p = R.params(**kw)
    outs = []
    for k, (img, T) in enumerate(frames):
        fe.maps = []
        outs.append(fe.track(p, img, k, T, k in poseframes))
    return fe, outs


# ---------------------------------------------------------------- float64 side ----

def project64(K4, Tc, Tr, u, v, xi):
    """Pixel in the camera at T_world_cam = Tc of the point at reference pixel (u, v), inverse depth xi, of the camera at Tr."""
    fx, fy, cx, cy = (float(x) for x in K4)
    M = lambda T: np.vstack([np.asarray(T, np.float64).reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])  # noqa: E731
    Tcr = np.linalg.inv(M(Tc)) @ M(Tr)
    X = Tcr[:3, :3] @ np.array([(u - cx) / fx, (v - cy) / fy, 1.0]) + xi * Tcr[:3, 3]
    return np.array([fx * X[0] / X[2] + cx, fy * X[1] / X[2] + cy])


def jacobian64(K4, Tc, Tr, u, v, xi, h=1e-3):
    """(J00, J01, J10, J11) by central differences of project64 (step h px: the truncation is below 1e-8, the noise below 1e-9)."""
    du = (project64(K4, Tc, Tr, u + h, v, xi) - project64(K4, Tc, Tr, u - h, v, xi)) / (2 * h)
    dv = (project64(K4, Tc, Tr, u, v + h, xi) - project64(K4, Tc, Tr, u, v - h, xi)) / (2 * h)
    return np.array([du[0], dv[0], du[1], dv[1]])


class Err:
    """A value with a first-order bound on its absolute error: every operation propagates its operands' bounds exactly to first
    order and adds one rounding, 2^-24 of the result's magnitude.  Counts the rounding band of jacobian32."""
    EPS = 2.0 ** -24

    def __init__(self, v, e=0.0):
        self.v, self.e = float(v), float(e)

    @classmethod
    def rounded(cls, v):
        return cls(v, cls.EPS * abs(float(v)))

    def _op(self, v, e):
        return Err(v, e + Err.EPS * abs(v))

    def __add__(self, o):
        return self._op(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return self._op(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        return self._op(self.v * o.v, abs(self.v) * o.e + abs(o.v) * self.e)

    def __truediv__(self, o):
        return self._op(self.v / o.v, self.e / abs(o.v) + abs(self.v) * o.e / (o.v * o.v))


def jacobian_band(K4, A64, c64, u, v, xi):
    """The bounds of the four entries of jacobian32: A and c rounded once, K and (u, v) exact, xi_J taken as given."""
    fx, fy, cx, cy = (Err(float(x)) for x in K4)
    A = [[Err.rounded(x) for x in row] for row in A64]
    c = [Err.rounded(x) for x in c64]
    b0, b1 = (Err(u) - cx) / fx, (Err(v) - cy) / fy
    a = [(A[r][0] * b0 + A[r][1] * b1) + A[r][2] for r in range(3)]
    xj = Err(xi)
    w = [a[r] + xj * c[r] for r in range(3)]
    px, py = w[0] / w[2], w[1] / w[2]
    gx = [A[r][0] / fx for r in range(3)]
    gy = [A[r][1] / fy for r in range(3)]
    J = [(gx[0] - px * gx[2]) / w[2], (gy[0] - px * gy[2]) / w[2], (gx[1] - py * gx[2]) / w[2], (gy[1] - py * gy[2]) / w[2]]
    return np.array([x.e for x in J])
