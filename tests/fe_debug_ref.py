"""The feature front end's search record and its two debug images (DESIGN.md 5.3 "Debug images"; include/flame_hip.h,
flame_hip_frontend_searches / _debug_image) restated in NumPy.  A helper, not a test: tests/test_fe_debug_ref.py checks it
against hand-written bytes, the GPU tests compare the library with it byte for byte.

`DebugRef` is tests/frontend_ref.py's FrontEndRef plus the record: `steps` is zeroed every frame and `seg` = {x0, y0, ex, ey}
is recomputed -- in the restatement's float32 operation order -- from the state each searching slot had BEFORE the frame.  Both are zero
for a slot that ran no search and for a slot a NEW feature took in this frame.  draw_matches / draw_detections draw the two
pictures by the statement from (image, status, kstar, seg, steps) and from the emitted list."""
import numpy as np

from tests import frontend_ref as R

F = np.float32
IMG_DETECTIONS, IMG_MATCHES = 0, 1
GREEN, RED, YELLOW, BLUE = (0, 255, 0), (0, 0, 255), (0, 255, 255), (255, 0, 0)  # (B, G, R)
DRAWS = (R.OK, R.OUTSIDE, R.BAD_MATCH, R.AMBIGUOUS, R.DIED)


class DebugRef(R.FrontEndRef):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.seg = np.zeros((self.F, 4), np.float32)
        self.image = None   # the image the last track() tracked
        self.emitted = None  # what the last track() returned

    def _segment(self, p, u, v, f, mu, var, poses):
        """{x0, y0, ex, ey} of the search FrontEndRef._track_one runs from this state (the same operations in the same order)."""
        fx, fy, cx, cy = self.K4
        A, c = poses[f]
        b0, b1 = (F(u) - cx) / fx, (F(v) - cy) / fy
        a0 = (A[0][0] * b0 + A[0][1] * b1) + A[0][2]
        a1 = (A[1][0] * b0 + A[1][1] * b1) + A[1][2]
        a2 = (A[2][0] * b0 + A[2][1] * b1) + A[2][2]
        c0, c1, c2 = c
        two = F(2.0) * np.sqrt(var)
        lo, hi = mu - two, mu + two
        idmin, idmax = F(p["idepth_min"]), F(p["idepth_max"])
        xi0 = lo if lo > idmin else idmin
        xi1 = hi if hi < idmax else idmax
        d0, d1 = a2 + xi0 * c2, a2 + xi1 * c2
        x0, y0 = (a0 + xi0 * c0) / d0, (a1 + xi0 * c1) / d0
        x1, y1 = (a0 + xi1 * c0) / d1, (a1 + xi1 * c1) / d1
        dx, dy = x1 - x0, y1 - y0
        L = np.sqrt(dx * dx + dy * dy)
        S = R.MAX_SAMPLES if L >= F(R.MAX_SAMPLES) else int(np.ceil(L))
        return (x0, y0, dx / F(S), dy / F(S)), S

    def _track_one(self, s, p, cur, poses):
        pre = (int(self.u[s]), int(self.v[s]), int(self.pf[s]), self.mu[s], self.var[s])
        res = super()._track_one(s, p, cur, poses)
        if self.steps[s] > 0:  # (zeroed before the frame: the base class ran a search for this slot)
            seg, S = self._segment(p, *pre, poses)
            assert S == self.steps[s]
            self.seg[s] = seg
        return res

    def track(self, p, img, img_id, T_world_cam, is_poseframe):
        self.steps[:] = 0
        self.seg[:] = 0
        out = super().track(p, img, img_id, T_world_cam, is_poseframe)
        new = self.status == R.NEW  # (a slot that died in this frame and was taken by a detection: its search goes with it)
        self.steps[new] = 0
        self.seg[new] = 0
        self.image = np.ascontiguousarray(img, np.uint8).copy()
        self.emitted = out
        return out

    def searches(self):
        return dict(seg=self.seg.copy(), steps=self.steps.copy())

    def debug_image(self, kind):
        if kind == IMG_MATCHES:
            return draw_matches(self.image, self.status, self.kstar, self.seg, self.steps)
        return draw_detections(self.image, self.emitted["vtx"], self.emitted["status"])


def background(image):
    image = np.asarray(image, np.uint8)
    return np.repeat(image[:, :, None], 3, axis=2)


def sample_pixels(seg, ks, W, H):
    """The pixels (X, Y) of the samples `ks` of a segment that are drawn: float32, every operation rounded on its own; the range
    test runs on the float values (NaN and infinities fail it)."""
    x0, y0, ex, ey = (F(a) for a in seg)
    k = np.asarray(ks, np.float32)
    with np.errstate(all="ignore"):
        px = x0 + k * ex
        py = y0 + k * ey
        X, Y = np.floor(px + F(0.5)), np.floor(py + F(0.5))
        ok = (X >= 0) & (X <= F(W - 1)) & (Y >= 0) & (Y <= F(H - 1))
    return X[ok].astype(np.int64), Y[ok].astype(np.int64)


def draw_matches(image, status, kstar, seg, steps):
    out = background(image)
    H, W = out.shape[:2]
    layer = np.zeros((H, W), np.int32)
    for s in range(len(status)):
        S, st = int(steps[s]), int(status[s])
        if S <= 0 or st not in DRAWS:
            continue
        X, Y = sample_pixels(seg[s], np.arange(S + 1), W, H)
        np.maximum.at(layer, (Y, X), 1 if st == R.OK else 2)
        if st == R.OK and 0 <= int(kstar[s]) <= S:
            X, Y = sample_pixels(seg[s], [int(kstar[s])], W, H)
            np.maximum.at(layer, (Y, X), 3)
    for l, colour in ((1, GREEN), (2, RED), (3, YELLOW)):
        out[layer == l] = colour
    return out


def draw_detections(image, vtx, status):
    out = background(image)
    H, W = out.shape[:2]
    layer = np.zeros((H, W), np.int32)
    for (x, y), st in zip(np.asarray(vtx, np.float32).reshape(-1, 2), status):
        with np.errstate(all="ignore"):
            X, Y = np.floor(x + F(0.5)), np.floor(y + F(0.5))
        if not (X >= -1 and X <= W and Y >= -1 and Y <= H):  # no pixel of the square is inside (or not a number)
            continue
        X, Y = int(X), int(Y)
        x0, x1, y0, y1 = max(X - 1, 0), min(X + 1, W - 1), max(Y - 1, 0), min(Y + 1, H - 1)
        if x0 <= x1 and y0 <= y1:
            sub = layer[y0:y1 + 1, x0:x1 + 1]
            np.maximum(sub, 2 if int(st) == R.NEW else 1, out=sub)
    out[layer == 1] = BLUE
    out[layer == 2] = GREEN
    return out
