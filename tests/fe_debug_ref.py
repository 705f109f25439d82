"""The feature front end's search record and its two debug images (DESIGN.md 5.3 "Debug images"; include/flame_hip.h,
flame_hip_frontend_searches / _debug_image) restated in NumPy.  A helper, not a test: tests/test_fe_debug_ref.py checks it
against hand-written bytes, the GPU tests compare the library with it byte for byte.

tests/frontend_ref.py's FrontEndRef keeps the record: `steps` and `seg` = {x0, y0, ex, ey} of every slot that ran a search in the
frame, zero for a slot that ran none and for a slot a NEW feature took in this frame.  draw_matches / draw_detections draw the two
pictures by the statement from (image, status, kstar, seg, steps) and from the emitted list."""
import numpy as np

from tests import frontend_ref as R

F = np.float32
IMG_DETECTIONS, IMG_MATCHES = 0, 1
GREEN, RED, YELLOW, BLUE = (0, 255, 0), (0, 0, 255), (0, 255, 255), (255, 0, 0)  # (B, G, R)
DRAWS = (R.OK, R.OUTSIDE, R.BAD_MATCH, R.AMBIGUOUS, R.DIED)


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
