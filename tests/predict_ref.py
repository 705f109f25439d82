"""NumPy restatement of the prediction stage (kernels: flame_ros_amd/csrc/predict.hip): the previous frame's
mesh warped into the current view, z-buffered, and read at the query pixels.  float32 with + - x / floor ceil only, every
operation rounded on its own, sums left to right -- operation by operation what the kernels do, so the GPU equals it bit for
bit.  The z-buffer is a plain maximum over the same 64-bit keys."""
import numpy as np

from tests.frontend_ref import pose_record  # A = K R, c = K t of T_cur_prev: the one routine the front end's pose table uses too

F = np.float32
NAN = np.float32(np.nan)  # 0x7fc00000, what the kernels write
EMPTY = np.uint64(0)


def e_fn(ax, ay, bx, by, px, py):
    """e(a, b, p) = (bx - ax) (py - ay) - (by - ay) (px - ax)"""
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def edge_w(ax, ay, bx, by, px, py):
    """The dense raster's watertight rule on e(): evaluated from the edge's lexicographically smaller end point."""
    if ax < bx or (ax == bx and ay < by):
        return e_fn(ax, ay, bx, by, px, py)
    return -e_fn(bx, by, ax, ay, px, py)


def interp(a, b, c, px, py):
    """(idepth, inside) of the point(s) (px, py) in the warped triangle a, b, c (each x, y, idepth as float32 scalars)."""
    wa = edge_w(b[0], b[1], c[0], c[1], px, py)
    wb = edge_w(c[0], c[1], a[0], a[1], px, py)
    wc = edge_w(a[0], a[1], b[0], b[1], px, py)
    inside = ((wa >= 0) & (wb >= 0) & (wc >= 0)) | ((wa <= 0) & (wb <= 0) & (wc <= 0))
    xi = ((wa * a[2] + wb * b[2]) + wc * c[2]) / ((wa + wb) + wc)
    return xi, inside


def raster_span(lo, hi, n):
    """The dense raster's bounding box along one axis of n pixels (clamped in float before the conversion)."""
    i0 = max(int(np.ceil(np.fmin(np.fmax(lo, F(-1.0)), F(n)))), 0)
    i1 = min(int(np.floor(np.fmin(np.fmax(hi, F(-1.0)), F(n)))), n - 1)
    return i0, i1


def project(K4, A, c, pos, x):
    """Step 1: (V, 4) float32 {warped pixel x, y, idepth in the current frame, ok}; zeros where not ok."""
    fx, fy, cx, cy = (F(k) for k in K4)
    pos = np.asarray(pos, F).reshape(-1, 2)
    x = np.asarray(x, F)
    b0, b1 = (pos[:, 0] - cx) / fx, (pos[:, 1] - cy) / fy
    w = [((A[r][0] * b0 + A[r][1] * b1) + A[r][2]) + x * c[r] for r in range(3)]
    ok = np.isfinite(x) & (x > 0) & (w[2] > 0) & np.isfinite(w[0]) & np.isfinite(w[1]) & np.isfinite(w[2])
    out = np.zeros((len(x), 4), F)
    out[ok, 0] = w[0][ok] / w[2][ok]
    out[ok, 1] = w[1][ok] / w[2][ok]
    out[ok, 2] = x[ok] / w[2][ok]
    out[ok, 3] = 1
    return out


def zbuffer(W, H, pos, proj, tris, tri_valid):
    """Step 2: (H, W) uint64 keys, bits(idepth) << 32 | 0xFFFFFFFF - t of the nearest surface; 0 = empty."""
    pos = np.asarray(pos, F).reshape(-1, 2)
    key = np.zeros((H, W), np.uint64)
    for t, (ia, ib, ic) in enumerate(np.asarray(tris).reshape(-1, 3)):
        if not tri_valid[t]:
            continue
        a, b, c = proj[ia], proj[ib], proj[ic]
        if a[3] == 0 or b[3] == 0 or c[3] == 0:
            continue
        Pa, Pb, Pc = pos[ia], pos[ib], pos[ic]
        area_prev = e_fn(Pa[0], Pa[1], Pb[0], Pb[1], Pc[0], Pc[1])
        area_cur = e_fn(a[0], a[1], b[0], b[1], c[0], c[1])
        if not ((area_prev > 0 and area_cur > 0) or (area_prev < 0 and area_cur < 0)):
            continue
        x0, x1 = raster_span(min(a[0], b[0], c[0]), max(a[0], b[0], c[0]), W)
        y0, y1 = raster_span(min(a[1], b[1], c[1]), max(a[1], b[1], c[1]), H)
        if x1 < x0 or y1 < y0:
            continue
        py, px = np.meshgrid(np.arange(y0, y1 + 1).astype(F), np.arange(x0, x1 + 1).astype(F), indexing="ij")
        xi, inside = interp(a, b, c, px, py)
        take = inside & np.isfinite(xi) & (xi > 0)
        k = (xi.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(0xFFFFFFFF - t)
        sub = key[y0:y1 + 1, x0:x1 + 1]
        np.maximum(sub, np.where(take, k, EMPTY), out=sub)
    return key


def sample(W, H, key, proj, tris, pix):
    """Step 3: the prediction at every query pixel (float, current frame), NaN = none."""
    pix = np.asarray(pix, F).reshape(-1, 2)
    tris = np.asarray(tris).reshape(-1, 3)
    out = np.full(len(pix), NAN, F)
    for q, (x, y) in enumerate(pix):
        fj, fi = np.floor(x + F(0.5)), np.floor(y + F(0.5))
        if not (fj >= 0 and fj < F(W) and fi >= 0 and fi < F(H)):
            continue
        k = int(key[int(fi), int(fj)])
        if k == 0:
            continue
        t = 0xFFFFFFFF - (k & 0xFFFFFFFF)
        xi, _ = interp(proj[tris[t, 0]], proj[tris[t, 1]], proj[tris[t, 2]], x, y)
        if np.isfinite(xi) and xi > 0:
            out[q] = xi
    return out


def dense_map(key):
    """The high word of a non-empty key as float, NaN where empty."""
    m = (key >> np.uint64(32)).astype(np.uint32).view(F).copy()
    m[key == EMPTY] = NAN
    return m


def predict(K4, W, H, T_world_prev, T_world_cur, pos, x, tris, tri_valid, pix):
    """The whole stage: (prediction[n], dense map[H, W], keys[H, W])."""
    with np.errstate(all="ignore"):
        A, c = pose_record(K4, T_world_cur, T_world_prev)
        proj = project(K4, A, c, pos, x)
        key = zbuffer(W, H, pos, proj, tris, tri_valid)
        pred = sample(W, H, key, proj, tris, pix)
    return pred, dense_map(key), key
