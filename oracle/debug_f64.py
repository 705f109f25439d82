"""Independent statement of the four mesh debug images (WIREFRAME, FEATURES, NORMALS, IDEPTHMAP).

TEST INFRASTRUCTURE (see oracle/__init__.py), a sibling of frame_f64.py.  Written from the rule block above
nltgv2_coverage in nltgv2_oracle.c, NOT from its code, and in another shape: primitives write their index
into a key map (the largest index wins), colours are looked up afterwards per primitive, the colour map is
evaluated over whole arrays, pixels are decided with exact arithmetic, and the normals image takes its
owner from frame_f64.raster.

Float32 inputs are dyadic rationals.  A pixel of a coordinate is decided exactly (float64 holds a float32
value and its fractional part without rounding); Bresenham runs in Python integers without a guard; the
colour map is evaluated in float64, whose rounding (2^-53) is far inside the float32 band below, and in
exact rationals by jet_exact, which the tests hold the array version against.

Beside every channel value stands whether a correct float32 evaluation is CERTAIN to give it: the exact
value of 255 c + 0.5 lies outside the float32 error band around an integer, or every float32 operation on
the way is exact (dyadic inputs: the band is empty).  Inside the band the two neighbouring levels are both
right; lo / hi hold them.

Every function takes `rules`: the stated rules by default; the tests pass deliberately wrong ones (mutants)
to show that the corpus tells them apart.
"""
from fractions import Fraction

import numpy as np

from oracle import frame_f64 as F

U32 = F.U32
# ---- float32 error bands of the value y = 255 c + 0.5 whose floor is the channel (unit: 256 u, the rounding
# ---- of one operation whose result is below 256), derived from the operation counts:
# jet: p / 2 and 4 t are exact; then four rounded operations: 4t - k (below 4: error <= 2u), 1.5 - |.| (below 2:
#   <= u), so c errs by <= 3u, carried through * 255: 765 u; 255 * c (below 256: <= 128 u), + 0.5 (<= 128 u):
#   1021 u <= 4 * 256 u.
K_JET = 4
# normals: each edge function is four rounded operations (two differences, a product, the fma): |dw_k| <= 4u m_k;
#   the blend adds three (product, fma, fma): <= 3u sum |w_k|; over three components (sqrt 3 < 2):
#   |d num| <= K_BLEND u sum_k (m_k + |w_k|), and the direction errs by |d num| / |num|; the division by the
#   sum of the weights is common to the three components and cancels in the normalisation.
K_BLEND = 8
#   per channel afterwards: / s, the length (a common factor: fma, fma, sqrt <= 2.5u), / length, 0.5 n + 0.5,
#   * 255, + 0.5: 127.5 * 4.5u + 255 u + 128 u + 128 u = 1085 u <= 5 * 256 u.
K_CHAN = 5
BAND_JET = K_JET * 256 * U32


class Rules:
    """The stated rules; a mutant overrides one field."""
    rounding = "exact"   # "exact": half away from zero | "floor": floor(v + 0.5) | "f32": trunc(v +- 0.5f) in float32
    winner = "largest"   # the largest primitive index wins a pixel | "lowest"
    side_colour = "mean"  # jet(0.5 (x_a + x_b) scale) | "a": jet(x_a scale)
    reach = True         # sides with an end point out of reach are absent | False: the walk stops after 4 (W + H) steps
    tie = ">="           # Bresenham's x step: e2 >= dy | ">"
    blue_shift = 0       # the blue ramp moved by this many levels
    nan_colour = "top"   # NaN reads as the top of the scale | "black"
    normals_order = (2, 1, 0)  # B = n_z, G = n_y, R = n_x

    def __init__(self, **kw):
        for k, v in kw.items():
            assert hasattr(Rules, k), k
            setattr(self, k, v)


STATED = Rules()


# ---------------------------------------------------------------- pixel of a coordinate, reach
def pixel(v32, rules=STATED):
    """Round half away from zero, exactly: float64 array of integers (the caller has tested the reach)."""
    v32 = np.asarray(v32, np.float32)
    v = v32.astype(np.float64)
    if rules.rounding == "floor":
        return np.floor(v + 0.5)
    if rules.rounding == "f32":
        return np.trunc((v32 + np.where(v32 >= 0, np.float32(0.5), np.float32(-0.5)).astype(np.float32)).astype(np.float64))
    a = np.abs(v)
    whole = np.floor(a)
    return np.copysign(whole + (a - whole >= 0.5), v)   # a - whole is exact


def in_reach(c32, W, H):
    """-(float)R <= c <= (float)(2 R), R = W + H, compared in float32 (a NaN fails)."""
    c = np.asarray(c32, np.float32)
    R = W + H
    with np.errstate(invalid="ignore"):
        return (c >= -np.float32(R)) & (c <= np.float32(2 * R))


def feature_drawn(fp32, W, H):
    fp = np.asarray(fp32, np.float32).reshape(-1, 2)
    u, v = fp[:, 0], fp[:, 1]
    with np.errstate(invalid="ignore"):
        return (u > np.float32(-2)) & (u < np.float32(W + 1)) & (v > np.float32(-2)) & (v < np.float32(H + 1))


# ---------------------------------------------------------------- colour map
def jet_exact(p, rules=STATED):
    """jet(p, 0, 2) of one float32 product p in exact rationals: (B, G, R) levels."""
    p = float(np.float32(p))
    if np.isnan(p):
        if rules.nan_colour == "black":
            return (0, 0, 0)
        t = Fraction(1)
    elif np.isinf(p):
        t = Fraction(1 if p > 0 else 0)
    else:
        t = min(Fraction(1), max(Fraction(0), Fraction(p) / 2))
    out = []
    for k in (1, 2, 3):
        c = Fraction(3, 2) - abs(4 * t - k)
        if k == 1:
            c += Fraction(rules.blue_shift, 255)
        c = min(Fraction(1), max(Fraction(0), c))
        y = 255 * c + Fraction(1, 2)
        out.append(y.numerator // y.denominator)
    return tuple(out)


def _is32(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return a.astype(np.float32).astype(np.float64) == a


def jet(p32, rules=STATED):
    """jet(p, 0, 2) of float32 products: (lo[n,3], hi[n,3], certain[n]) in B, G, R order.  NaN and +inf read as
    the top of the scale (0, 0, 128), -inf and everything below 0 as the bottom (128, 0, 0), everything above
    2 as the top."""
    p = np.asarray(p32, np.float32).astype(np.float64).ravel()
    nan = np.isnan(p)
    # 0 < p < 2^-26: 4 t < 2^-25 is below half an ulp of every k, so any float32 evaluation of 4 t - k returns -k, the
    # value at p = 0; and the exact y lies above that of p = 0 by 1020 t < 1 at most, on the same level: the colour of 0
    with np.errstate(invalid="ignore"):
        p = np.where((p > 0) & (p < 2.0 ** -26), 0.0, p)
    with np.errstate(invalid="ignore"):
        t = np.where(nan, 1.0, np.clip(p / 2.0, 0.0, 1.0))
        clipped = nan | (p <= 0) | (p >= 2)
        exact = clipped | (np.abs(p) >= 2.0 ** -20)   # float64 then evaluates every step without rounding
    lo = np.zeros((len(p), 3), np.int64)
    hi = np.zeros((len(p), 3), np.int64)
    certain = np.ones(len(p), bool)
    for ch, k in enumerate((1.0, 2.0, 3.0)):
        a1 = 4.0 * t - k
        a2 = 1.5 - np.abs(a1)
        if ch == 0:
            a2 = a2 + rules.blue_shift / 255.0
        c = np.clip(a2, 0.0, 1.0)
        a3 = 255.0 * c
        y = a3 + 0.5
        ex = exact & _is32(a1) & _is32(a2) & _is32(a3) & _is32(y)
        lo[:, ch] = np.where(ex, np.floor(y), np.floor(y - BAND_JET))
        hi[:, ch] = np.where(ex, np.floor(y), np.floor(y + BAND_JET))
        certain &= lo[:, ch] == hi[:, ch]
    if rules.nan_colour == "black":
        lo[nan] = hi[nan] = 0
    return lo, hi, certain


class Image:
    """Per pixel (row-major): drawn, lo / hi [npix, 3] (the levels a correct float32 evaluation may show; equal
    where certain), uncertain (drawn and some channel inside the band), free (no bound exists: any colour),
    key (the winning primitive, -1 where none)."""

    def __init__(self, npix):
        self.drawn = np.zeros(npix, bool)
        self.lo = np.zeros((npix, 3), np.int64)
        self.hi = np.zeros((npix, 3), np.int64)
        self.uncertain = np.zeros(npix, bool)
        self.free = np.zeros(npix, bool)
        self.key = np.full(npix, -1, np.int64)

    def _paint(self, lo, hi, certain, rules):
        if rules.winner != "largest":
            self.key = np.where(self.key >= 0, _BIG - self.key, -1)
        d = self.key >= 0
        self.drawn = d
        self.lo[d], self.hi[d] = lo[self.key[d]], hi[self.key[d]]
        self.uncertain[d] = ~certain[self.key[d]]
        return self


_BIG = 1 << 40


def _put(key, pix, idx, rules):
    """Primitive idx claims the pixels pix: the largest index keeps a pixel (the mutant: the lowest, held as
    _BIG - idx until _paint)."""
    np.maximum.at(key, pix, idx if rules.winner == "largest" else _BIG - idx)


# ---------------------------------------------------------------- wireframe
def bresenham(x0, y0, x1, y1, rules=STATED, max_steps=None):
    """The pixels of the walk from (x0, y0) to (x1, y1), both included, in Python integers: with
    dx = |x1 - x0|, dy = -|y1 - y0|, err = dx + dy, at every pixel e2 = 2 err; x steps iff e2 >= dy (then
    err += dy), y steps iff e2 <= dx (then err += dx), both tests on the same e2."""
    x0, y0, x1, y1 = int(x0), int(y0), int(x1), int(y1)
    dx, dy = abs(x1 - x0), -abs(y1 - y0)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    err = dx + dy
    out = []
    while max_steps is None or len(out) < max_steps:
        out.append((x0, y0))
        if x0 == x1 and y0 == y1:
            break
        e2 = 2 * err
        step_x = e2 >= dy if rules.tie == ">=" else e2 > dy
        step_y = e2 <= dx
        if step_x:
            err += dy
            x0 += sx
        if step_y:
            err += dx
            y0 += sy
    return out


def wireframe(W, H, pos, x, tris, tri_valid, scale, rules=STATED):
    pos = np.asarray(pos, np.float32).reshape(-1, 2)
    x = np.asarray(x, np.float32)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    valid = np.asarray(tri_valid, bool)
    img = Image(W * H)
    a = tris.reshape(-1)                      # side 3t + k starts at vertex k ...
    b = np.roll(tris, -1, axis=1).reshape(-1)  # ... and ends at vertex (k + 1) % 3
    reach = in_reach(pos, W, H).all(1)
    if not rules.reach:  # (the mutant walks whatever an integer holds)
        with np.errstate(invalid="ignore"):
            reach = (np.abs(pos) < 1e9).all(1)
    live = np.repeat(valid, 3) & reach[a] & reach[b]
    px = pixel(pos, rules)
    for s in np.flatnonzero(live):
        pts = bresenham(px[a[s], 0], px[a[s], 1], px[b[s], 0], px[b[s], 1], rules, None if rules.reach else 4 * (W + H))
        pts = np.asarray(pts, np.int64)
        inside = (pts[:, 0] >= 0) & (pts[:, 0] < W) & (pts[:, 1] >= 0) & (pts[:, 1] < H)
        pts = pts[inside]
        _put(img.key, pts[:, 1] * W + pts[:, 0], s, rules)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.float32(0.5) * (x[a] + x[b]) if rules.side_colour == "mean" else x[a]
        p = (v * np.float32(scale)).astype(np.float32)
    return img._paint(*jet(p, rules), rules)


# ---------------------------------------------------------------- features
def features(W, H, feat_pos, feat_mu, scale, rules=STATED):
    fp = np.asarray(feat_pos, np.float32).reshape(-1, 2)
    mu = np.asarray(feat_mu, np.float32)
    img = Image(W * H)
    ok = feature_drawn(fp, W, H)
    f = np.flatnonzero(ok)
    c = pixel(fp[f], rules).astype(np.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            xx, yy = c[:, 0] + dx, c[:, 1] + dy
            inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            _put(img.key, yy[inside] * W + xx[inside], f[inside], rules)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (mu * np.float32(scale)).astype(np.float32)
    return img._paint(*jet(p, rules), rules)


# ---------------------------------------------------------------- idepthmap
def idepth_image(idm32, scale, rules=STATED):
    """jet(id * scale) of a filtered dense map (the implementation's own); NaN pixels stay black."""
    idm = np.asarray(idm32, np.float32).ravel()
    img = Image(len(idm))
    d = ~np.isnan(idm)
    img.key[d] = np.flatnonzero(d)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (idm * np.float32(scale)).astype(np.float32)
    return img._paint(*jet(p, rules), STATED)   # (one value per pixel: nothing competes)


# ---------------------------------------------------------------- normals
def _blend(W, pos, tris, vn, pix, t, rules):
    """Colour range of pixel pix under owner t: (lo, hi, certain, free)."""
    P = pos[tris[t]]                                  # n x 3 x 2
    N = vn[tris[t]]                                   # n x 3 x 3
    q = np.stack([(pix % W).astype(np.float64), (pix // W).astype(np.float64)], 1)
    w = np.empty((len(t), 3))
    m = np.empty((len(t), 3))
    for k in range(3):                                # weight of vertex k: the edge opposite to it
        o, d = P[:, (k + 1) % 3], P[:, (k + 2) % 3]
        e, r, r2 = d - o, q - o, q - d
        w[:, k] = e[:, 0] * r[:, 1] - e[:, 1] * r[:, 0]
        m[:, k] = np.maximum(np.abs(e[:, 0] * r[:, 1]) + np.abs(e[:, 1] * r[:, 0]),   # from either end of the edge
                             np.abs(e[:, 0] * r2[:, 1]) + np.abs(e[:, 1] * r2[:, 0]))
    # float32 evaluates the weights exactly where the vertices lie on the quarter-pixel grid within 512 px of the pixel:
    # the differences are multiples of 1/4 below 2^9, their products multiples of 1/16 below 2^18 (22 bits)
    exact_w = (np.floor(4 * P) == 4 * P).all((1, 2)) & (np.abs(P - q[:, None, :]) <= 512).all((1, 2)) & \
        (np.abs(P[:, :, None, :] - P[:, None, :, :]) <= 512).all((1, 2, 3))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        S = w.sum(1)
        num = (w[:, :, None] * N).sum(1) / S[:, None]
        L = np.linalg.norm(num, axis=1)
        M = (np.where(exact_w[:, None], 0.0, m) + np.abs(w)).sum(1) / np.abs(S)
        n = num / L[:, None]
        zero = L == 0
        n[zero] = (0.0, 0.0, -1.0)
        y = 255.0 * (0.5 * n + 0.5) + 0.5
        band = 128.0 * K_BLEND * U32 * M / L + K_CHAN * 256 * U32
        # every float32 operation exact: integer weights and three equal axis normals (num = s N, n = N, length 1),
        # or integer weights and integer normals that sum to the zero vector
        whole = exact_w & (np.floor(N) == N).all((1, 2))
        axis = whole & (N == N[:, :1]).all((1, 2)) & (L == 1.0)
        band = np.where(zero, np.where(whole, 0.0, np.inf), np.where(axis, 0.0, band))
        free = ~(band < 0.5)                          # the blend nearly cancels (or is not a number): no bound
        band = np.where(free, 0.0, band)
        y = np.where(free[:, None], 0.5, y)
        lo, hi = np.floor(y - band[:, None]).astype(np.int64), np.floor(y + band[:, None]).astype(np.int64)
    order = list(rules.normals_order)
    lo, hi = lo[:, order], hi[:, order]
    return lo, hi, (lo == hi).all(1) & ~free, free


def normals(W, H, pos, x, tris, tri_valid, vtx_normals, R=None, rules=STATED):
    """The normals image over the exact owner of frame_f64.raster (pass R to share one raster).  Returns
    (Image, cand): at R.ambiguous pixels any candidate owner's colour is right; cand = (pix, lo, hi, free)."""
    if R is None:
        R = F.raster(W, H, pos, x, tris, np.asarray(tri_valid, bool))
    pos = np.asarray(pos, np.float32).reshape(-1, 2).astype(np.float64)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    vn = np.asarray(vtx_normals, np.float32).reshape(-1, 3).astype(np.float64)
    img = Image(W * H)
    pix = np.flatnonzero(R.owner >= 0)
    img.key[pix] = R.owner[pix]
    img.drawn[pix] = True
    lo, hi, certain, free = _blend(W, pos, tris, vn, pix, R.owner[pix], rules)
    img.lo[pix], img.hi[pix], img.uncertain[pix], img.free[pix] = lo, hi, ~certain, free
    clo, chi, _, cfree = _blend(W, pos, tris, vn, R.cand_pix, R.cand_t, rules)
    return img, (R.cand_pix, clo, chi, cfree)
