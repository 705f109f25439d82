"""Independent float64 statement of the frame-results stage: rows a6 (costs), a8 (triangle stage,
vertex normals), a9 (graph filters), f1 (mesh), f2 (dense idepth / depth map, cloud) and coverage.

TEST INFRASTRUCTURE (see oracle/__init__.py), like nltgv2_np.py.  Written from the contracts in the
comment blocks of nltgv2_oracle.c and the reference's own formulas (src/utils.cc:184-230: mesh
points, u / v and faces; :290-312: the cloud; src/flame_offline_tum.cc:650-661: depth), vectorised
and deliberately NOT in the C code's operation order.

The raster is decided EXACTLY.  Float32 inputs are dyadic rationals, so the sign of an edge
function at a pixel centre is a property of the inputs: it is taken from float64 where the value is
clearly away from 0 and from fractions.Fraction inside an error band around 0.  Beside every exact
answer this module returns the float32 error band a correct float32 implementation may show (a
pixel whose decision lies inside it is `ambiguous`; a filter decision inside it is `flag_amb`), and
the magnitudes from which the tests build their tolerances (`scale`, `ang_tol`, `mag`).
"""
from fractions import Fraction

import numpy as np

EPS32 = 2.0 ** -23   # float32 machine epsilon (2 u)
U32 = 2.0 ** -24
_U64_BAND = 2.0 ** -46  # float64 evaluation of an edge function is trusted outside this relative band


def _f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# ---------------------------------------------------------------- exact edge functions
def _edge(px, py, qx, qy, sx, sy):
    """Edge function of P->Q at S, (Q - P) x (S - P), for float64 arrays holding float32 values.
    Returns (w, m, exact32): the value (sign exact, magnitude to float64 rounding), the magnitude
    |dx1 dy2| + |dy1 dx2| the float32 error is relative to, and whether float32 evaluates it
    exactly (all operands small integers)."""
    a, b, c, d = qx - px, sy - py, qy - py, sx - px
    ab, cd = a * b, c * d
    w = ab - cd
    m = np.abs(ab) + np.abs(cd)
    near = np.abs(w) <= _U64_BAND * m
    for k in np.flatnonzero(near):  # decide the sign exactly
        fx = [Fraction(float(v[k])) for v in (px, py, qx, qy, sx, sy)]
        w[k] = float((fx[2] - fx[0]) * (fx[5] - fx[1]) - (fx[3] - fx[1]) * (fx[4] - fx[0]))
    ints = [np.floor(v) == v for v in (px, py, qx, qy, sx, sy)]
    small = np.maximum.reduce([np.abs(v) for v in (a, b, c, d)]) <= 2048.0
    exact32 = np.logical_and.reduce(ints) & small
    return w, m, exact32


def _area32_is_zero(ax, ay, bx, by, cx, cy):
    """Whether the float32 area test fmaf(bx-ax, cy-ay, -((by-ay)*(cx-ax))) yields exactly 0 (the
    implementations skip such triangles).  Float32 products are exact in float64, so this is exact."""
    f = np.float32
    a, b = (bx.astype(f) - ax.astype(f)), (cy.astype(f) - ay.astype(f))
    c, d = (by.astype(f) - ay.astype(f)), (cx.astype(f) - ax.astype(f))
    p = (c * d).astype(np.float64)
    return a.astype(np.float64) * b.astype(np.float64) - p == 0.0


class Raster:
    """Per pixel (row-major H x W): owner (exact lowest-index covering triangle or -1), value (float64
    barycentric idepth of that owner), scale (tolerance unit: sum_k (|w_k| + m_k) |x_k| / |sum w|),
    margin (exact min_k |w_k| of the owner), ambiguous (some kept triangle's decision lies inside
    the float32 band), interior (covered, and every edge within the band is shared by two triangles:
    no float32 rasteriser that is watertight may leave it uncovered).  cand_*: every kept triangle
    that covers an ambiguous pixel exactly or within the band, with its own value and scale."""


def raster(W, H, pos, x, tris, keep=None, max_pairs=1 << 20):
    pos, x = _f64(pos).reshape(-1, 2), _f64(x)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    T, npix = len(tris), W * H
    keep = np.ones(T, bool) if keep is None else np.asarray(keep, bool)
    R = Raster()
    R.owner = np.full(npix, -1, np.int64)
    R.value = np.full(npix, np.nan)
    R.scale = np.zeros(npix)
    R.margin = np.full(npix, np.nan)
    R.ambiguous = np.zeros(npix, bool)
    R.interior = np.zeros(npix, bool)
    cand = []
    # edges shared by two kept, non-degenerate triangles (by vertex id)
    V = pos[tris]  # T x 3 x 2
    area_exact = _edge(V[:, 0, 0], V[:, 0, 1], V[:, 1, 0], V[:, 1, 1], V[:, 2, 0], V[:, 2, 1])[0]
    area32_zero = _area32_is_zero(V[:, 0, 0], V[:, 0, 1], V[:, 1, 0], V[:, 1, 1], V[:, 2, 0], V[:, 2, 1])
    live = keep & (area_exact != 0)
    ekey = np.sort(np.stack([tris[:, [1, 2]], tris[:, [2, 0]], tris[:, [0, 1]]], 1), axis=2)  # edge k opposite vertex k
    ekey = ekey[:, :, 0] * (len(pos) + 1) + ekey[:, :, 1]
    uk, cnt = np.unique(ekey[live].ravel(), return_counts=True)
    shared = np.zeros(ekey.shape, bool)
    shared[live] = np.isin(ekey[live], uk[cnt >= 2])
    # bounding boxes, clamped in float64 (no integer conversion of an unclamped coordinate)
    lo = np.ceil(V.min(1))
    hi = np.floor(V.max(1))
    x0 = np.clip(lo[:, 0], 0, W).astype(np.int64)
    y0 = np.clip(lo[:, 1], 0, H).astype(np.int64)
    x1 = np.clip(hi[:, 0], -1, W - 1).astype(np.int64)
    y1 = np.clip(hi[:, 1], -1, H - 1).astype(np.int64)
    bw, bh = np.maximum(x1 - x0 + 1, 0), np.maximum(y1 - y0 + 1, 0)
    n = np.where(keep & ~(area32_zero & (area_exact == 0)), bw * bh, 0)
    order = np.flatnonzero(n)
    start = 0
    while start < len(order):
        csum = np.cumsum(n[order[start:]])
        stop = start + max(1, int(np.searchsorted(csum, max_pairs, side="right")))
        ts = order[start:stop]
        start = stop
        cnts = n[ts]
        t = np.repeat(ts, cnts)
        k = np.arange(len(t)) - np.repeat(np.cumsum(cnts) - cnts, cnts)
        jj = x0[t] + k % bw[t]
        ii = y0[t] + k // bw[t]
        px, py = jj.astype(np.float64), ii.astype(np.float64)
        A, B, C = V[t, 0], V[t, 1], V[t, 2]
        wa, ma, ea = _edge(B[:, 0], B[:, 1], C[:, 0], C[:, 1], px, py)
        wb, mb, eb = _edge(C[:, 0], C[:, 1], A[:, 0], A[:, 1], px, py)
        wc, mc, ec = _edge(A[:, 0], A[:, 1], B[:, 0], B[:, 1], px, py)
        w = np.stack([wa, wb, wc], 1)
        m = np.stack([ma, mb, mc], 1)
        ex = np.stack([ea, eb, ec], 1)
        band = np.where(ex, 0.0, 8 * U32 * m)
        dec = ex | (np.abs(w) > band)          # float32 sign == exact sign (zero included)
        pos_ = dec & (w > 0)
        neg_ = dec & (w < 0)
        out_robust = pos_.any(1) & neg_.any(1)
        inside = (w >= 0).all(1) | (w <= 0).all(1)
        deg = area_exact[t] == 0
        cover = inside & ~deg
        amb = ~out_robust & (~dec.all(1) | (deg != area32_zero[t]))
        xs = x[tris[t]]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            S = w.sum(1)
            val = (w * xs).sum(1) / S
            scale = ((np.abs(w) + m) * np.abs(xs)).sum(1) / np.abs(S)
        pix = ii * W + jj
        near_ok = (dec | shared[t]).all(1)
        # lowest index wins: visit the covering pairs in ascending (pixel, triangle)
        c = np.flatnonzero(cover)
        if len(c):
            srt = c[np.lexsort((t[c], pix[c]))]
            first = srt[np.r_[True, pix[srt][1:] != pix[srt][:-1]]]
            p = pix[first]
            better = (R.owner[p] < 0) | (t[first] < R.owner[p])
            p, f = p[better], first[better]
            R.owner[p], R.value[p], R.scale[p] = t[f], val[f], scale[f]
            R.margin[p] = np.abs(w[f]).min(1)
            R.interior[pix[c[near_ok[c]]]] = True
        R.ambiguous[pix[amb]] = True
        keepc = cover | amb
        cand.append((pix[keepc], t[keepc], val[keepc], scale[keepc]))
    R.interior &= R.owner >= 0
    if cand:
        cp, ct, cv, cs = (np.concatenate(z) for z in zip(*cand))
        sel = R.ambiguous[cp]
        R.cand_pix, R.cand_t, R.cand_val, R.cand_scale = cp[sel], ct[sel], cv[sel], cs[sel]
    else:
        R.cand_pix = R.cand_t = np.zeros(0, np.int64)
        R.cand_val = R.cand_scale = np.zeros(0)
    return R


def coverage(R):
    """Exact covered-pixel count and the float32 coverage a correct implementation reports when no
    pixel is ambiguous; plus the number of ambiguous pixels (the count's uncertainty)."""
    cnt = int(np.count_nonzero(~np.isnan(R.value)))
    npix = len(R.value)
    return cnt, float(np.float32(cnt) / np.float32(npix)), int(np.count_nonzero(R.ambiguous))


# ---------------------------------------------------------------- triangle stage (row a8)
def backproject(Kinv, pos, x):
    """P = Kinv (u, v, 1)^T / idepth, and the magnitude |Kinv| |(u, v, 1)| / |idepth| of each row."""
    Kinv = _f64(Kinv).reshape(3, 3)
    pos, x = _f64(pos).reshape(-1, 2), _f64(x)
    h = np.column_stack([pos, np.ones(len(pos))])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        P = (h @ Kinv.T) / x[:, None]
        Pm = (np.abs(h) @ np.abs(Kinv).T) / np.abs(x)[:, None]
    return P, Pm


def triangles(Kinv, pos, x, tris, tp):
    """Returns dict: ok[T] (all three idepths finite and > 0), normal[T,3] (unit, n . P_a <= 0; zero
    rows where not ok), ang_tol[T] (float32 angle error unit, radians / eps32), orient_amb[T] (the plane
    passes so near the camera that either orientation is right), valid[T], flag_amb[T]
    (a filter decision within its float32 band), vtx[V,3], vtx_tol[V] (angle, radians / eps32),
    vtx_zero[V] (the float64 sum is exactly zero)."""
    pos, x = _f64(pos).reshape(-1, 2), _f64(x)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    T = len(tris)
    P, Pm = backproject(Kinv, pos, x)
    xa = x[tris]
    ok = np.isfinite(xa).all(1) & (xa > 0).all(1)
    Pa, Pb, Pc = (P[tris[:, k]] for k in range(3))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        e1, e2 = Pb - Pa, Pc - Pa
        n = np.cross(e1, e2)
        ln = np.linalg.norm(n, axis=1)
        l1, l2 = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)
        cond = l1 * l2 / ln
        pmag = np.max([np.linalg.norm(Pm[tris[:, k]], axis=1) for k in range(3)], axis=0)
        # float32 backprojection errors (~eps |P|) relative to the shorter edge, times the condition
        ang_tol = cond * (1.0 + 2.0 * pmag / np.minimum(l1, l2))
        unit = n / ln[:, None]
    unit = np.where((ln > 0)[:, None], unit, np.array([0.0, 0.0, -1.0]))
    with np.errstate(invalid="ignore"):
        facing = (unit * Pa).sum(1)
    unit[facing > 0] *= -1
    unit[~ok] = 0.0
    # float32 products of the edge vectors underflow (tiny triangles far away) or overflow: no bound
    with np.errstate(invalid="ignore", over="ignore"):
        lost = ~((l1 * l2 > 2.0 ** -100) & (pmag * pmag < 2.0 ** 120))
    ang_tol = np.where(ok & (ln > 0) & ~lost, ang_tol, np.where(ok, np.inf, 0.0))
    # a plane through (almost) the camera centre: n . P_a within the error, so either orientation is right
    with np.errstate(invalid="ignore", divide="ignore"):
        orient_amb = ok & ~(np.abs(facing) / np.linalg.norm(Pa, axis=1) > 16 * EPS32 * ang_tol + 8 * EPS32)
    # validity filters
    valid = ok.copy()
    amb = np.zeros(T, bool)
    xmin, xmax = xa.min(1), xa.max(1)
    if tp.do_idepth_triangle_filter:
        valid &= ~(xmin < np.float32(tp.min_triangle_idepth))  # one float32 compare: exact
    if tp.do_edge_length_filter:
        ml = float(np.float32(tp.edge_length_thresh)) * tp.width
        ml2 = ml * ml
        ml_exact = float(np.float32(ml)) == ml and float(np.float32(ml2)) == ml2
        for k in range(3):
            d = pos[tris[:, k]] - pos[tris[:, (k + 1) % 3]]
            l2_ = (d * d).sum(1)
            exact = ml_exact & (np.floor(d) == d).all(1) & (np.abs(d) < 2048).all(1) & (l2_ < 2 ** 24)
            over = l2_ > ml2
            valid &= ~over
            amb |= ok & ~exact & (np.abs(l2_ - ml2) <= 8 * U32 * (l2_ + ml2))
    if tp.do_oblique_triangle_filter:
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            r = Pa + Pb + Pc
            rl = np.linalg.norm(r, axis=1)
            cosang = -(unit * r).sum(1) / rl
            cth = np.cos(float(np.float32(tp.oblique_normal_thresh)))
            ray_tol = 8 * pmag / rl
            valid &= ~((rl > 0) & (cosang < cth))
            amb |= ok & (rl > 0) & (np.abs(cosang - cth) <= 16 * EPS32 * (ang_tol + ray_tol) + U32)
            diff = xmax - xmin
            fa, ff = float(np.float32(tp.oblique_idepth_diff_abs)), float(np.float32(tp.oblique_idepth_diff_factor))
            fx = ff * xmax
            valid &= ~((diff > fa) & (diff > fx))
            d_exact = diff.astype(np.float32).astype(np.float64) == diff
            f_exact = fx.astype(np.float32).astype(np.float64) == fx
            amb |= ok & ~d_exact & (np.abs(diff - fa) <= 2 * EPS32 * np.abs(diff))
            amb |= ok & ~(d_exact & f_exact) & (np.abs(diff - fx) <= 2 * EPS32 * (np.abs(diff) + np.abs(fx)))
    # vertex normals: normalised sum of the incident triangle normals
    Vn = len(pos)
    s = np.zeros((Vn, 3))
    tol_sum = np.zeros(Vn)
    deg = np.zeros(Vn)
    for k in range(3):
        np.add.at(s, tris[:, k], unit)
        np.add.at(tol_sum, tris[:, k], np.where(ok, ang_tol + orient_amb / EPS32, 0.0))
        np.add.at(deg, tris[:, k], ok.astype(np.float64))
    sl = np.linalg.norm(s, axis=1)
    vzero = sl == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        vtx = np.where(vzero[:, None], np.array([0.0, 0.0, -1.0]), s / sl[:, None])
        vtx_tol = (16 * tol_sum + 4 * deg * deg) / sl
    vtx_tol[vzero] = 0.0
    return dict(ok=ok, normal=unit, ang_tol=ang_tol, orient_amb=orient_amb, valid=valid, flag_amb=amb, P=P, vtx=vtx,
                vtx_tol=vtx_tol, vtx_zero=vzero)


def angle(a, b):
    """Angle between the rows of a and b (radians, float64; 0 for two zero rows)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    c = np.cross(a, b)
    return np.arctan2(np.linalg.norm(c, axis=1), (a * b).sum(1))


# ---------------------------------------------------------------- mesh (f1), depth and cloud (f2)
def mesh(Kinv, pos, x, W, H):
    """PointNormalUV rows without the normals: (valid[V], xyz[V,3], xyz_mag[V,3], uv[V,2])."""
    pos, x = _f64(pos).reshape(-1, 2), _f64(x)
    valid = ~np.isnan(x) & (x > 0)
    P, Pm = backproject(Kinv, pos, x)
    uv = pos / np.array([W - 1.0, H - 1.0])
    return valid, P, Pm, uv


def depth(idm32):
    """depth = 1 / idepth where idepth is a number > 0 (float32 rounding of the exact reciprocal)."""
    d = _f64(idm32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        out = np.where(~np.isnan(d) & (d > 0), 1.0 / d, np.nan)
        return out.astype(np.float32).astype(np.float64)


def cloud(Kinv, depth32, min_depth, max_depth):
    """Kinv (j d, i d, d) per pixel (H x W x 3) where min_depth <= d <= max_depth, else NaN; and the
    magnitude |Kinv| |(j d, i d, d)|."""
    Kinv = _f64(Kinv).reshape(3, 3)
    d = _f64(depth32)
    H, W = d.shape
    ii, jj = np.mgrid[0:H, 0:W].astype(np.float64)
    q = np.stack([jj * d, ii * d, d], -1)
    with np.errstate(invalid="ignore", over="ignore"):
        c = q @ Kinv.T
        cm = np.abs(q) @ np.abs(Kinv).T
    bad = np.isnan(d) | (d < float(np.float32(min_depth))) | (d > float(np.float32(max_depth)))
    c[bad] = np.nan
    return c, cm


# ---------------------------------------------------------------- costs (a6), graph filters (a9)
def costs(pos, edges, alpha, beta, x, w1, w2, z, wgt, lam, emask=None, vmask=None):
    """float64 (smooth, data, smooth_mag, data_mag): sums of |K(x, w)| and lam wgt |x - z|, and the
    matching sums of magnitudes."""
    pos = _f64(pos).reshape(-1, 2)
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    a, b = _f64(alpha), _f64(beta)
    x, w1, w2, z, wgt = (_f64(v) for v in (x, w1, w2, z, wgt))
    lam = float(np.float32(lam))
    i, j = e[:, 0], e[:, 1]
    d = pos[i] - pos[j]
    k1 = x[i] - x[j] - w1[i] * d[:, 0] - w2[i] * d[:, 1]
    sm = a * np.abs(k1) + b * (np.abs(w1[i] - w1[j]) + np.abs(w2[i] - w2[j]))
    smm = a * (np.abs(x[i]) + np.abs(x[j]) + np.abs(w1[i] * d[:, 0]) + np.abs(w2[i] * d[:, 1])) + \
        b * (np.abs(w1[i]) + np.abs(w1[j]) + np.abs(w2[i]) + np.abs(w2[j]))
    da = lam * wgt * np.abs(x - z)
    dam = lam * np.abs(wgt) * (np.abs(x) + np.abs(z))
    em = np.ones(len(e), bool) if emask is None else np.asarray(emask, bool)
    vm = np.ones(len(x), bool) if vmask is None else np.asarray(vmask, bool)
    return float(sm[em].sum()), float(da[vm].sum()), float(smm[em].sum()), float(dam[vm].sum())


def neighbourhoods(V, edges):
    """Per vertex: [self] + the other end of every incident edge, in ascending edge id."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    nb = [[v] for v in range(V)]
    for k, (i, j) in enumerate(e):
        nb[i].append(j)
        nb[j].append(i)
    return nb


def graph_filter(x, edges, kind):
    """kind 0: the element (n-1)//2 of the stable ascending order of the neighbourhood's values
    (NaN last, ties -- -0.0 beside +0.0 included -- by position); returned as the float32 value
    itself.  kind 1: the float64 mean, and the magnitude mean(|x|) for its tolerance."""
    x = np.asarray(x, np.float32)
    out = np.empty(len(x), np.float64 if kind else np.float32)
    mag = np.zeros(len(x))
    for v, nb in enumerate(neighbourhoods(len(x), edges)):
        vals = x[nb]
        if kind == 0:
            out[v] = vals[np.argsort(vals, kind="stable")[(len(vals) - 1) // 2]]
        else:
            vv = vals.astype(np.float64)
            with np.errstate(invalid="ignore", over="ignore"):
                out[v] = vv.sum() / len(vv)
            mag[v] = np.abs(vv).sum() * (len(vv) - 1) / len(vv)  # sequential float32 sum: (n-1) u sum|x| / n
    return out, mag
