"""Corpus of the four mesh debug images (tests/test_debug_f64_oracle.py, tests/test_gpu_debug_f64.py): every case
of tests/frame_corpus.py, whole, plus small seeded cases aimed at the drawing rules.

A case is a frame-corpus dict (W, H, pos, x, tris, edges, Kinv, tp, lattice, far, ...) with, added here:
scale (scene_color_scale), feat_pos [n,2] / feat_mu [n] (the raw features of the FEATURES image), dyadic (the
idepths, the feature idepths and the scale are dyadic with few bits: float32 evaluates every colour exactly; in a
dyadic or lattice case no pixel of any of the four images may be uncertain), draws (the kinds whose image must not be
black).  Where a frame-corpus case cannot meet that as it stands, the copy here is adapted and says so (_tilted,
_dyadic_plane, _unfiltered); the frame corpus itself is untouched.

`far` (frame_corpus: "vertices beyond the debug images' reach") now has a defined picture: the sides that end at
such a vertex are absent.  corpus() checks the flag against the reach rule.
"""
import numpy as np

from tests import frame_corpus as FC
from tests.frame_checks import KINDS

TP_OFF = (0, 1.57, 0.35, 0.1, 0, 0.333, 0, 0.01)   # no validity filter: a triangle is valid iff its idepths are > 0
P25 = 2.0 ** -25
HALF_PRED = np.float32(0.5) - np.float32(P25)       # the float32 predecessor of 0.5: 0.5 - 2^-25
SCALE_NON_DYADIC = 0.7


def _pred(v):
    return float(np.nextafter(np.float32(v), np.float32(-np.inf)))


def _succ(v):
    return float(np.nextafter(np.float32(v), np.float32(np.inf)))


def segs_to_soup(segs):
    """Every segment (A, B) as the degenerate soup triangle (A, B, A): its sides draw A -> B, then B -> A, then the
    single pixel of A.  Its area is exactly 0, so the raster skips it."""
    P = []
    for a, b in segs:
        P += [a, b, a]
    return P


def _dyadic_x(n, step=1.0 / 256):
    return (0.25 + step * np.arange(n)).astype(np.float32)


def _finish(c, scale, feat_pos=None, feat_mu=None, dyadic=False):
    c = dict(c)
    c["scale"] = float(scale)
    c["feat_pos"] = np.asarray(c["pos"] if feat_pos is None else feat_pos, np.float32).reshape(-1, 2)
    c["feat_mu"] = np.asarray(c["x"] if feat_mu is None else feat_mu, np.float32)
    c["dyadic"] = dyadic
    c["draws"] = KINDS
    return c


def _octants():
    W, H = 64, 48
    segs = []
    # sides in all eight octants, horizontal, vertical, and the tie slopes 1, 1/2, 2 -- each from four centres,
    # each drawn in both directions (segs_to_soup)
    dirs = [(10, 3), (3, 10), (-3, 10), (-10, 3), (-10, -3), (-3, -10), (3, -10), (10, -3),   # one per octant
            (11, 0), (-11, 0), (0, 11), (0, -11),
            (8, 8), (-8, 8), (8, -8), (-8, -8),                                                   # slope 1
            (10, 5), (-10, 5), (10, -5), (-10, -5),                                               # slope 1/2
            (5, 10), (-5, 10), (5, -10), (-5, -10)]                                               # slope 2
    centres = [(16, 12), (48, 12), (16, 36), (48, 36)]
    for k, (dx, dy) in enumerate(dirs):
        cx, cy = centres[k % 4]
        segs.append(((cx, cy), (cx + dx, cy + dy)))
    # end points at k + 0.5, its float32 neighbours, -0.5, -(0.5 - 2^-25), 0.5 - 2^-25; negative coordinates
    for x_, y0, y1 in ((7.5, 20, 23), (_pred(7.5), 24, 27), (_succ(7.5), 28, 31), (-0.5, 2, 6), (-float(HALF_PRED), 8, 12),
                       (float(HALF_PRED), 14, 18), (-1.5, 20, 24), (_pred(2.5), 40, 44), (-3.25, 30, 34)):
        segs.append(((x_, y0), (x_, y1)))
    for y_, x0, x1 in ((float(HALF_PRED), 30, 34), (-float(HALF_PRED), 36, 40), (-0.5, 42, 46), (47.5, 50, 54),
                       (_pred(47.5), 56, 60), (46.5, 44, 48)):
        segs.append(((x0, y_), (x1, y_)))
    # sides that start outside the image and cross it from each of the four borders (in reach: R = 112)
    segs += [((-20, 5), (30, 20)), ((80, 7), (30, 30)), ((5, -30), (12, 20)), ((40, 90), (20, 10)),
             ((-15, -9), (70, 60)), ((-30, 40), (90, 3))]
    P = segs_to_soup(segs)
    # a triangle whose three vertices round to one pixel, and two proper triangles for the dense images
    P += [(58.1, 2.1), (58.3, 2.2), (58.2, 2.4), (20, 20), (44, 22), (30, 40), (2, 30), (14, 46), (3, 45)]
    pos, tris = FC.soup(P)
    c = FC.mk("octants", W, H, pos, _dyadic_x(len(pos)), tris, K=FC.K_ID, tp=TP_OFF)
    return _finish(c, 1.0, dyadic=True)


def _reach():
    W, H = 32, 24   # R = 56
    R = W + H
    # a coordinate exactly at -R and at 2 R (drawn) and one float32 step beyond each (absent), in x and in y; the rows
    # and columns of the absent ones (rows 4, 8, 12, column 30, rows 0..1 of column 28) are touched by nothing else
    segs = [((-R, 2), (20, 2)), ((_pred(-R), 4), (20, 4)), ((2 * R, 6), (22, 6)), ((_succ(2 * R), 8), (22, 8)),
            ((26, -R), (26, 1)), ((28, _pred(-R)), (28, 1)), ((24, 2 * R), (24, 16)), ((30, _succ(2 * R)), (30, 16)),
            ((-200, 12), (200, 12)), ((200, 12), (-200, 12)),   # crosses the whole image; out of reach from either end
            ((-R, -R), (1, 1)), ((2 * R, 2 * R), (16, 16))]
    pos, tris = FC.soup(segs_to_soup(segs) + [(4, 15), (28, 16), (10, 22)])
    c = FC.mk("reach", W, H, pos, _dyadic_x(len(pos)), tris, K=FC.K_ID, tp=TP_OFF, far=True)
    return _finish(c, 1.0, dyadic=True)


def _fan():
    # twelve soup triangles around (24, 24), each with its own constant idepth: all their sides through one pixel
    W = H = 48
    ring = [(24 + 20 * np.cos(a), 24 + 20 * np.sin(a)) for a in np.arange(12) * (np.pi / 6)]
    ring = [(round(4 * u) / 4.0, round(4 * v) / 4.0) for u, v in ring]
    P, x = [], []
    for k in range(12):
        P += [(24, 24), ring[k], ring[(k + 1) % 12]]
        x += [0.25 + k / 8.0] * 3
    pos, tris = FC.soup(P)
    c = FC.mk("overwrite_fan", W, H, pos, x, tris, K=FC.K_ID, tp=TP_OFF)
    return _finish(c, 1.0, dyadic=True)


def jet_values(scale):
    """Feature idepths whose product with `scale` lands on t = 0, 1/8, 3/8, 5/8, 7/8, 1 (t = p / 2) and on the
    float32 neighbours of each, then -1, 2, 2.5, NaN, +inf, -inf."""
    s = np.float32(scale)
    v = []
    for t in (0.0, 1 / 8, 3 / 8, 5 / 8, 7 / 8, 1.0):
        m = np.float32(np.float32(2 * t) / s)
        v += [float(np.nextafter(m, np.float32(-np.inf))), float(m), float(np.nextafter(m, np.float32(np.inf)))]
    return np.asarray(v + [-1.0, 2.0, 2.5, np.nan, np.inf, -np.inf], np.float32)


def _jet_table(scale, name):
    # the breakpoint values, then a sweep over the whole scale (p = k / 256 at scale 1: every ramp, exactly).
    # Of the 24 listed values, 23 are CERTAIN at scales 1 and 0.5 (held byte for byte): every breakpoint, both neighbours
    # of t = 0, 1/8, 3/8, 5/8, 7/8, the successor of t = 1 and the six specials.  One is inside the band at every scale:
    # the float32 predecessor of t = 1 (p = 2 - 2^-23), whose red ramp is 255 * (0.5 + 2^-22) + 0.5 = 128.00006, a
    # rounding above the level 127 | 128 (held to {127, 128}).  At scale 0.7 the idepth 2.0 (p = 1.4: green
    # 255 * 0.7 + 0.5 = 179 up to the rounding of 1.4) is in the band as well.  tests/test_debug_f64_oracle.py asserts
    # exactly this split.  Because of that one value the case is not marked dyadic; it stays far below the cap
    W, H = 96, 64
    mu = np.concatenate([jet_values(scale), (np.arange(-6, 580) / np.float32(256 * scale)).astype(np.float32)])
    k = np.arange(len(mu))
    assert len(mu) <= 32 * 21
    fp = np.stack([1 + 3 * (k % 32), 1 + 3 * (k // 32)], 1)   # a 3 px grid: the squares tile without overlap
    c = FC.mk(name, W, H, [(2, 40), (30, 42), (6, 60)], [0.5, 0.75, 1.0], [[0, 1, 2]], K=FC.K_ID, tp=TP_OFF)
    return _finish(c, scale, fp, mu)


def _features_edge(rng):
    W, H = 37, 29   # 1073 pixels: no multiple of 256
    low = [-1.0, -1.5, -2.0, -0.5, 0.0, float(HALF_PRED)]     # at, on and beyond the left / top border ...
    high = [-1.0, -0.5, 0.0, 0.5, 1.0]                        # ... and the right / bottom one (offsets from W, H)
    fp = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    # every border value on a row (column) of its own, 4 px apart: no square hides what its neighbour leaves out
    fp += [(u, 4.0 + 4 * k) for k, u in enumerate(low)] + [(W + u, 4.0 + 4 * k) for k, u in enumerate(high)]
    fp += [(6.0 + 4 * k, v) for k, v in enumerate(low)] + [(6.0 + 4 * k, H + v) for k, v in enumerate(high)]
    # overlapping squares: later features partly cover earlier ones
    fp += [(16, 14), (17, 15), (18, 14), (17, 13), (16.5, 14.5)]
    # positions that no pixel holds: they draw nothing -- (0, 0) stays with the corner feature listed before them
    bad = [np.nan, np.inf, -np.inf, 3e9, -3e9]
    fp += [(b, 3.0) for b in bad] + [(3.0, b) for b in bad] + [(np.nan, np.nan), (3e9, -3e9)]
    fp = np.asarray(fp, np.float64)
    # filler up to 257 features (a second block of one thread), listed first: the designed ones lie on top
    more = rng.uniform(-3, [W + 3, H + 3], (257 - len(fp), 2))
    fp = np.concatenate([more, fp]).astype(np.float32)
    assert len(fp) == 257
    mu = (np.arange(257) / 128.0).astype(np.float32)   # dyadic, all different: the colour names the feature
    c = FC.mk("features_edge", W, H, [(5, 5), (30, 6), (8, 25)], [0.5, 0.75, 1.0], [[0, 1, 2]], K=FC.K_ID, tp=TP_OFF)
    return _finish(c, 1.0, fp, mu, dyadic=True)


def _mesh86(rng):
    # 86 triangles = 258 sides: a second block of the line kernel with two live threads
    pos, tris = FC.lattice(43, 1, 3.0, x0=2.5, y0=3.25, diag=2, jitter=0.3, rng=rng)
    assert len(tris) == 86
    x = FC.planar(pos, 0.4, 9e-3, 1e-2)
    c = FC.mk("mesh_86_triangles", 140, 12, pos, x, tris, K=FC.K_TUM, tp=TP_OFF)
    return _finish(c, SCALE_NON_DYADIC)


def _tilted(c):
    """idepth_specials_96x64 is three fronto-parallel planes: every normal is (~0, ~0, -1), so the G and R channels of
    the normals image sit a rounding away from the level 127 | 128 over most of the image -- inside the band by
    geometry.  The debug corpus tilts the idepths (signs, zeros, NaN and infinities stay what they are), which moves the
    normals off the axis; the frame corpus keeps the original."""
    c = dict(c)
    p = c["pos"].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        c["x"] = (c["x"] * (1.0 + 3.7e-3 * p[:, 0] + 7.3e-3 * p[:, 1])).astype(np.float32)
    c["name"] = "idepth_specials_tilted_96x64"
    return c


def _dyadic_plane(c):
    """lattice_752x480_backslash with the idepth plane 0.5 + u / 4096 - v / 8192 in place of its decimal one.  No pixel
    of a lattice case may be uncertain, and a decimal plane interpolates to values of which a few always fall inside
    the colour map's band.  On this lattice (32 px cells: weights are integers up to 1024, the idepths multiples of
    2^-13 below 1) float32 interpolates the plane without rounding, so the dense map holds multiples of 2^-13 and, at
    scale 1, every colour of all four images is exact.  The frame corpus keeps the original."""
    c = dict(c)
    p = c["pos"].astype(np.float64)
    assert (np.floor(p) == p).all()
    c["x"] = (0.5 + p[:, 0] / 4096.0 - p[:, 1] / 8192.0).astype(np.float32)
    c["name"] = "lattice_752x480_backslash_dyadic"
    return c


def _unfiltered(c):
    """row_517x1, col_1x389 and edge_on_cancel with the validity filters off: under the frame corpus's thresholds every
    one of their triangles is invalid, and the wireframe, normals and idepthmap images would be black."""
    c = dict(c)
    c["tp"] = TP_OFF + (c["W"], c["H"])
    return c


def corpus():
    rng = np.random.default_rng(20261020)
    # (0.45, not 0.5: the frame corpus's idepths are short decimals, and 0.8 * 0.5 puts a ramp at 0.3 -- 255 * 0.3 + 0.5
    # is the integer 77, a rounding away from level 76)
    scales = [1.0, SCALE_NON_DYADIC, 1.9, 0.45]
    cases = []
    for k, c in enumerate(FC.corpus().values()):
        dy = c["name"] in ("lattice_soup_both_diagonals", "lattice_752x480_backslash")   # (the soup: 0.25 + k / 1024)
        if c["name"] == "idepth_specials_96x64":
            c = _tilted(c)
        elif c["name"] == "lattice_752x480_backslash":
            c = _dyadic_plane(c)
        elif c["name"] in ("row_517x1", "col_1x389", "edge_on_cancel"):
            c = _unfiltered(c)
        c = _finish(c, 1.0 if dy else scales[k % 4], dyadic=dy)
        # the features: the vertices with their idepths, then 40 more around the image (dyadic idepths in a dyadic case)
        extra = rng.uniform(-4, [c["W"] + 4, c["H"] + 4], (40, 2))
        extra_mu = rng.uniform(-0.1, 2.6, 40)
        c["feat_pos"] = np.concatenate([c["feat_pos"], extra]).astype(np.float32)
        c["feat_mu"] = np.concatenate([c["feat_mu"], np.round(extra_mu * 64) / 64 if dy else extra_mu]).astype(np.float32)
        if c["name"] == "far_quad_beyond_2p31":
            # every vertex is 3e9 px out: the sides are out of reach, so the wireframe is black BY RULE (what the case is
            # here for: the line kernel must convert none of these positions), and the edge-length filter drops both
            # triangles, so the dense images are black too (outside_1e4 / outside_1e6 draw far triangles)
            c["draws"] = ("features",)
        cases.append(c)
    cases += [_octants(), _reach(), _fan(), _jet_table(1.0, "jet_table_scale_1"), _jet_table(0.5, "jet_table_scale_0.5"),
              _jet_table(SCALE_NON_DYADIC, "jet_table_scale_0.7"), _features_edge(rng), _mesh86(rng)]
    return {c["name"]: c for c in cases}
