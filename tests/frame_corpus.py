"""Adversarial corpus of the frame-results stage: named, seeded, small cases (tests/test_frame_f64_oracle.py,
tests/test_gpu_frame_f64.py).

Each case is a dict: W, H, pos [V,2] f32, x [V] f32 (the vertex idepths), tris [T,3] i32, edges [E,2] (the
unique triangle edges, i < j, plus any extra), Kinv [3,3] f32, tp (TriParams field values), min_depth /
max_depth, lattice (every vertex on the integer grid: the float32 edge functions are exact, so the owner
of every pixel is decided exactly), far (vertices beyond the debug images' reach, [-(W+H), 2(W+H)] per coordinate:
the triangle sides that end there are absent from the wireframe; tests/debug_corpus.py reads the flag).
"""
import numpy as np

K_TUM = np.array([[525.0, 0, 319.5], [0, 525.0, 239.5], [0, 0, 1]])
K_SKEW = np.array([[520.0, 3.0, 301.25], [0, 480.5, 251.75], [0, 0, 1]])  # fx != fy, skew
K_ID = np.eye(3)
# (do_oblique, normal_thresh, diff_factor, diff_abs, do_edge, edge_len_thresh, do_idepth, min_idepth)
TP_DEFAULT = (1, 1.57, 0.35, 0.1, 1, 0.333, 1, 0.01)
TP_DYADIC = (1, 1.4, 0.25, 0.125, 1, 0.25, 1, 0.0625)  # thresholds float32 hits exactly


def kinv(K):
    return np.linalg.inv(np.asarray(K, np.float64)).astype(np.float32)


def tri_edges(tris, extra=()):
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]) if len(t) else np.zeros((0, 2), np.int64)
    e = np.sort(e, 1)
    if len(extra):
        e = np.concatenate([e, np.sort(np.asarray(extra, np.int64).reshape(-1, 2), 1)])
    e = e[e[:, 0] != e[:, 1]]
    return np.unique(e, axis=0).astype(np.int32)


def lattice(nx, ny, step, x0=0.0, y0=0.0, diag=0, jitter=None, rng=None):
    """(nx+1) x (ny+1) vertices on a grid, two triangles per cell; diag 0: '/' split, 1: '\\', 2: alternate."""
    gx, gy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1))
    pos = np.stack([x0 + gx.ravel() * step, y0 + gy.ravel() * step], 1).astype(np.float64)
    if jitter is not None:
        pos += jitter * rng.choice([-1.0, 1.0], pos.shape)
    tris = []
    vid = lambda i, j: j * (nx + 1) + i  # noqa: E731
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = vid(i, j), vid(i + 1, j), vid(i, j + 1), vid(i + 1, j + 1)
            dd = diag if diag < 2 else (i + j) % 2
            tris += ([[a, b, d], [a, d, c]] if dd else [[a, b, c], [b, d, c]])
    return pos.astype(np.float32), np.asarray(tris, np.int32)


def planar(pos, a, b, c):
    return (a + b * pos[:, 0].astype(np.float64) + c * pos[:, 1]).astype(np.float32)


def mk(name, W, H, pos, x, tris, K=K_TUM, tp=TP_DEFAULT, min_depth=0.1, max_depth=100.0, lattice=False, far=False,
       extra_edges=()):
    pos = np.asarray(pos, np.float32).reshape(-1, 2)
    tris = np.asarray(tris, np.int32).reshape(-1, 3)
    return dict(name=name, W=W, H=H, pos=pos, x=np.asarray(x, np.float32), tris=tris, edges=tri_edges(tris, extra_edges),
                Kinv=kinv(K), tp=tuple(tp) + (W, H), min_depth=min_depth, max_depth=max_depth, lattice=lattice, far=far)


def soup(tris_pos):
    """Triangle soup: every triangle its own three vertices."""
    p = np.asarray(tris_pos, np.float32).reshape(-1, 2)
    return p, np.arange(len(p), dtype=np.int32).reshape(-1, 3)


def _lattice_soup():
    # every 8 px cell split by BOTH diagonals into four overlapping triangles, each with its own vertices
    # and its own constant idepth: the map's value names the owner, so the lowest-index rule is observed
    P = []
    for j in range(6):
        for i in range(8):
            a, b, c, d = (8 * i, 8 * j), (8 * i + 8, 8 * j), (8 * i, 8 * j + 8), (8 * i + 8, 8 * j + 8)
            P += [a, b, c, b, d, c, a, b, d, a, d, c]
    pos, tris = soup(P)
    x = np.repeat(0.25 + np.arange(len(tris)) / 1024.0, 3).astype(np.float32)
    return mk("lattice_soup_both_diagonals", 64, 48, pos, x, tris, K=K_ID, lattice=True)


def _lattice_narrow():
    # 37 x 1001: a 6 px lattice ('/' diagonals) over rows 0..600 (mean area < 64: 8 lanes per triangle), then
    # tall slivers over rows 600..1000 at indices 8k..8k+5 -- one 8-lane wave holds six > 256 px triangles
    pos, tris = lattice(6, 100, 6.0, diag=0)
    tris = list(tris)
    while len(tris) % 8:
        tris.append(tris[-1][[1, 2, 0]])
    base = len(pos)
    extra = []
    for k in range(6):
        x0 = 6.0 * k
        extra += [(x0, 600.0), (x0 + 6.0, 600.0), (x0 + 3.0, 1000.0)]
    pos = np.concatenate([pos, np.asarray(extra, np.float32)])
    tris += [[base + 3 * k, base + 3 * k + 1, base + 3 * k + 2] for k in range(6)]
    x = planar(pos, 0.6, 1e-3, 2e-4)
    return mk("lattice_37x1001_slivers", 37, 1001, pos, x, np.asarray(tris), lattice=True)


def _lattice_wide():
    pos, tris = lattice(23, 15, 32.0, diag=1)  # '\' diagonals, 752 x 480, mean area 512
    x = planar(pos, 0.4, 2e-4, -1e-4)
    return mk("lattice_752x480_backslash", 752, 480, pos, x, tris, K=K_SKEW, lattice=True)


def _offset(rng):
    # vertices 2^-20 off the integer lattice: pixel centres a few ulp from an edge
    pos, tris = lattice(51, 15, 24.0, x0=1.0, y0=2.0, diag=2, jitter=2.0 ** -20, rng=rng)
    x = planar(pos, 0.5, 3e-4, 1e-4)
    return mk("offset_2m20_1241x376", 1241, 376, pos, x, tris, K=K_SKEW)


def _offset_dense(rng):
    pos, tris = lattice(7, 199, 5.0, x0=0.5, y0=0.25, diag=2, jitter=2.0 ** -20, rng=rng)
    x = planar(pos, 0.9, -2e-3, 3e-4)
    return mk("offset_2m20_37x1001_dense", 37, 1001, pos, x, tris, K=K_SKEW)


def _slivers(rng):
    pos, tris = lattice(8, 8, 8.0, diag=0)
    n0 = len(pos)
    sl = [(3.0, 3.0), (60.0, 3.0 + 2.0 ** -18), (31.5, 3.0 + 2.0 ** -19),   # near-collinear
          (2.0, 40.0), (62.0, 50.0), (32.0, 45.0),                            # exactly collinear (zero area)
          (10.0, 10.0), (10.0, 10.0), (20.0, 30.0),                           # repeated vertex
          (5.0, 60.0), (61.0, 61.0), (33.0, 60.5 + 2.0 ** -20)]               # near-collinear
    pos = np.concatenate([pos, np.asarray(sl, np.float32)])
    tris = np.concatenate([np.asarray([[n0 + 3 * k, n0 + 3 * k + 1, n0 + 3 * k + 2] for k in range(4)]), tris])
    x = planar(pos, 0.7, 1e-3, -1e-3)
    return mk("slivers_64x64", 64, 64, pos, x, tris, K=K_TUM)


def _outside(W, H, R, name, rng, far=False):
    # an inner lattice, then a quad whose corners are R px out (two triangles), then triangles partly and
    # wholly outside the image with vertices in -5 .. W+5
    nx, ny = max(1, (W - 10) // 40), max(1, (H - 10) // 40)
    pos, tris = lattice(nx, ny, 40.0, x0=5.0, y0=5.0, diag=0)
    n0 = len(pos)
    quad = [(-R, -R), (W + R, -R), (W + R, H + R), (-R, H + R)]
    part = [(-5.0, -5.0), (W / 2.0 + 0.5, -5.0), (-5.0, H + 5.0),
            (W + 5.0, H + 5.0), (W + 5.0, -5.0), (W - 30.25, H / 2.0),
            (W + 1.0, 2.0), (W + 5.0, 2.0), (W + 3.0, H + 5.0)]  # wholly outside
    pos = np.concatenate([pos, np.asarray(quad + part, np.float32)])
    tris = np.concatenate([tris, [[n0, n0 + 1, n0 + 2], [n0, n0 + 2, n0 + 3]],
                           [[n0 + 4 + 3 * k, n0 + 5 + 3 * k, n0 + 6 + 3 * k] for k in range(3)]])
    x = planar(pos, 0.5, 1e-8, -1e-8) if R < 1e7 else np.full(len(pos), 0.5, np.float32)
    x[:n0] = planar(pos[:n0], 0.5, 2e-4, 1e-4)
    return mk(name, W, H, pos, x, tris, K=K_TUM, far=far)


def _thin(W, H, name):
    pos = np.asarray([(-0.5, -0.5), (W - 0.5, -0.5), (-0.5, H - 0.5), (W - 0.5, H - 0.5),
                      (W / 3.0, -3.0), (W / 2.0, H + 2.0)], np.float32)
    tris = [[0, 1, 4], [0, 3, 1], [0, 2, 3], [2, 5, 3]]
    x = planar(pos, 0.8, 1e-3, 1e-3)
    return mk(name, W, H, pos, x, tris, K=K_ID)


def _far_2p31():
    # two triangles forming a quad over the whole image, corners ~3e9 px out (beyond 2^31)
    R = 3.0e9
    pos = [(-R, -R), (R, -R), (R, R), (-R, R)]
    return mk("far_quad_beyond_2p31", 640, 480, pos, [0.5, 0.5, 0.5, 0.5], [[0, 1, 2], [0, 2, 3]], far=True)


def _specials():
    # a 12 x 8 lattice of 8 px cells (96 x 64) whose idepths hit every special value and threshold
    pos, tris = lattice(12, 8, 8.0, diag=2)
    x = planar(pos, 0.5, 0.0, 0.0)
    x[pos[:, 1] >= 40] = 0.25   # depth exactly 4 = max_depth
    x[(pos[:, 0] >= 56) & (pos[:, 1] < 40)] = 0.375  # with 0.5: diff 0.125 = abs limit, 0.25 * 0.5 = factor limit
    spec = {3: np.nan, 5: 0.0, 7: -0.0, 9: -0.5, 11: np.inf, 15: 1e-40, 17: 1e30, 31: 0.0625, 33: 0.0625,
            45: 0.0625 + 2.0 ** -27}
    for v, val in spec.items():
        x[v] = val
    n0 = len(pos)
    # an edge exactly at max_len = 0.25 * 96 = 24 (valid) and one just over (invalid), both soup
    ext = [(70.0, 2.0), (94.0, 2.0), (82.0, 6.0), (70.0, 12.0), (94.0 + 2.0 ** -15, 12.0), (82.0, 16.0)]
    pos = np.concatenate([pos, np.asarray(ext, np.float32)])
    x = np.concatenate([x, np.full(6, 0.5, np.float32)])
    tris = np.concatenate([[[n0, n0 + 1, n0 + 2], [n0 + 3, n0 + 4, n0 + 5]], tris])
    # degree-0 vertices, and a vertex only in a triangle with a NaN idepth
    pos = np.concatenate([pos, [(50.0, 50.0), (51.0, 51.0), (1.0, 60.0), (2.0, 63.0)]]).astype(np.float32)
    x = np.concatenate([x, [0.5, np.nan, 0.5, 0.5]]).astype(np.float32)
    m = len(pos)
    tris = np.concatenate([tris, [[3, m - 2, m - 1]]])
    return mk("idepth_specials_96x64", 96, 64, pos, x, tris, K=K_TUM, tp=TP_DYADIC, min_depth=2.0, max_depth=4.0)


def _cancel():
    # triangles seen edge-on (image-collinear on u = 0, identity K): their planes contain the camera, the
    # normals are exactly +-(1, 0, 0), and vertex 0 sits in two whose normals cancel exactly
    pos = [(0.0, 0.0), (0.0, 4.0), (0.0, 9.0), (0.0, -3.0), (20.0, 20.0), (30.0, 20.0), (20.0, 30.0)]
    x = [0.5, 0.25, 0.75, 0.4, 0.5, 0.5, 0.5]
    tris = [[0, 1, 2], [0, 2, 1], [4, 5, 6], [0, 3, 1]]
    return mk("edge_on_cancel", 40, 40, pos, x, tris, K=K_ID)


def _delaunayish(rng, W, H, n, name, K):
    # jittered grid: a generic mesh with random positions (mean area on either side of 64 by n)
    nx = int(np.sqrt(n * W / H))
    ny = max(1, n // nx)
    pos, tris = lattice(nx, ny, 1.0, diag=2)
    pos = pos * np.array([W / nx, H / ny], np.float32)
    pos += rng.uniform(-0.3, 0.3, pos.shape).astype(np.float32) * np.array([W / nx, H / ny], np.float32)
    x = (planar(pos, 0.6, 4e-4, -3e-4) * (1.0 + 0.05 * rng.random(len(pos)))).astype(np.float32)
    return mk(name, W, H, pos, x, tris, K=K)


def corpus():
    rng = np.random.default_rng(20261016)
    cases = [
        _lattice_soup(), _lattice_narrow(), _lattice_wide(), _offset(rng), _offset_dense(rng), _slivers(rng),
        _outside(640, 480, 5.0, "outside_5px", rng),
        _outside(640, 480, 1.0e4, "outside_1e4", rng, far=True),
        _outside(752, 480, 1.0e6, "outside_1e6", rng, far=True),
        _far_2p31(), _thin(517, 1, "row_517x1"), _thin(1, 389, "col_1x389"), _specials(), _cancel(),
        _delaunayish(rng, 640, 480, 2500, "random_640x480_sparse", K_TUM),
        _delaunayish(rng, 752, 480, 9000, "random_752x480_dense", K_SKEW),
    ]
    return {c["name"]: c for c in cases}


def filter_cases():
    """Graph-filter neighbourhoods: (name, x[V], edges[E,2]) -- even and odd sizes, ties, -0.0 beside +0.0,
    NaN, degree 0."""
    rng = np.random.default_rng(7)
    out = []
    star = [(0, k) for k in range(1, 6)] + [(k, 0) for k in range(6, 9)]  # degree 8 (n = 9) and 1 (n = 2)
    out.append(("star_zeros", np.array([0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.0], np.float32), star))
    out.append(("star_signed_zero_first", np.array([-0.0, 0.0, 0.0, 1.0, -1.0, 0.0, -0.0, 2.0, 0.0], np.float32), star))
    out.append(("star_nan", np.array([1.0, np.nan, 3.0, 2.0, np.nan, 5.0, 0.0, 4.0, 1.0], np.float32), star))
    out.append(("pair_nan", np.array([np.nan, 1.0, 1.0, np.nan], np.float32), [(0, 1), (2, 3)]))
    out.append(("path_even_odd", np.array([1, 5, 2, 9, 9, 2, 7, 7], np.float32), [(k, k + 1) for k in range(6)]))
    c = corpus()["random_640x480_sparse"]
    vals = np.array([0.0, -0.0, 0.5, 0.5, 1.0, np.nan, -1.0, np.inf], np.float32)
    x = vals[rng.integers(0, len(vals), len(c["x"]))]
    out.append(("mesh_ties", x, c["edges"]))
    x = (0.3 + rng.random(len(c["x"]))).astype(np.float32)
    out.append(("mesh_generic", x, c["edges"]))
    return [(n, np.asarray(x, np.float32), np.asarray(e, np.int32).reshape(-1, 2)) for n, x, e in out]
