"""Cases of the prediction stage shared by tests/test_predict_ref.py (CPU: the restatement against ground truth and its rules)
and tests/test_gpu_predict.py (GPU: the kernels against the restatement, bit for bit).  A case is a dict: W, H, K4, Tp / Tc
(T_world_prev / T_world_cur, 3x4 float64), pos (V x 2 float32), x (V float32), tris (T x 3 int32), tri_valid (T uint8), pix
(n x 2 float32) and, where the GPU's triangle stage has to reproduce tri_valid with a filter, min_idepth."""
import numpy as np
from scipy.spatial import ConvexHull, Delaunay

from tests import frontend_scenes as S

F = np.float32
W, H, K4 = S.W, S.H, S.K4
IDENT = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)


def pose(t=(0.0, 0.0, 0.0), r=(0.0, 0.0, 0.0)):
    return np.concatenate([S.rotation(*r), np.array(t, np.float64)[:, None]], axis=1)


def case(pos, x, tris, Tp, Tc, pix, tri_valid=None, w=W, h=H, **extra):
    tris = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
    c = dict(W=w, H=h, K4=K4, Tp=np.asarray(Tp, np.float64), Tc=np.asarray(Tc, np.float64),
             pos=np.ascontiguousarray(pos, F).reshape(-1, 2), x=np.ascontiguousarray(x, F), tris=tris,
             tri_valid=np.ones(len(tris), np.uint8) if tri_valid is None else np.ascontiguousarray(tri_valid, np.uint8),
             pix=np.ascontiguousarray(pix, F).reshape(-1, 2))
    c.update(extra)
    return c


def warp_f64(c):
    """The vertices' pixels in the current view, in float64 geometry (no restatement involved)."""
    fx, fy, cx, cy = K4
    p, x = c["pos"].astype(np.float64), c["x"].astype(np.float64)
    X = np.stack([(p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy, np.ones(len(p))], -1) / x[:, None]
    Xw = X @ c["Tp"][:, :3].T + c["Tp"][:, 3]
    Xc = (Xw - c["Tc"][:, 3]) @ c["Tc"][:, :3]
    return np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], -1)


def inside_hull_by(pts, q, margin):
    """q (n x 2) lies at least `margin` px inside the convex hull of pts (float64)."""
    hull = ConvexHull(pts)
    # hull.equations: unit normal n and offset d with n . p + d <= 0 inside
    dist = q @ hull.equations[:, :2].T + hull.equations[:, 2]
    return (dist <= -margin).all(axis=1)


# ---- ground truth on planes ----
def lattice(seed, step=12.0, jitter=3.0):
    rng = np.random.default_rng(seed)
    xs, ys = np.meshgrid(np.arange(step / 2, W, step), np.arange(step / 2, H, step))
    p = np.stack([xs.ravel(), ys.ravel()], -1) + rng.uniform(-jitter, jitter, (xs.size, 2))
    return p.astype(F)


def plane_case(name, k, seed=0, pos=None, n_query=300):
    """Pose 0 -> pose k of a scene of tests/frontend_scenes.py; the previous mesh carries the plane's exact idepths."""
    Tp, Tc = S.scene_pose(name, 0), S.scene_pose(name, k)
    pos = lattice(seed) if pos is None else pos
    x = S.plane_idepth(K4, Tp, pos[:, 0].astype(np.float64), pos[:, 1].astype(np.float64))[0].astype(F)
    tris = Delaunay(pos.astype(np.float64)).simplices
    rng = np.random.default_rng(1000 + seed + k)
    pix = np.stack([rng.uniform(0, W - 1, n_query), rng.uniform(0, H - 1, n_query)], -1).astype(F)
    c = case(pos, x, tris, Tp, Tc, pix)
    q = c["pix"].astype(np.float64)
    c["truth"] = S.plane_idepth(K4, Tc, q[:, 0], q[:, 1])[0]
    c["must"] = inside_hull_by(warp_f64(c), q, 2.0)  # (every query is inside the image by construction)
    return c


def dense_plane_case():
    """~2 500 vertices on 160 x 120: triangles of a few pixels (the 8-lanes-per-triangle scheme), and a 40 x 30 px window
    without vertices that the triangulation bridges with long triangles, whose pixel boxes are far above 256 pixels."""
    rng = np.random.default_rng(7)
    pos = np.unique(np.stack([rng.uniform(0.5, W - 1.5, 2650), rng.uniform(0.5, H - 1.5, 2650)], -1).astype(F), axis=0)
    pos = pos[~((pos[:, 0] > 60) & (pos[:, 0] < 100) & (pos[:, 1] > 45) & (pos[:, 1] < 75))]
    return plane_case("forward", 3, seed=7, pos=pos, n_query=300)


# ---- rules, each on a hand-built mesh ----
def grid_mesh(nx, ny, x0, y0, step):
    xs, ys = np.meshgrid(x0 + step * np.arange(nx), y0 + step * np.arange(ny))
    pos = np.stack([xs.ravel(), ys.ravel()], -1).astype(F)
    tris = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a = j * nx + i
            tris += [(a, a + 1, a + nx + 1), (a, a + nx + 1, a + nx)]
    return pos, np.array(tris, np.int32)


def all_pixels(w=W, h=H):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([xx.ravel(), yy.ravel()], -1).astype(F)


def identity_case():
    """Identity motion; queries: the interior vertices' own pixels, then one outside the image on every side, a huge one, a
    NaN one, and one on an empty pixel."""
    pos, tris = grid_mesh(4, 4, 20.0, 15.0, 11.0)
    x = (0.2 + 0.05 * np.arange(16) % 0.37).astype(F)
    interior = np.array([5, 6, 9, 10])
    odd = np.array([[-3.0, 20.0], [20.0, -0.75], [W - 0.25, 20.0], [20.0, H + 4.0], [1e12, 20.0], [np.nan, 20.0], [150.5, 100.25]], F)
    return case(pos, x, tris, IDENT, IDENT, np.concatenate([pos[interior], odd]), interior=interior, n_odd=len(odd))


def occlusion_case():
    """Far patch (idepth 0.3) left of a near patch (1.0); the camera moves 0.1 to the right: the near patch slides 14 px to
    the left, over the far one (4.2 px)."""
    pf, tf = grid_mesh(3, 3, 10.0, 10.0, 10.0)   # x 10 .. 30
    pn, tn = grid_mesh(3, 3, 34.0, 10.0, 8.0)    # x 34 .. 50
    pos = np.concatenate([pf, pn])
    x = np.concatenate([np.full(9, 0.3), np.full(9, 1.0)]).astype(F)
    return case(pos, x, np.concatenate([tf, tn + 9]), IDENT, pose((0.1, 0.0, 0.0)), all_pixels(), n_far_tris=len(tf))


def flip_case():
    """a left of b in the previous view, b left of a in the current one: the triangle is seen from behind."""
    pos = np.array([[20.0, 10.0], [24.0, 10.0], [22.0, 30.0]], F)
    return case(pos, np.array([0.2, 1.0, 0.5], F), [(0, 1, 2)], IDENT, pose((0.1, 0.0, 0.0)), all_pixels())


def poisoned_case(kind):
    """A 3 x 3 grid (8 triangles) under a forward motion of 1.0; vertex 4, the centre, is poisoned: idepth 2 puts it behind the
    current camera (w2 = 1 - 2 <= 0), or its idepth is 0, negative or NaN."""
    pos, tris = grid_mesh(3, 3, 60.0, 35.0, 14.0)
    x = np.full(9, 0.2, F)
    x[4] = {"behind": 2.0, "zero": 0.0, "negative": -0.5, "nan": np.nan}[kind]
    return case(pos, x, tris, IDENT, pose((0.0, 0.0, 1.0)), all_pixels(), poisoned=4)


def hole_case():
    """One corner vertex below min_triangle_idepth: the idepth filter of the triangle stage makes its triangles invalid."""
    pos, tris = grid_mesh(3, 3, 60.0, 35.0, 14.0)
    x = np.full(9, 0.4, F)
    x[8] = 0.1
    tv = (~(tris == 8).any(axis=1)).astype(np.uint8)
    return case(pos, x, tris, IDENT, pose((0.02, -0.01, 0.0)), all_pixels(), tri_valid=tv, min_idepth=0.15)


def shared_edge_case():
    """Two triangles whose shared edge is the diagonal through the pixel centres (4, 4) .. (24, 24)."""
    pos = np.array([[4.0, 4.0], [24.0, 4.0], [24.0, 24.0], [4.0, 24.0]], F)
    return case(pos, np.full(4, 0.5, F), [(0, 1, 2), (0, 2, 3)], IDENT, IDENT, all_pixels())


def two_triangle_case():
    """A 64 x 48 image covered by two triangles: boxes far above 256 pixels, a whole wave per triangle."""
    w, h = 64, 48
    pos = np.array([[-2.0, -2.0], [66.0, -2.0], [66.0, 50.0], [-2.0, 50.0]], F)
    x = np.array([0.3, 0.5, 0.45, 0.25], F)
    return case(pos, x, [(0, 1, 2), (0, 2, 3)], IDENT, pose((0.01, 0.005, 0.02), (0.002, -0.001, 0.003)), all_pixels(w, h)[::7], w=w, h=h)


RULE_CASES = {
    "identity": identity_case, "occlusion": occlusion_case, "flip": flip_case,
    "behind": lambda: poisoned_case("behind"), "zero": lambda: poisoned_case("zero"),
    "negative": lambda: poisoned_case("negative"), "nan": lambda: poisoned_case("nan"),
    "hole": hole_case, "shared_edge": shared_edge_case,
}


def winners(key):
    """The triangle ids that own at least one pixel of a key map."""
    k = key[key != 0]
    return set((0xFFFFFFFF - (k & np.uint64(0xFFFFFFFF))).astype(np.int64).tolist())
