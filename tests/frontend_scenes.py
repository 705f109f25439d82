"""General-motion plane scenes for the feature front end: fx != fy, an off-centre principal point, full rotations, vertical
and forward motion, a reference pose that is not the identity.  Rendered analytically per pixel in float64 (no kernel,
no restatement involved), so the plane's inverse depth at any pixel of any frame is ground truth."""
import math

import numpy as np

W, H = 160, 120
K4 = (140.0, 155.0, 83.5, 55.5)  # fx, fy, cx, cy
K = np.array([K4[0], 0, K4[2], 0, K4[1], K4[3], 0, 0, 1], np.float32)
PLANE_P0, PLANE_N = np.array([0.0, 0.0, 3.0]), np.array([0.2, -0.1, 1.0])
FRAMES = 6

# name -> k -> (translation, (rx, ry, rz)); T_world_cam = [Rz Ry Rx | t]; frame 0 is the pose frame
SCENES = {
    "sideways": lambda k: ((0.03 * k, 0.0, 0.0), (0.0, 0.004 * k, 0.0)),
    "vertical": lambda k: ((0.0, 0.03 * k, 0.0), (0.004 * k, 0.0, 0.0)),
    "diagonal_roll": lambda k: ((0.02 * k, -0.025 * k, 0.0), (0.0, 0.0, 0.01 * k)),
    "forward": lambda k: ((0.01 * k, 0.006 * k, 0.08 * k), (0.002 * k, -0.003 * k, 0.004 * k)),
    "backward_side": lambda k: ((-0.025 * k, 0.01 * k, -0.06 * k), (-0.003 * k, 0.002 * k, -0.006 * k)),
    "refpose_nonidentity": lambda k: ((0.5 - 0.02 * k, -0.3 + 0.02 * k, 0.2 + 0.02 * k), (0.05, -0.08 + 0.003 * k, 0.1)),
}
NAMES = tuple(SCENES)


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    Rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    return Rz @ Ry @ Rx


def scene_pose(name, k):
    t, r = SCENES[name](k)
    return np.concatenate([rotation(*r), np.array(t, np.float64)[:, None]], axis=1)


def plane_idepth(K4, T, x, y):
    """(true inverse depth, world point) of the plane at pixel (x, y) (arrays) of the camera at T_world_cam [R|t]."""
    fx, fy, cx, cy = (float(a) for a in K4)
    T = np.asarray(T, np.float64).reshape(3, 4)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    ray = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones_like(x)], -1) @ T[:, :3].T  # world direction, camera z = 1
    s = (PLANE_N @ (PLANE_P0 - T[:, 3])) / (ray @ PLANE_N)                              # = depth along the camera's z
    return 1.0 / s, T[:, 3] + s[..., None] * ray


def render(T, tex):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    _, X = plane_idepth(K4, T, xx, yy)
    tu, tv = 3.0 * X[..., 0] + 32.0, 3.0 * X[..., 1] + 32.0
    u0, v0 = np.floor(tu).astype(int), np.floor(tv).astype(int)
    fu, fv = tu - u0, tv - v0
    val = (1 - fv) * (1 - fu) * tex[v0, u0] + (1 - fv) * fu * tex[v0, u0 + 1] + fv * (1 - fu) * tex[v0 + 1, u0] + \
        fv * fu * tex[v0 + 1, u0 + 1]
    return np.floor(val + 0.5).astype(np.uint8)


_cache = {}


def scene(name, seed, frames=FRAMES):
    """[(image, T_world_cam)] of the scene; cached, treat as read-only."""
    key = (name, seed, frames)
    if key not in _cache:
        tex = np.random.default_rng(seed).integers(0, 256, (96, 96)).astype(np.float64)
        out = []
        for k in range(frames):
            T = scene_pose(name, k)
            img = render(T, tex)
            img.setflags(write=False)
            out.append((img, T))
        _cache[key] = out
    return _cache[key]
