"""Cases of the evaluate stage shared by tests/test_eval_ref.py (CPU: the restatement against hand-derived values and ground
truth) and tests/test_gpu_eval.py (GPU = restatement, bit for bit).  A case is a dict: K4, W, H, Tcmp / Tcur (T_world_cam of
the comparison and the current frame, 3x4 float64), idepth float32[H, W], cur / cmp uint8[H, W].  Cached; treat as read-only."""
import functools
import math

import numpy as np

from tests import frontend_scenes as S

F = np.float32
IDENT = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
K4_SMALL = (128.0, 128.0, 31.5, 23.5)  # with these every float32 operand of the shift cases is exact
W_SMALL, H_SMALL = 64, 48


def k9(K4):
    fx, fy, cx, cy = K4
    return np.array([fx, 0, cx, 0, fy, cy, 0, 0, 1], np.float32)


def kinv9(K4):
    fx, fy, cx, cy = K4
    return np.array([1 / fx, 0, -cx / fx, 0, 1 / fy, -cy / fy, 0, 0, 1], np.float32)


def translated(tx, ty=0.0, tz=0.0):
    T = IDENT.copy()
    T[:, 3] = (tx, ty, tz)
    return T


def _case(K4, Tcmp, Tcur, idepth, cur, cmp):
    H, W = cur.shape
    c = dict(K4=K4, W=W, H=H, Tcmp=np.asarray(Tcmp, np.float64), Tcur=np.asarray(Tcur, np.float64),
             idepth=np.ascontiguousarray(idepth, F), cur=np.ascontiguousarray(cur), cmp=np.ascontiguousarray(cmp))
    for a in (c["idepth"], c["cur"], c["cmp"]):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def exact_shift_case():
    """Constant map 0.5, T_cmp_cur translation (1/16, 0, 0): 128 x 0.5 / 16 = 4 pixels to the right, exactly."""
    rng = np.random.default_rng(11)
    cmp = rng.integers(0, 256, (H_SMALL, W_SMALL)).astype(np.uint8)
    cur = rng.integers(0, 256, (H_SMALL, W_SMALL)).astype(np.uint8)
    cur[:, :W_SMALL - 4] = cmp[:, 4:]
    return _case(K4_SMALL, IDENT, translated(1.0 / 16.0), np.full((H_SMALL, W_SMALL), 0.5, F), cur, cmp)


@functools.lru_cache(maxsize=None)
def half_pixel_case():
    """Translation 1/128: half a pixel to the right, both images random."""
    rng = np.random.default_rng(12)
    cmp = rng.integers(0, 256, (H_SMALL, W_SMALL)).astype(np.uint8)
    cur = rng.integers(0, 256, (H_SMALL, W_SMALL)).astype(np.uint8)
    return _case(K4_SMALL, IDENT, translated(1.0 / 128.0), np.full((H_SMALL, W_SMALL), 0.5, F), cur, cmp)


NO_IDEPTH_ROWS = {"nan": 3, "zero": 10, "negative": 17, "inf": 24}


@functools.lru_cache(maxsize=None)
def no_idepth_case():
    """The exact-shift case with one row each of NaN, 0, negative and +inf idepths."""
    c = exact_shift_case()
    m = c["idepth"].copy()
    for kind, v in (("nan", np.nan), ("zero", 0.0), ("negative", -0.5), ("inf", np.inf)):
        m[NO_IDEPTH_ROWS[kind]] = v
    return _case(c["K4"], c["Tcmp"], c["Tcur"], m, c["cur"], c["cmp"])


BEHIND_THETA = 1.45  # rotation about y: w2 = cos - sin x b0 <= 0 where b0 >= cot(1.45) = 0.1214, i.e. column >= 47.04


@functools.lru_cache(maxsize=None)
def behind_case():
    """The current camera turned by 1.45 rad about y against the comparison camera: the rays of the right-hand columns
    point behind it."""
    c = exact_shift_case()
    s, co = math.sin(BEHIND_THETA), math.cos(BEHIND_THETA)
    T = np.array([[co, 0.0, s, 0.0], [0.0, 1.0, 0.0, 0.0], [-s, 0.0, co, 0.0]])
    return _case(c["K4"], IDENT, T, c["idepth"], c["cur"], c["cmp"])


@functools.lru_cache(maxsize=None)
def scene_case(name, k, gain=1.0):
    """Frame k of a scene of tests/frontend_scenes.py against frame 0, with gain x the plane's exact idepth map."""
    frames = S.scene(name, 5)
    (cmp, Tcmp), (cur, Tcur) = frames[0], frames[k]
    yy, xx = np.mgrid[0:S.H, 0:S.W].astype(np.float64)
    idepth = (gain * S.plane_idepth(S.K4, Tcur, xx, yy)[0]).astype(F)
    return _case(S.K4, Tcmp, Tcur, idepth, cur, cmp)


@functools.lru_cache(maxsize=None)
def odd_case():
    """37 x 29 = 1 073 pixels (one full block of 1 024 and a tail of 49), both images in rows padded to 41 bytes; general
    motion, a map with holes and every class present."""
    W, H, pitch = 37, 29, 41
    rng = np.random.default_rng(13)
    cmp_p = rng.integers(0, 256, (H, pitch)).astype(np.uint8)
    cur_p = rng.integers(0, 256, (H, pitch)).astype(np.uint8)
    K4 = (40.0, 43.0, 17.5, 14.25)
    idepth = rng.uniform(0.2, 1.5, (H, W)).astype(F)
    idepth[rng.random((H, W)) < 0.15] = np.nan
    idepth[5, 7], idepth[6, 7], idepth[7, 7] = 0.0, -1.0, np.inf
    idepth[8, 0:6] = 40.0  # with tz = -0.05: w2 = 1 - 2 <= 0, behind
    T = np.concatenate([S.rotation(0.01, -0.02, 0.03), np.array([[0.08], [-0.03], [-0.05]])], axis=1)
    c = _case(K4, IDENT, T, idepth, cur_p[:, :W], cmp_p[:, :W])
    c["cur_padded"], c["cmp_padded"], c["pitch"] = cur_p, cmp_p, pitch
    return c


@functools.lru_cache(maxsize=None)
def truth_case(W, H, seed=14):
    """(idepth, depth) float32[H, W] holding all four classes: NaN / 0 / negative depths (no truth), NaN idepths (no
    estimate), and an infinite idepth with and without truth (an estimate, as in the reference)."""
    rng = np.random.default_rng(seed)
    depth = rng.uniform(0.5, 8.0, (H, W)).astype(F)
    idepth = (1.0 / depth.astype(np.float64) * rng.uniform(0.8, 1.25, (H, W))).astype(F)
    r = rng.random((H, W))
    depth[r < 0.1] = np.nan
    depth[(r >= 0.1) & (r < 0.2)] = 0.0
    depth[(r >= 0.2) & (r < 0.25)] = -1.0
    idepth[rng.random((H, W)) < 0.3] = np.nan
    depth[0, 0], idepth[0, 0] = 2.0, np.inf
    depth[0, 1], idepth[0, 1] = 0.0, np.inf
    depth[0, 2], idepth[0, 2] = 2.0, np.nan
    depth[0, 3], idepth[0, 3] = np.nan, np.nan
    depth[0, 4], idepth[0, 4] = -1.0, 0.25
    idepth.setflags(write=False)
    depth.setflags(write=False)
    return idepth, depth


PHOTO_CASES = {
    "exact_shift": exact_shift_case,
    "half_pixel": half_pixel_case,
    "no_idepth": no_idepth_case,
    "behind": behind_case,
    "odd": odd_case,
    "forward_3": lambda: scene_case("forward", 3),
    "refpose_nonidentity_5": lambda: scene_case("refpose_nonidentity", 5),
}
