"""Scenes for the warped matching window (DESIGN.md 5.3 "Warped window"): the plane, the camera and the renderer of
tests/fe_zm_scenes.py (texture seed 5, 160 x 120), eight frames, frame 0 the pose frame at the identity; the frames 1 ... 7 are rolled
by one constant angle about the optical axis and moved by one constant step along it against the pose frame, and drift sideways as
the other scenes do:  T_k = [rotation(0, 0.004 k, roll [k > 0]) | (0.03 k, 0.01 k, fwd [k > 0])].  Rendered per pixel in float64 (no
kernel, no restatement involved): the plane's inverse depth at any pixel of any frame is ground truth.  Also the pure translation
on which the switch may change no bit, the same renderer at other image sizes, and the two refusal cases."""
import math

import numpy as np

from tests import fe_zm_scenes as ZS
from tests import frontend_scenes as SC

W, H, K, K4 = ZS.W, ZS.H, ZS.K, ZS.K4
SEED, FRAMES = 5, 8
# name -> (roll in degrees, forward step in metres)
CASES = {"roll30": (30.0, 0.0), "roll90": (90.0, 0.0), "roll180": (180.0, 0.0), "back": (0.0, -1.0), "roll30_closer": (30.0, 0.6)}
NAMES = tuple(CASES)
ROLL_ONLY = ("roll30", "roll90", "roll180")


def case_pose(roll_deg, fwd, k):
    on = 1.0 if k > 0 else 0.0
    return np.concatenate([SC.rotation(0.0, 0.004 * k, math.radians(roll_deg) * on),
                           np.array([[0.03 * k], [0.01 * k], [fwd * on]])], axis=1)


_cache = {}


def _frames(key, poses, render):
    if key not in _cache:
        out = []
        for T in poses:
            img = render(T).astype(np.uint8)
            img.setflags(write=False)
            out.append((img, T))
        _cache[key] = out
    return _cache[key]


def custom(roll_deg, fwd, frames=FRAMES):
    """[(image, T_world_cam)] of the family at any roll and forward step (the measurement tools' table)."""
    tex = ZS.texture(SEED)
    return _frames(("case", float(roll_deg), float(fwd), frames), [case_pose(roll_deg, fwd, k) for k in range(frames)],
                   lambda T: ZS.render(T, tex))


def scene(name, frames=FRAMES):
    return custom(*CASES[name], frames=frames)


def translation(frames=6):
    """R = I and t_z = 0 in every frame: A / f and w2 are exact in float32 and Jq = (256, 0, 0, 256) for every feature."""
    tex = ZS.texture(SEED)
    poses = [np.concatenate([np.eye(3), np.array([[0.03 * k], [-0.02 * k], [0.0]])], axis=1) for k in range(frames)]
    return _frames(("translation", frames), poses, lambda T: ZS.render(T, tex))


def render_at(T, tex, w, h, k4):
    """fe_zm_scenes.render at another image size and camera."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    _, X = SC.plane_idepth(k4, T, xx, yy)
    tu, tv = ZS.TEX_SCALE * X[..., 0] + ZS.TEX_ORIGIN, ZS.TEX_SCALE * X[..., 1] + ZS.TEX_ORIGIN
    u0, v0 = np.floor(tu).astype(int), np.floor(tv).astype(int)
    assert u0.min() >= 0 and v0.min() >= 0 and u0.max() + 1 < ZS.TEX_SIZE and v0.max() + 1 < ZS.TEX_SIZE
    fu, fv = tu - u0, tv - v0
    val = (1 - fv) * (1 - fu) * tex[v0, u0] + (1 - fv) * fu * tex[v0, u0 + 1] + fv * (1 - fu) * tex[v0 + 1, u0] + \
        fv * fu * tex[v0 + 1, u0 + 1]
    return np.floor(val + 0.5).astype(np.int64)


SMALL_W, SMALL_H = 48, 36
SMALL_K4 = (140.0, 140.0, 23.5, 17.5)  # (K_4836 of the GPU tests)


def small(roll_deg=45.0, frames=4):
    """48 x 36 under a roll of 45 degrees: most windows touch a border, and a turned window reaches further than an upright one."""
    tex = ZS.texture(SEED)
    return _frames(("small", float(roll_deg), frames), [case_pose(roll_deg, 0.0, k) for k in range(frames)],
                   lambda T: render_at(T, tex, SMALL_W, SMALL_H, SMALL_K4))


# The refusal cases run with a prior at the plane's depth and a narrow interval (the wide default prior reaches behind a camera that
# close): params(idepth_init=1/3, var_init=1e-4).  The second image is the pose frame's again: a refused feature reads no pixel.
REFUSAL_PRIOR = dict(idepth_init=1.0 / 3.0, var_init=1e-4)


def refusal(kind):
    """(pose of frame 1) of a refusal case against the pose frame at the identity.  "closer": 2.45 m forward towards a patch taken
    at 3 m, five and a half times closer: a stretch above 4.  "grazing": on the circle of radius 3 around the point (0, 0, 3),
    turned by 87 degrees towards it: a fronto-parallel patch there is seen edge-on, an area scale of cos 87 = 0.052 < 1/16."""
    if kind == "closer":
        return np.concatenate([np.eye(3), np.array([[0.01], [0.0], [2.45]])], axis=1)
    phi = math.radians(87.0)
    C = np.array([0.0, 0.0, 3.0]) - 3.0 * np.array([-math.sin(phi), 0.0, math.cos(phi)])
    return np.concatenate([SC.rotation(0.0, -phi, 0.0), C[:, None]], axis=1)
