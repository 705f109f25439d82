"""Exposure scenes for the zero-mean matching cost: the plane and the poses of tests/frontend_scenes.py under a finer texture --
texture coordinates 9 X + 128 on a 256 x 256 integer texture, about 5 px per texel, so a 7 x 7 window holds structure and not one
ramp -- whose values are restricted to [40, 215].  A frame's grey offset b (|b| <= 24) is added to the rendered integers, so it
never clips and the offset image is EXACTLY the plain image + b: floor(v + 0.5) + b = floor(v + b + 0.5).  The renderer asserts
both.  Rendered per pixel in float64 (no kernel, no restatement involved): the plane's inverse depth at any pixel of any frame is
ground truth (frontend_scenes.plane_idepth)."""
import numpy as np

from tests import frontend_scenes as SC

W, H, K, K4 = SC.W, SC.H, SC.K, SC.K4
TEX_LO, TEX_HI, MAX_OFFSET = 40, 215, 24
TEX_SCALE, TEX_ORIGIN, TEX_SIZE = 9.0, 128.0, 256


def texture(seed):
    return np.random.default_rng(seed).integers(TEX_LO, TEX_HI + 1, (TEX_SIZE, TEX_SIZE)).astype(np.float64)


def render(T, tex):
    """The plane from T_world_cam as integers (int64) in [TEX_LO, TEX_HI]."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    _, X = SC.plane_idepth(K4, T, xx, yy)
    tu, tv = TEX_SCALE * X[..., 0] + TEX_ORIGIN, TEX_SCALE * X[..., 1] + TEX_ORIGIN
    u0, v0 = np.floor(tu).astype(int), np.floor(tv).astype(int)
    assert u0.min() >= 0 and v0.min() >= 0 and u0.max() + 1 < TEX_SIZE and v0.max() + 1 < TEX_SIZE
    fu, fv = tu - u0, tv - v0
    val = (1 - fv) * (1 - fu) * tex[v0, u0] + (1 - fv) * fu * tex[v0, u0 + 1] + fv * (1 - fu) * tex[v0 + 1, u0] + \
        fv * fu * tex[v0 + 1, u0 + 1]
    out = np.floor(val + 0.5).astype(np.int64)
    assert out.min() >= TEX_LO and out.max() <= TEX_HI
    return out


_cache = {}


def _plain(name, seed, frames):
    key = (name, seed, frames)
    if key not in _cache:
        tex = texture(seed)
        _cache[key] = [(render(SC.scene_pose(name, k), tex), SC.scene_pose(name, k)) for k in range(frames)]
    return _cache[key]


def scene(name, seed, offsets=None, frames=SC.FRAMES, gain=None):
    """[(image, T_world_cam)] of the scene; frame k is the plain rendering + offsets[k] grey levels (the pose frame included).
    `gain` (measurement tools only): frames 1... are floor(gain * plain + offset + 0.5), which may not clip either."""
    offsets = [0] * frames if offsets is None else [int(b) for b in offsets]
    assert len(offsets) == frames and all(abs(b) <= MAX_OFFSET for b in offsets)
    out = []
    for k, ((base, T), b) in enumerate(zip(_plain(name, seed, frames), offsets)):
        v = base + b if gain is None or k == 0 else np.floor(gain * base + b + 0.5).astype(np.int64)
        assert v.min() >= 0 and v.max() <= 255, "the scene clips"
        img = v.astype(np.uint8)
        img.setflags(write=False)
        out.append((img, T))
    return out


def random_offsets(seed, frames=SC.FRAMES):
    """Per-frame offsets within +-MAX_OFFSET, none zero, the pose frame's included."""
    rng = np.random.default_rng(seed)
    return [int(b) for b in rng.choice(np.r_[-MAX_OFFSET:0, 1:MAX_OFFSET + 1], frames, replace=False)]


def relative_errors(out, T, var_max=0.01):
    """|mu - truth| / truth of the emitted features with var < var_max, and the number emitted."""
    conv = out["idepth_var"] < np.float32(var_max)
    vtx = out["vtx"][conv].astype(np.float64)
    truth, _ = SC.plane_idepth(K4, T, vtx[:, 0], vtx[:, 1])
    return np.abs(out["idepth_mu"][conv].astype(np.float64) - truth) / truth, len(out["slot"])
