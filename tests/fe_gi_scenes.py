"""Scenes for the gain-invariant matching cost, built on tests/fe_zm_scenes.py without touching it.

"Halved" scenes: every frame of a plain fe_zm_scenes scene integer-divided by two, values 20 ... 107, so that twice the image plus
any offset within +-24 stays inside 0 ... 255.  Their gained copies: a frame that is no pose frame becomes 2 v + b with b from
fe_zm_scenes.random_offsets(7) -- a power-of-two gain and an offset, EXACTLY, no rounding --, a pose frame becomes v + |b| (an offset
only: a gain on a pose frame is not claimed invariant).  The builder asserts that nothing clips.  Halved scenes serve invariance
only: `// 2` is no rendering of the plane, so they are not compared with ground truth.

Ground truth under a general gain comes from fe_zm_scenes.scene(gain=...) itself (frames 1 ... are floor(gain v + 0.5))."""
import numpy as np

from tests import fe_zm_scenes as ZS
from tests import frontend_scenes as SC

W, H, K, K4 = ZS.W, ZS.H, ZS.K, ZS.K4
HALF_LO, HALF_HI = ZS.TEX_LO // 2, ZS.TEX_HI // 2  # 20, 107
POSEFRAMES = (0, 4)
GAIN = 2


def halved(name, seed=1, frames=SC.FRAMES):
    """[(image, T_world_cam)]: the plain scene // 2."""
    out = []
    for img, T in ZS.scene(name, seed, frames=frames):
        v = img.astype(np.int64) // 2
        assert v.min() >= HALF_LO and v.max() <= HALF_HI
        h = v.astype(np.uint8)
        h.setflags(write=False)
        out.append((h, T))
    return out


def gained(name, seed=1, frames=SC.FRAMES, poseframes=POSEFRAMES, offsets=None):
    """The halved scene with frame k turned into 2 v + b_k (no pose frame) or v + |b_k| (a pose frame); returns (frames, offsets)."""
    offsets = ZS.random_offsets(7, frames) if offsets is None else [int(b) for b in offsets]
    assert len(offsets) == frames and all(0 < abs(b) <= ZS.MAX_OFFSET for b in offsets)
    out = []
    for k, ((img, T), b) in enumerate(zip(halved(name, seed, frames), offsets)):
        v = img.astype(np.int64)
        g = v + abs(b) if k in poseframes else GAIN * v + b
        assert g.min() >= 0 and g.max() <= 255, "the scene clips"
        gi = g.astype(np.uint8)
        gi.setflags(write=False)
        out.append((gi, T))
    return out, offsets
