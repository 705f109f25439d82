"""What an edge parallel to the epipolar line does to the feature front end, with the reference-patch gradient gate
(GpuFrontEnd.set_ref_grad) off and on, per window size: the table of DESIGN.md 6 "Reference-patch gradient".  A measurement tool,
not a gate.

Scenes: tests/fe_rg_ref.py half_striped() -- tests/frontend_scenes.py's plane and poses ("sideways", "vertical": 160 x 120, six
frames, frame 0 the pose frame) under tests/fe_zm_scenes.py's renderer; the left half of the texture is isotropic, the right half
is stripes that are constant along the camera's motion.  With --isotropic also the six scenes of tests/fe_zm_scenes.py (no
stripes: what the gate costs where it is not needed).  Per run: the features refused in the last frame out of those tested, the
emitted features of the last frame that are converged (var < 0.01), how many of those are off by more than 10 % against the
plane, and the worst relative error.

    python tools/aperture_robustness.py [--device] [--isotropic] [--min-grad 5.0]

By default the restatement tests/fe_rg_ref.py runs on the CPU; --device runs the library (which equals it bit for bit:
tests/test_gpu_fe_rg.py).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run(frames, win, min_grad, device):
    from tests import fe_rg_ref as RG
    from tests import fe_zm_scenes as ZS
    from tests import frontend_ref as R
    if device:
        from flame_ros_amd.frontend import GpuFrontEnd, default_frontend_params
        fe, p = GpuFrontEnd(ZS.W, ZS.H, ZS.K, 256, 4), default_frontend_params(win_size=win)
        counts = lambda: (fe.info("fail_ref_grad"), sum(fe.info(k) for k in ("ok", "bad_match", "ambiguous")) + fe.info("fail_ref_grad"))  # noqa: E731
    else:
        fe, p = R.FrontEndRef(ZS.W, ZS.H, ZS.K, 256, 4), R.params(win_size=win)
        counts = lambda: (fe.counts.get(RG.REF_GRAD, 0), sum(fe.counts.get(k, 0) for k in (R.OK, R.BAD_MATCH, R.AMBIGUOUS, RG.REF_GRAD)))  # noqa: E731
    fe.set_ref_grad(min_grad)
    for k, (img, T) in enumerate(frames):
        out = fe.track(p, img, k, T, k == 0)
    refused, tested = counts()
    err, _ = ZS.relative_errors(out, T)
    if device:
        fe.close()
    return refused, tested, len(err), int((err > 0.10).sum()), 100 * float(err.max()) if len(err) else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--isotropic", action="store_true")
    ap.add_argument("--min-grad", type=float, default=5.0)
    a = ap.parse_args()
    from tests import fe_rg_ref as RG
    from tests import fe_zm_scenes as ZS
    from tests import frontend_scenes as SC
    scenes = [("half-striped " + n, RG.half_striped(n)) for n in RG.HALF_STRIPED]
    if a.isotropic:
        scenes += [(n, ZS.scene(n, 5)) for n in SC.NAMES]
    print("refused / searched in the last frame; converged, of those off by > 10 %% (worst %%); min_grad %.1f\n" % a.min_grad)
    print("| scene | win | gate off | gate on |\n|---|---|---|---|")
    for label, frames in scenes:
        for win in (5, 7, 9):
            cells = []
            for g in (0.0, a.min_grad):
                refused, tested, conv, off, worst = run(frames, win, g, a.device)
                cells.append("%d / %d; %d, %d (%.1f %%)" % (refused, tested, conv, off, worst))
            print("| %s | %d | %s | %s |" % (label, win, cells[0], cells[1]))


if __name__ == "__main__":
    main()
