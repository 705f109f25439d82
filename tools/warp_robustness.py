"""What a roll or a change of distance against the pose frame does to the feature front end, with the warped matching window
(GpuFrontEnd.set_warp) off and on, per window size and matching cost: the table of DESIGN.md 6 "Warped window".  A measurement
tool, not a gate.

Scenes: tests/fe_warp_scenes.py -- tests/fe_zm_scenes.py's plane, camera and renderer (160 x 120, texture seed 5), eight frames,
frame 0 the pose frame; the frames 1 ... 7 are rolled by one angle and moved along the optical axis by one step against it.  Per
run, in the last frame: the emitted features, those of them that are converged (var < 0.01), the median relative inverse-depth
error of the converged ones against the plane, how many are off by more than 10 %, and the features the warp refused.

    python tools/warp_robustness.py [--device] [--wins 5,7,9] [--costs ssd,zssd,gi]

By default the restatement tests/fe_warp_ref.py runs on the CPU; --device runs the library (which equals it bit for bit:
tests/test_gpu_fe_warp.py).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# label -> (roll in degrees, forward step in metres)
SCENES = [("roll 0", (0.0, 0.0)), ("roll 10", (10.0, 0.0)), ("roll 20", (20.0, 0.0)), ("roll 30", (30.0, 0.0)), ("roll 90", (90.0, 0.0)),
          ("roll 180", (180.0, 0.0)), ("1 m back", (0.0, -1.0)), ("roll 30, 0.6 m closer", (30.0, 0.6))]


def run(frames, win, cost, warp, device):
    from tests import fe_warp_scenes as WS
    from tests import frontend_ref as R
    if device:
        from flame_ros_amd.frontend import GpuFrontEnd, default_frontend_params
        fe, p = GpuFrontEnd(WS.W, WS.H, WS.K, 256, 4), default_frontend_params(win_size=win)
        refused = lambda: fe.info("warp_refused")  # noqa: E731
    else:
        fe, p = R.FrontEndRef(WS.W, WS.H, WS.K, 256, 4), R.params(win_size=win)
        refused = fe.warp_refused
    fe.set_cost(cost == "zssd")
    fe.set_gain_invariant(cost == "gi")
    fe.set_warp(warp)
    for k, (img, T) in enumerate(frames):
        out = fe.track(p, img, k, T, k == 0)
    n = refused()
    err, emitted = WS.ZS.relative_errors(out, T)
    if device:
        fe.close()
    return emitted, len(err), 100 * float(np.median(err)) if len(err) else float("nan"), int((err > 0.10).sum()), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--wins", default="5,7,9")
    ap.add_argument("--costs", default="ssd,zssd,gi")
    a = ap.parse_args()
    from tests import fe_warp_scenes as WS
    print("last frame: emitted, converged (median error %, off by > 10 %), refused by the warp\n")
    print("| scene | win | cost | switch off | switch on |\n|---|---|---|---|---|")
    for label, (roll, fwd) in SCENES:
        frames = WS.custom(roll, fwd)
        for win in (int(w) for w in a.wins.split(",")):
            for cost in a.costs.split(","):
                cells = []
                for warp in (False, True):
                    emitted, conv, med, off, refused = run(frames, win, cost, warp, a.device)
                    cells.append("%d, %d (%.2f %%, %d), %d" % (emitted, conv, med, off, refused))
                print("| %s | %d | %s | %s | %s |" % (label, win, cost, cells[0], cells[1]), flush=True)


if __name__ == "__main__":
    main()
