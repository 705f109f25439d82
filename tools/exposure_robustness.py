"""What a brightness step between a pose frame and the frames tracked against it does to the feature front end, per matching cost
(GpuFrontEnd.set_cost: SSD / ZSSD; GpuFrontEnd.set_gain_invariant: GI) and window size: the tables of DESIGN.md 6 "Matching cost".
A measurement tool, not a gate.

Scene: tests/fe_zm_scenes.py "sideways" (the slanted plane, 160 x 120, six frames, frame 0 the pose frame, about 5 px per texel,
grey levels in [40, 215]); frames 1...5 get gain * I + b.  With --smooth also tests/frontend_scenes.py's texture (about 15 px per
texel: a 5 x 5 window sees one ramp), its offset images clipped at 0 / 255.  Per run: the emitted features of the last frame, how
many of them are converged (var < 0.01), the median and the worst relative inverse-depth error of those against the plane, and
the BAD_MATCH count over the five tracking frames.

--gain-table: the exposure-step table instead -- win_size 7, the scenes "sideways", "diagonal_roll" and "refpose_nonidentity" at
gains 1, 0.8 and 0.6 (frames 1...5 are floor(gain * I + 0.5), nothing clips), ZSSD beside the gain-invariant cost: converged /
emitted features of the last frame and the median relative inverse-depth error of the converged ones.

    python tools/exposure_robustness.py [--smooth] [--gain-table] [--restatement]

--restatement runs tests/frontend_ref.py with the gain-invariant cost of tests/fe_gi_ref.py on the CPU instead of the device (the device equals
it bit for bit: tests/test_gpu_fe_zm.py, tests/test_gpu_fe_gi.py).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

INPUTS = (("b = 0", None, 0), ("b = +12", None, 12), ("gain 1.08, b = +8", 1.08, 8), ("gain 0.8", 0.8, 0), ("gain 0.6", 0.6, 0))
GAIN_SCENES, GAINS = ("sideways", "diagonal_roll", "refpose_nonidentity"), (1.0, 0.8, 0.6)
SMOOTH_INPUTS = (("b = 0", None, 0), ("b = +6", None, 6))


def frames_of(smooth, gain, b):
    from tests import fe_zm_scenes as ZS
    from tests import frontend_scenes as SC
    if not smooth:
        return ZS.scene("sideways", 1, [0] + [b] * (SC.FRAMES - 1), gain=gain)
    out = []
    for k, (img, T) in enumerate(SC.scene("sideways", 1)):
        v = img.astype(np.float64) if k == 0 else np.floor((gain or 1.0) * img + b + 0.5)
        out.append((np.clip(v, 0, 255).astype(np.uint8), T))
    return out


def run(frames, win, zero_mean, restatement, gain_invariant=False):
    from tests import fe_zm_scenes as ZS
    if restatement:
        from tests import frontend_ref as R
        fe, p = R.FrontEndRef(ZS.W, ZS.H, ZS.K, 256, 4), R.params(win_size=win)
        bad = lambda: fe.counts.get(R.BAD_MATCH, 0)  # noqa: E731
    else:
        from flame_ros_amd.frontend import GpuFrontEnd, default_frontend_params
        fe, p = GpuFrontEnd(ZS.W, ZS.H, ZS.K, 256, 4), default_frontend_params(win_size=win)
        bad = lambda: fe.info("bad_match")  # noqa: E731
    fe.set_cost(zero_mean=zero_mean)
    if gain_invariant:
        fe.set_gain_invariant(True)
    n_bad = 0
    for k, (img, T) in enumerate(frames):
        out = fe.track(p, img, k, T, k == 0)
        n_bad += bad()
    err, emitted = ZS.relative_errors(out, T)
    if not restatement:
        fe.close()
    return emitted, len(err), (100 * float(np.median(err)), 100 * float(err.max())) if len(err) else (float("nan"), float("nan")), n_bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--smooth", action="store_true")
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--gain-table", action="store_true")
    a = ap.parse_args()
    if a.gain_table:
        from tests import fe_zm_scenes as ZS
        print("\nwin_size 7, frames 1...5 = floor(gain * I + 0.5): converged / emitted, median %\n")
        print("| scene | gain | ZSSD | gain-invariant |\n|---|---|---|---|")
        for name in GAIN_SCENES:
            for gain in GAINS:
                frames = ZS.scene(name, 1, gain=None if gain == 1.0 else gain)
                cells = []
                for gi in (False, True):
                    emitted, conv, (med, worst), n_bad = run(frames, 7, True, a.restatement, gain_invariant=gi)
                    cells.append("%d/%d, %.2f %% (worst %.1f %%)" % (conv, emitted, med, worst))
                print("| %s | %g | %s | %s |" % (name, gain, cells[0], cells[1]), flush=True)
        return
    for smooth in ([False, True] if a.smooth else [False]):
        print("\n%s texture: emitted / converged, median %% (worst %%), BAD_MATCH\n" % ("smooth (15 px per texel)" if smooth else "fine (5 px per texel)"))
        print("| input | win | SSD | ZSSD | gain-invariant |\n|---|---|---|---|---|")
        for label, gain, b in (SMOOTH_INPUTS if smooth else INPUTS):
            frames = frames_of(smooth, gain, b)
            for win in (5, 7, 9):
                cells = []
                for zm, gi in ((False, False), (True, False), (False, True)):
                    emitted, conv, (med, worst), n_bad = run(frames, win, zm, a.restatement, gain_invariant=gi)
                    cells.append("%d / %d, %.2f %% (%.1f %%), %d" % (emitted, conv, med, worst, n_bad))
                print("| %s | %d | %s |" % (label, win, " | ".join(cells)), flush=True)


if __name__ == "__main__":
    main()
