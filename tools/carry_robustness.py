"""What the eviction of a pose frame does to the feature front end of a hovering camera, with the hand-over
(GpuFrontEnd.set_carry) off and on, per ring size: the table of DESIGN.md 6 "What the hand-over buys".  A measurement tool, not a
gate.

Scene: tests/fe_carry_ref.py -- frontend_ref's slanted plane at 160 x 120 (texture seed 1); the camera swings sideways and back with
period 8, x = 0.06 (0, 1, 2, 3, 4, 3, 2, 1, ...) m and yaw 0.004 rad times the same numbers; 60 frames, default parameters.  Ring of
1: a pose frame every 2nd frame; rings of 2 and 4: every 3rd.  Per run: the graph's vertices per frame (emitted features with
idepth_var < 0.01) over the frames from `first` on -- their range and the frames without any --, the median relative inverse-depth
error of the vertices in each of the last 10 frames (its range), the worst frame's number of vertices off by more than 5 %, and the
features carried / lost over all evictions.

    python tools/carry_robustness.py [--ref] [--rings 1,2,4] [--frames 60]

By default the library runs on the device; --ref runs the restatement tests/fe_carry_ref.py on the CPU (which the device equals bit
for bit: tests/test_gpu_fe_carry.py), so the table can be made on a machine without a GPU.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run(frames, ring, every, on, ref):
    from tests import fe_carry_ref as CR
    from tests import frontend_ref as R
    if ref:
        fe, p = CR.CarryRef(R.SCENE_W, R.SCENE_H, R.SCENE_K, 256, ring), R.params()
    else:
        from flame_ros_amd.frontend import GpuFrontEnd, default_frontend_params
        fe, p = GpuFrontEnd(R.SCENE_W, R.SCENE_H, R.SCENE_K, 256, ring), default_frontend_params()
    fe.set_carry(on)
    rows = CR.hover_run(fe, p, frames, every)
    if not ref:
        fe.close()
    first = every * ring  # the first evicting frame
    n = [r[0] for r in rows[first:]]
    empty = [first + k for k, x in enumerate(n) if x == 0]
    med = [100 * float(np.median(r[1])) for r in rows[-10:] if len(r[1])]
    off5 = max(int((r[1] > 0.05).sum()) for r in rows[first:])
    cell = "%d … %d" % (min(n), max(n))
    if empty:
        cell += "; 0 at %s" % ", ".join(str(k) for k in empty[:6]) + (" …" if len(empty) > 6 else "")
    err = "%.2f … %.2f %%" % (min(med), max(med)) if med else "-"
    return cell, err, off5, sum(r[2] for r in rows), sum(r[3] for r in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", action="store_true")
    ap.add_argument("--rings", default="1,2,4")
    ap.add_argument("--frames", type=int, default=60)
    a = ap.parse_args()
    from tests import fe_carry_ref as CR
    frames = CR.hover_scene(1, a.frames)
    print("%s; frames from the first evicting one on: graph vertices | median relative idepth error, last 10 frames | "
          "most vertices off by > 5 %% in a frame | carried, lost\n" % ("restatement" if a.ref else "device"))
    print("| ring | pose frame every | switch off | switch on |\n|---|---|---|---|")
    for ring in (int(r) for r in a.rings.split(",")):
        every = 2 if ring == 1 else 3
        cells = []
        for on in (False, True):
            n, err, off5, carried, lost = run(frames, ring, every, on, a.ref)
            cells.append("%s | %s | %d | %d, %d" % (n, err, off5, carried, lost))
        print("| %d | %d | %s | %s |" % (ring, every, cells[0].replace(" | ", "; "), cells[1].replace(" | ", "; ")), flush=True)


if __name__ == "__main__":
    main()
