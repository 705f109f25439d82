"""The feature front end's gates (DESIGN.md 5.3 "Gates"; include/flame_hip.h, flame_hip_frontend_set_gates) restated in NumPy:
the rules tests/frontend_ref.py's FrontEndRef applies after `set_gates`.  A helper, not a test: tests/test_fe_gates_ref.py checks it
rule by rule and against ground truth, tests/test_gpu_fe_gates.py compares the library with it bit for bit.

With a gate set the letterbox is part of the projection test (a refused projection is a failed one: the frame's one dropout, death
past max_dropouts), then comes the height band (a held feature keeps everything and is no candidate, its cell is remembered), and
the frame detects inside the band only and counts the held cells as occupied."""
import numpy as np

from tests import frontend_corpus as FC
from tests import frontend_ref as R

F = np.float32
BIG = float(np.finfo(np.float32).max)


# The bands of the ground-truth test (tests/test_fe_gates_ref.py) and of the GPU parity test, (min_height, max_height) along
# up = (0, 1, 0).  The margin 3 |d height / d xi| sigma = 3 |height - camera height| sigma / xi grows with the distance from the
# camera's own height (about 0.4 at the median converged feature), so an edge far from it leaves a third of the features
# undecided.  The edges therefore sit near the camera's height in the later frames (0 in "sideways", -0.2 in
# "refpose_nonidentity"), where the band still cuts the plane's image in two: one band keeps the lower side, the other the upper.
BANDS = {"sideways": (None, 0.05), "refpose_nonidentity": (-0.2, None)}


def band(H):
    """Rows y_lo <= y <= y_hi - 1 of the letterbox."""
    return H // 3, H - H // 3


def check_band(H, win):
    y_lo, y_hi = band(H)
    if y_hi - y_lo < 2 * (win // 2 + 1) + 1:
        raise ValueError("letterbox band of %d rows is narrower than a detection row with its windows" % (y_hi - y_lo))


def gate_record(T_world_cam, up):
    """hr = n^T R, h0 = n . t of T_world_cam = [R|t] in double (sums left to right), each rounded once to float32."""
    T = [[float(x) for x in row] for row in np.asarray(T_world_cam, np.float64).reshape(3, 4)]
    n = [float(F(a)) for a in up]
    h = [F((n[0] * T[0][j] + n[1] * T[1][j]) + n[2] * T[2][j]) for j in range(4)]
    return h[:3], h[3]


def height32(K4, hr, h0, px, py, xc):
    """Height of the projected feature (px, py, inverse depth xc) along the up vector: float32, every operation rounded."""
    fx, fy, cx, cy = K4
    bx, by = (px - cx) / fx, (py - cy) / fy
    return ((hr[0] * bx + hr[1] * by) + hr[2]) / xc + h0


def colliding_runs():
    """frontend_corpus._colliding's frames: after the step back several features share a cell.  Returns the case, an ungated
    run's record of frame 2 (a vacuous band, so that the restatement keeps every projection) and a pair (winner, loser) of one
    cell with their heights along up = (0, 1, 0)."""
    c = FC.case("colliding_then_poseframe")
    p = R.params(**c.kw)
    ref = R.FrontEndRef(FC.W, FC.H, c.K, FC.SLOTS, FC.RING)
    for call in c.calls[:2]:
        ref.track(p, call[1], call[4], call[2], call[3])
    ref.set_gates(min_height=-1e14, max_height=1e14, up=(0, 1, 0))
    _, img, T, is_pf, img_id = c.calls[2]
    out = ref.track(p, img, img_id, T, is_pf)
    assert ref.held == 0
    dws, ncx = p["detection_win_size"], (FC.W + p["detection_win_size"] - 1) // p["detection_win_size"]
    cells = {}
    for s, (px, py, xc, vc) in ref.proj_all.items():
        cells.setdefault((int(py) // dws) * ncx + int(px) // dws, []).append(s)
    hr, h0 = gate_record(T, (0, 1, 0))
    h = {s: height32(ref.K4, hr, h0, *ref.proj_all[s][:3]) for s in ref.proj_all}
    pairs = []
    for cell, ss in cells.items():
        if len(ss) >= 2:
            ss = sorted(ss, key=lambda s: (int(F(ref.proj_all[s][3]).view(np.uint32)), s))
            if h[ss[0]] != h[ss[1]] and not any(h[s] == h[ss[1]] for s in ss[2:]):
                pairs.append((cell, ss[0], ss[1]))
    assert pairs
    return c, p, ref, out, pairs[0], h
