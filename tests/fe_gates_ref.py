"""The feature front end's gates (DESIGN.md 5.3 "Gates"; include/flame_hip.h, flame_hip_frontend_set_gates) restated in NumPy on
top of tests/frontend_ref.py.  A helper, not a test: tests/test_fe_gates_ref.py checks it rule by rule and against ground truth,
tests/test_gpu_fe_gates.py compares the library with it bit for bit.

`GatesRef` is FrontEndRef plus `set_gates`.  With no gate set every call goes to the base class untouched.  With one set:
  * `_track_one` lets the base class track, fuse and project the feature, recomputes the projection from the state the base class
    left -- the same float32 operations in the same order -- and applies the letterbox (a refused projection is a failed one: the
    frame's one dropout, death past max_dropouts) and then the height band (a held feature keeps everything and returns no
    candidate, its cell is remembered);
  * `track` is the base class's frame with the band in the detection rows and the held cells counted as occupied.
`GatesDebugRef` adds fe_debug_ref.DebugRef's search record and pictures for the GPU comparison."""
import numpy as np

from tests import fe_debug_ref as D
from tests import frontend_corpus as FC
from tests import frontend_ref as R

F = np.float32
FAILED = (R.OUTSIDE, R.BAD_MATCH, R.AMBIGUOUS)
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


class GatesRef(R.FrontEndRef):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.gates = None  # dict(letterbox, height, min_height, max_height, up) or None
        self._g = None     # the current frame's record
        self.held = self.refused = 0
        self.held_slots = []
        self._held_cells = set()
        self.proj_all = {}  # slot -> (px, py, xc, vc) of every acceptable projection of the frame, before the gates (gated frames only)

    def set_gates(self, letterbox=False, min_height=None, max_height=None, up=(0, -1, 0)):
        height = min_height is not None or max_height is not None
        if not letterbox and not height:
            self.gates = None
            return
        lo = F(-BIG if min_height is None else min_height)
        hi = F(BIG if max_height is None else max_height)
        if height:
            vals = [lo, hi] + [F(a) for a in up]
            if not all(np.isfinite(x) for x in vals):
                raise ValueError("non-finite gate")
            if lo > hi or not any(F(a) != 0 for a in up):
                raise ValueError("empty band or zero up vector")
        self.gates = dict(letterbox=bool(letterbox), height=height, min_height=lo, max_height=hi, up=tuple(up))

    def _projection(self, s, poses):
        """The projection FrontEndRef._track_one makes from the state it left in slot s: (pok, px, py, xc, vc)."""
        fx, fy, cx, cy = self.K4
        u, v, f = int(self.u[s]), int(self.v[s]), int(self.pf[s])
        mu, var = self.mu[s], self.var[s]
        A, c = poses[f]
        b0, b1 = (F(u) - cx) / fx, (F(v) - cy) / fy
        a0 = (A[0][0] * b0 + A[0][1] * b1) + A[0][2]
        a1 = (A[1][0] * b0 + A[1][1] * b1) + A[1][2]
        a2 = (A[2][0] * b0 + A[2][1] * b1) + A[2][2]
        c0, c1, c2 = c
        w0, w1, w2 = a0 + mu * c0, a1 + mu * c1, a2 + mu * c2
        if not w2 > 0:
            return False, None, None, None, None
        px, py, xc = w0 / w2, w1 / w2, mu / w2
        g = a2 / (w2 * w2)
        vc = var * (g * g)
        pok = bool(px >= 0 and px <= F(self.W - 1) and py >= 0 and py <= F(self.H - 1) and np.isfinite(xc) and np.isfinite(vc) and vc >= 0)
        return pok, px, py, xc, vc

    def _track_one(self, s, p, cur, poses):
        g = self._g
        if g is None:
            return super()._track_one(s, p, cur, poses)
        res = super()._track_one(s, p, cur, poses)
        pok, px, py, xc, vc = self._projection(s, poses)
        if res is not None:  # the base class's candidate is this projection
            want = np.array([px, py, xc, vc], np.float32).view(np.uint32)
            assert pok and np.array_equal(np.array(res[1], np.float32).view(np.uint32), want)
        if not pok:
            return None
        self.proj_all[s] = (px, py, xc, vc)
        # letterbox first: it is part of the projection test
        if not (py >= F(g["y_lo"]) and py <= F(g["y_hi"] - 1)):
            self.refused += 1
            if res is None:  # died of its failed search
                return None
            if int(self.status[s]) not in FAILED:  # (a failed search took the frame's one dropout already)
                self.drop[s] += 1
                if self.drop[s] > p["max_dropouts"]:
                    self.alive[s], self.status[s] = 0, R.DIED
                    self.counts[R.DIED] = self.counts.get(R.DIED, 0) + 1
            return None
        if res is None:
            return None
        if g["height"]:
            h = height32(self.K4, g["hr"], g["h0"], px, py, xc)
            if not (h >= g["min_height"] and h <= g["max_height"]):  # (a NaN height fails both)
                self.held += 1
                self.held_slots.append(s)
                self._held_cells.add(res[0])
                return None
        return res

    def track(self, p, img, img_id, T_world_cam, is_poseframe):
        self.held = self.refused = 0
        self.held_slots = []
        self._held_cells = set()
        self.proj_all = {}
        if self.gates is None:
            self._g = None
            return super().track(p, img, img_id, T_world_cam, is_poseframe)
        W, H, win, dws = self.W, self.H, p["win_size"], p["detection_win_size"]
        gs = self.gates
        if gs["letterbox"]:
            check_band(H, win)
        y_lo, y_hi = band(H) if gs["letterbox"] else (0, H)
        self._g = dict(y_lo=y_lo, y_hi=y_hi, height=gs["height"], min_height=gs["min_height"], max_height=gs["max_height"])
        if gs["height"]:
            self._g["hr"], self._g["h0"] = gate_record(T_world_cam, gs["up"])
        # ---- FrontEndRef.track with the band in the detection rows and the held cells occupied ----
        img = np.ascontiguousarray(img, np.uint8)
        assert img.shape == (H, W)
        cur = img.astype(np.int64)
        T = np.asarray(T_world_cam, np.float64).reshape(3, 4)
        self.counts = {}
        cur_pf = -1
        if is_poseframe:
            cur_pf = self.pf_added % self.P
            if self.pf_used[cur_pf]:
                self.pf_used[cur_pf] = False
                self._kill()
        poses = [R.pose_record(self.K4, T, self.pf_T[q]) if self.pf_used[q] else None for q in range(self.P)]
        ncx, ncy = (W + dws - 1) // dws, (H + dws - 1) // dws
        cell_key, cell_of, proj = {}, {}, {}
        with np.errstate(all="ignore"):
            for s in range(self.F):
                if not self.alive[s]:
                    self.status[s], self.kstar[s] = R.FREE, -1
                    continue
                res = self._track_one(s, p, cur, poses)
                if res is not None:
                    cell, pr = res
                    key = (int(np.float32(pr[3]).view(np.uint32)), s)
                    if cell not in cell_key or key < cell_key[cell]:
                        cell_key[cell] = key
                    cell_of[s], proj[s] = cell, pr
        n_new = dropped = 0
        if is_poseframe:
            g2 = R.g2_image(img)
            thr, m = R.g2_threshold(p["min_grad_mag"]), win // 2 + 1
            free = [s for s in range(self.F) if not self.alive[s]]
            for cell in range(ncx * ncy):
                if cell in cell_key or cell in self._held_cells:
                    continue
                ccx, ccy = cell % ncx, cell // ncx
                xlo, xhi = max(ccx * dws, m), min(ccx * dws + dws, W - m)
                ylo, yhi = max(ccy * dws, m, y_lo), min(ccy * dws + dws, H - m, y_hi)
                if xhi <= xlo or yhi <= ylo:
                    continue
                sub = g2[ylo:yhi, xlo:xhi]
                i = int(np.argmax(sub))
                if sub.flat[i] < thr:
                    continue
                if n_new >= len(free):
                    dropped += 1
                    continue
                s = free[n_new]
                n_new += 1
                y, x = ylo + i // (xhi - xlo), xlo + i % (xhi - xlo)
                self.alive[s], self.u[s], self.v[s], self.pf[s], self.drop[s] = 1, x, y, cur_pf, 0
                self.mu[s], self.var[s] = F(p["idepth_init"]), F(p["var_init"])
                self.status[s], self.kstar[s] = R.NEW, -1
                cell_of[s], proj[s] = cell, (F(x), F(y), F(p["idepth_init"]), F(p["var_init"]))
                cell_key[cell] = (int(F(p["var_init"]).view(np.uint32)), s)
            self.pf_used[cur_pf], self.pf_id[cur_pf], self.pf_T[cur_pf], self.pf_img[cur_pf] = True, int(img_id), T.copy(), cur
            self.pf_added += 1
        self.counts[R.NEW], self.dropped = n_new, dropped
        em = [s for s in sorted(cell_of) if self.alive[s] and cell_key[cell_of[s]][1] == s]
        return dict(vtx=np.array([[proj[s][0], proj[s][1]] for s in em], np.float32).reshape(-1, 2),
                    idepth_mu=np.array([proj[s][2] for s in em], np.float32), idepth_var=np.array([proj[s][3] for s in em], np.float32),
                    slot=np.array(em, np.int32), status=np.array([self.status[s] for s in em], np.int32))


def colliding_runs():
    """frontend_corpus._colliding's frames: after the step back several features share a cell.  Returns the case, an ungated
    run's record of frame 2 (a vacuous band, so that the restatement keeps every projection) and a pair (winner, loser) of one
    cell with their heights along up = (0, 1, 0)."""
    c = FC.case("colliding_then_poseframe")
    p = R.params(**c.kw)
    ref = GatesRef(FC.W, FC.H, c.K, FC.SLOTS, FC.RING)
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


class GatesDebugRef(D.DebugRef, GatesRef):
    """GatesRef with DebugRef's search record and pictures (DebugRef's calls reach GatesRef's through the MRO)."""
