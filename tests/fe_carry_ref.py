"""The hand-over of the feature front end (DESIGN.md 5.3 "Hand-over", flame_hip_frontend_set_carry) restated in NumPy: the rule of
k_fe_carry as a pure function, and FrontEndRef with the evicting frame's other order around its unchanged `track`.  The GPU must
equal this bit for bit (tests/test_gpu_fe_carry.py); tests/test_fe_carry_ref.py pins it on hand-built states and against ground
truth.  Also the hovering sequence the tests and tools/carry_robustness.py share."""
import numpy as np

from tests import frontend_ref as R

F = np.float32


def band(H, win, y_lo=0, y_hi=None):
    """The rows and columns k_fe_detect can put a detection in: (m, max(m, y_lo), min(H - m, y_hi))."""
    m = win // 2 + 1
    return m, max(m, y_lo), min(H - m, H if y_hi is None else y_hi)


def carry_rule(a, alive, pf, status, cell_of, cell_winner, proj, W, H, win, y_lo=0, y_hi=None):
    """Step 3 on the state k_fe_compact leaves.  `a`: the evicted ring slot; alive, pf, status, cell_of: per slot; cell_winner: cell
    -> the slot in the low word of its key; proj: slot -> (px, py, xc, vc) float32.  Returns (carried, lost): carried maps a slot to
    its new (u, v, mu, var), lost lists the slots that die."""
    m, v_lo, v_hi = band(H, win, y_lo, y_hi)
    carried, lost = {}, []
    for s in range(len(alive)):
        if not alive[s] or pf[s] != a or status[s] == R.NEW:
            continue
        c = int(cell_of[s])
        if status[s] in (R.OK, R.NO_PARALLAX) and c >= 0 and cell_winner.get(c) == s:
            px, py, xc, vc = (F(x) for x in proj[s])
            ur, vr = int(np.floor(px + F(0.5))), int(np.floor(py + F(0.5)))
            if m <= ur < W - m and v_lo <= vr < v_hi:
                carried[s] = (ur, vr, xc, vc)
                continue
        lost.append(s)
    return carried, lost


class CarryRef(R.FrontEndRef):
    """FrontEndRef with `set_carry`.  The base is built with one ring slot more, the spare; `pf_added` is steered before every pose
    frame so that the unchanged `track` puts an evicting frame of the switched-on handle into the spare slot (nothing is killed, the
    old pose frame's record serves the frame) and every other pose frame into `count mod P`; behind `track` the rule runs, the spare
    slot's record moves into the ring slot and its detections are relabelled."""

    def __init__(self, W, H, K, max_features=2048, max_poseframes=8):
        super().__init__(W, H, K, max_features, max_poseframes + 1)
        self.ring = max_poseframes
        self.count = 0  # pose frames so far
        self.carry = False
        self.carried = self.carry_lost = 0  # of the last frame
        self.carried_slots, self.lost_slots = [], []
        self.evicted = None  # the ring slot the last frame evicted with the switch on, else None

    def set_carry(self, on=True):
        self.carry = bool(on)

    def track(self, p, img, img_id, T_world_cam, is_poseframe):
        self.carried = self.carry_lost = 0
        self.carried_slots, self.lost_slots, self.evicted = [], [], None
        if not is_poseframe:
            return super().track(p, img, img_id, T_world_cam, is_poseframe)
        a, spare = self.count % self.ring, self.ring
        handover = self.carry and self.pf_used[a]
        self.pf_added = spare if handover else a  # (both below P + 1: the base's `mod` leaves them)
        out = super().track(p, img, img_id, T_world_cam, is_poseframe)
        if handover:
            g = self._g or dict(y_lo=0, y_hi=self.H)
            winner = {}  # the emitted features are the winners of their cells
            dws = p["detection_win_size"]
            ncx = (self.W + dws - 1) // dws
            cell_of = np.full(self.F, -1, np.int64)
            proj = {}
            for i, s in enumerate(out["slot"]):
                px, py = out["vtx"][i]
                cell_of[s] = (int(py) // dws) * ncx + int(px) // dws
                winner[int(cell_of[s])] = int(s)
                proj[int(s)] = (px, py, out["idepth_mu"][i], out["idepth_var"][i])
            carried, lost = carry_rule(a, self.alive, self.pf, self.status, cell_of, winner, proj, self.W, self.H, p["win_size"],
                                       g["y_lo"], g["y_hi"])
            for s, (ur, vr, xc, vc) in carried.items():
                self.u[s], self.v[s], self.mu[s], self.var[s] = ur, vr, xc, vc
            for s in lost:
                self.alive[s] = 0
            self.carried, self.carry_lost = len(carried), len(lost)
            self.carried_slots, self.lost_slots, self.evicted = sorted(carried), list(lost), a
            # the spare slot's record becomes ring slot a's; its detections refer to a
            self.pf_id[a], self.pf_T[a], self.pf_img[a] = self.pf_id[spare], self.pf_T[spare], self.pf_img[spare]
            self.pf_used[spare], self.pf_id[spare], self.pf_T[spare], self.pf_img[spare] = False, 0, None, None
            self.pf[(self.pf == spare) & (self.alive != 0)] = a
        self.count += 1
        self.pf_added = self.count
        return out


# ---------------------------------------------------------------- the hovering sequence ----

SWING = (0, 1, 2, 3, 4, 3, 2, 1)


def hover_pose(k, step=0.06, yaw=0.004):
    """The camera swings sideways and back with period 8: x = step * (0, 1, 2, 3, 4, 3, 2, 1, ...), yaw = 0.004 * the same."""
    n = SWING[k % 8]
    return R.pose((step * n, 0.0, 0.0), yaw * n)


def hover_scene(seed, frames):
    """frontend_ref's slanted plane (160 x 120, its texture) seen from the hovering camera: [(img, T_world_cam)]."""
    rng = np.random.default_rng(seed)
    low = rng.integers(0, 256, (64, 64)).astype(np.float64)
    yy, xx = np.mgrid[0:R.SCENE_H, 0:R.SCENE_W].astype(np.float64)
    cache, out = {}, []
    for k in range(frames):
        n = SWING[k % 8]
        if n not in cache:
            T = hover_pose(k)
            _, X = R.plane_idepth(T, xx, yy)
            tu, tv = 3.0 * X[..., 0] + 32.0, 3.0 * X[..., 1] + 32.0
            u0, v0 = np.floor(tu).astype(int), np.floor(tv).astype(int)
            fu, fv = tu - u0, tv - v0
            val = (1 - fv) * (1 - fu) * low[v0, u0] + (1 - fv) * fu * low[v0, u0 + 1] + fv * (1 - fu) * low[v0 + 1, u0] + \
                fv * fu * low[v0 + 1, u0 + 1]
            cache[n] = (np.floor(val + 0.5).astype(np.uint8), T)
        out.append(cache[n])
    return out


GRAPH_VAR = 0.01  # idepth_var_max_graph: an emitted feature below it is a vertex of the graph


def graph_vertices(out, T):
    """(number of emitted features with idepth_var < 0.01, their relative inverse-depth errors against the plane)."""
    sel = out["idepth_var"] < F(GRAPH_VAR)
    vtx = out["vtx"][sel].astype(np.float64)
    if not len(vtx):
        return 0, np.zeros(0)
    truth, _ = R.plane_idepth(T, vtx[:, 0], vtx[:, 1])
    return int(sel.sum()), np.abs(out["idepth_mu"][sel].astype(np.float64) - truth) / truth


def hover_run(fe, p, frames, every):
    """Feeds the hovering frames, a pose frame every `every`-th; per frame (vertices, errors, carried, lost)."""
    rows = []
    info = fe.info if hasattr(fe, "info") else None
    for k, (img, T) in enumerate(frames):
        out = fe.track(p, img, k, T, k % every == 0)
        n, err = graph_vertices(out, T)
        rows.append((n, err, info("carried") if info else fe.carried, info("carry_lost") if info else fe.carry_lost))
    return rows


def hover_small(frames, step=0.06):
    """The hovering camera at 48 x 36 (fe_warp_scenes' small camera and renderer, fe_zm_scenes' plane and texture): every cell
    touches a border or the letterbox band, so the hand-over's pixel test decides."""
    from tests import fe_warp_scenes as WS
    tex = WS.ZS.texture(WS.SEED)
    cache, out = {}, []
    for k in range(frames):
        n = SWING[k % 8]
        if n not in cache:
            T = hover_pose(k, step)
            cache[n] = (WS.render_at(T, tex, WS.SMALL_W, WS.SMALL_H, WS.SMALL_K4).astype(np.uint8), T)
        out.append(cache[n])
    return out
