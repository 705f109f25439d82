"""The feature front end's contract (DESIGN.md "Feature front end") stated in float64 FROM THE GEOMETRY, with rounding bands.

Independent of the float32 restatement (tests/frontend_ref.py) and of the package: 4x4 poses, T_cur_ref =
inv(T_world_cur) @ T_world_ref, back-projection K^-1 (u, v, 1), X(xi) = R b + xi t, projection K X -- never the kernel's
precomposed A = K R, c = K t.  Values are float64; image costs are Python / int64 integers.

What a float32 implementation of the contract may return is a SET: every real quantity carries a band
BAND[.] * EPS32 * M, M a magnitude propagated through the contract's float32 form (the sum of the absolute values of the
terms of every sum, divided through every quotient: first-order rounding analysis, so the cancelling forms
(a0 - x a2) / (x c2 - c0) and xi(p* + e) - xi(p* - e) get the wide bands they need), and every discrete decision whose
operand lies within its band of the threshold FORKS: both branches are admissible.  A sample whose 16 p + 0.5 lies within
the band of an integer gets both quanta and both integer costs; k* is certain when one sample wins under every combination.
A feature with more than one admissible branch is UNCERTAIN; the tests cap the share of those.

`track_feature` gives one feature's admissible outcomes, `project` the projection of a (mu, var) into the current frame,
`FrontEndF64.check_frame` holds a whole frame (pre-state -> post-state + emitted features) against them, with the
frame-level rules: one emitted feature per detection cell, detections by brute force, untouched state.
"""
import math

import numpy as np

EPS32 = 2.0 ** -24
OK, NO_PARALLAX, OUTSIDE, BAD_MATCH, AMBIGUOUS, NEW, DIED, FREE = 0, 1, 2, 3, 4, 5, 6, -1
FAILED = (OUTSIDE, BAD_MATCH, AMBIGUOUS)
MAX_SAMPLES = 256
INF = math.inf

# The band constants, stated once: 4 x the worst |float32 restatement - float64| / (EPS32 * M) measured on the CPU over the
# whole corpus of tests/frontend_corpus.py (tests/test_frontend_f64.py prints the ratios it sees; measured values beside
# each constant).  "pos" also sizes the bands of the decisions made on the same chain (depths, L, S, the dominant axis).
BAND = {
    "pos": 4 * 1.08,    # sample positions p_k                      measured worst ratio 1.079 (168 440 axis samples)
    "meas": 4 * 0.083,  # mu', var' after the fusion                measured worst ratio 0.083
    "proj": 4 * 1.23,   # projected pixel, xi_cur, var_cur          measured worst ratio 1.223
}


def pose44(T):
    M = np.eye(4)
    M[:3, :] = np.asarray(T, np.float64).reshape(3, 4)
    return M


def rel_pose(T_world_cur, T_world_ref):
    return np.linalg.inv(pose44(T_world_cur)) @ pose44(T_world_ref)


class _Geo:
    """One feature's geometry against the current frame: r = R K^-1 (u, v, 1), t, and the abs-sums of r's terms."""

    def __init__(self, K4, T_cur_ref, u, v):
        self.fx, self.fy, self.cx, self.cy = (float(a) for a in K4)
        R, self.t = T_cur_ref[:3, :3], T_cur_ref[:3, 3]
        b = np.array([(u - self.cx) / self.fx, (v - self.cy) / self.fy, 1.0])
        self.r = R @ b
        self.rabs = np.abs(R) @ np.abs(b)
        # magnitudes of the contract's a = K r, c = K t, per image axis (0: x, 1: y)
        self.f, self.c0 = (self.fx, self.fy), (self.cx, self.cy)
        self.Ma = [self.f[i] * self.rabs[i] + abs(self.c0[i]) * self.rabs[2] for i in (0, 1)]
        self.Mc = [self.f[i] * abs(self.t[i]) + abs(self.c0[i] * self.t[2]) for i in (0, 1)]

    def forward(self, xi, mxi=0.0):
        """Pixel of X(xi) with its magnitudes, the depth X2 and its magnitude.  mxi: magnitude of xi itself."""
        X = self.r + xi * self.t
        Xabs = self.rabs + np.abs(xi * self.t) + np.abs(self.t) * mxi
        d, Md = X[2], Xabs[2] + abs(X[2])
        if d == 0.0:
            return None, None, d, Md
        p, Mp = [], []
        for i in (0, 1):
            x = self.c0[i] + self.f[i] * X[i] / d
            p.append(x)
            Mp.append((self.f[i] * Xabs[i] + abs(self.c0[i]) * Xabs[2]) / abs(d) + abs(x) * Md / abs(d) + abs(x))
        return p, Mp, d, Md

    def inverse(self, axis, x, Mx):
        """xi of the pixel coordinate x on `axis`: (r_i - xn r2) / (xn t2 - t_i), xn the normalised coordinate; magnitudes in
        the contract's form (a_i - x a2) / (x c2 - c_i).  Returns (xi, M) or (None, None) when the quotient's denominator
        lies within its band of zero."""
        f, c = self.f[axis], self.c0[axis]
        xn = (x - c) / f
        num, den = self.r[axis] - xn * self.r[2], xn * self.t[2] - self.t[axis]
        Mn = self.Ma[axis] + abs(x) * self.rabs[2] + Mx * abs(self.r[2]) + abs(f * num)
        Md = abs(x * self.t[2]) + Mx * abs(self.t[2]) + self.Mc[axis] + abs(f * den)
        if abs(f * den) <= 4.0 * BAND["pos"] * EPS32 * Md:
            return None, None
        xi = num / den
        return xi, Mn / abs(f * den) + abs(xi) * Md / abs(f * den) + abs(xi)


def _near(x, M, key="pos"):
    return BAND[key] * EPS32 * M


def _sample_costs(cur, ref, W, H, u, v, win, px, py, bx, by):
    """The set of costs (INF: invalid) of the sample at (px, py) +- (bx, by): every admissible quantum pair."""
    r = win // 2
    out = set()
    zx, zy = 16.0 * px + 0.5, 16.0 * py + 0.5
    refw = ref[v - r:v + r + 1, u - r:u + r + 1]
    qxs = range(int(math.floor(zx - 16.0 * bx)), int(math.floor(zx + 16.0 * bx)) + 1)
    qys = range(int(math.floor(zy - 16.0 * by)), int(math.floor(zy + 16.0 * by)) + 1)
    if len(qxs) * len(qys) > 64:
        raise AssertionError("a sample's position band spans %d x %d quanta: outside what this statement bounds" % (len(qxs), len(qys)))
    for qx in qxs:
        for qy in qys:
            if qx < 0 or qx > 16 * W or qy < 0 or qy > 16 * H:
                out.add(INF)
                continue
            ix, iy = qx >> 4, qy >> 4
            if ix - r < 0 or iy - r < 0 or ix + r + 1 > W - 1 or iy + r + 1 > H - 1:
                out.add(INF)
                continue
            wx1, wy1 = qx & 15, qy & 15
            wx0, wy0 = 16 - wx1, 16 - wy1
            c = cur[iy - r:iy + r + 2, ix - r:ix + r + 2]
            D = (wx0 * wy0) * c[:-1, :-1] + (wx1 * wy0) * c[:-1, 1:] + (wx0 * wy1) * c[1:, :-1] + (wx1 * wy1) * c[1:, 1:] - 256 * refw
            out.add(int((D * D).sum()))
    return out


def _outcome(status, kstar, mu, var, Mmu=0.0, Mvar=0.0, unbounded=False):
    if unbounded:
        return dict(status=status, kstar=kstar, mu=(-INF, INF), var=(-INF, INF), mid=(mu, var), M=(INF, INF))
    bm, bv = _near(mu, Mmu, "meas"), _near(var, Mvar, "meas")
    return dict(status=status, kstar=kstar, mu=(mu - bm, mu + bm), var=(var - bv, var + bv), mid=(mu, var), M=(Mmu, Mvar))


def track_feature(p, K4, W, H, cur, T_world_cur, ref, T_world_ref, feat):
    """Admissible outcomes of one live feature: a list of dicts {status, kstar, mu: (lo, hi), var: (lo, hi), mid, M}.
    cur / ref: int64 images; feat: dict(u, v, mu, var) of the pre-state (mu, var the float32 values).  More than one
    entry = at least one decision forked."""
    u, v, mu, var = int(feat["u"]), int(feat["v"]), float(feat["mu"]), float(feat["var"])
    win = int(p["win_size"])
    rw = win // 2
    same = lambda st, k=-1: _outcome(st, k, mu, var)
    g = _Geo(K4, rel_pose(T_world_cur, T_world_ref), u, v)
    sd = math.sqrt(var)
    idmin, idmax = float(np.float32(p["idepth_min"])), float(np.float32(p["idepth_max"]))
    Mxi = abs(mu) + 2.0 * sd
    xi0, xi1 = max(mu - 2.0 * sd, idmin), min(mu + 2.0 * sd, idmax)
    p0, Mp0, d0, Md0 = g.forward(xi0, Mxi)
    p1, Mp1, d1, Md1 = g.forward(xi1, Mxi)
    ref_in = u - rw >= 0 and v - rw >= 0 and u + rw <= W - 1 and v + rw <= H - 1
    if not ref_in:
        return [same(OUTSIDE)]
    out = []
    behind = [d <= _near(d, Md) for d, Md in ((d0, Md0), (d1, Md1))]
    front = [d > -_near(d, Md) for d, Md in ((d0, Md0), (d1, Md1))]
    if any(behind):
        out.append(same(OUTSIDE))
    if not all(front) or p0 is None or p1 is None:
        return out
    dx, dy = p1[0] - p0[0], p1[1] - p0[1]
    Mdx, Mdy = Mp0[0] + Mp1[0] + abs(dx), Mp0[1] + Mp1[1] + abs(dy)
    L = math.hypot(dx, dy)
    ML = (abs(dx) * Mdx + abs(dy) * Mdy) / L + 2.0 * L if L > 0 else Mdx + Mdy
    bL = _near(L, ML)
    if L - bL < 2.0:
        out.append(same(NO_PARALLAX))
    if L + bL < 2.0:
        return out
    if L - bL >= MAX_SAMPLES:
        Ss = [MAX_SAMPLES]
    else:
        Ss = sorted({min(MAX_SAMPLES, int(math.ceil(max(L - bL, 2.0)))), min(MAX_SAMPLES, int(math.ceil(L + bL)))})
    bad = int(float(np.float32(p["max_match_error"])) * float(win * win) * 65536.0)
    elv = float(np.float32(p["epipolar_line_var"]))
    for S in Ss:
        e = (dx / S, dy / S)
        Me = (Mdx / S + abs(e[0]), Mdy / S + abs(e[1]))
        pos = lambda k, i: p0[i] + k * e[i]
        Mpos = lambda k, i: Mp0[i] + abs(k) * Me[i] + abs(k * e[i]) + abs(pos(k, i))
        CS = [_sample_costs(cur, ref, W, H, u, v, win, pos(k, 0), pos(k, 1), _near(0, Mpos(k, 0)), _near(0, Mpos(k, 1)))
              for k in range(S + 1)]
        if all(INF in c for c in CS):
            out.append(same(OUTSIDE))
        hi = sorted((max(c), k) for k, c in enumerate(CS))  # the keys the rivals can be pushed up to
        for k in range(S + 1):
            rival = hi[0] if hi[0][1] != k else (hi[1] if len(hi) > 1 else (INF, S + 1))
            for cb in sorted(c for c in CS[k] if c < INF and (c, k) < rival):
                if cb > bad:
                    out.append(same(BAD_MATCH, k))
                    continue
                far = [CS[j] for j in range(S + 1) if abs(j - k) > 2]
                if any(any((cb, k) < (c, j) and 2 * c < 3 * cb for c in CS[j]) for j in range(S + 1) if abs(j - k) > 2):
                    out.append(same(AMBIGUOUS, k))
                if any(all(2 * c < 3 * cb for c in cs) for cs in far):
                    continue
                cms = sorted(c for c in CS[k - 1] if c > cb) if k > 0 else [INF]
                cps = sorted(c for c in CS[k + 1] if c >= cb) if k + 1 <= S else [INF]
                for cm in cms:
                    for cp in cps:
                        out.extend(_measure(g, k, cm, cb, cp, pos, Mpos, e, Me, mu, var, elv))
    # drop duplicates (the same branch reached with costs that do not matter to it)
    uniq = []
    for o in out:
        if not any(o["status"] == q["status"] and o["kstar"] == q["kstar"] and o["mu"] == q["mu"] and o["var"] == q["var"] for q in uniq):
            uniq.append(o)
    return uniq


def _measure(g, k, cm, cb, cp, pos, Mpos, e, Me, mu, var, elv):
    """The OK path from the winner k and its neighbours' costs: refinement, measurement, fusion (with their forks)."""
    deltas = [(0.0, 0.0)]
    if cm < INF and cp < INF:
        fm, f0, fp = float(cm), float(cb), float(cp)
        den = (fm - 2.0 * f0) + fp
        Mden = 2.0 * (fm + 2.0 * f0 + fp)
        bden = _near(den, Mden)
        deltas = []
        if den <= bden:
            deltas.append((0.0, 0.0))
        if den > -bden and den != 0.0:
            d = 0.5 * (fm - fp) / den
            deltas.append((d, (0.5 * (fm + fp) + abs(0.5 * (fm - fp))) / abs(den) + abs(d) * Mden / abs(den) + abs(d)))
    res = []
    for delta, Mdelta in deltas:
        t, Mt = k + delta, Mdelta + abs(k + delta)
        ps = [pos(0, i) + t * e[i] for i in (0, 1)]
        Mps = [Mpos(0, i) + abs(t) * Me[i] + abs(e[i]) * Mt + abs(t * e[i]) + abs(ps[i]) for i in (0, 1)]
        gap, bgap = abs(e[0]) - abs(e[1]), _near(0, Me[0] + Me[1])
        axes = ([0] if gap >= -bgap else []) + ([1] if gap < bgap else [])
        for ax in axes:
            xm, Mxm = g.inverse(ax, ps[ax], Mps[ax])
            xp, Mxp = g.inverse(ax, ps[ax] + e[ax], Mps[ax] + Me[ax] + abs(ps[ax] + e[ax]))
            xn, Mxn = g.inverse(ax, ps[ax] - e[ax], Mps[ax] + Me[ax] + abs(ps[ax] - e[ax]))
            if xm is None or xp is None or xn is None:
                res.append(_outcome(OK, k, mu, var, unbounded=True))
                res.append(_outcome(BAD_MATCH, k, mu, var))
                continue
            s = 0.5 * (xp - xn)
            Ms = 0.5 * (Mxp + Mxn) + abs(s)
            vm = s * s * elv
            Mvm = (2.0 * abs(s) * Ms + s * s) * elv + vm
            den = var + vm
            Mden = Mvm + den
            num = mu * vm + xm * var
            Mnum = abs(mu) * Mvm + abs(mu * vm) + Mxm * var + abs(xm * var) + abs(num)
            muf, varf = num / den, var * vm / den
            Mmuf = Mnum / den + abs(muf) * Mden / den + abs(muf)
            Mvarf = (var * Mvm + var * vm) / den + varf * Mden / den + varf
            res.append(_outcome(OK, k, muf, varf, Mmuf, Mvarf))
    return res


def project(p, K4, W, H, T_world_cur, T_world_ref, u, v, mu, var, Mmu=0.0, Mvar=0.0):
    """Projection of a feature's (mu, var) into the current frame: dict(px, py, xi, vc: (lo, hi) intervals, mid, M,
    pok: the set of admissible verdicts of "w2 > 0 and the pixel inside [0, W-1] x [0, H-1]")."""
    g = _Geo(K4, rel_pose(T_world_cur, T_world_ref), int(u), int(v))
    mu, var = float(mu), float(var)
    pp, Mp, w2, Mw2 = g.forward(mu, Mmu)
    pok = set()
    bw = _near(w2, Mw2, "proj")
    if w2 <= bw:
        pok.add(False)
    if not w2 > -bw or pp is None:
        return dict(pok=pok)
    bx, by = _near(0, Mp[0], "proj"), _near(0, Mp[1], "proj")
    if pp[0] - bx < 0 or pp[0] + bx > W - 1 or pp[1] - by < 0 or pp[1] + by > H - 1:
        pok.add(False)
    if pp[0] + bx >= 0 and pp[0] - bx <= W - 1 and pp[1] + by >= 0 and pp[1] - by <= H - 1:
        pok.add(True)
    xc = mu / w2
    Mxc = Mmu / abs(w2) + abs(xc) * Mw2 / abs(w2) + abs(xc)
    gg = g.r[2] / (w2 * w2)
    Mg = g.rabs[2] / (w2 * w2) + abs(gg) * (2.0 * Mw2 / abs(w2) + 1.0) + abs(gg)
    vc = var * gg * gg
    Mvc = Mvar * gg * gg + var * 2.0 * abs(gg) * Mg + 3.0 * vc
    iv = lambda x, M: (x - _near(0, M, "proj"), x + _near(0, M, "proj"))
    return dict(pok=pok, px=iv(pp[0], Mp[0]), py=iv(pp[1], Mp[1]), xi=iv(xc, Mxc), vc=iv(vc, Mvc),
                mid=(pp[0], pp[1], xc, vc), M=(Mp[0], Mp[1], Mxc, Mvc))


def feature_outcomes(p, K4, W, H, cur, T_world_cur, ref, T_world_ref, feat):
    """track_feature's outcomes, each completed with its projection from the outcome's own (mu', var') interval: px, py, xi,
    vc intervals under "proj", pok, the admissible dropout counts `drop` (feat["drop"] is the pre-state's counter) and `dies`."""
    outs = track_feature(p, K4, W, H, cur, T_world_cur, ref, T_world_ref, feat)
    scale = BAND["meas"] / BAND["proj"]
    for o in outs:
        if o["M"][0] == INF:
            o.update(proj=None, pok={True, False}, drop={0, 1})
        else:
            o["proj"] = project(p, K4, W, H, T_world_cur, T_world_ref, feat["u"], feat["v"], o["mid"][0], o["mid"][1],
                                o["M"][0] * scale, o["M"][1] * scale)
            o["pok"] = o["proj"]["pok"]
            base = 0 if o["status"] == OK else int(feat["drop"])
            o["drop"] = set(base + (1 if (o["status"] in FAILED or not ok) else 0) for ok in o["pok"])
        o["dies"] = set(d > int(p["max_dropouts"]) for d in o["drop"])
    return outs


def detections(img, win, dws, min_grad_mag, occupied):
    """Per cell not in `occupied` the pixel of the largest g2 = (I(x+1,y)-I(x-1,y))^2 + (I(x,y+1)-I(x,y-1))^2 at or above
    max(1, ceil(4 min_grad_mag^2)), margin m = win/2 + 1, ties to the smallest y, then the smallest x: plain loops over
    Python integers.  Returns [(cell, x, y)] in cell-major (row-major) order."""
    Hh, Ww = img.shape
    I = [[int(a) for a in row] for row in img]
    m = win // 2 + 1
    mg = float(np.float32(min_grad_mag))
    thr = max(1, int(math.ceil(4.0 * mg * mg)))
    ncx = (Ww + dws - 1) // dws
    best = {}
    for y in range(m, Hh - m):
        for x in range(m, Ww - m):
            g2 = (I[y][x + 1] - I[y][x - 1]) ** 2 + (I[y + 1][x] - I[y - 1][x]) ** 2
            cell = (y // dws) * ncx + x // dws
            if g2 >= thr and cell not in occupied and (cell not in best or g2 > best[cell][0]):
                best[cell] = (g2, x, y)
    return [(cell, best[cell][1], best[cell][2]) for cell in sorted(best)]


def _in(x, iv):
    return iv[0] <= float(x) <= iv[1]


def _bits(x):
    return np.float32(x).view(np.uint32)


class FrontEndF64:
    """The ring of pose frames (images, world poses, ids) and the frame-level check.  Feed it the same calls as the
    implementation under test: check_frame for every track(), set_poses, prune."""

    def __init__(self, W, H, K, max_features, max_poseframes):
        K = np.asarray(K, np.float32).reshape(9)
        self.W, self.H, self.F, self.P = int(W), int(H), int(max_features), int(max_poseframes)
        self.K4 = (float(K[0]), float(K[4]), float(K[2]), float(K[5]))
        self.used, self.ids = [False] * self.P, [0] * self.P
        self.T, self.img = [None] * self.P, [None] * self.P
        self.added = 0

    def set_poses(self, ids, poses):
        for i, T in zip(ids, poses):
            for q in range(self.P):
                if self.used[q] and self.ids[q] == int(i):
                    self.T[q] = np.asarray(T, np.float64).reshape(3, 4).copy()

    def prune(self, keep_ids):
        keep = set(int(i) for i in keep_ids)
        for q in range(self.P):
            if self.used[q] and self.ids[q] not in keep:
                self.used[q] = False

    def check_frame(self, p, img, img_id, T_world_cam, is_poseframe, pre, post, emitted, info=None):
        """pre / post: dicts of per-slot arrays (alive, u, v, pf, mu, var, drop, status, kstar) before / after the frame;
        emitted: dict(vtx, idepth_mu, idepth_var, slot, status); info: optional counters {status: count, "dropped": n,
        "emitted": n}.  Raises AssertionError on anything inadmissible, returns a report (tracked, uncertain, per-status
        certain / possible counts, the worst observed band ratios)."""
        W, H, K4 = self.W, self.H, self.K4
        win, dws, maxdrop = int(p["win_size"]), int(p["detection_win_size"]), int(p["max_dropouts"])
        cur = np.ascontiguousarray(img).astype(np.int64)
        assert cur.shape == (H, W)
        T = np.asarray(T_world_cam, np.float64).reshape(3, 4)
        ncx = (W + dws - 1) // dws
        alive0 = np.asarray(pre["alive"]).astype(bool).copy()
        cur_pf = -1
        if is_poseframe:
            cur_pf = self.added % self.P
            if self.used[cur_pf]:  # the pose frame this one overwrites takes its features with it
                self.used[cur_pf] = False
        for s in np.flatnonzero(alive0):
            if not self.used[int(pre["pf"][s])]:
                alive0[s] = False
        rep = dict(tracked=0, uncertain=0, certain={}, possible={}, ratio=dict(meas=0.0, proj=0.0), statuses={})
        em = {int(s): i for i, s in enumerate(emitted["slot"])}
        assert len(em) == len(emitted["slot"]) and (np.diff(np.asarray(emitted["slot"], np.int64)) > 0).all(), "emitted slots not ascending"
        after = np.zeros(self.F, bool)  # alive after the tracking, before the detections take slots
        proj, cands = {}, {}
        for s in range(self.F):
            st_post, ks_post = int(post["status"][s]), int(post["kstar"][s])
            if not alive0[s]:
                if st_post != NEW:
                    assert st_post == FREE and ks_post == -1 and not post["alive"][s], "slot %d: a free slot shows status %d" % (s, st_post)
                continue
            f = int(pre["pf"][s])
            feat = dict(u=pre["u"][s], v=pre["v"][s], mu=pre["mu"][s], var=pre["var"][s])
            outs = track_feature(p, K4, W, H, cur, T, self.img[f], self.T[f], feat)
            assert outs, "slot %d: the statement admits no outcome" % s
            rep["tracked"] += 1
            rep["uncertain"] += len(outs) > 1
            sts = set(o["status"] for o in outs)
            for x in sts:
                rep["possible"][x] = rep["possible"].get(x, 0) + 1
            if len(sts) == 1:
                rep["certain"][min(sts)] = rep["certain"].get(min(sts), 0) + 1
            reused = st_post == NEW
            if reused:  # the feature died and a detection of this frame took its slot: only the death can be checked
                mu_s, var_s = float(pre["mu"][s]), float(pre["var"][s])
            else:
                mu_s, var_s = float(post["mu"][s]), float(post["var"][s])
                assert (int(post["u"][s]), int(post["v"][s]), int(post["pf"][s])) == (int(pre["u"][s]), int(pre["v"][s]), f), "slot %d moved" % s
            why, good = [], False
            for o in outs:
                if not reused:
                    if st_post != DIED and st_post != o["status"]:
                        why.append("status %d" % o["status"])
                        continue
                    if ks_post != o["kstar"]:
                        why.append("k* %d" % o["kstar"])
                        continue
                    if o["status"] != OK:  # untouched state: bit for bit
                        if _bits(post["mu"][s]) != _bits(pre["mu"][s]) or _bits(post["var"][s]) != _bits(pre["var"][s]):
                            why.append("status %d must leave mu / var untouched" % o["status"])
                            continue
                    elif not (_in(mu_s, o["mu"]) and _in(var_s, o["var"])):
                        why.append("mu %r not in %r or var %r not in %r" % (mu_s, o["mu"], var_s, o["var"]))
                        continue
                    elif len(outs) == 1:  # (the ratios are taken on certain features only)
                        rep["ratio"]["meas"] = max(rep["ratio"]["meas"], abs(mu_s - o["mid"][0]) / (EPS32 * o["M"][0]),
                                                   abs(var_s - o["mid"][1]) / (EPS32 * o["M"][1]))
                    pr = project(p, K4, W, H, T, self.T[f], pre["u"][s], pre["v"][s], mu_s, var_s)
                else:
                    if o["status"] == OK:  # mu' unknown: project the interval's centre with its magnitude
                        if o["M"][0] == INF:
                            good = True
                            break
                        pr = project(p, K4, W, H, T, self.T[f], pre["u"][s], pre["v"][s], o["mid"][0], o["mid"][1],
                                     o["M"][0] * BAND["meas"] / BAND["proj"], o["M"][1] * BAND["meas"] / BAND["proj"])
                    else:
                        pr = project(p, K4, W, H, T, self.T[f], pre["u"][s], pre["v"][s], mu_s, var_s)
                base = 0 if o["status"] == OK else int(pre["drop"][s])
                drops = set(base + (1 if (o["status"] in FAILED or not ok) else 0) for ok in pr["pok"])
                if reused:
                    if any(d > maxdrop for d in drops):
                        good = True
                        break
                    why.append("status %d does not kill the feature" % o["status"])
                    continue
                d_post = int(post["drop"][s])
                if d_post not in drops:
                    why.append("dropouts %d not in %s" % (d_post, sorted(drops)))
                    continue
                dead = d_post > maxdrop
                if bool(post["alive"][s]) == dead or (st_post == DIED) != dead:
                    why.append("alive %d / status %d with %d dropouts of %d" % (post["alive"][s], st_post, d_post, maxdrop))
                    continue
                good = True
                rep["statuses"][s] = o["status"]
                if not dead:
                    after[s] = True
                    pr = dict(pr)
                    pr["pok"] = set(ok for ok in pr["pok"] if base + (1 if (o["status"] in FAILED or not ok) else 0) == d_post)
                    proj[s] = pr
                break
            assert good, "slot %d (u %d v %d pf %d mu %r var %r drop %d): post status %d k* %d mu %r var %r drop %d is not admissible: %s" % (
                s, pre["u"][s], pre["v"][s], f, float(pre["mu"][s]), float(pre["var"][s]), pre["drop"][s], st_post, ks_post,
                float(post["mu"][s]), float(post["var"][s]), post["drop"][s], "; ".join(why))
        # ---- emission: one feature per detection cell, the smallest var_cur, ties to the lower slot ----
        cell_em = {}
        for s, i in em.items():
            st = int(emitted["status"][i])
            assert st == int(post["status"][s]) and post["alive"][s], "emitted slot %d: status %d, state %d" % (s, st, post["status"][s])
            if st == NEW:
                continue
            assert s in proj and True in proj[s]["pok"], "slot %d is emitted but its projection fails" % s
            pr = proj[s]
            x, y = float(emitted["vtx"][i][0]), float(emitted["vtx"][i][1])
            xc, vc = float(emitted["idepth_mu"][i]), float(emitted["idepth_var"][i])
            assert _in(x, pr["px"]) and _in(y, pr["py"]), "slot %d: emitted pixel (%r, %r) not in %r x %r" % (s, x, y, pr["px"], pr["py"])
            assert _in(xc, pr["xi"]), "slot %d: emitted xi_cur %r not in %r" % (s, xc, pr["xi"])
            assert _in(vc, pr["vc"]), "slot %d: emitted var_cur %r not in %r" % (s, vc, pr["vc"])
            assert 0 <= x <= W - 1 and 0 <= y <= H - 1
            for got, mid, M in zip((x, y, xc, vc), pr["mid"], pr["M"]):
                if pr["pok"] == {True}:
                    rep["ratio"]["proj"] = max(rep["ratio"]["proj"], abs(got - mid) / (EPS32 * M))
            cell = (int(y) // dws) * ncx + int(x) // dws
            assert cell not in cell_em, "cell %d holds two emitted features: slots %d and %d" % (cell, cell_em[cell], s)
            cell_em[cell] = s
        for s, pr in proj.items():
            if s in em or pr["pok"] != {True}:
                continue
            cells = set((int(math.floor(y)) // dws) * ncx + int(math.floor(x)) // dws
                        for x in (max(pr["px"][0], 0.0), min(pr["px"][1], W - 1.0)) for y in (max(pr["py"][0], 0.0), min(pr["py"][1], H - 1.0)))
            if len(cells) != 1:
                continue
            cell = min(cells)
            assert cell in cell_em, "slot %d projects into cell %d, which emits nothing" % (s, cell)
            w = cell_em[cell]
            vw = float(emitted["idepth_var"][em[w]])
            assert vw <= pr["vc"][1], "cell %d emits slot %d (var_cur %r) although slot %d has var_cur <= %r" % (cell, w, vw, s, pr["vc"][1])
            if pr["vc"][0] == pr["vc"][1] == vw:
                assert w < s, "cell %d: an exact tie goes to the lower slot %d, not %d" % (cell, s, w)
        # ---- detection: brute force over exactly the cells without an emitted feature ----
        new_slots = [s for s in range(self.F) if int(post["status"][s]) == NEW]
        dropped = 0
        if is_poseframe:
            det = detections(np.asarray(img), win, dws, p["min_grad_mag"], set(cell_em))
            free = [s for s in range(self.F) if not after[s]]
            dropped = max(0, len(det) - len(free))
            det = det[:len(free)]
            assert new_slots == free[:len(det)], "NEW slots %s..., the free slots in ascending order are %s..." % (new_slots[:8], free[:8])
            mu0, var0 = np.float32(p["idepth_init"]), np.float32(p["var_init"])
            for s, (cell, x, y) in zip(new_slots, det):
                assert s in em, "the new feature of slot %d is not emitted" % s
                i = em[s]
                assert (int(post["u"][s]), int(post["v"][s]), int(post["pf"][s]), int(post["drop"][s]), int(post["kstar"][s])) == \
                    (x, y, cur_pf, 0, -1) and post["alive"][s], "slot %d: detection of cell %d should be (%d, %d)" % (s, cell, x, y)
                assert _bits(post["mu"][s]) == _bits(mu0) and _bits(post["var"][s]) == _bits(var0)
                assert tuple(emitted["vtx"][i]) == (float(x), float(y)) and _bits(emitted["idepth_mu"][i]) == _bits(mu0) and \
                    _bits(emitted["idepth_var"][i]) == _bits(var0)
            self.used[cur_pf], self.ids[cur_pf], self.T[cur_pf], self.img[cur_pf] = True, int(img_id), T.copy(), cur
            self.added += 1
        else:
            assert not new_slots, "NEW features on an ordinary frame: %s" % new_slots[:8]
        assert sorted(em) == sorted(list(cell_em.values()) + new_slots), "emitted features outside the cells' winners and the detections"
        rep["new"], rep["dropped"] = len(new_slots), dropped
        if info is not None:
            for st in (OK, NO_PARALLAX, OUTSIDE, BAD_MATCH, AMBIGUOUS):
                n = int(info.get(st, 0))
                assert rep["certain"].get(st, 0) <= n <= rep["possible"].get(st, 0), "counter of status %d: %d outside [%d, %d]" % (
                    st, n, rep["certain"].get(st, 0), rep["possible"].get(st, 0))
            assert int(info.get(NEW, 0)) == len(new_slots) and int(info.get("dropped", 0)) == dropped
            assert int(info.get("emitted", len(em))) == len(em)
            n_died = sum(1 for s in range(self.F) if alive0[s] and not after[s])
            assert int(info.get(DIED, 0)) == n_died, "counter of DIED: %d, the states show %d" % (info.get(DIED, 0), n_died)
        return rep
