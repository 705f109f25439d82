"""The feature front end's gain-invariant matching cost (DESIGN.md 5.3 "Matching cost"; include/flame_hip.h,
flame_hip_frontend_set_gain_invariant) restated on top of tests/fe_zm_ref.py.  A helper, not a test: tests/test_fe_gi_ref.py checks it
on hand-written windows, for exact invariance under a power-of-two gain with offsets and against ground truth,
tests/test_gpu_fe_gi.py compares the library with it bit for bit.

`GiRef` is ZmRef plus `set_gain_invariant`.  With the switch off every call goes to ZmRef untouched (SSD or ZSSD, whatever `set_cost`
set: the switch does not touch `cost_mode`).  With it on
  * `_cost` is the base class's window with the rule of `gi_cost`: the sums in Python integers (no width to overflow; the kernel
    holds SI in 32 bits and the others in 64) and three np.float64 operations, each rounded once;
  * `_track_one` is ZmRef's search -- the same float32 operations in the same order -- with that cost in every decision, BAD_MATCH
    at C > n bad (ZSSD's threshold) and, before the threshold, BAD_MATCH for a reference window with ZR == 0.
`GiDebugRef` / `GiGatesDebugRef` / `RgGiDebugRef` / `RgGiGatesDebugRef` add fe_debug_ref.DebugRef's search record and pictures,
fe_gates_ref.GatesRef's gates and fe_rg_ref.RgRef's gradient gate for the GPU comparison."""
import numpy as np

from tests import fe_debug_ref as D
from tests import fe_gates_ref as G
from tests import fe_rg_ref as RG
from tests import fe_zm_ref as Z
from tests import frontend_ref as R

F = np.float32
F64 = np.float64


def window_sums(Iw, Rw):
    """(n, ZI, ZR, ZIR) of a window: Iw = the bilinear sums of the current image (0 ... 65 280), Rw = 256 x the reference pixels."""
    a = [int(x) for x in np.asarray(Iw).reshape(-1)]
    b = [int(x) for x in np.asarray(Rw).reshape(-1)]
    assert len(a) == len(b)
    n = len(a)
    SI, SII = sum(a), sum(x * x for x in a)
    SR, SRR = sum(b), sum(x * x for x in b)
    SIR = sum(x * y for x, y in zip(a, b))
    return n, n * SII - SI * SI, n * SRR - SR * SR, n * SIR - SI * SR


def gi_from_sums(ZI, ZR, ZIR):
    """C of the three integers: ZR when ZI == 0 or ZIR <= 0, else floor(ZR - ZIR^2 / ZI) clamped at 0, in float64."""
    assert 0 <= ZI < 2 ** 45 and 0 <= ZR < 2 ** 45 and abs(ZIR) < 2 ** 45
    if ZI == 0 or ZIR <= 0:
        return ZR
    z = F64(ZIR)  # (< 2^53: exact)
    q = (z * z) / F64(ZI)
    Cd = F64(ZR) - q
    return int(np.floor(Cd)) if Cd > 0 else 0


def gi_cost(Iw, Rw):
    """The rule on a window; returns (C, ZR)."""
    _, ZI, ZR, ZIR = window_sums(Iw, Rw)
    return gi_from_sums(ZI, ZR, ZIR), ZR


class GiRef(Z.ZmRef):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.gain_invariant = False

    def set_gain_invariant(self, on=True):
        self.gain_invariant = bool(on)

    def _windows(self, cur, ref, u, v, px, py, win):
        """(I, R) of the sample at (px, py), or None when the window leaves the image: ZmRef._cost's window, not differenced."""
        r = win // 2
        fqx, fqy = np.floor(px * F(16.0) + F(0.5)), np.floor(py * F(16.0) + F(0.5))
        if not (fqx >= 0 and fqx <= F(16 * self.W) and fqy >= 0 and fqy <= F(16 * self.H)):
            return None
        qx, qy = int(fqx), int(fqy)
        ix, iy = qx >> 4, qy >> 4
        if ix - r < 0 or iy - r < 0 or ix + r + 1 > self.W - 1 or iy + r + 1 > self.H - 1:
            return None
        wx1, wy1 = qx & 15, qy & 15
        wx0, wy0 = 16 - wx1, 16 - wy1
        c = cur[iy - r:iy + r + 2, ix - r:ix + r + 2].astype(np.int64)
        Iw = (wx0 * wy0) * c[:-1, :-1] + (wx1 * wy0) * c[:-1, 1:] + (wx0 * wy1) * c[1:, :-1] + (wx1 * wy1) * c[1:, 1:]
        return Iw, 256 * ref[v - r:v + r + 1, u - r:u + r + 1].astype(np.int64)

    def _cost(self, cur, ref, u, v, px, py, win):
        if not self.gain_invariant:
            return super()._cost(cur, ref, u, v, px, py, win)
        w = self._windows(cur, ref, u, v, px, py, win)
        return None if w is None else gi_cost(*w)[0]

    def _track_one(self, s, p, cur, poses):
        if not self.gain_invariant:
            return super()._track_one(s, p, cur, poses)
        OK, NO_PARALLAX, OUTSIDE, BAD_MATCH, AMBIGUOUS, DIED = R.OK, R.NO_PARALLAX, R.OUTSIDE, R.BAD_MATCH, R.AMBIGUOUS, R.DIED
        W, H, win = self.W, self.H, p["win_size"]
        fx, fy, cx, cy = self.K4
        u, v, f = int(self.u[s]), int(self.v[s]), int(self.pf[s])
        mu, var, drop = self.mu[s], self.var[s], int(self.drop[s])
        A, c = poses[f]
        ref = self.pf_img[f]
        b0, b1 = (F(u) - cx) / fx, (F(v) - cy) / fy
        a0 = (A[0][0] * b0 + A[0][1] * b1) + A[0][2]
        a1 = (A[1][0] * b0 + A[1][1] * b1) + A[1][2]
        a2 = (A[2][0] * b0 + A[2][1] * b1) + A[2][2]
        c0, c1, c2 = c
        two = F(2.0) * np.sqrt(var)
        lo, hi = mu - two, mu + two
        idmin, idmax = F(p["idepth_min"]), F(p["idepth_max"])
        xi0 = lo if lo > idmin else idmin
        xi1 = hi if hi < idmax else idmax
        d0, d1 = a2 + xi0 * c2, a2 + xi1 * c2
        r = win // 2
        ref_in = u - r >= 0 and v - r >= 0 and u + r <= W - 1 and v + r <= H - 1
        ks = -1
        mu_new, var_new = mu, var
        if not (d0 > 0 and d1 > 0) or not ref_in:
            status = OUTSIDE
        else:
            x0, y0 = (a0 + xi0 * c0) / d0, (a1 + xi0 * c1) / d0
            x1, y1 = (a0 + xi1 * c0) / d1, (a1 + xi1 * c1) / d1
            dx, dy = x1 - x0, y1 - y0
            L = np.sqrt(dx * dx + dy * dy)
            if not (L >= F(2.0)):
                status = NO_PARALLAX
            else:
                S = R.MAX_SAMPLES if L >= F(R.MAX_SAMPLES) else int(np.ceil(L))
                ex, ey = dx / F(S), dy / F(S)
                self.steps[s] = S
                Rw = 256 * ref[v - r:v + r + 1, u - r:u + r + 1].astype(np.int64)
                ZR = window_sums(Rw, Rw)[2]  # of the feature, not of the sample
                C = [self._cost(cur, ref, u, v, x0 + F(k) * ex, y0 + F(k) * ey, win) for k in range(S + 1)]
                valid = [k for k in range(S + 1) if C[k] is not None]
                if not valid:
                    status = OUTSIDE
                else:
                    ks = min(valid, key=lambda k: (C[k], k))  # the key (C << 9) | k: smallest cost, then smallest k
                    Cb = C[ks]
                    assert all(0 <= C[k] <= ZR < 2 ** 45 for k in valid)
                    if ZR == 0:
                        status = BAD_MATCH  # a flat reference window: nothing to correlate
                    elif Cb > Z.bad_threshold(p["max_match_error"], win, Z.COST_ZSSD):
                        status = BAD_MATCH
                    elif any(abs(k - ks) > 2 and 2 * C[k] < 3 * Cb for k in valid):
                        status = AMBIGUOUS
                    else:
                        Cm = C[ks - 1] if ks > 0 else None
                        Cp = C[ks + 1] if ks + 1 <= S else None
                        delta = F(0.0)
                        if Cm is not None and Cp is not None:
                            fm, f0, fp = F(Cm), F(Cb), F(Cp)  # (< 2^53: exact in the double NumPy goes through, rounded once)
                            den = (fm - F(2.0) * f0) + fp
                            if den > 0:
                                delta = (F(0.5) * (fm - fp)) / den
                        t = F(ks) + delta
                        xs, ys = x0 + t * ex, y0 + t * ey
                        if abs(ex) >= abs(ey):
                            xp, xn = xs + ex, xs - ex
                            xi_m = (a0 - xs * a2) / (xs * c2 - c0)
                            xi_p = (a0 - xp * a2) / (xp * c2 - c0)
                            xi_n = (a0 - xn * a2) / (xn * c2 - c0)
                        else:
                            yp, yn = ys + ey, ys - ey
                            xi_m = (a1 - ys * a2) / (ys * c2 - c1)
                            xi_p = (a1 - yp * a2) / (yp * c2 - c1)
                            xi_n = (a1 - yn * a2) / (yn * c2 - c1)
                        sl = (xi_p - xi_n) * F(0.5)
                        var_m = (sl * sl) * F(p["epipolar_line_var"])
                        den = var + var_m
                        mu_f = (mu * var_m + xi_m * var) / den
                        var_f = (var * var_m) / den
                        if np.isfinite(xi_m) and np.isfinite(var_m) and np.isfinite(mu_f) and np.isfinite(var_f):
                            status, mu_new, var_new = OK, mu_f, var_f
                            self.pstar[s] = (xs, ys)
                        else:
                            status = BAD_MATCH
        failed = status in (OUTSIDE, BAD_MATCH, AMBIGUOUS)
        if status == OK:
            mu, var, drop = mu_new, var_new, 0
        w0, w1, w2 = a0 + mu * c0, a1 + mu * c1, a2 + mu * c2
        pok, proj = False, None
        if w2 > 0:
            px, py, xc = w0 / w2, w1 / w2, mu / w2
            g = a2 / (w2 * w2)
            vc = var * (g * g)
            pok = bool(px >= 0 and px <= F(W - 1) and py >= 0 and py <= F(H - 1) and np.isfinite(xc) and np.isfinite(vc) and vc >= 0)
            proj = (px, py, xc, vc)
        if failed or not pok:
            drop += 1
        self.mu[s], self.var[s], self.drop[s], self.kstar[s] = mu, var, drop, ks
        self.counts[status] = self.counts.get(status, 0) + 1
        if drop > p["max_dropouts"]:
            self.alive[s], self.status[s] = 0, DIED
            self.counts[DIED] = self.counts.get(DIED, 0) + 1
            return None
        self.status[s] = status
        if not pok:
            return None
        dws = p["detection_win_size"]
        ncx = (W + dws - 1) // dws
        return (int(py) // dws) * ncx + int(px) // dws, proj


class GiDebugRef(D.DebugRef, GiRef):
    """GiRef with DebugRef's search record and pictures (DebugRef's calls reach GiRef's through the MRO)."""


class GiGatesDebugRef(D.DebugRef, G.GatesRef, GiRef):
    """... and GatesRef's gates between the two: the gates act on the projection the search left."""


class RgGiDebugRef(D.DebugRef, RG.RgRef, GiRef):
    """... the gradient gate in front of the search: it does not look at the cost."""


class RgGiGatesDebugRef(D.DebugRef, RG.RgGatesRef, GiRef):
    """... and all three."""
