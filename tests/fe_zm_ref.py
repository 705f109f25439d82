"""The feature front end's matching cost (DESIGN.md 5.3 "Matching cost"; include/flame_hip.h, flame_hip_frontend_set_cost) restated
in NumPy on top of tests/frontend_ref.py.  A helper, not a test: tests/test_fe_zm_ref.py checks it on hand-written windows, for exact
offset invariance and against ground truth, tests/test_gpu_fe_zm.py compares the library with it bit for bit.

`ZmRef` is FrontEndRef plus `set_cost`.  In mode SSD every call goes to the base class untouched.  In mode ZSSD
  * `_cost` is the base class's window with the integer rule  n = win^2, S1 = sum D, S2 = sum D^2, C = n S2 - S1^2  (Python integers:
    no width to overflow; the kernel forms S1 in an int32, S2 and C in 64 bits);
  * `_track_one` is the base class's search -- the same float32 operations in the same order -- with that cost in every decision and
    BAD_MATCH at C > n bad, the product saturated at 2^64 - 1.
`ZmDebugRef` / `ZmGatesDebugRef` add fe_debug_ref.DebugRef's search record and pictures (and fe_gates_ref.GatesRef's gates) for
the GPU comparison."""
import numpy as np

from tests import fe_debug_ref as D
from tests import fe_gates_ref as G
from tests import frontend_ref as R

F = np.float32
COST_SSD, COST_ZSSD = 0, 1
U64_MAX = 2 ** 64 - 1


def sat_mul(n, bad):
    """n * bad, saturated at UINT64_MAX the way the host forms it (the quotient test, no wide product)."""
    return U64_MAX if bad > U64_MAX // n else n * bad


def bad_threshold(max_match_error, win, mode):
    """BAD_MATCH is C > this: bad = (uint64)(max_match_error win^2 65536) for SSD, n bad (saturated) for ZSSD."""
    n = win * win
    bad = int(float(F(max_match_error)) * float(n) * 65536.0)
    return bad if mode == COST_SSD else sat_mul(n, bad)


def zssd(Dm):
    """The rule on a window of differences D_i (any integer array)."""
    d = [int(x) for x in np.asarray(Dm).reshape(-1)]
    n, S1, S2 = len(d), sum(d), sum(x * x for x in d)
    return n * S2 - S1 * S1


class ZmRef(R.FrontEndRef):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.cost_mode = COST_SSD

    def set_cost(self, zero_mean=True):
        self.cost_mode = COST_ZSSD if zero_mean else COST_SSD

    def _cost(self, cur, ref, u, v, px, py, win):
        if self.cost_mode == COST_SSD:
            return super()._cost(cur, ref, u, v, px, py, win)
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
        c = cur[iy - r:iy + r + 2, ix - r:ix + r + 2]
        Dm = (wx0 * wy0) * c[:-1, :-1] + (wx1 * wy0) * c[:-1, 1:] + (wx0 * wy1) * c[1:, :-1] + (wx1 * wy1) * c[1:, 1:] \
            - 256 * ref[v - r:v + r + 1, u - r:u + r + 1]
        return zssd(Dm)

    def _track_one(self, s, p, cur, poses):
        if self.cost_mode == COST_SSD:
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
                C = [self._cost(cur, ref, u, v, x0 + F(k) * ex, y0 + F(k) * ey, win) for k in range(S + 1)]
                valid = [k for k in range(S + 1) if C[k] is not None]
                if not valid:
                    status = OUTSIDE
                else:
                    ks = min(valid, key=lambda k: (C[k], k))  # the key (C << 9) | k: smallest cost, then smallest k
                    Cb = C[ks]
                    assert all(0 <= C[k] < 2 ** 45 for k in valid)
                    if Cb > bad_threshold(p["max_match_error"], win, COST_ZSSD):
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


class ZmDebugRef(D.DebugRef, ZmRef):
    """ZmRef with DebugRef's search record and pictures (DebugRef's calls reach ZmRef's through the MRO)."""


class ZmGatesDebugRef(D.DebugRef, G.GatesRef, ZmRef):
    """... and GatesRef's gates between the two: the gates act on the projection the ZSSD search left."""
