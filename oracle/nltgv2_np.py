"""Independent float64 NumPy restatement of the NLTGV2-L1 primal-dual iteration.

TEST INFRASTRUCTURE (see oracle/__init__.py).  Written from the paper-level formulas in SURVEY.md
section 8a rows a2-a6 in vectorised form (scatter by np.add.at), deliberately NOT sharing code or
operation order with nltgv2_oracle.c: agreement of the two (K9: <= 1e-5 RMS after 200 iterations)
is what pins the C restatement in the absence of reference golden vectors (PARITY UNPINNED).
"""
import numpy as np


class NpSolver:
    def __init__(self, pos, edges, alpha, beta, z, wgt, x0=None, dtype=np.float64):
        f = lambda a: np.asarray(a, dtype=dtype)  # noqa: E731
        self.pos = f(pos).reshape(-1, 2)
        self.edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
        self.alpha, self.beta, self.z, self.wgt = f(alpha), f(beta), f(z), f(wgt)
        self.V, self.E = len(self.z), len(self.alpha)
        self.i, self.j = self.edges[:, 0], self.edges[:, 1]
        self.d = self.pos[self.i] - self.pos[self.j]
        self.x = (self.z if x0 is None else f(x0)).copy()
        self.w = np.zeros((self.V, 2), dtype)
        self.xb, self.wb = self.x.copy(), self.w.copy()
        self.q = np.zeros((self.E, 3), dtype)

    def K(self, x, w):
        i, j = self.i, self.j
        k1 = self.alpha * (x[i] - x[j] - (w[i] * self.d).sum(1))
        k23 = self.beta[:, None] * (w[i] - w[j])
        return np.column_stack([k1, k23])

    def KT(self, q):
        i, j = self.i, self.j
        kx = np.zeros(self.V, q.dtype)
        kw = np.zeros((self.V, 2), q.dtype)
        aq = self.alpha * q[:, 0]
        bq = self.beta[:, None] * q[:, 1:]
        np.add.at(kx, i, aq)
        np.add.at(kx, j, -aq)
        np.add.at(kw, i, -aq[:, None] * self.d + bq)
        np.add.at(kw, j, -bq)
        return kx, kw

    def step(self, lam, tau, sigma, theta, x_min=0.0, x_max=10.0):
        v = self.q + sigma * self.K(self.xb, self.wb)
        self.q = v / np.maximum(1.0, np.abs(v))
        xp, wp = self.x, self.w
        kx, kw = self.KT(self.q)
        x = xp - tau * kx
        w = wp - tau * kw
        t = tau * lam * self.wgt
        r = x - self.z
        x = np.where(r > t, x - t, np.where(r < -t, x + t, self.z))
        x = np.clip(x, x_min, x_max)
        self.x, self.w = x, w
        self.xb = x + theta * (x - xp)
        self.wb = w + theta * (w - wp)

    def solve(self, n, lam=0.15, tau=1e-3, sigma=125.0, theta=0.25, x_min=0.0, x_max=10.0):
        for _ in range(n):
            self.step(lam, tau, sigma, theta, x_min, x_max)
        return self.x

    def costs(self, lam=0.15):
        k = self.K(self.x, self.w)
        smooth = np.abs(k).sum()
        data = (lam * self.wgt * np.abs(self.x - self.z)).sum()
        return float(smooth), float(data)


# ---- One PD step and the graph sync (rows a2-a5, a7), float64, with the float32 error bands ----
# Written from the formulas, like NpSolver and oracle/frame_f64.py: no operation order is shared with the C oracle or the
# kernels.  A float32 implementation is held against them by tests/solver_corpus.py check_step / check_sync.
#
# Every band is K * EPS32 * (a magnitude this statement propagates stage by stage); the K are stated here once.  Each
# stage is 1-Lipschitz (the dual projection, soft-thresholding toward z, the clamp) or scales by a known factor (the
# extra-gradient), so no stage amplifies what came in by more than its magnitude says.
EPS32 = 2.0 ** -23
K_DUAL = 4    # v = q + sigma K u: K_DUAL eps32 (|q| + sigma |alpha| (|xb_i| + |xb_j| + |w1b_i dx| + |w2b_i dy|)), ditto beta
K_PRIMAL = 2  # u - tau K^T q': K_PRIMAL eps32 (deg + 2) (|u| + tau sum |terms|), plus tau sum |weight| band(q')
K_T = 2       # t = tau lambda wgt: K_T eps32 t
K_ROUND = 2   # one rounding of a stage's output: K_ROUND eps32 (the operands' magnitudes)
K_SYNC = 4    # alpha, beta of the sync: K_SYNC eps32 relative
TINY = 2.0 ** -140  # absolute floor: an operation whose result is subnormal errs by up to 2^-150


def _bin(idx, w, n):
    return np.bincount(idx, weights=w, minlength=n)


def pd_step_f64(st, pos, edges, alpha, beta, z, wgt, lam, tau, sigma, theta, x_min, x_max, d_sign=1):
    """One PD iteration (dual; primal with prox and clamp; extra-gradient) from the float32 state `st` (x, w1, w2, xb,
    w1b, w2b [V], q [E,3]) in float64.  d = d_sign (pos_i - pos_j), exact.  Returns (next, band, exact):
    next / band map each state name to the float64 value and the absolute float32 band around it; exact maps a state
    name to (mask, value) pairs where the outcome is certain and a float32 implementation must hit `value` exactly (a
    value that is a state name: the implementation's own next value of that state)."""
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    x, w1, w2, xb, w1b, w2b = (f(st[k]) for k in ("x", "w1", "w2", "xb", "w1b", "w2b"))
    q = f(st["q"]).reshape(-1, 3)
    P = f(pos).reshape(-1, 2)
    ed = np.asarray(edges, np.int64).reshape(-1, 2)
    i, j = ed[:, 0], ed[:, 1]
    a, b, z, wgt = f(alpha), f(beta), f(z), f(wgt)
    V, E = len(x), len(a)
    lam, tau, sigma, theta, x_min, x_max = (float(v) for v in (lam, tau, sigma, theta, x_min, x_max))
    d = float(d_sign) * (P[i] - P[j])
    dx, dy = d[:, 0], d[:, 1]
    ab, bb = np.abs(a), np.abs(b)

    # dual ascent and projection onto [-1, 1]
    v = np.column_stack([q[:, 0] + sigma * a * (xb[i] - xb[j] - w1b[i] * dx - w2b[i] * dy),
                         q[:, 1] + sigma * b * (w1b[i] - w1b[j]),
                         q[:, 2] + sigma * b * (w2b[i] - w2b[j])])
    mv = np.column_stack([np.abs(q[:, 0]) + sigma * ab * (np.abs(xb[i]) + np.abs(xb[j]) + np.abs(w1b[i] * dx) +
                                                          np.abs(w2b[i] * dy)),
                          np.abs(q[:, 1]) + sigma * bb * (np.abs(w1b[i]) + np.abs(w1b[j])),
                          np.abs(q[:, 2]) + sigma * bb * (np.abs(w2b[i]) + np.abs(w2b[j]))])
    bv = K_DUAL * EPS32 * mv + TINY
    qn = np.clip(v, -1.0, 1.0)
    q_sat = np.abs(v) - 1.0 > bv
    bq = np.minimum(bv, 2.0)  # (q' lies in [-1, 1] whatever v's error)

    # primal descent u - tau K^T q'
    aq, b2, b3 = a * qn[:, 0], b * qn[:, 1], b * qn[:, 2]
    kx = _bin(i, aq, V) - _bin(j, aq, V)
    kw1 = _bin(i, b2 - dx * aq, V) - _bin(j, b2, V)
    kw2 = _bin(i, b3 - dy * aq, V) - _bin(j, b3, V)
    xh, w1n, w2n = x - tau * kx, w1 - tau * kw1, w2 - tau * kw2
    deg = (np.bincount(i, minlength=V) + np.bincount(j, minlength=V)).astype(np.float64)
    s = lambda wi, wj: _bin(i, wi, V) + _bin(j, wj, V)  # noqa: E731  (sum over the incident edges)
    maq = np.abs(aq)
    mx = np.abs(x) + tau * s(maq, maq)
    mw1 = np.abs(w1) + tau * s(np.abs(dx) * maq + np.abs(b2), np.abs(b2))
    mw2 = np.abs(w2) + tau * s(np.abs(dy) * maq + np.abs(b3), np.abs(b3))
    pa = ab * bq[:, 0]
    bxh = K_PRIMAL * EPS32 * (deg + 2) * mx + tau * s(pa, pa) + TINY
    bw1 = K_PRIMAL * EPS32 * (deg + 2) * mw1 + tau * s(np.abs(dx) * pa + bb * bq[:, 1], bb * bq[:, 1]) + TINY
    bw2 = K_PRIMAL * EPS32 * (deg + 2) * mw2 + tau * s(np.abs(dy) * pa + bb * bq[:, 2], bb * bq[:, 2]) + TINY

    # L1 prox toward z (soft-thresholding by t = tau lambda wgt), then the clamp
    t = tau * lam * wgt
    bt = K_T * EPS32 * t
    r = xh - z
    xt = np.where(r > t, xh - t, np.where(r < -t, xh + t, z))
    rnd = K_ROUND * EPS32 * (np.abs(xh) + np.abs(z) + t)
    bxt = bxh + bt + rnd + TINY
    snap = np.abs(r) + bxh + bt + rnd < t
    xn = np.clip(xt, x_min, x_max)
    at_min, at_max = xt < x_min - bxt, xt > x_max + bxt

    # extra-gradient
    xbn = xn + theta * (xn - x)
    w1bn = w1n + theta * (w1n - w1)
    w2bn = w2n + theta * (w2n - w2)
    th = abs(theta)
    eg = lambda bu, un, u, ubn: (1 + th) * bu + K_ROUND * EPS32 * (th * (np.abs(un) + np.abs(u)) + np.abs(ubn)) + TINY  # noqa: E731

    nxt = dict(x=xn, w1=w1n, w2=w2n, xb=xbn, w1b=w1bn, w2b=w2bn, q=qn, v=v)  # (v: the dual before its projection)
    band = dict(x=bxt, w1=bw1, w2=bw2, xb=eg(bxt, xn, x, xbn), w1b=eg(bw1, w1n, w1, w1bn), w2b=eg(bw2, w2n, w2, w2bn),
                q=bq)
    iso = deg == 0
    exact = dict(q=[(q_sat, np.sign(v))],
                 x=[(at_min, np.full(V, x_min)), (at_max, np.full(V, x_max)),
                    (snap & ~at_min & ~at_max, np.clip(z, x_min, x_max))],
                 w1=[(iso, w1)], w2=[(iso, w2)], w1b=[(iso, w1)], w2b=[(iso, w2)])
    if theta == 0.0:
        exact["xb"] = [(np.ones(V, bool), "x")]  # a name: the implementation's own next x (w1, w2)
        exact["w1b"].append((np.ones(V, bool), "w1"))
        exact["w2b"].append((np.ones(V, bool), "w2"))
    return nxt, band, exact


def graph_sync_f64(pos, mu, var, tris, prediction=None, adaptive=0, rescale=0, init_pred=1, rule=0, alpha_gain=0.0,
                   beta_gain=0.0, scale=None):
    """Row a7 in float64: the unique undirected edges (i < j, lexicographic), alpha / beta by rule and gain (rule 0:
    both 1/len; 1: both 1; 2: alpha 1/len, beta 1; 3: alpha 1, beta 1/len; a gain of 0 reads 1), the admissible
    data scales (the float32 neighbours of the exact mean of mu when rescaling, a mean that is not > 0 reads 1) and,
    for the scale an implementation chose (`scale`, default the first admissible one), the data terms z = mu / scale,
    wgt = 1 / var (or 1), x0 = prediction / scale where it is finite (or z): each the correctly rounded float32 quotient
    (rounding the float64 quotient of two float32 values once is exactly that)."""
    from fractions import Fraction
    P = np.asarray(pos, np.float64).reshape(-1, 2)
    mu32 = np.asarray(mu, np.float32)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1)
    edges = np.unique(e, axis=0).reshape(-1, 2)
    i, j = edges[:, 0], edges[:, 1]
    inv = 1.0 / np.hypot(P[i, 0] - P[j, 0], P[i, 1] - P[j, 1])
    one = np.ones(len(edges))
    alpha = (one if rule in (1, 3) else inv) * (float(alpha_gain) or 1.0)
    beta = (one if rule in (1, 2) else inv) * (float(beta_gain) or 1.0)
    scales = [np.float32(1.0)]
    if rescale and len(mu32):
        mean = sum((Fraction(float(m)) for m in mu32), Fraction(0)) / len(mu32)
        m32 = np.float32(float(mean))
        if Fraction(float(m32)) == mean:
            scales = [m32]
        elif Fraction(float(m32)) < mean:
            scales = [m32, np.nextafter(m32, np.float32(np.inf))]
        else:
            scales = [np.nextafter(m32, np.float32(-np.inf)), m32]
        scales = [s if s > 0 else np.float32(1.0) for s in scales]
    s = np.float32(scales[0] if scale is None else scale)
    z = (mu32.astype(np.float64) / float(s)).astype(np.float32)
    wgt = ((1.0 / np.asarray(var, np.float64)).astype(np.float32) if adaptive else np.ones(len(mu32), np.float32))
    x0 = z.copy()
    if init_pred and prediction is not None:
        pr = np.asarray(prediction, np.float32)
        ok = np.isfinite(pr)
        x0[ok] = (pr[ok].astype(np.float64) / float(s)).astype(np.float32)
    return dict(edges=edges.astype(np.int32), alpha=alpha, beta=beta, scales=scales, z=z, wgt=wgt, x0=x0)
