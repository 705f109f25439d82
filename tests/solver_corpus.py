"""Adversarial corpus of the primal-dual solver: named, seeded, small cases generated in code
(tests/test_solver_f64_oracle.py, tests/test_gpu_solver_f64.py), and the checks of one step against oracle/nltgv2_np.py.

Each case is a dict: name; the graph pos [V,2] f32, edges [E,2] i32 (oriented source -> target), alpha, beta [E] f32,
z, wgt [V] f32; p (lam, tau, sigma, theta, x_min, x_max); d_sign; the start state st (x, w1, w2, xb, w1b, w2b [V] and
q [E,3], f32); tile (plan options that give the case its tile count on the tile paths); claims (what the case is there
to reach: test_corpus_reaches_what_it_claims); global_only (no tile path takes the graph).
"""
import numpy as np

from flame_ros_amd import graphgen
from oracle import nltgv2_np as N

STATE = ("x", "w1", "w2", "xb", "w1b", "w2b", "q")
DEFAULT = dict(lam=0.15, tau=1e-3, sigma=125.0, theta=0.25, x_min=0.0, x_max=10.0)
FAT_V = 256 * 196  # beyond this many vertices a graph gets fat tiles (one per CU)


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def mk(name, pos, edges, alpha, beta, z, wgt, st, d_sign=1, tile=None, claims=(), **p):
    edges = np.ascontiguousarray(edges, np.int32).reshape(-1, 2)
    c = dict(name=name, pos=f32(pos).reshape(-1, 2), edges=edges, alpha=f32(alpha), beta=f32(beta), z=f32(z),
             wgt=f32(wgt), p=dict(DEFAULT, **p), d_sign=int(d_sign), tile=dict(tile or {}), claims=tuple(claims))
    c["st"] = {k: (f32(v).reshape(-1, 3) if k == "q" else f32(v)) for k, v in st.items()}
    V, E = len(c["z"]), len(edges)
    assert c["pos"].shape == (V, 2) and c["alpha"].shape == (E,) and c["beta"].shape == (E,) and c["wgt"].shape == (V,)
    assert all(c["st"][k].shape == (V,) for k in STATE[:6]) and c["st"]["q"].shape == (E, 3)
    return c


def state(z, E, rng, xs=0.05, ws=1e-3, qs=0.8):
    V = len(z)
    x = np.asarray(z, np.float64) + rng.normal(0, xs, V)
    w1, w2 = rng.normal(0, ws, (2, V))
    return dict(x=x, w1=w1, w2=w2, xb=x + rng.normal(0, xs / 5, V), w1b=w1 + rng.normal(0, ws / 10, V),
                w2b=w2 + rng.normal(0, ws / 10, V), q=np.clip(rng.normal(0, qs, (E, 3)), -1, 1))


def free_beta(alpha, rng):
    return f32(alpha) * rng.uniform(0.25, 4.0, len(alpha)).astype(np.float32)


def wide_wgt(V, rng, zero_every=11):
    w = f32(1.0 / 10.0 ** rng.uniform(-4.0, 1.0, V))  # 1 / var: 0.1 .. 1e4
    w[::zero_every] = 0.0
    return w


def inv_len(pos, edges):
    d = pos[edges[:, 0]] - pos[edges[:, 1]]
    return (np.float32(1.0) / np.sqrt((d * d).sum(1, dtype=np.float32))).astype(np.float32)


def _graph_case(name, g, rng, tile=None, claims=(), alpha=None, beta=None, wgt=None, d_sign=1, **p):
    alpha = g.alpha if alpha is None else alpha
    beta = free_beta(g.alpha, rng) if beta is None else beta
    wgt = wide_wgt(g.V, rng) if wgt is None else wgt
    return mk(name, g.pos, g.edges, alpha, beta, g.z, wgt, state(g.z, g.E, rng), d_sign=d_sign, tile=tile, claims=claims,
              **p)


def _sync_rule(rule, ag, bg, seed):
    """The edge weights flame_hip_graph_sync gives under edge_weight_rule 1-3 with non-unit gains (float32, as in
    tests/test_graph_sync.py test_sync_upstream_recall_switches)."""
    g = graphgen.synthetic(700, seed=seed)
    rng = np.random.default_rng(seed)
    inv = g.alpha
    a = (np.ones_like(inv) if rule in (1, 3) else inv) * np.float32(ag)
    b = (np.ones_like(inv) if rule in (1, 2) else inv) * np.float32(bg)
    return _graph_case("sync_rule%d" % rule, g, rng, alpha=f32(a), beta=f32(b), wgt=np.ones(g.V, np.float32),
                       claims=("beta_ne_alpha",))


def _prox_ties():
    """Isolated vertices with dyadic tau, lambda, wgt, z and x = z +- t (exact ties of the soft threshold), x = z +- t +-
    2^-20 (just outside / inside), beside a 4 x 4 lattice so that the graph has edges."""
    rng = np.random.default_rng(60)
    n_iso = 96
    k = rng.integers(-3, 6, n_iso)
    wgt_iso = 2.0 ** k
    tau, lam = 2.0 ** -8, 2.0 ** -2
    t = tau * lam * wgt_iso
    z_iso = 0.5 + rng.integers(-64, 64, n_iso) * 2.0 ** -12
    off = np.array([1, -1, 1 + 2.0 ** -8, -1 - 2.0 ** -8, 1 - 2.0 ** -8, -1 + 2.0 ** -8])[np.arange(n_iso) % 6]
    x_iso = z_iso + off * t
    gx, gy = np.meshgrid(np.arange(4), np.arange(4))
    lat = np.c_[gx.ravel(), gy.ravel()] * 9.0 + 300.0
    e = [(a, a + 1) for a in range(16) if a % 4 != 3] + [(a, a + 4) for a in range(12)]
    pos = np.concatenate([rng.uniform(0, 640, (n_iso, 2)), lat])
    edges = np.asarray(e, np.int32) + n_iso
    alpha = inv_len(f32(pos), edges)
    z = np.concatenate([z_iso, rng.uniform(0.3, 0.7, 16)])
    st = state(z, len(edges), rng)
    st["x"][:n_iso] = x_iso
    st["xb"][:n_iso] = x_iso
    wgt = np.concatenate([wgt_iso, np.ones(16)])
    return mk("prox_ties", pos, edges, alpha, free_beta(alpha, rng), z, wgt, st, claims=("tie", "tiles:1"), tau=tau,
              lam=lam)


def _duals_edge():
    """|v| exactly 1 (edges whose K u is exactly 0: equal x_bar and zero w_bar on both ends, q = +-1), q = -0.0, and
    saturated duals."""
    rng = np.random.default_rng(61)
    gx, gy = np.meshgrid(np.arange(20), np.arange(20))
    pos = np.c_[gx.ravel(), gy.ravel()] * 7.0 + rng.uniform(-1, 1, (400, 2))
    vid = lambda i, j: j * 20 + i  # noqa: E731
    e = [(vid(i, j), vid(i + 1, j)) for j in range(20) for i in range(19)] + \
        [(vid(i, j), vid(i, j + 1)) for j in range(19) for i in range(20)]
    edges = np.asarray(e, np.int32)
    alpha = inv_len(f32(pos), edges)
    z = rng.uniform(0.4, 0.6, 400)
    st = state(z, len(edges), rng, qs=2.0)
    flat = gy.ravel() < 10  # the lower half: x_bar = 0.5, w_bar = 0
    for k in ("xb",):
        st[k][flat] = 0.5
    for k in ("w1b", "w2b"):
        st[k][flat] = 0.0
    inner = flat[edges[:, 0]] & flat[edges[:, 1]]
    q = st["q"]
    q[inner] = rng.choice([1.0, -1.0, -0.0], (int(inner.sum()), 3))
    return mk("duals_edge", pos, edges, alpha, free_beta(alpha, rng), z, wide_wgt(400, rng), st,
              claims=("dual_unit", "dual_sat", "neg_zero"), sigma=900.0)


def _hub_parallel():
    """A hub of degree 330 (edges of both orientations), a ring through its leaves, parallel and reversed edges, and a
    second component (a small lattice) beside it.  (No LDS tile holds a row of 200 incidences: on its own the library
    solves this graph on the global path, and a forced tile path is refused.)"""
    rng = np.random.default_rng(62)
    n = 320
    ang = np.linspace(0, 2 * np.pi, n, endpoint=False)
    leaves = np.c_[320 + 150 * np.cos(ang), 240 + 150 * np.sin(ang)]
    gx, gy = np.meshgrid(np.arange(6), np.arange(6))
    lat = np.c_[gx.ravel(), gy.ravel()] * 11.0 + 20.0
    pos = np.concatenate([[[320.0, 240.0]], leaves, lat])
    e = [(0, k) if k % 2 else (k, 0) for k in range(1, n + 1)]
    e += [(k, k % n + 1) for k in range(1, n + 1)]
    e += [(0, k) for k in range(1, 11)]                     # parallel to hub edges
    e += [(k % n + 1, k) for k in range(1, 40, 3)]         # reversed copies of ring edges
    b0 = n + 1
    e += [(b0 + a, b0 + a + 1) for a in range(36) if a % 6 != 5] + [(b0 + a + 6, b0 + a) for a in range(30)]
    edges = np.asarray(e, np.int32)
    alpha = inv_len(f32(pos), edges)
    z = rng.uniform(0.3, 0.9, len(pos))
    c = mk("hub_parallel", pos, edges, alpha, free_beta(alpha, rng), z, wide_wgt(len(pos), rng),
           state(z, len(edges), rng), claims=("hub", "parallel", "reversed", "components"))
    c["global_only"] = True  # an incidence list this long fits no LDS tile: the library picks the global path itself
    return c


def _two_vertices():
    rng = np.random.default_rng(63)
    pos = [[10.0, 20.0], [13.0, 24.0]]
    edges = [[0, 1], [1, 0]]
    alpha = inv_len(f32(pos), np.asarray(edges))
    z = [0.4, 0.9]
    return mk("two_vertices", pos, edges, alpha, alpha * np.float32(3.0), z, [1.0, 250.0], state(z, 2, rng, qs=0.5),
              claims=("two_vertices", "parallel", "reversed"), theta=1.0)


def _long_short():
    """Pixel coordinates up to 1e4, edges of 0.01 and of 2500 / 5000 px, a plane of slope ~1e2 in x and w: the w d terms
    (~5e5) cancel against x_bar_i - x_bar_j."""
    rng = np.random.default_rng(64)
    gx, gy = np.meshgrid(np.arange(5), np.arange(5))
    base = np.c_[gx.ravel(), gy.ravel()].astype(np.float64) * 2500.0
    pos = f32(np.concatenate([base, base + [0.01, 0.0]]))
    vid = lambda i, j: j * 5 + i  # noqa: E731
    e = [(vid(i, j), vid(i + 1, j)) for j in range(5) for i in range(4)] + \
        [(vid(i, j), vid(i, j + 1)) for j in range(4) for i in range(5)] + \
        [(vid(i, j), vid(i + 2, j)) for j in range(5) for i in range(3)] + [(k, k + 25) for k in range(25)]
    edges = np.asarray(e, np.int32)
    alpha = inv_len(pos, edges)
    sx, sy = 100.0, -60.0
    z = 3e5 + sx * pos[:, 0].astype(np.float64) + sy * pos[:, 1]
    st = state(z, len(edges), rng, xs=1e-2, ws=0.0)
    for k, s in (("w1", sx), ("w2", sy), ("w1b", sx), ("w2b", sy)):
        st[k] = s + rng.normal(0, 1e-3, len(z))
    return mk("long_short", pos, edges, alpha, free_beta(alpha, rng), z, wide_wgt(len(z), rng), st,
              claims=("long_short", "cancel"), x_min=-2e6, x_max=2e6)


def _clamp_pinch():
    g = graphgen.synthetic(300, seed=66)
    rng = np.random.default_rng(66)
    z = f32(rng.uniform(0.0, 1.0, g.V))
    return mk("clamp_pinch", g.pos, g.edges, g.alpha, free_beta(g.alpha, rng), z, wide_wgt(g.V, rng),
              state(z, g.E, rng), claims=("pinch", "z_outside", "tiles:1"), x_min=0.5, x_max=0.5)


def _clamp_ends():
    g = graphgen.synthetic(600, seed=67)
    rng = np.random.default_rng(67)
    z = f32(rng.uniform(-0.5, 1.5, g.V))
    st = state(z, g.E, rng, xs=0.3)
    return mk("clamp_ends", g.pos, g.edges, g.alpha, free_beta(g.alpha, rng), z, wide_wgt(g.V, rng), st,
              claims=("clamp_min", "clamp_max", "z_outside"), x_min=0.25, x_max=0.75)


def corpus(with_fat=True):
    rng = np.random.default_rng
    cases = [
        _graph_case("beta_free_synth", graphgen.synthetic(1500, seed=41), rng(41), claims=("beta_ratio",)),
        _graph_case("beta_free_grid", graphgen.dataset_shaped(640, 480, 16, seed=42), rng(42),
                    claims=("beta_ratio", "tiles:32")),
        _zero_weights(),
        _sync_rule(1, 2.5, 0.75, 44), _sync_rule(2, 0.5, 3.0, 45), _sync_rule(3, 1.5, 0.25, 46),
        _graph_case("wgt_wide", graphgen.synthetic(2000, seed=1), rng(47), tile=dict(tile_own=61),
                    claims=("wgt_wide", "snap", "tiles:33"), theta=1.0),
        _prox_ties(), _clamp_ends(), _clamp_pinch(), _duals_edge(),
        _graph_case("unstable", graphgen.synthetic(800, seed=50), rng(50), claims=("unstable",), tau=0.02, sigma=400.0,
                    theta=0.3),
        _hub_parallel(), _two_vertices(), _long_short(),
        _graph_case("dsign_neg", graphgen.dataset_shaped(320, 240, 8, seed=51), rng(51), claims=("d_sign",), d_sign=-1),
        _graph_case("tiles256", graphgen.synthetic(5120, seed=1), rng(52), tile=dict(tile_own=20),
                    claims=("tiles:256",), theta=0.3),
    ]
    if with_fat:
        cases.append(_graph_case("fat60k", graphgen.synthetic(60000, seed=60000), rng(53), claims=("fat", "tiles:256")))
    return cases


def _zero_weights():
    g = graphgen.synthetic(900, seed=43)
    rng = np.random.default_rng(43)
    alpha = g.alpha.copy()
    beta = free_beta(alpha, rng)
    alpha[::5] = 0.0
    beta[2::5] = 0.0
    return mk("zero_weights", g.pos, g.edges, alpha, beta, g.z, wide_wgt(g.V, rng), state(g.z, g.E, rng),
              tile=dict(tile_own=450), claims=("alpha_zero", "beta_zero", "tiles:2"), theta=0.0)


# ---- checks ----
def step_f64(case, st):
    p = case["p"]
    return N.pd_step_f64(st, case["pos"], case["edges"], case["alpha"], case["beta"], case["z"], case["wgt"], p["lam"],
                         p["tau"], p["sigma"], p["theta"], p["x_min"], p["x_max"], case["d_sign"])


def check_step(case, prev, got, what):
    """got (float32 state) is one PD step from prev: within the float64 statement's bands everywhere, exact where the
    outcome is certain.  Returns {state name: largest band / largest |got - prev|} (how tight the bands are)."""
    nxt, band, exact = step_f64(case, prev)
    tight = {}
    for k in STATE:
        g = np.asarray(got[k], np.float32).reshape(nxt[k].shape).astype(np.float64)
        assert np.isfinite(g).all(), "%s %s: non-finite values" % (what, k)
        err = np.abs(g - nxt[k])
        bad = ~(err <= band[k])
        if bad.any():
            idx = np.argwhere(bad)[:5].tolist()
            r = (err / band[k])[bad]
            raise AssertionError("%s %s: %d values outside the float64 band (worst %.3g x band), first at %s: got %s, "
                                 "want %s +- %s" % (what, k, int(bad.sum()), float(r.max()), idx,
                                                    g[bad][:3].tolist(), nxt[k][bad][:3].tolist(), band[k][bad][:3].tolist()))
        for mask, val in exact.get(k, []):
            want = np.asarray(got[val], np.float32).reshape(g.shape) if isinstance(val, str) else val
            off = mask & (g != want)
            assert not off.any(), "%s %s: %d certain outcomes missed, first at %s: got %s, want %s" % (
                what, k, int(off.sum()), np.argwhere(off)[:5].tolist(), g[off][:3].tolist(),
                np.broadcast_to(want, g.shape)[off][:3].tolist())
        moved = np.abs(g - np.asarray(prev[k], np.float64).reshape(g.shape))
        tight[k] = float(band[k].max() / moved.max()) if moved.size and moved.max() > 0 else 0.0
    return tight


def check_sync(got, pos, mu, var, tris, pred, adaptive, rescale, init_pred, rule=0, ag=0.0, bg=0.0, what="sync"):
    """got: dict(edges, alpha, beta, z, wgt, x0, scale) of an implementation, against graph_sync_f64."""
    s = np.float32(got["scale"])
    want = N.graph_sync_f64(pos, mu, var, tris, pred, adaptive, rescale, init_pred, rule, ag, bg, scale=s)
    assert any(s == c for c in want["scales"]), "%s: scale %r is no float32 neighbour of the exact mean %r" % (
        what, float(s), [float(c) for c in want["scales"]])
    assert np.array_equal(np.asarray(got["edges"]), want["edges"]), what + ": edges"
    for k in ("alpha", "beta"):
        g = np.asarray(got[k], np.float64)
        err = np.abs(g - want[k])
        bad = ~(err <= N.K_SYNC * N.EPS32 * np.abs(want[k]))
        assert not bad.any(), "%s %s: %d outside K_SYNC eps32 relative, worst %.3g" % (
            what, k, int(bad.sum()), float((err / np.abs(want[k]))[bad].max()))
    for k in ("z", "wgt", "x0"):
        g = np.asarray(got[k], np.float32)
        bad = g.view(np.uint32) != want[k].view(np.uint32)
        assert not bad.any(), "%s %s: %d values are not the correctly rounded quotient, first at %s" % (
            what, k, int(bad.sum()), np.flatnonzero(bad)[:5].tolist())


def state_of(o):
    """The state of a COracle (or of any object with the seven state arrays), copied."""
    return {k: np.array(getattr(o, k), np.float32) for k in STATE}


def reached(case):
    """The facts behind a case's claims, from the case itself and the float64 step from its start state."""
    a, b, pos, ed = case["alpha"], case["beta"], case["pos"], case["edges"].astype(np.int64)
    V, E = len(case["z"]), len(a)
    p, st = case["p"], case["st"]
    nxt, band, exact = step_f64(case, st)
    tp = p["tau"] * p["lam"] * case["wgt"].astype(np.float64)
    deg = np.bincount(ed.ravel(), minlength=V)
    isolated = deg == 0
    r_iso = np.abs(st["x"].astype(np.float64) - case["z"])[isolated]
    q64 = st["q"].astype(np.float64)
    P = pos.astype(np.float64) * case["d_sign"]
    d = P[ed[:, 0]] - P[ed[:, 1]]
    length = np.hypot(d[:, 0], d[:, 1])
    xb, w1b, w2b = (st[k].astype(np.float64) for k in ("xb", "w1b", "w2b"))
    wd = np.abs(w1b[ed[:, 0]] * d[:, 0] + w2b[ed[:, 0]] * d[:, 1])
    v1 = xb[ed[:, 0]] - xb[ed[:, 1]] - w1b[ed[:, 0]] * d[:, 0] - w2b[ed[:, 0]] * d[:, 1]
    ratio = (b / np.where(a > 0, a, 1))[a > 0]
    pairs = np.sort(ed, 1)
    facts = dict(
        beta_ratio=len(ratio) > 0 and ratio.min() <= 0.3 and ratio.max() >= 3.5,  # beta / alpha spans U(0.25, 4)
        beta_ne_alpha=bool((a != b).all()),
        alpha_zero=bool(((a == 0) & (b != 0)).any()), beta_zero=bool(((b == 0) & (a != 0)).any()),
        wgt_wide=bool(case["wgt"].max() >= 1e3 and (case["wgt"] == 0).any()),
        snap=bool(exact["x"][2][0].sum() >= 10),
        tie=bool((r_iso == tp[isolated]).sum() >= 10),
        clamp_min=bool(exact["x"][0][0].any()), clamp_max=bool(exact["x"][1][0].any()),
        pinch=p["x_min"] == p["x_max"],
        z_outside=bool(((case["z"] < p["x_min"]) | (case["z"] > p["x_max"])).any()),
        dual_unit=bool((np.abs(nxt["v"]) == 1.0).sum() >= 10),
        dual_sat=bool(exact["q"][0][0].sum() >= 10),
        neg_zero=bool((np.signbit(st["q"]) & (st["q"] == 0)).any()),
        unstable=p["tau"] * p["sigma"] * float((np.maximum(a, b) ** 2).max()) * 2 > 1,
        hub=int(deg.max()) >= 300,
        parallel=len(np.unique(pairs, axis=0)) < E,
        reversed=bool((ed[:, 0] > ed[:, 1]).any()),
        components=_components(V, ed) >= 2,
        two_vertices=V == 2,
        long_short=bool(length.min() <= 0.011 and length.max() >= 4999),
        cancel=bool(wd.max() >= 1e5 and np.abs(v1)[wd >= 1e5].max() <= 1e-3 * wd.max()),
        d_sign=case["d_sign"] == -1,
        fat=V > FAT_V,
    )
    return facts


def _components(V, ed):
    parent = np.arange(V)

    def find(u):
        while parent[u] != u:
            parent[u] = parent[parent[u]]
            u = parent[u]
        return u
    for i, j in ed:
        ri, rj = find(i), find(j)
        if ri != rj:
            parent[ri] = rj
    return len({find(u) for u in range(V)})
