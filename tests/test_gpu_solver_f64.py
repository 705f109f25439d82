"""-m gpu: the HIP solver paths held against the float64 statement of one PD step (oracle/nltgv2_np.py pd_step_f64)
directly, not through the C oracle: a slip the kernels share with the oracle fails here.

For each case of tests/solver_corpus.py and each path, the state S_n is the device's after n iterations from the case's
start state S0 (set_state, solve, download), for n in {0, 1, D - 1, D, D + 1} (D = the plan's halo depth) and one ragged
split of two solves; S_(n+1) is checked against the float64 step from S_n.  Each check starts from the device's own state,
so nothing builds up over iterations, and the inner iterations of a round and the hand-offs between rounds are each
checked.  Then row a7: the device sync (rule 0) and the host sync (rules 1-3, gains) against graph_sync_f64, a step on
the synced graph, and scale_state (fl32(x s), bit for bit)."""
import numpy as np
import pytest

from flame_ros_amd.regularizer import GraphRegularizer, default_params, default_sync_params
from oracle import nltgv2_np as N
from oracle.cbind import SyncParams as OSync, graph_sync as oracle_sync
from tests.solver_corpus import FAT_V, STATE, check_step, corpus, f32, state
from tests.test_graph_sync import features

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in corpus()}
PATHS = {
    "global": dict(path=1),
    "launches": dict(path=2, persist=0),
    "halo_small_deep": dict(path=2, tile_own=48, tile_depth=6),
    "resident": {},  # the default: resident tiles (one XCD for 2 .. 32 tiles, fat tiles beyond 256 x 196 vertices)
    "host_plan": dict(plan_device=0),
}
COMBOS = [(c, p) for c in CASES for p in PATHS if not (c == "fat60k" and p == "halo_small_deep") and
          not (CASES[c].get("global_only") and p not in ("global", "resident"))]


def params_of(case):
    p = case["p"]
    return default_params(p["lam"], p["tau"], p["sigma"], p["theta"], p["x_min"], p["x_max"])


def download_all(r):
    x, w1, w2, q = r.download()
    xb, w1b, w2b = r.download_bar()
    return dict(x=x, w1=w1, w2=w2, xb=xb, w1b=w1b, w2b=w2b, q=q)


def solve_from(r, st, P, chunks):
    r.set_state(**st)
    for n in chunks:
        if n:
            r.step(P, n)
    return download_all(r)


@pytest.mark.parametrize("name,path", COMBOS)
def test_kernel_steps_against_f64(gpu, name, path):
    c = CASES[name]
    opts = dict(PATHS[path])
    if path in ("launches", "resident", "host_plan"):
        opts = dict(c["tile"], **opts)
    P = params_of(c)
    with GraphRegularizer(c["pos"], c["edges"], c["alpha"], c["beta"], c["z"], c["wgt"], device=0,
                          d_sign=c["d_sign"], **opts) as r:
        D = r.info("tile_depth") or 4
        tiles = r.info("num_tiles") if r.info("path") == 2 else 0
        if path == "resident" and c["pos"].shape[0] > FAT_V:
            assert tiles == 256, tiles  # fat tiles: one per CU
        S = {}
        for n in sorted({0, 1, 2, max(D - 1, 0), D, D + 1, D + 2}):
            S[(n,)] = solve_from(r, c["st"], P, [n])
            if path == "resident" and n > D and 2 <= tiles <= 256:
                assert r.info("persist_used") == 1, (n, D)
                if tiles <= 32:
                    assert r.info("one_xcd_used") == 1
        for n in sorted({0, 1, max(D - 1, 0), D, D + 1}):
            check_step(c, S[(n,)], S[(n + 1,)], "%s %s: step %d (D = %d)" % (name, path, n + 1, D))
        a = solve_from(r, c["st"], P, [D + 2, D - 1])
        b = solve_from(r, c["st"], P, [D + 2, D])
        check_step(c, a, b, "%s %s: step %d after a ragged split (D = %d)" % (name, path, 2 * D + 2, D))


# ---- row a7 on the device: sync, then step ----
SYNCS = [(1, 1, 1, 0, 0.0, 0.0), (0, 1, 1, 0, 0.0, 0.0), (0, 1, 1, 2, 0.5, 3.0), (1, 1, 0, 3, 1.5, 0.25),
         (0, 0, 1, 1, 2.5, 0.75)]


@pytest.mark.parametrize("adaptive,rescale,init_pred,rule,ag,bg", SYNCS)
def test_sync_then_step_against_f64(gpu, adaptive, rescale, init_pred, rule, ag, bg):
    g, var, pred = features(3000, 70 + rule)
    if adaptive:  # 1/var up to 500: the data step stays inside the clamp range
        var = np.maximum(var, np.float32(2e-3))
    mu = g.z * np.float32(3.7)
    args = (adaptive, rescale, init_pred, 0.01, rule, ag, bg)
    with GraphRegularizer.empty(device=0) as r:
        scale = r.sync_features(g.pos, mu, var, g.tris, default_sync_params(*args), prediction=pred)
        if rule == 0:
            assert r.info("plan_on_device") == 1  # the device sync
        want = N.graph_sync_f64(g.pos, mu, var, g.tris, pred, adaptive, rescale, init_pred, rule, ag, bg,
                                scale=np.float32(scale))
        assert any(np.float32(scale) == s for s in want["scales"]), (scale, want["scales"])
        edges = r.edges()
        assert np.array_equal(edges, want["edges"])
        S0 = download_all(r)
        assert np.array_equal(f32(S0["x"]).view(np.uint32), want["x0"].view(np.uint32)), "x0"
        # the graph the solver holds: float32 alpha / beta as the oracle states them (the library's host sync equals
        # them bit for bit, tests/test_graph_sync.py), within K_SYNC eps32 of float64
        o = oracle_sync(OSync(*args), g.pos, mu, var, g.tris, pred)
        for k in ("alpha", "beta"):
            assert np.all(np.abs(o[k] - want[k]) <= N.K_SYNC * N.EPS32 * np.abs(want[k])), k
        case = dict(pos=g.pos, edges=edges, alpha=o["alpha"], beta=o["beta"], z=want["z"], wgt=want["wgt"],
                    p=dict(lam=0.15, tau=1e-3, sigma=125.0, theta=0.25, x_min=0.0, x_max=10.0), d_sign=1)
        P = params_of(case)
        r.step(P, 1)
        check_step(case, S0, download_all(r), "sync %s: first step" % (args,))
        st = {k: f32(v) for k, v in state(want["z"], len(edges), np.random.default_rng(rule), ws=0.05).items()}
        r.set_state(**st)
        r.step(P, 1)
        S1 = download_all(r)
        check_step(case, st, S1, "sync %s: step from a random state" % (args,))
        s = np.float32(scale if scale != 1.0 else 1.7)
        r.scale_state(float(s))
        S2 = download_all(r)
        for k in STATE[:6]:
            assert np.array_equal(S2[k].view(np.uint32), (S1[k] * s).astype(np.float32).view(np.uint32)), "scale_state " + k
        assert np.array_equal(S2["q"].view(np.uint32), S1["q"].view(np.uint32)), "scale_state q"
