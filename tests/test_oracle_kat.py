"""CPU: pins the oracle (oracle/nltgv2_oracle.c).  The reference holds no tests or golden vectors
for this path and the solver source is absent (PARITY UNPINNED), so the oracle is
pinned by the analytic known-answer tests K1-K9 of SURVEY.md 8c, an independent float64 NumPy
restatement, and the frozen fixtures in tests/golden/ (made by tests/golden/make_golden.py)."""
import copy
import os

import numpy as np
import pytest

from oracle import COracle
from oracle.cbind import default_params, triangles, TriParams
from oracle.nltgv2_np import NpSolver
from tests.util import assert_bit_equal, graphgen, random_state

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def g5k():
    return graphgen.synthetic(5000, seed=0)


def orc(g, **kw):
    return COracle(g.pos, g.edges, g.alpha, g.beta, g.z, g.wgt, **kw)


def test_golden_graph_is_reproducible(g5k):
    """The committed 5k fixture equals what the generator makes today (config 2: E = 14 978)."""
    d = np.load(os.path.join(GOLD, "g5k.npz"))
    assert g5k.E == 14978 and g5k.V == 5000
    assert np.array_equal(d["edges"], g5k.edges) and np.array_equal(d["pos"], g5k.pos)
    assert_bit_equal(d["z"], g5k.z, "z")
    assert_bit_equal(d["alpha"], g5k.alpha, "alpha")


def test_golden_5k_states():
    d = np.load(os.path.join(GOLD, "g5k.npz"))
    o = COracle(d["pos"], d["edges"], d["alpha"], d["beta"], d["z"], d["wgt"])
    p = default_params()
    done = 0
    for n in (1, 10, 200):
        o.solve(p, n - done)
        done = n
        assert_bit_equal(o.x, d["x_after_%d" % n], "x after %d" % n)
    assert_bit_equal(o.w1, d["w1_after_200"], "w1")
    assert_bit_equal(o.q, d["q_after_200"], "q")
    assert np.allclose(o.costs(p), d["costs_after_200"], rtol=1e-12)


def test_golden_12_vertex():
    d = np.load(os.path.join(GOLD, "g12.npz"))
    o = COracle(d["pos"], d["edges"], d["alpha"], d["beta"], d["z"], d["wgt"])
    o.solve(default_params(), 1)
    assert_bit_equal(o.x, d["x_after_1"], "x1")
    o.solve(default_params(), 4)
    assert_bit_equal(o.x, d["x_after_5"], "x5")
    assert_bit_equal(o.q, d["q_after_5"], "q5")


def test_K1_adjointness(g5k):
    """<K u, q> == <u, K^T q>: pins the primal scatter against the dual gather."""
    o = orc(g5k)
    rng = np.random.default_rng(1)
    x, w1, w2 = rng.normal(size=(3, g5k.V))
    q = rng.normal(size=(g5k.E, 3))
    Ku = o.apply_K(x, w1, w2).astype(np.float64)
    kx, k1, k2 = (a.astype(np.float64) for a in o.apply_KT(q))
    lhs = float((Ku * q).sum())
    rhs = float((kx * x).sum() + (k1 * w1).sum() + (k2 * w2).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs), 1.0)


def planar(g, a=1e-3, b=-5e-4, c=0.5):
    return (a * g.pos[:, 0].astype(np.float64) + b * g.pos[:, 1] + c).astype(np.float32)


@pytest.fixture(scope="module")
def ggrid():
    """Feature-grid graph (one feature per 8x8 cell, like FLaME's detector): edge lengths are
    bounded below, so alpha = 1/len stays < 1 and the YAML step sizes are in their stable range.
    (On i.i.d. random points a few edges are far shorter than a pixel, alpha reaches ~7 and
    tau*sigma*|K|^2 >> 1 there: rounding noise is then amplified in float64 just the same.)"""
    return graphgen.dataset_shaped(640, 480, 8)


def test_K2_planar_fixed_point(ggrid):
    """z planar, x = z, w = plane slopes, q = 0 is a fixed point with zero cost (to rounding)."""
    g = ggrid
    a, b = 1e-3, -5e-4
    z = planar(g, a, b)
    o = COracle(g.pos, g.edges, g.alpha, g.beta, z, g.wgt)
    w1 = np.full(g.V, a, np.float32)
    w2 = np.full(g.V, b, np.float32)
    o.set_state(w1=w1, w2=w2, w1b=w1, w2b=w2)
    p = default_params()
    o.solve(p, 50)
    assert np.abs(o.x - z).max() < 1e-6 and np.abs(o.w1 - a).max() < 1e-6
    s, d = o.costs(p)
    assert s < 1e-3 and d < 1e-6  # float32 rounding of the plane only


def test_K3_planar_recovery(ggrid):
    """Same planar data, w = 0 start: the smoothness cost collapses and w -> (a, b)."""
    g5k = ggrid
    a, b = 1e-3, -5e-4
    z = planar(g5k, a, b)
    o = COracle(g5k.pos, g5k.edges, g5k.alpha, g5k.beta, z, g5k.wgt)
    p = default_params()
    s0, _ = o.costs(p)
    o.solve(p, 3000)
    s1, _ = o.costs(p)
    assert s1 < 0.05 * s0
    assert abs(np.median(o.w1) - a) < 1e-4 and abs(np.median(o.w2) - b) < 1e-4


def test_K4_two_vertex_closed_form():
    d = np.load(os.path.join(GOLD, "two_vertex.npz"))
    o = COracle(d["pos"], [[0, 1]], [float(d["alpha"])], [float(d["beta"])], d["z"], [1.0, 1.0])
    o.solve(default_params(), 1)
    assert abs(o.q[0, 0] - d["q1"]) <= 1e-7
    assert np.abs(o.x - d["x"]).max() <= 1.2e-7  # 1 ulp at 0.8
    assert abs(o.w1[0] - d["w1_0"]) <= 1e-9 and o.w1[1] == 0.0
    assert np.abs(o.xb - d["xb"]).max() <= 2.4e-7


def test_K5_invariants(g5k):
    o = orc(g5k)
    p = default_params()
    st = random_state(g5k, 5)
    st["x"] = np.clip(st["x"], 0.02, 9.0)  # start inside the clamp so only tau-sized moves occur
    o.set_state(**st)
    bound = p.step_x * p.data_factor + p.step_x * np.bincount(
        g5k.edges.ravel(), weights=np.repeat(g5k.alpha, 2), minlength=g5k.V)
    for _ in range(20):
        prev = o.x.copy()
        o.solve(p, 1)
        assert np.abs(o.q).max() <= 1.0
        assert o.x.min() >= p.x_min and o.x.max() <= p.x_max
        assert np.all(np.abs(o.x - prev) <= bound + 1e-6)  # 1e-6: float32 rounding at x ~ 1


def test_K6_relabel_invariance(g5k, ggrid):
    """Permuting vertex labels and edge order changes the result by float32 summation order only:
    < 1e-6 RMS on the feature-grid graph; on i.i.d. points the over-stepped short edges amplify
    that noise to a few 1e-5 (still inside the 1e-4 north_star tolerance) -- which is why the HIP
    path reproduces the oracle's summation order exactly instead of relying on a tolerance."""
    for g, tol in ((ggrid, 1e-6), (g5k, 1e-4)):
        rng = np.random.default_rng(6)
        pv, pe = rng.permutation(g.V), rng.permutation(g.E)
        inv = np.empty_like(pv)
        inv[pv] = np.arange(g.V)
        o1 = orc(g)
        o2 = COracle(g.pos[pv], inv[g.edges[pe]], g.alpha[pe], g.beta[pe], g.z[pv], g.wgt[pv])
        p = default_params()
        o1.solve(p, 100)
        o2.solve(p, 100)
        assert np.sqrt(np.mean((o1.x[pv] - o2.x) ** 2)) < tol


def test_K7_orientation_is_honoured(g5k):
    """K1 uses the SOURCE vertex's slopes: flipping an edge changes the iteration."""
    st = random_state(g5k, 7)
    o1, o2 = orc(g5k), COracle(g5k.pos, g5k.edges[:, ::-1].copy(), g5k.alpha, g5k.beta, g5k.z, g5k.wgt)
    for o in (o1, o2):
        o.set_state(**{k: v for k, v in st.items() if k != "q"})
        o.solve(default_params(), 20)
    assert np.abs(o1.x - o2.x).max() > 1e-5


def test_K8_energy_decreases(g5k):
    o = orc(g5k)
    p = default_params()
    e0 = sum(o.costs(p))
    o.solve(p, 200)
    e1 = sum(o.costs(p))
    o.solve(p, 1800)
    e2 = sum(o.costs(p))
    assert e2 < e1 < 0.5 * e0  # survey probe: 109.4 -> 41.6 -> 22.8
    assert abs(o.x.mean() - g5k.z.mean()) < 2e-3


def test_K9_float64_numpy_restatement(g5k, ggrid):
    """The 5k graph from rest (beta = alpha, wgt = 1), and the feature-grid graph with beta = alpha x U(0.5, 2) and
    non-uniform data weights (zeros among them): a beta read as alpha, or a prox without its weight, shows here."""
    rng = np.random.default_rng(9)
    dec = copy.copy(ggrid)
    dec.beta = (ggrid.alpha * rng.uniform(0.5, 2.0, ggrid.E)).astype(np.float32)
    dec.wgt = rng.uniform(0.25, 4.0, ggrid.V).astype(np.float32)
    dec.wgt[::17] = 0.0
    for g in (g5k, dec):
        o = orc(g)
        s = NpSolver(g.pos, g.edges, g.alpha, g.beta, g.z, g.wgt)
        o.solve(default_params(), 200)
        s.solve(200)
        assert np.sqrt(np.mean((s.x - o.x) ** 2)) <= 1e-5
        sc, dc = o.costs(default_params())
        sn, dn = s.costs()
        assert abs(sc - sn) < 1e-3 * sn and abs(dc - dn) < 1e-3 * dn


def test_projection_equals_clamp():
    """v / max(1,|v|) == clamp(v,-1,1) bit-for-bit (what lets the GPU use one v_med3_f32)."""
    rng = np.random.default_rng(9)
    v = np.concatenate([rng.normal(0, 2, 100000), rng.normal(0, 1e-30, 1000),
                        [0.0, -0.0, 1.0, -1.0, np.nextafter(1, 2), 1e30, -1e30]]).astype(np.float32)
    div = (v / np.maximum(np.float32(1), np.abs(v))).astype(np.float32)
    assert_bit_equal(np.clip(v, np.float32(-1), np.float32(1)), div, "projection")


def test_step_is_dual_primal_extragradient(g5k):
    o1, o2 = orc(g5k), orc(g5k)
    st = random_state(g5k, 10)
    p = default_params()
    for o in (o1, o2):
        o.set_state(**st)
    o1.solve(p, 1)
    o2.dual_step(p)
    prev = o2.primal_step(p)
    o2.extragradient_step(p, *prev)
    assert_bit_equal(o1.x, o2.x, "x")
    assert_bit_equal(o1.xb, o2.xb, "xb")
    assert_bit_equal(o1.q, o2.q, "q")


def test_threaded_variant_is_bit_identical(g5k):
    """The OpenMP baseline variant (edge-parallel dual + CSR primal) equals the sequential step."""
    o1, o2 = orc(g5k), orc(g5k)
    st = random_state(g5k, 11)
    for o in (o1, o2):
        o.set_state(**st)
    o1.solve(default_params(), 25)
    o2.solve_threads(default_params(), 25, 3)
    for a in ("x", "w1", "w2", "xb", "w1b", "w2b", "q"):
        assert_bit_equal(getattr(o2, a), getattr(o1, a), a)


def test_graph_filters_known_answers():
    """Row a9 on a 4-vertex path 0-1-2-3 with values (1, 5, 2, 9)."""
    o = COracle([[0, 0], [1, 0], [2, 0], [3, 0]], [[0, 1], [1, 2], [2, 3]], [1, 1, 1], [1, 1, 1],
                [1.0, 5.0, 2.0, 9.0], [1, 1, 1, 1])
    o.graph_filter(0)  # lower medians of {1,5} {5,1,2} {2,5,9} {9,2}
    assert o.x.tolist() == [1.0, 2.0, 5.0, 2.0] and o.xb.tolist() == o.x.tolist()
    o.set_state(x=[1.0, 5.0, 2.0, 9.0])
    o.graph_filter(1)  # plain averages
    assert np.allclose(o.x, [3.0, 8.0 / 3.0, 16.0 / 3.0, 5.5], rtol=1e-6)


def test_edge_cases():
    p = default_params()
    o = COracle(np.zeros((0, 2)), np.zeros((0, 2), np.int32), [], [], [], [])
    o.solve(p, 3)
    o = COracle([[0.0, 0.0]], np.zeros((0, 2), np.int32), [], [], [0.7], [1.0])
    o.solve(p, 3)
    assert o.x[0] == np.float32(0.7)
    # clamp: data far above x_max
    o = COracle([[0.0, 0.0], [10.0, 0.0]], [[0, 1]], [0.1], [0.1], [50.0, 50.0], [1.0, 1.0])
    o.solve(p, 2)
    assert np.all(o.x == np.float32(p.x_max))


def test_triangle_stage_known_answers():
    """Fronto-parallel plane: normals (0,0,-1), all valid; one far vertex: idepth filter trips;
    a depth step: oblique filter trips; an over-long edge: length filter trips."""
    K = np.array([[525.0, 0, 319.5], [0, 525.0, 239.5], [0, 0, 1]])
    Kinv = np.linalg.inv(K).astype(np.float32)
    pos = np.array([[100, 100], [140, 100], [100, 140], [140, 140], [500, 100]], np.float32)
    tris = np.array([[0, 1, 2], [1, 3, 2], [1, 4, 3]], np.int32)
    tp = TriParams(1, 1.2, 0.35, 0.1, 1, 0.333, 1, 0.01, 640, 480)
    x = np.full(5, 0.5, np.float32)
    tn, tv, vn = triangles(tp, Kinv, pos, x, tris)
    assert np.allclose(tn, [0, 0, -1], atol=1e-6) and np.allclose(vn, [0, 0, -1], atol=1e-6)
    assert tv.tolist() == [1, 1, 0]  # third triangle has a 360 px edge > 0.333 * 640
    x2 = x.copy(); x2[3] = 0.005
    assert triangles(tp, Kinv, pos, x2, tris)[1].tolist() == [1, 0, 0]
    x3 = x.copy(); x3[0] = 1.0  # idepth jump 0.5 -> 1.0: relative and absolute difference trip
    tn3, tv3, _ = triangles(tp, Kinv, pos, x3, tris)
    Pa = Kinv.astype(np.float64) @ np.array([pos[0, 0], pos[0, 1], 1.0]) / x3[0]
    assert tv3[0] == 0 and tv3[1] == 1 and abs(np.linalg.norm(tn3[0]) - 1) < 1e-6
    assert float(tn3[0].astype(np.float64) @ Pa) <= 0  # faces the camera
    x4 = x.copy(); x4[1] = np.nan
    tn4, tv4, vn4 = triangles(tp, Kinv, pos, x4, tris)
    assert tv4.tolist() == [0, 0, 0] and np.all(tn4 == 0) and np.all(np.isfinite(vn4))


def test_oracle_is_clean_under_asan_ubsan(tmp_path):
    """The oracle compiled with -fsanitize=address,undefined,float-cast-overflow runs every entry point on a small
    graph without a report (sanitizer build of the CPU checker) -- nltgv2_coverage and the four
    nltgv2_debug_image kinds included, with feature positions NaN, +-inf, +-3e9 and sides out of reach, which used to
    be converted to int unchecked."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "oracle_sanitize")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow",
                           "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-fopenmp", os.path.join(root, "tests", "cpp", "oracle_sanitize.c"),
                           os.path.join(root, "oracle", "nltgv2_oracle.c"), "-lm", "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", OMP_NUM_THREADS="2")
    p = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr[-3000:])
    assert p.stdout.startswith("E=") and " far=0" in p.stdout
