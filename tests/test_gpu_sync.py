"""-m gpu: row a7 end to end on the device: graph sync -> solve -> (un-scale) -> triangle stage,
against the oracle's statements of each (bit-exact), for every combination of the sync switches
(reference cfg/flame_offline_tum.yaml:89-92)."""
import numpy as np
import pytest

from flame_ros_amd.regularizer import GraphRegularizer, default_params, default_sync_params, default_tri_params
from oracle import COracle
from oracle.cbind import SyncParams as OSync, graph_sync as oracle_sync, triangles as oracle_triangles, TriParams as OTri
from tests.test_graph_sync import features
from tests.util import assert_bit_equal, graphgen, hooks_env, oracle_params, settle_lease, with_hooks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("adaptive,rescale,init_pred,rule", [pytest.param(0, 0, 1, 0, id="0-0-1"), pytest.param(1, 0, 1, 0, id="1-0-1"),
                                                             pytest.param(0, 1, 0, 0, id="0-1-0"), pytest.param(1, 1, 1, 0, id="1-1-1"),
                                                             pytest.param(1, 1, 1, 3, id="1-1-1-rule3")])
def test_sync_solve_unscale_triangles(gpu, adaptive, rescale, init_pred, rule):
    """(rule 3, gains 1.5 / 0.25: alpha = 1.5, beta = 0.25 / len -- the host sync, beta independent of alpha)"""
    ag, bg = (1.5, 0.25) if rule else (0.0, 0.0)
    K = np.array([[525.0, 0, 319.5], [0, 525.0, 239.5], [0, 0, 1]])
    Kinv = np.linalg.inv(K).astype(np.float32)
    tp = default_tri_params(640, 480)
    otp = OTri(*[getattr(tp, f[0]) for f in tp._fields_])
    r = GraphRegularizer.empty(device=0)
    for frame, V in enumerate((6000, 2500)):  # two frames of a stream on one handle
        g, var, pred = features(V, 20 + frame)
        # adaptive weights 1/var reach 1e5: keep the data step tau*lambda*w inside the clamp range
        if adaptive:
            var = np.maximum(var, np.float32(2e-3))
        sp = default_sync_params(adaptive, rescale, init_pred, 0.01, rule, ag, bg)
        s = oracle_sync(OSync(adaptive, rescale, init_pred, 0.01, rule, ag, bg), g.pos, g.z, var, g.tris, pred)
        o = COracle(g.pos, s["edges"], s["alpha"], s["beta"], s["z"], s["wgt"], x0=s["x0"])
        scale = r.sync_features(g.pos, g.z, var, g.tris, sp, prediction=pred)
        assert np.float32(scale) == np.float32(s["scale"])
        if rule == 0:
            assert r.info("plan_on_device") == 1  # sync + plan both ran on the GPU
        assert np.array_equal(r.edges(), s["edges"])
        o.solve(oracle_params(), 150)
        r.step(default_params(), 150)
        so, do = o.costs(oracle_params())
        sg, dg = r.costs(default_params())
        assert abs(sg - so) <= 1e-9 * so and abs(dg - do) <= 1e-9 * max(do, 1e-30)
        o.scale_state(scale)
        r.scale_state(scale)
        x, w1, w2, q = r.download()
        xb, _, _ = r.download_bar()
        assert_bit_equal(x, o.x, "x")
        assert_bit_equal(w1, o.w1, "w1")
        assert_bit_equal(w2, o.w2, "w2")
        assert_bit_equal(xb, o.xb, "xb")
        assert_bit_equal(q, o.q, "q")
        if rescale:  # back in the caller's units: close to the measured idepths again
            assert abs(float(np.mean(x)) - float(np.mean(g.z))) < 0.02
        tn_o, tv_o, vn_o = oracle_triangles(otp, Kinv, g.pos, o.x, g.tris)
        tn, tv, vn = r.triangles(Kinv, tp)
        assert np.array_equal(tv, tv_o)
        assert_bit_equal(vn, vn_o, "vertex normals")
    r.close()


@pytest.mark.parametrize("rescale", [0, 1])
def test_frame_results_one_call(gpu, rescale):
    """flame_hip_frame_results (what flame::Flame::update reads back, one synchronisation) against
    the oracle: costs in the solver's units, then idepths / normals / validity in the caller's."""
    K = np.array([[525.0, 0, 319.5], [0, 525.0, 239.5], [0, 0, 1]])
    Kinv = np.linalg.inv(K).astype(np.float32)
    tp = default_tri_params(640, 480)
    otp = OTri(*[getattr(tp, f[0]) for f in tp._fields_])
    for V in (5000, 900):  # device-built plan / one isolated tile (host sync + host plan)
        g, var, pred = features(V, 50 + V)
        sp = default_sync_params(0, rescale, 1, 0.01)
        s = oracle_sync(OSync(0, rescale, 1, 0.01), g.pos, g.z, var, g.tris, pred)
        o = COracle(g.pos, s["edges"], s["alpha"], s["beta"], s["z"], s["wgt"], x0=s["x0"])
        o.solve(oracle_params(), 80)
        so, do = o.costs(oracle_params())
        o.scale_state(s["scale"])
        tn_o, tv_o, vn_o = oracle_triangles(otp, Kinv, g.pos, o.x, g.tris)
        r = GraphRegularizer.empty(device=0, tile_single_max=2048)
        scale = r.sync_features(g.pos, g.z, var, g.tris, sp, prediction=pred)
        r.step(default_params(), 80, sync=False)  # frame_results orders itself behind the solve
        sg, dg, x, vn, tv, e = r.frame_results(default_params(), Kinv, tp, scale_back=scale, with_edges=True)
        assert abs(sg - so) <= 1e-9 * so and abs(dg - do) <= 1e-9 * max(do, 1e-30)
        assert_bit_equal(x, o.x, "x")
        assert_bit_equal(vn, vn_o, "vertex normals")
        assert np.array_equal(tv, tv_o) and np.array_equal(e, s["edges"])
        r.close()


def test_device_sync_flags_non_finite_derived_values(gpu):
    """The non-finite-input check rides in the kernels that derive the values (r03): a zero variance
    under adaptive weights (wgt = 1/var = inf) and two features on one pixel (alpha = 1/0 = inf) must
    still come back as FLAME_HIP_ERR_NAN from the device path, and the handle stays usable."""
    from flame_ros_amd import lib
    from flame_ros_amd.regularizer import FlameHipError
    g = graphgen.synthetic(6000, seed=21)
    var = np.full(g.V, 1e-4, np.float32)
    r = GraphRegularizer.empty(device=0)
    bad = var.copy(); bad[17] = 0.0
    with pytest.raises(FlameHipError) as e:
        r.sync_features(g.pos, g.z, bad, g.tris, default_sync_params(adaptive_data_weights=True))
    assert e.value.code == lib.ERR_NAN
    pos = g.pos.copy(); pos[g.tris[5, 1]] = pos[g.tris[5, 0]]   # an edge of length zero
    with pytest.raises(FlameHipError) as e:
        r.sync_features(pos, g.z, var, g.tris, default_sync_params())
    assert e.value.code == lib.ERR_NAN
    r.sync_features(g.pos, g.z, var, g.tris, default_sync_params())  # a good frame afterwards
    assert r.info("plan_on_device") == 1 and r.E == g.E
    r.close()


def test_edge_count_is_predicted_and_verified(gpu):
    """The device graph sync does not wait for the edge count: E = V + T + (offset of the previous
    frame, -1 for a triangulated disk = Euler) is assumed and checked at the plan builder's first
    synchronisation; a wrong guess (a mesh with holes after a Delaunay frame and vice versa) costs a
    second build and must give the same result: edges, alpha and the solve equal the oracle's."""
    r = GraphRegularizer.empty(device=0)
    rng = np.random.default_rng(4)
    kinds = ["disk", "disk", "holes", "holes", "holes", "disk", "disk", "two_parts"]
    for k, kind in enumerate(kinds):
        g = graphgen.synthetic(6000 + 50 * k, seed=90 + k)
        tris = g.tris
        if kind == "holes":      # drop a fifth of the triangles: holes and notches, E != V + T - 1
            tris = tris[rng.random(len(tris)) > 0.2]
        elif kind == "two_parts":  # keep only triangles left of x = 300 and right of x = 340: two components
            cx = g.pos[tris].mean(1)[:, 0]
            tris = tris[(cx < 300) | (cx > 340)]
        var = np.full(g.V, 1e-4, np.float32)
        s = oracle_sync(OSync(0, 0, 1, 0.01), g.pos, g.z, var, tris, None)
        E = len(s["edges"])
        if kind == "disk":
            assert E == g.V + len(tris) - 1
        else:
            assert E != g.V + len(tris) - 1
        r.sync_features(g.pos, g.z, var, tris, default_sync_params())
        assert r.info("plan_on_device") == 1 and r.E == E, (kind, r.E, E)
        assert np.array_equal(r.edges(), s["edges"])
        o = COracle(g.pos, s["edges"], s["alpha"], s["beta"], s["z"], s["wgt"], x0=s["x0"])
        o.solve(oracle_params(), 20)
        r.step(default_params(), 20)
        x, w1, w2, q = r.download()
        assert_bit_equal(x, o.x, "frame %d (%s) x" % (k, kind))
        assert_bit_equal(q, o.q, "frame %d (%s) q" % (k, kind))
    r.close()


def test_mispredicted_edge_count_on_a_growing_small_frame(gpu):
    """small frames planned by ONE launch (k_mini_plan) that find their predicted edge count wrong leave
    early -- the stages behind the launch must then run on a valid (empty) plan, not on the previous frame's tables or,
    when the frame is larger than any before it on the handle, on arrays that were never written.  Frames grow from
    1.0 k to 1.9 k vertices and alternate between disks and meshes with holes, so every other prediction fails on
    arrays that have just been re-allocated; the hooks library's fill_alloc fills new allocations with 0xff (out-of-range
    indices wherever something reads what it should not).  Every frame: the oracle's edges and bits."""
    import os, subprocess, sys
    code = r'''
import numpy as np, sys
sys.path.insert(0, %r)
from flame_ros_amd import graphgen
from flame_ros_amd.regularizer import GraphRegularizer, default_params, default_sync_params
from oracle import COracle
from oracle.cbind import default_params as oparams, SyncParams as OSync, graph_sync as oracle_sync
r = GraphRegularizer.empty(device=0, tile_single_max=640, stream_depth=5)
rng = np.random.default_rng(7)
mini = wrong = 0
for k in range(14):
    g = graphgen.synthetic(1000 + 70 * k, seed=400 + k)
    tris = g.tris
    if k %% 2 == 1 and k > 2:  # holes: E != V + T - 1, the prediction carried over from the disk before fails
        tris = tris[rng.random(len(tris)) > 0.15]
    var = np.full(g.V, 1e-4, np.float32)
    s = oracle_sync(OSync(0, 0, 1, 0.01), g.pos, g.z, var, tris, None)
    r.sync_features(g.pos, g.z, var, tris, default_sync_params())
    mini += r.info("plan_mini")
    assert r.E == len(s["edges"]) and np.array_equal(r.edges(), s["edges"]), k
    o = COracle(g.pos, s["edges"], s["alpha"], s["beta"], s["z"], s["wgt"], x0=s["x0"]); o.solve(oparams(), 30)
    r.step(default_params(), 30)
    x, w1, w2, q = r.download()
    assert np.array_equal(x.view(np.uint32), o.x.view(np.uint32)) and np.array_equal(q.view(np.uint32), o.q.view(np.uint32)), k
r.close()
print("frames ok, planned by one launch:", mini)
''' % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", with_hooks(code, fill_alloc=255)], env=hooks_env(), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0 and "frames ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_large_frames_take_the_unfused_chains(gpu):
    """Two frames of 120 k vertices through the graph sync: beyond 114 k vertices the edge derivation is the
    unfused rows / mark / scan / compact chain, and 512 tiles exceed the fused tile pass's look-back grid
    (plain pass 1 / offsets / pass 2) -- the same edges and the oracle's bits all the same.  (persist = 0: a handle that solves
    by resident tiles gets 256 FAT tiles at this size since r05 -- the second handle below, same frames, same bits.)"""
    sp, p = default_sync_params(), default_params()
    settle_lease()  # (the assertions below are about a free lease: resident sizing, persist_used)
    for k in range(2):
        g = graphgen.synthetic(120000, 1280, 1024, seed=90 + k)
        var = np.full(g.V, 1e-4, np.float32)
        with GraphRegularizer.empty(device=0) as rf:
            rf.sync_features(g.pos, g.z, var, g.tris, sp)
            assert rf.info("plan_on_device") == 1 and rf.info("num_tiles") == 256
            assert np.array_equal(rf.edges(), g.edges)
            o = COracle(g.pos, g.edges, g.alpha, g.beta, g.z, g.wgt)
            o.solve(oracle_params(), 9)
            rf.step(p, 9)
            assert rf.info("persist_used") == 1
            assert_bit_equal(rf.download()[0], o.x, "fat frame %d x" % k)
    r = GraphRegularizer.empty(device=0, persist=0)
    for k in range(2):
        g = graphgen.synthetic(120000, 1280, 1024, seed=90 + k)
        var = np.full(g.V, 1e-4, np.float32)
        r.sync_features(g.pos, g.z, var, g.tris, sp)
        assert r.info("plan_on_device") == 1 and r.info("num_tiles") > 448
        assert np.array_equal(r.edges(), g.edges)
        o = COracle(g.pos, g.edges, g.alpha, g.beta, g.z, g.wgt)
        o.solve(oracle_params(), 6)
        r.step(p, 6)
        x, w1, w2, q = r.download()
        assert_bit_equal(x, o.x, "frame %d x" % k)
        assert_bit_equal(q, o.q, "frame %d q" % k)
    r.close()
