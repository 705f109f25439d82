"""The prediction stage on the GPU (flame_hip_predict / flame_hip_predict_map; kernels: flame_ros_amd/csrc/predict.hip) equals
its NumPy restatement tests/predict_ref.py BIT FOR BIT -- the predictions and the whole dense map, as uint32 views -- on the
cases of tests/predict_cases.py, which tests/test_predict_ref.py pins against ground truth and rule by rule.  The previous
frame is built with GraphRegularizer from explicit vertices, edges and triangles; tri_valid is what the triangle stage of the
handle made (read back and handed to the restatement)."""
import ctypes as C

import numpy as np
import pytest

from flame_ros_amd import lib
from flame_ros_amd.regularizer import GraphRegularizer, TriParams, default_params, default_sync_params
from tests import predict_cases as PC
from tests import predict_ref as R

pytestmark = pytest.mark.gpu

fx, fy, cx, cy = PC.K4
K = np.array([fx, 0, cx, 0, fy, cy, 0, 0, 1], np.float32)
KINV = np.array([1 / fx, 0, -cx / fx, 0, 1 / fy, -cy / fy, 0, 0, 1], np.float32)
U32 = np.uint32


def tri_params(c):
    """All filters off, or only the idepth filter where the case asks for an invalid triangle."""
    return TriParams(0, 1.57, 0.35, 0.1, 0, 0.333, int("min_idepth" in c), c.get("min_idepth", 0.0), c["W"], c["H"])


def edges_of(tris):
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [0, 2]]])
    return np.unique(np.sort(e, axis=1), axis=0).astype(np.int32)


def previous_frame(c, tri_stage=True):
    """The handle as the previous frame left it: the case's mesh, its idepths as the state, the triangle stage run once."""
    e = edges_of(c["tris"])
    ones = np.ones(len(e), np.float32)
    z = np.where(np.isfinite(c["x"]) & (c["x"] > 0), c["x"], np.float32(0.5)).astype(np.float32)
    r = GraphRegularizer(c["pos"], e, ones, ones, z, np.ones(len(z), np.float32), tris=c["tris"])
    r.set_state(x=c["x"])  # (takes what an upload refuses: zero, negative and NaN idepths)
    tv = r.triangles(KINV, tri_params(c))[1] if tri_stage else None
    return r, tv


def restated(c, tv):
    return R.predict(c["K4"], c["W"], c["H"], c["Tp"], c["Tc"], c["pos"], c["x"], c["tris"], tv, c["pix"])


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got.view(U32).ravel() != want.view(U32).ravel())
    assert bad.size == 0, (what, bad.size, bad[:5], got.ravel()[bad[:5]], want.ravel()[bad[:5]])


def check(c, expect_all_valid=True):
    r, tv = previous_frame(c)
    with r:
        if expect_all_valid:
            assert tv.all()
        pred = r.predict(c["W"], c["H"], K, c["Tp"], c["Tc"], c["pix"])
        dense = r.predicted_map(c["W"], c["H"])
        want_pred, want_map, key = restated(c, tv)
        same_bits(pred, want_pred, "prediction")
        same_bits(dense, want_map, "dense map")
        assert r.last_predicted == int(np.isfinite(want_pred).sum())
        assert r.info("predict_us") > 0 and r.info("predict_device_us") > 0
    return want_pred, key, tv


@pytest.mark.parametrize("name", ["forward", "refpose_nonidentity"])
def test_planes(gpu, name):
    for k in range(1, 6):
        c = PC.plane_case(name, k)
        pred, _, _ = check(c)
        assert np.isfinite(pred[c["must"]]).all()


@pytest.mark.parametrize("name", sorted(PC.RULE_CASES))
def test_rules(gpu, name):
    c = PC.RULE_CASES[name]()
    # (the triangle stage itself drops triangles with a zero, negative or NaN vertex; `behind` keeps all of them valid)
    _, key, tv = check(c, expect_all_valid=name not in ("zero", "negative", "nan", "hole"))
    if name == "hole":
        assert np.array_equal(tv, c["tri_valid"])
    if name in ("behind", "zero", "negative", "nan"):
        touching = set(np.flatnonzero((c["tris"] == c["poisoned"]).any(axis=1)).tolist())
        assert PC.winners(key) == set(range(len(c["tris"]))) - touching


def test_two_triangles_cover_the_image(gpu):
    """Boxes of 64 x 48 pixels: a whole wave per triangle."""
    c = PC.two_triangle_case()
    _, key, _ = check(c)
    assert (key != 0).all() and PC.winners(key) == {0, 1}


def test_dense_mesh(gpu):
    """~5 000 triangles of a few pixels on 160 x 120: 8 lanes per triangle, and the long triangles across the window without
    vertices -- boxes above 256 pixels -- by the whole wave afterwards."""
    c = PC.dense_plane_case()
    assert c["W"] * c["H"] // len(c["tris"]) < 64
    p = c["pos"][c["tris"]]
    box = np.prod(np.floor(p.max(axis=1)) - np.ceil(p.min(axis=1)) + 1, axis=1)
    assert (box > 256).any() and np.median(box) < 40  # (previous-view boxes; the warp of this case moves them by a few per cent)
    check(c)


def test_no_queries_makes_only_the_map(gpu):
    c = PC.plane_case("forward", 2)
    r, tv = previous_frame(c)
    with r:
        assert r.predict(c["W"], c["H"], K, c["Tp"], c["Tc"], np.zeros((0, 2), np.float32)).shape == (0,)
        same_bits(r.predicted_map(c["W"], c["H"]), restated(c, tv)[1], "dense map")


def test_call_order_and_arguments(gpu):
    c = PC.plane_case("forward", 2)
    r, _ = previous_frame(c, tri_stage=False)
    with r:
        with pytest.raises(lib.FlameHipError) as e:  # no triangle stage since the upload: tri_valid does not exist
            r.predict(c["W"], c["H"], K, c["Tp"], c["Tc"], c["pix"])
        assert e.value.code == lib.ERR_STATE
        L = lib.load()
        assert L.flame_hip_predict_map(r._h, np.zeros(4, np.float32).ctypes.data_as(C.c_void_p)) == lib.ERR_STATE
        r.triangles(KINV, tri_params(c))
        bad = c["Tc"].copy()
        bad[1, 3] = np.inf
        for args, code in (((c["W"], c["H"], K, c["Tp"], bad, c["pix"]), lib.ERR_NAN),
                           ((0, c["H"], K, c["Tp"], c["Tc"], c["pix"]), lib.ERR_ARG)):
            with pytest.raises(lib.FlameHipError) as e:
                r.predict(*args)
            assert e.value.code == code
        r.predict(c["W"], c["H"], K, c["Tp"], c["Tc"], c["pix"])
        # a new upload on the handle: the old tri_valid is not this graph's
        e2 = edges_of(c["tris"])
        ones = np.ones(len(e2), np.float32)
        r.reupload(c["pos"], e2, ones, ones, c["x"], np.ones(len(c["x"]), np.float32), tris=c["tris"])
        with pytest.raises(lib.FlameHipError) as e:
            r.predict(c["W"], c["H"], K, c["Tp"], c["Tc"], c["pix"])
        assert e.value.code == lib.ERR_STATE


def test_prediction_is_in_the_callers_units_after_rescale_data(gpu):
    """A frame as the facade runs it: graph sync under rescale_data, a short solve, flame_hip_frame_results un-scaling the
    state -- the prediction is made from idepths in the caller's units."""
    c = PC.plane_case("refpose_nonidentity", 3)
    tp = tri_params(c)
    with GraphRegularizer.empty() as r:
        scale = r.sync_features(c["pos"], c["x"], np.full(len(c["x"]), 1e-4, np.float32), c["tris"],
                                default_sync_params(rescale_data=True))
        assert abs(scale - float(c["x"].mean())) < 1e-3 * scale and not 0.8 < scale < 1.25
        p = default_params()
        r.step(p, 20)
        _, _, x, _, tv, _ = r.frame_results(p, KINV, tp, scale_back=scale)
        same_bits(r.download()[0], x, "resident state, un-scaled")
        pred = r.predict(c["W"], c["H"], K, c["Tp"], c["Tc"], c["pix"])
        want_pred, want_map, _ = restated(dict(c, x=x), tv)
        same_bits(pred, want_pred, "prediction")
        same_bits(r.predicted_map(c["W"], c["H"]), want_map, "dense map")
        m = c["must"]
        assert np.isfinite(pred[m]).all() and np.median(np.abs(pred[m] / c["truth"][m] - 1.0)) < 0.1  # (units off would be 3 x)


def test_repeatable_and_reads_only(gpu):
    c = PC.plane_case("forward", 4)
    r, _ = previous_frame(c)
    with r:
        before = r.download() + r.download_bar()
        tv0 = r.triangles(KINV, tri_params(c))[1]
        a, ma = r.predict(c["W"], c["H"], K, c["Tp"], c["Tc"], c["pix"]), r.predicted_map(c["W"], c["H"])
        b, mb = r.predict(c["W"], c["H"], K, c["Tp"], c["Tc"], c["pix"]), r.predicted_map(c["W"], c["H"])
        same_bits(a, b, "prediction, second call")
        same_bits(ma, mb, "dense map, second call")
        after = r.download() + r.download_bar()
        for x0, x1 in zip(before, after):
            same_bits(x0, x1, "state")
        assert np.array_equal(tv0, r.triangles(KINV, tri_params(c))[1])
