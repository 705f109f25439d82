"""Pins tests/predict_ref.py, the NumPy restatement of the prediction stage: against float64 ground truth on
the plane scenes of tests/frontend_scenes.py, and rule by rule on hand-built meshes.  No GPU; the GPU equals the restatement
bit for bit in tests/test_gpu_predict.py.  The last test is the ABI surface of the stage."""
import ctypes as C

import numpy as np
import pytest

from flame_ros_amd import graphgen, lib
from flame_ros_amd.regularizer import GraphRegularizer
from tests import frontend_scenes as S
from tests import predict_cases as PC
from tests import predict_ref as R

# Relative error of a prediction against the plane's float64 inverse depth at the query.  Measured worst value of the
# restatement over the 30 plane cases below (6 scenes x pose 0 -> 1 .. 5, 300 queries each): 2.2468e-7 (backward_side, k = 1).
# The bound is 4 x that, the margin DESIGN.md 5.3's constants use: rounding on other inputs of the same kind.
WORST_MEASURED = 2.2468e-7
REL_BOUND = 4 * WORST_MEASURED


def run(c):
    return R.predict(c["K4"], c["W"], c["H"], c["Tp"], c["Tc"], c["pos"], c["x"], c["tris"], c["tri_valid"], c["pix"])


@pytest.mark.parametrize("name", S.NAMES)
def test_planes_against_ground_truth(name):
    for k in range(1, 6):
        c = PC.plane_case(name, k)
        pred, dense, _ = run(c)
        must = c["must"]
        assert must.sum() >= 150, (k, int(must.sum()))  # (the cases are not vacuous)
        # a query at least 2 px inside the warped hull and inside the image gets a prediction: a condition, not a share
        assert np.isfinite(pred[must]).all(), (k, np.flatnonzero(must & ~np.isfinite(pred)))
        rel = np.abs(pred[must].astype(np.float64) - c["truth"][must]) / c["truth"][must]
        print("%s k=%d: %d queries, worst relative error %.4e (bound %.4e)" % (name, k, int(must.sum()), rel.max(), REL_BOUND))
        assert rel.max() < REL_BOUND, (k, rel.max())
        assert np.isfinite(dense).sum() > 0.5 * dense.size


def test_identity_reproduces_the_vertices_and_odd_queries_are_nan():
    c = PC.identity_case()
    pred, _, _ = run(c)
    ni = len(c["interior"])
    want = c["x"][c["interior"]].astype(np.float64)
    assert np.isfinite(pred[:ni]).all()
    assert (np.abs(pred[:ni] - want) / want).max() < REL_BOUND
    # outside the image on every side, a huge and a NaN pixel, an empty pixel: the canonical NaN
    assert (pred[ni:].view(np.uint32) == np.float32(np.nan).view(np.uint32)).all() and len(pred) == ni + c["n_odd"]


def test_the_nearer_surface_wins():
    c = PC.occlusion_case()
    pred, dense, key = run(c)
    # float64: the far patch lands on x 5.8 .. 25.8, the near one on 20 .. 36 (y 10 .. 30 / 10 .. 26); inside both by a pixel
    overlap = dense[12:25, 22:25]
    assert np.isfinite(overlap).all() and (np.abs(overlap - 1.0) < REL_BOUND).all(), overlap
    own = 0xFFFFFFFF - (key[12:25, 22:25] & np.uint64(0xFFFFFFFF))
    assert (own >= c["n_far_tris"]).all()                      # ... owned by triangles of the near patch
    assert (np.abs(dense[12:29, 8:19] - 0.3) < 0.3 * REL_BOUND).all()  # the far patch where nothing hides it
    assert (np.abs(pred.reshape(c["H"], c["W"])[12:25, 22:25] - 1.0) < REL_BOUND).all()


def test_a_flipped_triangle_contributes_nothing():
    c = PC.flip_case()
    pred, dense, key = run(c)
    assert (key == 0).all() and np.isnan(dense).all() and np.isnan(pred).all()
    still = dict(c, Tc=c["Tp"])  # the same triangle without the motion is drawn
    assert (run(still)[2] != 0).sum() > 20


@pytest.mark.parametrize("kind", ["behind", "zero", "negative", "nan"])
def test_a_bad_vertex_removes_exactly_its_triangles(kind):
    c = PC.poisoned_case(kind)
    _, _, key = run(c)
    touching = set(np.flatnonzero((c["tris"] == c["poisoned"]).any(axis=1)).tolist())
    assert 0 < len(touching) < len(c["tris"])
    assert PC.winners(key) == set(range(len(c["tris"]))) - touching


def test_an_invalid_triangle_is_a_hole():
    c = PC.hole_case()
    _, dense, key = run(c)
    invalid = set(np.flatnonzero(c["tri_valid"] == 0).tolist())
    assert len(invalid) == 2 and PC.winners(key) == set(range(len(c["tris"]))) - invalid
    everything = dict(c, tri_valid=np.ones_like(c["tri_valid"]))
    assert np.isfinite(run(everything)[1]).sum() > np.isfinite(dense).sum()


def test_a_shared_edge_through_pixel_centres_leaves_no_gap():
    c = PC.shared_edge_case()
    _, dense, key = run(c)
    assert np.isfinite(dense[5:24, 5:24]).all()  # every centre strictly inside the square, the diagonal's included
    diag = key[np.arange(5, 24), np.arange(5, 24)]
    assert (diag != 0).all()
    assert PC.winners(key) == {0, 1}


def test_abi_surface():
    """The library exports the stage, and without a device it says so: there is no CPU path."""
    L = lib.load()
    assert hasattr(L, "flame_hip_predict") and hasattr(L, "flame_hip_predict_map")
    assert L.flame_hip_version() >= 404
    g = graphgen.synthetic(300, seed=1)
    r = GraphRegularizer(g.pos, g.edges, g.alpha, g.beta, g.z, g.wgt, tris=g.tris, device=-1)
    K = np.array(S.K, np.float32)
    T = np.ascontiguousarray(PC.IDENT.reshape(12))
    pix = np.zeros((4, 2), np.float32)
    out = np.zeros(4, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.flame_hip_predict(r._h, S.W, S.H, vp(K), vp(T), vp(T), 4, vp(pix), vp(out), None) == lib.ERR_NODEVICE
    assert L.flame_hip_predict_map(r._h, vp(np.zeros(S.W * S.H, np.float32))) == lib.ERR_NODEVICE
    with pytest.raises(lib.FlameHipError) as e:
        r.predict(S.W, S.H, K, PC.IDENT, PC.IDENT, pix)
    assert e.value.code == lib.ERR_NODEVICE
