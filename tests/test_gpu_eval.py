"""The evaluate stage on the GPU (flame_hip_photo_reference / _photo_error / _truth_stats; kernels:
flame_ros_amd/csrc/evaluate.hip) equals its NumPy restatement tests/eval_ref.py BIT FOR BIT -- total256, the four counts and
the error map as uint32 views; the confusion counts and the truth error map -- on the cases of tests/eval_cases.py, which
tests/test_eval_ref.py pins against hand-derived values and ground truth."""
import numpy as np
import pytest

from flame_ros_amd import lib
from flame_ros_amd.regularizer import GraphRegularizer, TriParams
from tests import eval_cases as EC
from tests import eval_ref as R

pytestmark = pytest.mark.gpu

U32 = np.uint32
F = np.float32


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got.view(U32).ravel() != want.view(U32).ravel())
    assert bad.size == 0, (what, bad.size, bad[:5], got.ravel()[bad[:5]], want.ravel()[bad[:5]])


def tri_params(W, H, min_idepth=None):
    """All triangle filters off, or only the idepth filter."""
    return TriParams(0, 1.57, 0.35, 0.1, 0, 0.333, int(min_idepth is not None), min_idepth or 0.0, W, H)


def check_photo(r, c, cur=None, cmp=None, idepthmap="case", filtered=True, kinv=True, tp=None):
    """photo_reference + photo_error on handle r against the restatement; returns the device's (total256, counts, map)."""
    K, Kinv = EC.k9(c["K4"]), EC.kinv9(c["K4"]) if kinv else None
    tp = tp or tri_params(c["W"], c["H"])
    idm = c["idepth"] if isinstance(idepthmap, str) else idepthmap
    r.photo_reference(c["cmp"] if cmp is None else cmp, c["Tcmp"])
    assert r.info("photo_reference") == 1
    total, counts, err = r.photo_error(c["cur"] if cur is None else cur, c["Tcur"], K, Kinv, tp, idepthmap=idm, filtered=filtered,
                                       want_map=True)
    used = idm if idm is not None else r.depthmaps(EC.kinv9(c["K4"]), tp, filtered=filtered, cloud=False)[0]
    want_total, want_counts, want_err, _, _ = R.photo(c["K4"], c["Tcmp"], c["Tcur"], used, c["cur"], c["cmp"])
    print("total256 %d, counts %s (restatement %d, %s)" % (total, counts, want_total, want_counts))
    assert total == want_total and counts == want_counts and sum(counts) == c["W"] * c["H"]
    same_bits(err, want_err, "error map")
    assert r.info("photo_us") > 0 and r.info("photo_device_us") > 0
    # without the map the same numbers come back
    assert r.photo_error(c["cur"] if cur is None else cur, c["Tcur"], K, Kinv, tp, idepthmap=idm, filtered=filtered) == (total, counts)
    return total, counts, err


@pytest.mark.parametrize("name", sorted(EC.PHOTO_CASES))
def test_photo_bit_parity(gpu, name):
    """Caller's map on a handle without a graph; the two scenes are 160 x 120 (19 blocks, the last one partial)."""
    c = EC.PHOTO_CASES[name]()
    with GraphRegularizer.empty() as r:
        total, counts, _ = check_photo(r, c, kinv=name != "half_pixel")  # (Kinv may be NULL with a caller's map)
    if name == "exact_shift":
        assert total == 0 and counts == (2773, 0, 0, 64 * 48 - 2773)
    if name in ("odd", "no_idepth", "behind"):
        assert counts[{"odd": R.OUTSIDE, "no_idepth": R.NO_IDEPTH, "behind": R.BEHIND}[name]] > 0


def test_odd_size_with_padded_rows(gpu):
    """37 x 29 with pitch = 41 on both images: one full block of 1 024 pixels plus a tail of 49; the map is the caller's."""
    c = EC.odd_case()
    cur, cmp = c["cur_padded"][:, :c["W"]], c["cmp_padded"][:, :c["W"]]
    assert cur.strides == (41, 1) and cmp.strides == (41, 1) and c["W"] * c["H"] == 1024 + 49
    with GraphRegularizer.empty() as r:
        _, counts, _ = check_photo(r, c, cur=cur, cmp=cmp)
    assert all(n > 0 for n in counts)


def two_triangle_handle(c):
    """Two triangles over the 64 x 48 image of the case; vertex 1 lies below min_triangle_idepth, so the triangle stage makes
    triangle 0 invalid: a hole in the filtered map."""
    pos = np.array([[-2.0, -2.0], [66.0, -2.0], [66.0, 50.0], [-2.0, 50.0]], F)
    x = np.array([0.5, 0.1, 0.5, 0.45], F)
    tris = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    e = np.array([[0, 1], [0, 2], [0, 3], [1, 2], [2, 3]], np.int32)
    ones = np.ones(len(e), F)
    return GraphRegularizer(pos, e, ones, ones, x, np.ones(4, F), tris=tris), tri_params(c["W"], c["H"], min_idepth=0.15)


@pytest.mark.parametrize("filtered", [True, False])
def test_the_handles_own_map(gpu, filtered):
    """idepthmap = None: the handle's own raster (read back through depthmaps() for the restatement)."""
    c = EC.exact_shift_case()
    r, tp = two_triangle_handle(c)
    with r:
        _, counts, _ = check_photo(r, c, idepthmap=None, filtered=filtered, tp=tp)
        idm = r.depthmaps(EC.kinv9(c["K4"]), tp, filtered=filtered, cloud=False)[0]
        holes = int(np.isnan(idm).sum())
        assert counts[R.NO_IDEPTH] == holes and counts[R.EVALUATED] > 500
        if filtered:
            assert 0.3 * idm.size < holes < 0.7 * idm.size  # the invalid triangle
        else:
            assert holes < 0.1 * idm.size


def test_promotion_equals_an_explicit_upload(gpu):
    c1, c2 = EC.scene_case("forward", 1), EC.scene_case("forward", 2)
    K, tp = EC.k9(c1["K4"]), tri_params(c1["W"], c1["H"])
    with GraphRegularizer.empty() as r:
        r.photo_reference(c1["cmp"], c1["Tcmp"])
        r.photo_error(c1["cur"], c1["Tcur"], K, None, tp, idepthmap=c1["idepth"])
        r.photo_reference(None, None)  # frame 1 becomes the comparison frame: image and pose of the call above
        promoted = r.photo_error(c2["cur"], c2["Tcur"], K, None, tp, idepthmap=c2["idepth"], want_map=True)
        r.photo_reference(c1["cur"], c1["Tcur"])
        explicit = r.photo_error(c2["cur"], c2["Tcur"], K, None, tp, idepthmap=c2["idepth"], want_map=True)
        with pytest.raises(lib.FlameHipError) as e:  # promoted once: the current image of the call before is the reference now
            r.photo_reference(None, None)
            r.photo_reference(None, None)
        assert e.value.code == lib.ERR_STATE
    assert promoted[:2] == explicit[:2]
    same_bits(promoted[2], explicit[2], "error map")
    want = R.photo(c1["K4"], c1["Tcur"], c2["Tcur"], c2["idepth"], c2["cur"], c1["cur"])
    assert promoted[:2] == want[:2] and want[1][R.EVALUATED] > 0.4 * c1["W"] * c1["H"]


def test_state_errors(gpu):
    c, odd = EC.exact_shift_case(), EC.odd_case()
    K, tp = EC.k9(c["K4"]), tri_params(c["W"], c["H"])
    with GraphRegularizer.empty() as r:
        assert r.info("photo_reference") == 0
        with pytest.raises(lib.FlameHipError) as e:  # before any reference
            r.photo_error(c["cur"], c["Tcur"], K, None, tp, idepthmap=c["idepth"])
        assert e.value.code == lib.ERR_STATE
        r.photo_reference(odd["cmp"], odd["Tcmp"])
        with pytest.raises(lib.FlameHipError) as e:  # a reference of another size
            r.photo_error(c["cur"], c["Tcur"], K, None, tp, idepthmap=c["idepth"])
        assert e.value.code == lib.ERR_STATE
        r.photo_reference(c["cmp"], c["Tcmp"])
        for call in (lambda: r.photo_error(c["cur"], c["Tcur"], K, EC.kinv9(c["K4"]), tp),  # the handle has no graph to rasterise
                     lambda: r.truth_stats(np.ones((c["H"], c["W"]), F), EC.kinv9(c["K4"]), tp)):
            with pytest.raises(lib.FlameHipError) as e:
                call()
            assert e.value.code == lib.ERR_STATE
        assert r.photo_error(c["cur"], c["Tcur"], K, None, tp, idepthmap=c["idepth"])[0] == 0


def test_repeatable_and_reads_only(gpu):
    c = EC.exact_shift_case()
    r, tp = two_triangle_handle(c)
    K, Kinv = EC.k9(c["K4"]), EC.kinv9(c["K4"])
    depth = EC.truth_case(c["W"], c["H"])[1]
    with r:
        r.triangles(Kinv, tp)
        before = r.download() + r.download_bar()
        r.photo_reference(c["cmp"], c["Tcmp"])
        a = r.photo_error(c["cur"], c["Tcur"], K, Kinv, tp, want_map=True)
        ta = r.truth_stats(depth, Kinv, tp, want_map=True)
        b = r.photo_error(c["cur"], c["Tcur"], K, Kinv, tp, want_map=True)
        tb = r.truth_stats(depth, Kinv, tp, want_map=True)
        assert a[:2] == b[:2] and ta[0] == tb[0] and np.float64(ta[1]).view(np.uint64) == np.float64(tb[1]).view(np.uint64)
        same_bits(a[2], b[2], "photo error map, second call")
        same_bits(ta[2], tb[2], "truth error map, second call")
        after = r.download() + r.download_bar()
        for x0, x1 in zip(before, after):  # x, w1, w2, q and the bars
            same_bits(x0, x1, "state")
        # the handle's own map for the truth stage: the restatement over the map read back
        idm = r.depthmaps(Kinv, tp, filtered=True, cloud=False)[0]
        conf, _, err = R.truth(idm, depth)
        assert ta[0] == conf
        same_bits(ta[2], err, "truth error map, own map")


@pytest.mark.parametrize("shape", [(37, 29), (160, 120)])
def test_truth_counts_and_error_map(gpu, shape):
    W, H = shape
    idepth, depth = EC.truth_case(W, H)
    want_conf, want_total, want_err = R.truth(idepth, depth)
    with GraphRegularizer.empty() as r:
        conf, total, err = r.truth_stats(depth, None, tri_params(W, H), idepthmap=idepth, want_map=True)
        assert r.truth_stats(depth, None, tri_params(W, H), idepthmap=idepth)[0] == conf
        assert r.info("truth_us") > 0
    assert conf == want_conf and sum(conf) == W * H and min(conf) > 0
    same_bits(err, want_err, "idepth error map")
    assert total == np.inf == want_total  # (the case holds infinite idepths: estimates, as in the reference)


@pytest.mark.parametrize("shape", [(37, 29), (160, 120)])
def test_truth_total_error(gpu, shape):
    """Bitwise repeatable, and within 2 (n - 1) 2^-53 s of the float64 sum s of the float32 errors (n = W H): the bound of
    any summation of n non-negative terms in double."""
    W, H = shape
    idepth, depth = EC.truth_case(W, H)
    idepth = np.where(np.isinf(idepth), F(0.5), idepth)
    _, want_total, want_err = R.truth(idepth, depth)
    s = float(np.sum(want_err[~np.isnan(want_err)].astype(np.float64)))
    with GraphRegularizer.empty() as r:
        totals = [r.truth_stats(depth, None, tri_params(W, H), idepthmap=idepth)[1] for _ in range(3)]
    print("%d x %d: device %.17g, float64 sum %.17g, restated shape %.17g" % (W, H, totals[0], s, want_total))
    assert len({np.float64(t).view(np.uint64) for t in totals}) == 1
    n = W * H
    assert s > 0 and abs(totals[0] - s) <= 2 * (n - 1) * 2.0 ** -53 * s
    assert totals[0] == want_total  # the restatement adds in the device's shape
