"""Pins tests/eval_ref.py, the NumPy restatement of the evaluate stage: hand-derived exact values, one map per
pixel class, float64-rendered ground truth on the plane scenes of tests/frontend_scenes.py, and the reference's
getDepthConfusionMatrix as a literal double loop.  No GPU; the GPU equals the restatement bit for bit in
tests/test_gpu_eval.py.  The first test is the ABI surface of the stage."""
import ctypes as C

import numpy as np
import pytest

from flame_ros_amd import graphgen, lib
from flame_ros_amd.regularizer import GraphRegularizer, default_tri_params
from tests import eval_cases as EC
from tests import eval_ref as R
from tests import frontend_scenes as S

F = np.float32


def run(c, idepth=None):
    return R.photo(c["K4"], c["Tcmp"], c["Tcur"], c["idepth"] if idepth is None else idepth, c["cur"], c["cmp"])


def test_abi_surface():
    """The library exports the stage; argument errors come before any device work, and without a device it says so: there
    is no CPU path."""
    L = lib.load()
    for name in ("flame_hip_photo_reference", "flame_hip_photo_error", "flame_hip_truth_stats"):
        assert hasattr(L, name)
    assert L.flame_hip_version() >= 405
    c = EC.exact_shift_case()
    W, H = c["W"], c["H"]
    g = graphgen.synthetic(300, seed=1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    K, Kinv, tp = EC.k9(c["K4"]), EC.kinv9(c["K4"]), default_tri_params(W, H)
    T = np.ascontiguousarray(EC.IDENT.reshape(12))
    bad_T = T.copy()
    bad_T[7] = np.inf
    img, idm, depth = c["cur"], c["idepth"], np.ones((H, W), F)
    total, counts, conf, te = C.c_uint64(), np.zeros(4, np.int64), np.zeros(4, np.int64), C.c_double()
    with GraphRegularizer(g.pos, g.edges, g.alpha, g.beta, g.z, g.wgt, tris=g.tris, device=-1) as r:
        h = r._h
        ref = lambda W=W, H=H, img=vp(img), pitch=W, T=vp(T): L.flame_hip_photo_reference(h, W, H, img, pitch, T)  # noqa: E731

        def err(K=vp(K), tp=tp, img=vp(img), pitch=W, T=vp(T), total=C.byref(total), counts=vp(counts), idm=vp(idm)):
            return L.flame_hip_photo_error(h, K, vp(Kinv), C.byref(tp), 1, idm, img, pitch, T, total, counts, None)

        def truth(tp=tp, depth=vp(depth), conf=vp(conf), te=C.byref(te)):
            return L.flame_hip_truth_stats(h, vp(Kinv), C.byref(tp), 1, vp(idm), depth, conf, te, None)

        # valid arguments: the answer is "no device", also for the handle's own map and for a promotion
        assert ref() == lib.ERR_NODEVICE and ref(img=None, pitch=0, T=None) == lib.ERR_NODEVICE
        assert err() == lib.ERR_NODEVICE and err(idm=None) == lib.ERR_NODEVICE
        assert truth() == lib.ERR_NODEVICE
        # ARG: pitch < W, NULL, W = 0 (or above 8192), fx <= 0
        assert ref(pitch=W - 1) == lib.ERR_ARG and ref(T=None) == lib.ERR_ARG and ref(W=0) == lib.ERR_ARG and ref(H=8193) == lib.ERR_ARG
        assert err(pitch=W - 1) == lib.ERR_ARG and err(img=None) == lib.ERR_ARG and err(K=None) == lib.ERR_ARG
        assert err(total=None) == lib.ERR_ARG and err(counts=None) == lib.ERR_ARG and err(T=None) == lib.ERR_ARG
        assert err(tp=default_tri_params(0, H)) == lib.ERR_ARG and truth(tp=default_tri_params(W, 0)) == lib.ERR_ARG
        assert truth(depth=None) == lib.ERR_ARG and truth(conf=None) == lib.ERR_ARG and truth(te=None) == lib.ERR_ARG
        K0 = K.copy()
        K0[0] = 0.0
        assert err(K=vp(K0)) == lib.ERR_ARG
        # NAN: a non-finite pose or K
        assert ref(T=vp(bad_T)) == lib.ERR_NAN and err(T=vp(bad_T)) == lib.ERR_NAN
        Kn = K.copy()
        Kn[2] = np.nan
        assert err(K=vp(Kn)) == lib.ERR_NAN
        # the Python layer raises the same codes
        for call in (lambda: r.photo_reference(img, EC.IDENT), lambda: r.photo_error(img, EC.IDENT, K, Kinv, tp, idepthmap=idm),
                     lambda: r.truth_stats(depth, Kinv, tp, idepthmap=idm)):
            with pytest.raises(lib.FlameHipError) as e:
                call()
            assert e.value.code == lib.ERR_NODEVICE


def test_exact_shift():
    c = EC.exact_shift_case()
    total, counts, err, D, cls = run(c)
    assert total == 0
    assert counts[R.EVALUATED] == 59 * 47 == 2773 and counts[R.OUTSIDE] == 64 * 48 - 2773
    assert counts[R.NO_IDEPTH] == 0 and counts[R.BEHIND] == 0
    assert (cls[:47, :59] == R.EVALUATED).all() and (err[:47, :59] == 0).all() and np.isnan(err[cls != R.EVALUATED]).all()
    # a pixel landing on column W - 1 (column 59 -> 63) or row H - 1 is outside: its +1 neighbour would be
    assert (cls[:, 59] == R.OUTSIDE).all() and (cls[47, :] == R.OUTSIDE).all() and (cls[:47, 58] == R.EVALUATED).all()


def test_half_pixel():
    c = EC.half_pixel_case()
    total, counts, err, D, cls = run(c)
    cmp, cur = c["cmp"].astype(np.int64), c["cur"].astype(np.int64)
    # p = (j + 0.5, i): weights 8 x 16 = 128 on columns j and j + 1 of row i
    want = np.abs(128 * (cmp[:47, 0:63] + cmp[:47, 1:64]) - 256 * cur[:47, 0:63])
    assert (cls[:47, :63] == R.EVALUATED).all() and counts[R.EVALUATED] == 63 * 47  # (floor(j + 0.5) <= W - 2: columns 0 .. 62)
    assert np.array_equal(D[:47, :63], want) and total == int(want.sum()) and total > 0
    assert np.array_equal(err[:47, :63], (want / 256.0).astype(F))
    assert sum(counts) == c["W"] * c["H"]


def test_class_no_idepth():
    c = EC.no_idepth_case()
    _, counts, err, _, cls = run(c)
    for kind, row in EC.NO_IDEPTH_ROWS.items():
        assert (cls[row] == R.NO_IDEPTH).all(), kind
    assert counts[R.NO_IDEPTH] == 4 * c["W"] and sum(counts) == c["W"] * c["H"]
    assert counts[R.EVALUATED] == 59 * (47 - 4) and np.isnan(err[cls == R.NO_IDEPTH]).all()


def test_class_behind():
    c = EC.behind_case()
    _, counts, _, _, cls = run(c)
    assert (cls[:, 49:] == R.BEHIND).all() and (cls[:, :46] != R.BEHIND).all()  # (the boundary is at column 47.04)
    assert counts[R.BEHIND] >= 15 * c["H"] and counts[R.NO_IDEPTH] == 0 and sum(counts) == c["W"] * c["H"]


def test_odd_case_holds_every_class():
    c = EC.odd_case()
    total, counts, _, _, cls = run(c)
    assert all(n > 0 for n in counts) and sum(counts) == 37 * 29 == 1073 and total > 0
    assert (cls[5:8, 7] == R.NO_IDEPTH).all() and (cls[8, 0:6] == R.BEHIND).all()


@pytest.mark.parametrize("name", S.NAMES)
def test_the_true_map_has_the_smallest_error(name):
    """Ground truth: with the plane's exact idepth map the average error is smaller than with 1.25 x and with 0.8 x the map."""
    for k in range(1, 6):
        avg = {}
        for gain in (1.0, 1.25, 0.8):
            total, counts, _, _, _ = run(EC.scene_case(name, k, gain))
            assert counts[R.EVALUATED] > 0.4 * S.W * S.H, (k, gain, counts)  # (not vacuous)
            avg[gain] = total / (256.0 * counts[R.EVALUATED])
        print("%s k=%d: true %.4f, x1.25 %.4f, x0.8 %.4f, worst ratio %.3f" %
              (name, k, avg[1.0], avg[1.25], avg[0.8], avg[1.0] / min(avg[1.25], avg[0.8])))
        assert avg[1.0] < avg[1.25] and avg[1.0] < avg[0.8], (k, avg)


def confusion_loop(idepths, depth):
    """The loop of reference src/utils.cc:339-365, branch by branch, on float32 scalars."""
    H, W = depth.shape
    tp = tn = fp = fn = 0
    err = np.full((H, W), np.nan, F)
    total = F(0.0)
    with np.errstate(all="ignore"):
        for ii in range(H):
            for jj in range(W):
                if depth[ii, jj] > 0:
                    if not np.isnan(idepths[ii, jj]):
                        idepth_est = idepths[ii, jj]
                        idepth_true = F(1.0) / depth[ii, jj]
                        error = np.abs(idepth_est - idepth_true)
                        err[ii, jj] = error
                        total = total + error
                        tp += 1
                    else:
                        fn += 1
                elif not np.isnan(idepths[ii, jj]):
                    error = np.abs(idepths[ii, jj])
                    err[ii, jj] = error
                    total = total + error
                    fp += 1
                else:
                    tn += 1
    return (tp, tn, fp, fn), total, err


def test_truth_counts_and_error_map():
    idepth, depth = EC.truth_case(37, 29)
    conf, total, err = R.truth(idepth, depth)
    want_conf, want_total, want_err = confusion_loop(idepth, depth)
    assert conf == want_conf and min(conf) > 20 and sum(conf) == 37 * 29
    assert np.array_equal(err.view(np.uint32), want_err.view(np.uint32))
    # the hand-placed pixels: an infinite idepth is an estimate, with and without truth
    assert err[0, 0] == np.inf and err[0, 1] == np.inf and np.isnan(err[0, 2]) and np.isnan(err[0, 3]) and err[0, 4] == F(0.25)
    assert total == np.inf and want_total == np.inf
    tp, tn, fp, fn = conf
    avg, precision, recall = R.derived(conf, 1.0)
    assert precision == F(tp) / F(tp + fp) and recall == F(tp) / F(tp + fn) and 0.5 < precision < 1 and 0.5 < recall < 1
    assert avg == F(1.0) / F(tp + fp)


@pytest.mark.parametrize("shape", [(37, 29), (160, 120)])
def test_truth_total_error_bound(shape):
    """The one departure from the reference, bounded by derivation: against s, the float64 sum of the n float32 errors (all
    >= 0), the device's shape is within 2 (n - 1) 2^-53 s and the reference's float32 running sum within
    (n - 1) 2^-24 s (1 + (n - 1) 2^-24) (n - 1 additions, each with relative error <= 2^-24 of a partial sum <= the final one)."""
    W, H = shape
    idepth, depth = EC.truth_case(W, H)
    idepth = np.where(np.isinf(idepth), F(0.5), idepth)  # (finite errors: an infinite sum is compared above)
    conf, total, err = R.truth(idepth, depth)
    e = err[~np.isnan(err)]
    n = W * H
    s = float(np.sum(e.astype(np.float64)))
    assert s > 0 and np.isfinite(total)
    assert abs(total - s) <= 2 * (n - 1) * 2.0 ** -53 * s
    running = float(np.cumsum(e, dtype=F)[-1])  # float32, row-major: what the reference computes
    if (W, H) == (37, 29):  # (the literal loop is slow in Python: the small size only)
        assert running == float(confusion_loop(idepth, depth)[1])
    u = (n - 1) * 2.0 ** -24
    print("%d x %d: s = %.9g, device shape off by %.3e, float32 running sum off by %.3e (bound %.3e)" %
          (W, H, s, abs(total - s), abs(running - s), u * s * (1 + u)))
    assert abs(running - s) <= u * s * (1 + u)
