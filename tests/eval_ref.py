"""NumPy restatement of the evaluate stage (kernels: flame_ros_amd/csrc/evaluate.hip).  `photo`: float32
arrays with + - x / floor only, every operation rounded on its own, sums left to right, integer costs -- operation by
operation what k_ev_photo does, so the GPU equals it bit for bit.  `truth`: the branches of reference src/utils.cc:339-365
(getDepthConfusionMatrix) as masks; its total_error is summed in float64 in the device's fixed shape (`tree_sum`)."""
import numpy as np

from tests.frontend_ref import pose_record  # A = K R, c = K t in double, rounded once: the routine the library shares too

F = np.float32
NAN = np.float32(np.nan)  # 0x7fc00000, what the kernels write
EVALUATED, NO_IDEPTH, BEHIND, OUTSIDE = 0, 1, 2, 3
BLOCK = 1024


def photo(K4, T_world_cmp, T_world_cur, idepth, cur, cmp):
    """(total256, (evaluated, no_idepth, behind, outside), error map float32[H, W], D uint32[H, W], class[H, W])."""
    cur, cmp = np.asarray(cur, np.uint8), np.asarray(cmp, np.uint8)
    H, W = cur.shape
    assert cmp.shape == (H, W)
    xi = np.asarray(idepth, F).reshape(H, W)
    fx, fy, cx, cy = (F(k) for k in K4)
    A, c = pose_record(K4, T_world_cmp, T_world_cur)  # T_cmp_cur = T_world_cmp^-1 T_world_cur
    with np.errstate(all="ignore"):
        i, j = np.mgrid[0:H, 0:W]
        b0, b1 = (j.astype(F) - cx) / fx, (i.astype(F) - cy) / fy
        w = [((A[r][0] * b0 + A[r][1] * b1) + A[r][2]) + xi * c[r] for r in range(3)]
        has = np.isfinite(xi) & (xi > 0)
        front = (w[2] > 0) & np.isfinite(w[0]) & np.isfinite(w[1]) & np.isfinite(w[2])
        qx = np.floor((w[0] / w[2]) * F(16.0) + F(0.5))
        qy = np.floor((w[1] / w[2]) * F(16.0) + F(0.5))
        assert qx.dtype == F and w[0].dtype == F
        inside = (qx >= 0) & (qx < F(16 * (W - 1))) & (qy >= 0) & (qy < F(16 * (H - 1)))  # (in float: NaN and huge fail here)
    cls = np.where(~has, NO_IDEPTH, np.where(~front, BEHIND, np.where(~inside, OUTSIDE, EVALUATED))).astype(np.int32)
    ev = cls == EVALUATED
    qxi, qyi = np.where(ev, qx, 0).astype(np.int64), np.where(ev, qy, 0).astype(np.int64)
    ix, iy = qxi >> 4, qyi >> 4
    wx1, wy1 = qxi & 15, qyi & 15
    wx0, wy0 = 16 - wx1, 16 - wy1
    I = cmp.astype(np.int64)
    ix1, iy1 = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)  # (only to keep the masked-out lanes in range)
    S = wx0 * wy0 * I[iy, ix] + wx1 * wy0 * I[iy, ix1] + wx0 * wy1 * I[iy1, ix] + wx1 * wy1 * I[iy1, ix1]
    D = np.where(ev, np.abs(S - 256 * cur.astype(np.int64)), 0)
    err = np.where(ev, D.astype(F) / F(256.0), NAN).astype(F)
    counts = tuple(int((cls == k).sum()) for k in range(4))
    return int(D.sum()), counts, err, D.astype(np.uint32), cls


def tree_sum(err32):
    """The device's summation shape: float64; block b owns elements [1024 b, 1024 (b + 1)), thread t of its 256 adds its
    elements 256 r + t in ascending r, lane l of a wave takes lane l + o for o = 32 .. 1, the four wave sums are added left
    to right, and the block sums in ascending b.  (Missing elements are +0.0.)"""
    e = np.asarray(err32, F).ravel().astype(np.float64)
    nb = (len(e) + BLOCK - 1) // BLOCK
    pad = np.zeros(nb * BLOCK, np.float64)
    pad[:len(e)] = e
    v = pad.reshape(nb, 4, 4, 64)  # [block, r, wave, lane]
    with np.errstate(all="ignore"):
        v = ((v[:, 0] + v[:, 1]) + v[:, 2]) + v[:, 3]
        o = 32
        while o > 0:
            v = v[..., :o] + v[..., o:2 * o]
            o >>= 1
        part = ((v[:, 0, 0] + v[:, 1, 0]) + v[:, 2, 0]) + v[:, 3, 0]
        total = 0.0
        for p in part:
            total = total + float(p)
    return total


def truth(idepth, depth):
    """((true_pos, true_neg, false_pos, false_neg), total_error (float64, the device's shape), error map float32[H, W])."""
    est, depth = np.asarray(idepth, F), np.asarray(depth, F)
    assert est.shape == depth.shape
    with np.errstate(all="ignore"):
        has_truth = depth > 0          # (a NaN depth is no truth)
        has_est = ~np.isnan(est)       # (an infinite idepth is an estimate)
        tp, fn = has_truth & has_est, has_truth & ~has_est
        fp, tn = ~has_truth & has_est, ~has_truth & ~has_est
        err = np.full(est.shape, NAN, F)
        err[tp] = np.abs(est[tp] - F(1.0) / depth[tp])
        err[fp] = np.abs(est[fp])
    total = tree_sum(np.where(tp | fp, err, F(0.0)))
    return (int(tp.sum()), int(tn.sum()), int(fp.sum()), int(fn.sum())), total, err


def derived(conf, total_error):
    """(avg_error, precision, recall) as reference src/flame_offline_tum.cc:331-334 forms them (float32)."""
    tp, _, fp, fn = conf
    with np.errstate(all="ignore"):
        return (F(total_error) / F(tp + fp), F(tp) / F(tp + fp), F(tp) / F(tp + fn))
