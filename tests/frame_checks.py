"""Checks of a frame-results implementation (the C oracle or the HIP path) against oracle/frame_f64.py.

Every tolerance is k * eps32 * (a magnitude frame_f64 returns); the k are stated here once.  A decision
(pixel coverage, filter flag) is compared exactly wherever its exact margin lies outside the float32
error band; inside the band any outcome a correct float32 implementation could give is accepted.
"""
import numpy as np

from oracle import frame_f64 as F

EPS = F.EPS32
K_IDEPTH = 8     # dense idepth: |got - f64| <= K_IDEPTH eps32 sum_k (|w_k| + m_k) |x_k| / |sum_k w_k|
K_NORMAL = 16    # normals: angle <= K_NORMAL eps32 cond (1 + 2 |P| / min |e|)
K_POINT = 8      # mesh points, cloud: |got - f64| <= K_POINT eps32 |Kinv| |q|
K_COST = 8       # costs: |got - f64| <= K_COST eps32 (sum of magnitudes)


def close(got, want, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        return (got == want) | (np.abs(got - want) <= tol) | (np.isnan(got) & np.isnan(want))


def _where(mask, limit=6):
    idx = np.argwhere(mask)
    return "%d at %s" % (len(idx), idx[:limit].tolist())


def _ids(idx, limit=6):
    return "%d at %s" % (len(idx), np.asarray(idx)[:limit].tolist())


def tri_params_of(case, cls):
    return cls(*case["tp"])


def check_triangles(case, x, tn, tv, vn, what):
    R = F.triangles(case["Kinv"], case["pos"], x, case["tris"], tri_params_of(case, _TP))
    ok = R["ok"]
    tn, vn = np.asarray(tn, np.float64), np.asarray(vn, np.float64)
    assert np.all(tn[~ok] == 0) and np.all(tv[~ok] == 0), what + ": a triangle with a non-finite or non-positive idepth"
    tol = K_NORMAL * EPS * R["ang_tol"][ok] + 8 * EPS
    ang = F.angle(tn[ok], R["normal"][ok])
    ang = np.where(R["orient_amb"][ok], np.minimum(ang, np.pi - ang), ang)
    Pa = R["P"][case["tris"][ok, 0]]
    bad = ~(ang <= tol)
    assert not bad.any(), "%s: normal angle to float64 (max %.3g rad): %s" % (what, np.nanmax(ang), _ids(np.flatnonzero(ok)[bad]))
    assert np.all(np.abs(np.linalg.norm(tn[ok], axis=1) - 1) <= 4 * EPS), what + ": normals not unit"
    facing = (tn[ok] * Pa).sum(1) / np.linalg.norm(Pa, axis=1)
    bad = ~(facing <= tol)
    assert not bad.any(), "%s: normal faces away from the camera (n.P_a > 0): %s" % (what, _ids(np.flatnonzero(ok)[bad]))
    mism = (tv.astype(bool) != R["valid"])
    hard = mism & ~R["flag_amb"]
    assert not hard.any(), "%s: validity flags differ from float64: %s (got %s, want %s)" % (
        what, _where(hard), tv[hard][:6].tolist(), R["valid"][hard][:6].astype(int).tolist())
    # (a triangle whose float32 normal under- or overflows has no angle bound: its oblique test is not counted)
    namb = int((R["flag_amb"] & np.isfinite(R["ang_tol"])).sum())
    assert namb <= max(4, len(tv) // 100), "%s: %d flags within the float32 band: %s" % (what, namb, _where(R["flag_amb"]))
    z = R["vtx_zero"]
    assert np.all(vn[z] == np.array([0.0, 0.0, -1.0])), "%s: vertex normal of a zero sum: %s" % (what, _where(z & np.any(vn != [0, 0, -1], 1)))
    ang = F.angle(vn[~z], R["vtx"][~z])
    bad = ~(ang <= EPS * R["vtx_tol"][~z] + 8 * EPS)
    assert not bad.any(), "%s: vertex normal angle (max %.3g rad): %s" % (what, np.nanmax(ang), _ids(np.flatnonzero(~z)[bad]))
    return R


def check_raster(case, x, idm, keep, what):
    """Owner / coverage and idepth of a dense map (keep = the implementation's own tri_valid for a filtered
    map, None for an unfiltered one)."""
    W, H = case["W"], case["H"]
    R = F.raster(W, H, case["pos"], x, case["tris"], keep)
    got = np.asarray(idm, np.float64).ravel()
    assert got.shape == (W * H,)
    na, cov = ~R.ambiguous, R.owner >= 0
    if case["lattice"]:
        assert not R.ambiguous.any(), what + ": a lattice case must be decided exactly everywhere"
    bad = na & ~cov & ~np.isnan(got)
    assert not bad.any(), "%s: drawn where no triangle covers: %s" % (what, _where(bad.reshape(H, W)))
    ok = close(got, R.value, K_IDEPTH * EPS * R.scale)
    bad = na & cov & ~ok
    if bad.any():
        p = np.flatnonzero(bad)[:4]
        raise AssertionError("%s: idepth differs from the exact owner's float64 value: %s; got %s want %s (owner %s)" % (
            what, _where(bad.reshape(H, W)), got[p].tolist(), R.value[p].tolist(), R.owner[p].tolist()))
    amb_ok = np.zeros(W * H, bool)
    np.logical_or.at(amb_ok, R.cand_pix, close(got[R.cand_pix], R.cand_val, K_IDEPTH * EPS * R.cand_scale))
    bad = R.ambiguous & ~amb_ok & ~np.isnan(got)
    assert not bad.any(), "%s: near-edge idepth matches no candidate triangle: %s" % (what, _where(bad.reshape(H, W)))
    holes = R.ambiguous & R.interior & np.isnan(got) & ~amb_ok
    assert not holes.any(), "%s: holes (exactly covered, inside the mesh, NaN): %s" % (what, _where(holes.reshape(H, W)))
    return R


def check_coverage(R, cov, what):
    cnt, cov32, namb = F.coverage(R)
    n = len(R.value)
    if namb == 0:
        assert cov == cov32, "%s: coverage %r, exact %r (%d / %d)" % (what, cov, cov32, cnt, n)
    else:
        assert abs(cov * n - cnt) <= namb + 1e-6 * n, "%s: coverage %r vs %d / %d (%d ambiguous)" % (what, cov, cnt, n, namb)


def check_depth(idm, dm, what):
    want = F.depth(idm)
    got = np.asarray(dm, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: depth NaN pattern: %s" % (what, _where(np.isnan(got) != np.isnan(want)))
    bad = ~close(got, want, EPS * np.abs(want))
    assert not bad.any(), "%s: depth != 1/idepth: %s" % (what, _where(bad))


def check_cloud(case, dm, cl, what):
    want, mag = F.cloud(case["Kinv"], dm, case["min_depth"], case["max_depth"])
    got = np.asarray(cl, np.float64)
    wn = np.isnan(want).any(-1)
    assert np.array_equal(np.isnan(got).all(-1), wn) and not (np.isnan(got).any(-1) & ~wn).any(), \
        "%s: cloud NaN pattern: %s" % (what, _where(np.isnan(got).all(-1) != wn))
    bad = ~close(got, want, K_POINT * EPS * mag) & ~wn[..., None]
    assert not bad.any(), "%s: cloud differs from Kinv (j d, i d, d): %s" % (what, _where(bad))


def check_mesh(case, x, T_R, pts, faces, tv, what):
    W, H = case["W"], case["H"]
    valid, P, Pm, uv = F.mesh(case["Kinv"], case["pos"], x, W, H)
    pts = np.asarray(pts, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):  # float32 overflows (idepth ~1e-40): any non-finite point
        ovf_all = ~np.isfinite(P.astype(np.float32)).all(1) | ~np.isfinite(Pm.astype(np.float32)).all(1)
    bad = (~valid & ~np.isnan(pts[:, :3]).all(1)) | (valid & ~ovf_all & np.isnan(pts[:, :3]).any(1))
    assert not bad.any(), "%s: mesh point NaN pattern: %s" % (what, _where(bad))
    assert np.all(pts[~valid, 3:] == 0), what + ": invalid vertices carry data"
    v = valid
    ovf = ovf_all[v]
    good = close(pts[v, :3], P[v], K_POINT * EPS * Pm[v]).all(1)
    bad = ~np.where(ovf, ~np.isfinite(pts[v, :3]).all(1), good)
    assert not bad.any(), "%s: mesh points differ from Kinv (u, v, 1) / idepth: %s" % (what, _ids(np.flatnonzero(v)[bad]))
    assert np.all(pts[v][:, [3, 7, 10, 11]] == 0), what + ": PointNormalUV padding"
    z = T_R["vtx_zero"][v]
    ang = F.angle(pts[v, 4:7][~z], T_R["vtx"][v][~z])
    assert np.all(ang <= EPS * T_R["vtx_tol"][v][~z] + 8 * EPS), what + ": mesh normals"
    bad = ~close(pts[v, 8:10], uv[v], EPS * np.abs(uv[v])).all(1)
    assert not bad.any(), "%s: texture coordinates != (u / (W-1), v / (H-1)): %s" % (what, _ids(np.flatnonzero(v)[bad]))
    want = case["tris"][np.asarray(tv, bool)][:, ::-1]
    assert np.array_equal(np.asarray(faces), want), what + ": faces are not the valid triangles with reversed winding"


def check_costs(got, want, what):
    s, d = got
    s64, d64, sm, dm = want
    assert abs(s - s64) <= K_COST * EPS * sm, "%s: smoothness cost %r vs float64 %r (mag %r)" % (what, s, s64, sm)
    assert abs(d - d64) <= K_COST * EPS * dm, "%s: data cost %r vs float64 %r (mag %r)" % (what, d, d64, dm)


def check_filter(x, edges, kind, got, what):
    want, mag = F.graph_filter(x, edges, kind)
    got = np.asarray(got, np.float32)
    if kind == 0:
        bad = got.view(np.uint32) != want.view(np.uint32)
        bad &= ~(np.isnan(got) & np.isnan(want))
        assert not bad.any(), "%s: median: %s (got %s want %s)" % (what, _where(bad), got[bad][:6].tolist(), want[bad][:6].tolist())
    else:
        assert np.array_equal(np.isnan(got), np.isnan(want)), what + ": low-pass NaN pattern"
        sp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        bad = ~close(got, want, 2 * sp + 1.01 * F.U32 * mag)
        assert not bad.any(), "%s: low-pass differs from the float64 mean: %s" % (what, _where(bad))


class _TP:
    """The fields frame_f64.triangles reads, from a case's tp tuple."""
    def __init__(self, do_oblique_triangle_filter, oblique_normal_thresh, oblique_idepth_diff_factor, oblique_idepth_diff_abs,
                 do_edge_length_filter, edge_length_thresh, do_idepth_triangle_filter, min_triangle_idepth, width, height):
        self.__dict__.update(locals())
