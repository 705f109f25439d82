"""Checks of a frame-results implementation (the C oracle or the HIP path) against oracle/frame_f64.py.

Every tolerance is k * eps32 * (a magnitude frame_f64 returns); the k are stated here once.  A decision
(pixel coverage, filter flag) is compared exactly wherever its exact margin lies outside the float32
error band; inside the band any outcome a correct float32 implementation could give is accepted.
"""
import numpy as np

from oracle import debug_f64 as D
from oracle import frame_f64 as F

EPS = F.EPS32
K_IDEPTH = 8     # dense idepth: |got - f64| <= K_IDEPTH eps32 sum_k (|w_k| + m_k) |x_k| / |sum_k w_k|
K_NORMAL = 16    # normals: angle <= K_NORMAL eps32 cond (1 + 2 |P| / min |e|)
K_POINT = 8      # mesh points, cloud: |got - f64| <= K_POINT eps32 |Kinv| |q|
K_COST = 8       # costs: |got - f64| <= K_COST eps32 (sum of magnitudes)
from oracle.debug_f64 import K_BLEND, K_CHAN, K_JET  # noqa: E402,F401 -- the debug images' bands: derived and stated there, where they are applied
UNCERTAIN_CAP = 0.02  # share of an image's drawn pixels that may lie inside a band (none in a lattice or dyadic case)


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


# ---------------------------------------------------------------- debug images (oracle/debug_f64.py)
def _check_image(img, got, what, exact_case, skip=None):
    """got [H,W,3] BGR8 against a debug_f64.Image: black where nothing is drawn, byte equality where the statement is
    certain, one of the two neighbouring levels inside the band.  Returns (drawn, uncertain) pixel counts, after
    holding the uncertain share under its cap (none at all where exact_case)."""
    got = np.asarray(got).reshape(-1, 3).astype(np.int64)
    assert len(got) == len(img.drawn), what + ": image size"
    look = np.ones(len(got), bool) if skip is None else ~skip
    bad = look & ~img.drawn & got.any(1)
    assert not bad.any(), "%s: drawn where the statement draws nothing: %s %s" % (what, _ids(np.flatnonzero(bad)), got[bad][:3].tolist())
    ok = ((got >= img.lo) & (got <= img.hi)).all(1) | img.free
    bad = look & img.drawn & ~ok
    if bad.any():
        p = np.flatnonzero(bad)[:4]
        raise AssertionError("%s: %d pixels differ from the statement, first (flat index) %s: got %s want %s..%s (primitive %s)" % (
            what, int(bad.sum()), p.tolist(), got[p].tolist(), img.lo[p].tolist(), img.hi[p].tolist(), img.key[p].tolist()))
    drawn, unc = int((look & img.drawn).sum()), int((look & img.drawn & (img.uncertain | img.free)).sum())
    print("%s: %d of %d drawn pixels uncertain (%.3f %%)" % (what, unc, drawn, 100.0 * unc / max(drawn, 1)))
    if exact_case:
        assert unc == 0, "%s: %d uncertain pixels in a case that float32 evaluates exactly" % (what, unc)
    assert unc <= UNCERTAIN_CAP * drawn, "%s: %d of %d drawn pixels uncertain: above the cap" % (what, unc, drawn)
    return drawn, unc


def check_wireframe(case, x, tv, got, what, rules=D.STATED):
    img = D.wireframe(case["W"], case["H"], case["pos"], x, case["tris"], tv, case["scale"], rules)
    return _check_image(img, got, what + " wireframe", case["lattice"] or case["dyadic"])


def check_features_image(case, got, what, rules=D.STATED):
    img = D.features(case["W"], case["H"], case["feat_pos"], case["feat_mu"], case["scale"], rules)
    return _check_image(img, got, what + " features", case["lattice"] or case["dyadic"])


def check_idepth_image(case, idm, got, what, rules=D.STATED):
    """idm: the implementation's own filtered dense map (pinned by check_raster): only the colouring is judged."""
    img = D.idepth_image(idm, case["scale"], rules)
    return _check_image(img, got, what + " idepthmap", case["lattice"] or case["dyadic"])


def check_normals_image(case, x, tv, vn, idm, got, what, R=None, rules=D.STATED):
    """tv, vn, idm: the implementation's own tri_valid, vertex normals and filtered dense map.  The picture is drawn
    exactly where that map is a number; the colour is the float64 blend under the exact owner (any candidate owner
    at an ambiguous raster pixel)."""
    W, H = case["W"], case["H"]
    if R is None:
        R = F.raster(W, H, case["pos"], x, case["tris"], np.asarray(tv, bool))
    img, (cpix, clo, chi, cfree) = D.normals(W, H, case["pos"], x, case["tris"], tv, vn, R, rules)
    g = np.asarray(got).reshape(-1, 3).astype(np.int64)
    covered = ~np.isnan(np.asarray(idm, np.float64).ravel())
    bad = g.any(1) != covered
    assert not bad.any(), "%s normals: drawn pixels are not those of the filtered map: %s" % (what, _ids(np.flatnonzero(bad)))
    amb_ok = np.zeros(W * H, bool)
    np.logical_or.at(amb_ok, cpix, ((g[cpix] >= clo) & (g[cpix] <= chi)).all(1) | cfree)
    own_ok = img.drawn & (((g >= img.lo) & (g <= img.hi)).all(1) | img.free)
    bad = R.ambiguous & covered & ~amb_ok & ~own_ok
    assert not bad.any(), "%s normals: colour at a near-edge pixel matches no candidate owner: %s" % (what, _ids(np.flatnonzero(bad)))
    return _check_image(img, got, what + " normals", case["lattice"] or case["dyadic"], skip=R.ambiguous)


KINDS = ("wireframe", "features", "normals", "idepthmap")   # image kinds 0..3 (flame_hip.h FLAME_HIP_IMG_*)


def check_debug_images(case, x, tv, vn, idm, images, what, kinds=KINDS, rules=D.STATED, R=None):
    """The four images of one implementation (images: kind name -> [H,W,3]) with its own tri_valid, vertex normals and
    filtered dense map (R: frame_f64.raster of that tri_valid, if the caller has it).  Returns {kind: (drawn, uncertain)}."""
    out = {}
    if "wireframe" in kinds:
        out["wireframe"] = check_wireframe(case, x, tv, images["wireframe"], what, rules)
    if "features" in kinds:
        out["features"] = check_features_image(case, images["features"], what, rules)
    if "normals" in kinds:
        out["normals"] = check_normals_image(case, x, tv, vn, idm, images["normals"], what, R=R, rules=rules)
    if "idepthmap" in kinds:
        out["idepthmap"] = check_idepth_image(case, idm, images["idepthmap"], what, rules)
    for k, (drawn, _) in out.items():
        assert drawn > 0 or k not in case["draws"], "%s %s: the image is black: the case exercises nothing of this kind" % (what, k)
    return out


def check_read_offs(cases, images_of):
    """What the named cases are for, read off an implementation's images directly (images_of(name) -> {kind: [H,W,3]});
    the same read-offs for the C oracle and the device."""
    wire = images_of("reach")["wireframe"]
    assert not wire[12].any(), "the (-200, 12) <-> (200, 12) side is out of reach: row 12 stays black in both directions"
    assert wire[2, :21].any(1).all() and not wire[4].any(), "x = -R is in reach, its float32 predecessor is not"
    assert wire[6, 22:].any(1).all() and not wire[8].any(), "x = 2 R is in reach, its float32 successor is not"
    assert wire[:2, 26].any(1).all() and not wire[:2, 28].any(), "y = -R is in reach, its float32 predecessor is not"
    assert wire[16:, 24].any(1).all() and not wire[14:, 30].any(), "y = 2 R is in reach, its float32 successor is not"
    wire = images_of("octants")["wireframe"]
    assert wire[14:19, 0].any(1).all() and not wire[14:19, 1].any(), "x = 0.5 - 2^-25 is pixel 0"
    assert wire[8:13, 0].any(1).all(), "x = -(0.5 - 2^-25) is pixel 0"
    assert wire[0, 30:35].any(1).all() and not wire[1, 30:35].any(), "y = 0.5 - 2^-25 is pixel 0"
    c = cases["features_edge"]
    feat = images_of("features_edge")["features"]
    f = int(np.flatnonzero((c["feat_pos"] == 0).all(1))[0])    # the corner feature; the NaN positions come after it
    assert np.isnan(c["feat_pos"][f + 1:]).any()
    lo, hi, _ = D.jet(c["feat_mu"][f:f + 1] * np.float32(c["scale"]))
    img = D.features(c["W"], c["H"], c["feat_pos"], c["feat_mu"], c["scale"])
    assert img.key[0] == f and feat[0, 0].tolist() == lo[0].tolist() == hi[0].tolist(), \
        "(0, 0) belongs to the corner feature, not to a later feature at a NaN position"


class _TP:
    """The fields frame_f64.triangles reads, from a case's tp tuple."""
    def __init__(self, do_oblique_triangle_filter, oblique_normal_thresh, oblique_idepth_diff_factor, oblique_idepth_diff_abs,
                 do_edge_length_filter, edge_length_thresh, do_idepth_triangle_filter, min_triangle_idepth, width, height):
        self.__dict__.update(locals())
