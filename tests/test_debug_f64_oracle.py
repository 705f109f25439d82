"""CPU: the C oracle's four mesh debug images (nltgv2_debug_image) against the independent statement
oracle/debug_f64.py on the corpus of tests/debug_corpus.py, and the proof that the corpus tells the stated rules
from their nearest wrong versions.  The HIP kernels are held against the same statement by
tests/test_gpu_debug_f64.py."""
import numpy as np
import pytest

from oracle import debug_f64 as D
from oracle.cbind import TriParams, debug_image, depthmaps, triangles
from tests import frame_checks as chk
from tests.debug_corpus import HALF_PRED, corpus, jet_values

CASES = corpus()
_RENDERED = {}


def rendered(name):
    """The oracle's triangle stage, filtered map and four images of a case, computed once."""
    if name not in _RENDERED:
        c = CASES[name]
        tp = TriParams(*c["tp"])
        _, tv, vn = triangles(tp, c["Kinv"], c["pos"], c["x"], c["tris"])
        idm = depthmaps(c["W"], c["H"], c["pos"], c["x"], c["tris"], tv, True, c["Kinv"], c["min_depth"], c["max_depth"])[0]
        imgs = {k: debug_image(i, c["W"], c["H"], c["scale"], c["pos"], c["x"], c["tris"], tv, vn, idm, c["feat_pos"], c["feat_mu"])
                for i, k in enumerate(chk.KINDS)}
        _RENDERED[name] = (tv, vn, idm, imgs)
    return _RENDERED[name]


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_debug_images(oracle_built, name):
    c = CASES[name]
    tv, vn, idm, imgs = rendered(name)
    shares = chk.check_debug_images(c, c["x"], tv, vn, idm, imgs, name)
    print("%s uncertain shares: %s" % (name, {k: "%d/%d" % (u, d) for k, (d, u) in shares.items()}))


def test_jet_array_equals_exact_rationals():
    """The array colour map against jet_exact (fractions.Fraction) on the breakpoints, their float32 neighbours, the
    named specials and a dyadic sweep; and the named colours themselves."""
    for scale in (1.0, 0.5, 0.7):
        with np.errstate(invalid="ignore", over="ignore"):
            p = (jet_values(scale) * np.float32(scale)).astype(np.float32)
        # which of the 24 listed values are held byte for byte, and which to two levels (tests/debug_corpus.py _jet_table):
        # the predecessor of t = 1 (index 15) is inside the band at every scale, the idepth 2.0 (index 19) at scale 0.7
        assert np.flatnonzero(~D.jet(p)[2]).tolist() == ([15, 19] if scale == 0.7 else [15]), scale
        p = np.concatenate([p, (np.arange(-8, 530) / 256.0).astype(np.float32)])
        lo, hi, certain = D.jet(p)
        for k, v in enumerate(p):
            want = D.jet_exact(v)
            assert all(lo[k, c] <= want[c] <= hi[k, c] for c in range(3)), (scale, float(v), want, lo[k], hi[k])
            if certain[k]:
                assert tuple(lo[k]) == want
    assert certain[-538:].all()   # the dyadic sweep is exact in float32: an empty band
    top, bottom = (0, 0, 128), (128, 0, 0)
    for v, want in ((np.nan, top), (np.inf, top), (2.5, top), (2.0, top), (-np.inf, bottom), (-1.0, bottom), (0.0, bottom),
                    (0.25, (255, 0, 0)), (0.75, (255, 255, 0)), (1.0, (128, 255, 128)), (1.25, (0, 255, 255)), (1.75, (0, 0, 255))):
        assert D.jet_exact(v) == want, (v, D.jet_exact(v))


def test_pixel_is_half_away_from_zero():
    v = np.array([0.5, HALF_PRED, -0.5, -HALF_PRED, 1.5, -1.5, 2.5, np.nextafter(np.float32(7.5), np.float32(0)), 7.5, -0.0,
                  0.49999997, 8388607.5, -8388607.5], np.float32)
    assert D.pixel(v).tolist() == [1, 0, -1, 0, 2, -2, 3, 7, 8, 0, 0, 8388608, -8388608]
    assert D.in_reach(np.array([-56, np.nextafter(np.float32(-56), np.float32(-99)), 112, np.nextafter(np.float32(112), np.float32(999)),
                                np.nan, np.inf, -3e9], np.float32), 32, 24).tolist() == [True, False, True, False, False, False, False]


def test_bresenham_known_walks():
    # worked by hand from the rule (slope 1/2: e2 == dx ties step y; slope 2: e2 == dy ties step x): a tie steps, so the
    # walk depends on the end it starts from
    assert D.bresenham(0, 0, 4, 2) == [(0, 0), (1, 1), (2, 1), (3, 2), (4, 2)]
    assert D.bresenham(4, 2, 0, 0) == [(4, 2), (3, 1), (2, 1), (1, 0), (0, 0)]
    assert D.bresenham(0, 0, 2, 4) == [(0, 0), (1, 1), (1, 2), (2, 3), (2, 4)]
    assert D.bresenham(3, 3, 3, 3) == [(3, 3)]
    assert D.bresenham(0, 0, -3, 3) == [(0, 0), (-1, 1), (-2, 2), (-3, 3)]
    assert len(D.bresenham(-56, -56, 112, 0)) == 169   # in reach a walk has at most 3 R + 1 pixels (R = 56)


def test_reach_and_edges_read_as_stated(oracle_built):
    """What the issue's cases are for, read off the oracle's images directly."""
    chk.check_read_offs(CASES, lambda name: rendered(name)[3])


def test_far_flag_means_out_of_reach():
    for name, c in CASES.items():
        used = np.unique(c["tris"])
        out = ~D.in_reach(c["pos"][used], c["W"], c["H"]).all()
        assert bool(c["far"]) == bool(out), name


MUTANTS = [
    ("floor(v + 0.5) for negatives", dict(rounding="floor"), "octants", "wireframe"),
    ("floor(v + 0.5) for negatives", dict(rounding="floor"), "features_edge", "features"),
    ("float32 v + 0.5f", dict(rounding="f32"), "octants", "wireframe"),
    ("float32 v + 0.5f", dict(rounding="f32"), "features_edge", "features"),
    ("lowest index wins", dict(winner="lowest"), "lattice_soup_both_diagonals", "wireframe"),
    ("lowest index wins", dict(winner="lowest"), "overwrite_fan", "wireframe"),
    ("lowest index wins", dict(winner="lowest"), "features_edge", "features"),
    ("colour from x_a alone", dict(side_colour="a"), "octants", "wireframe"),
    ("colour from x_a alone", dict(side_colour="a"), "mesh_86_triangles", "wireframe"),
    ("4 (W + H) truncation instead of the reach", dict(reach=False), "reach", "wireframe"),
    ("e2 > dy", dict(tie=">"), "octants", "wireframe"),
    ("blue breakpoint moved by one level", dict(blue_shift=1), "jet_table_scale_1", "features"),
    ("blue breakpoint moved by one level", dict(blue_shift=-1), "jet_table_scale_0.7", "features"),
    ("NaN colour black", dict(nan_colour="black"), "jet_table_scale_0.5", "features"),
    ("NaN colour black", dict(nan_colour="black"), "idepth_specials_tilted_96x64", "features"),
    ("B and R swapped", dict(normals_order=(0, 1, 2)), "octants", "normals"),
    ("B and R swapped", dict(normals_order=(0, 1, 2)), "overwrite_fan", "normals"),
]


@pytest.mark.parametrize("what,rule,name,kind", MUTANTS, ids=["%s:%s:%s" % (m[1], m[2], m[3]) for m in MUTANTS])
def test_corpus_tells_the_rules_from_their_mutants(oracle_built, what, rule, name, kind):
    """Each wrong version of the STATEMENT must disagree with the oracle's image of a named case pixel by pixel (the
    stated version agrees: test_oracle_debug_images)."""
    c = CASES[name]
    tv, vn, idm, imgs = rendered(name)
    with pytest.raises(AssertionError, match="differ from the statement|draws nothing|matches no candidate owner"):
        chk.check_debug_images(c, c["x"], tv, vn, idm, imgs, name, kinds=(kind,), rules=D.Rules(**rule))
