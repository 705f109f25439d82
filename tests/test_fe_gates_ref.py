"""CPU: the gates' restatement tests/fe_gates_ref.py (DESIGN.md 5.3 "Gates") rule by rule on hand-built inputs, its float32 height
against the float64 geometry, its decisions against the ground truth of the plane scenes, and the C ABI's surface
(flame_hip_frontend_set_gates) on a handle without a device.  tests/test_gpu_fe_gates.py then holds the device to the restatement
bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

from flame_ros_amd import lib
from tests import fe_gates_ref as G
from tests import frontend_corpus as FC
from tests import frontend_ref as R
from tests import frontend_scenes as SC

F = np.float32
K_SMALL = np.array([50, 0, 24, 0, 50, 18, 0, 0, 1], np.float32)  # 48 x 36, the principal point on a pixel


def same_bits(a, b):
    """Two dicts of arrays (emitted features, or states) hold the same bits."""
    return all(np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                              b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]) for k in a)


# ---- 1. band arithmetic ----

def test_band_arithmetic():
    assert G.band(36) == (12, 24)   # rows 12 ... 23
    assert G.band(37) == (12, 25)   # rows 12 ... 24
    G.check_band(36, 5)
    G.check_band(37, 5)
    with pytest.raises(ValueError):
        G.check_band(8, 5)          # rows 2 ... 5: four rows, a candidate row with its windows needs seven
    ref = R.FrontEndRef(48, 8, K_SMALL, 16, 2)
    ref.set_gates(letterbox=True)
    with pytest.raises(ValueError):
        ref.track(R.params(), np.zeros((8, 48), np.uint8), 0, R.pose(), True)


# ---- 2. detection under the letterbox ----

def _spots(spots, W=48, H=36):
    img = np.full((H, W), 100, np.uint8)
    for x, y, val in spots:
        img[y, x] = val
    return img


def test_letterbox_detection_rows():
    """48 x 36, cells of 16, win 5 (m = 3): band rows 12...23.  Cell row 0 is clipped to rows 12...15, cell row 2 (rows 32...35) lies
    outside the band.  A spot of 255 at (8, 10) gives the cell's strongest gradient at rows 9...11, just outside the band; the
    weaker spot at (8, 14) gives the strongest one inside.  The spot at (24, 33) gives a gradient at (24, 32), a candidate row of
    the ungated detector (32 < H - m) in cell row 2."""
    img = _spots([(8, 10, 255), (8, 14, 130), (24, 33, 255), (40, 20, 200)])
    p = R.params()
    plain, gated = R.FrontEndRef(48, 36, K_SMALL, 32, 2), R.FrontEndRef(48, 36, K_SMALL, 32, 2)
    gated.set_gates(letterbox=True)
    o0, o1 = plain.track(p, img, 0, R.pose(), True), gated.track(p, img, 0, R.pose(), True)
    at0 = {(int(x), int(y)) for x, y in o0["vtx"]}
    at1 = {(int(x), int(y)) for x, y in o1["vtx"]}
    assert (8, 9) in at0 and (24, 32) in at0 and (40, 19) in at0
    assert at1 == {(8, 13), (40, 19)}       # the in-band maximum of cell (0, 0); cell row 1 as before; nothing in cell row 2
    assert all(12 <= y <= 23 for _, y in at1)
    # the clip of cell row 0 is rows 12...15 exactly: a spot whose gradient sits at rows 11 and 16 is seen by cell row 1 only
    img2 = _spots([(8, 17, 255)])            # gradient at (8, 16), (8, 18), (7, 17), (9, 17)
    g2 = R.FrontEndRef(48, 36, K_SMALL, 32, 2)
    g2.set_gates(letterbox=True)
    assert {(int(x), int(y)) for x, y in g2.track(p, img2, 0, R.pose(), True)["vtx"]} == {(8, 16)}
    img3 = _spots([(8, 11, 255)])            # gradient at (8, 10), (8, 12), (7, 11), (9, 11): row 12 is the band's first
    g3 = R.FrontEndRef(48, 36, K_SMALL, 32, 2)
    g3.set_gates(letterbox=True)
    assert {(int(x), int(y)) for x, y in g3.track(p, img3, 0, R.pose(), True)["vtx"]} == {(8, 12)}


# ---- 3. projection under the letterbox ----

@pytest.mark.parametrize("ty,refused", [(-0.02, True), (0.02, False)])
def test_letterbox_projection_crossing_the_last_row(ty, refused):
    """A feature at row 23 = y_hi - 1 of the 48 x 36 image, prior 0.5, fy = 50: a camera step of ty along y moves its projection to
    23 - 25 ty while the search stays shorter than 2 px (NO_PARALLAX: nothing but the projection decides the frame).  At 23.5 the
    letterbox refuses it: not emitted, one dropout, status as it was, and -- on this second pose frame -- its cell is not occupied,
    so the detector plants a new feature there.  At 22.5 it is emitted and the cell stays its own."""
    img = _spots([(8, 24, 255)])  # the band's last row carries the gradient: detection at (8, 23)
    p = R.params()
    ref = R.FrontEndRef(48, 36, K_SMALL, 32, 2)
    ref.set_gates(letterbox=True)
    o = ref.track(p, img, 0, R.pose(), True)
    assert [(int(x), int(y)) for x, y in o["vtx"]] == [(8, 23)]
    o = ref.track(p, img, 1, R.pose((0.0, ty, 0.0)), True)
    py = ref.proj_all[0][1]
    assert abs(float(py) - (23.0 - 25.0 * ty)) < 1e-4
    assert ref.status[0] == R.NO_PARALLAX and ref.alive[0]
    if refused:
        assert ref.refused == 1 and ref.drop[0] == 1
        assert list(o["slot"]) == [1] and o["status"][0] == R.NEW and tuple(o["vtx"][0]) == (8.0, 23.0)
    else:
        assert ref.refused == 0 and ref.drop[0] == 0
        assert list(o["slot"]) == [0] and o["status"][0] == R.NO_PARALLAX and ref.counts[R.NEW] == 0
    # the same frames without the letterbox: emitted either way
    plain = R.FrontEndRef(48, 36, K_SMALL, 32, 2)
    plain.track(p, img, 0, R.pose(), True)
    assert (plain.u[0], plain.v[0]) == (8, 23)
    o = plain.track(p, img, 1, R.pose((0.0, ty, 0.0)), False)
    assert 0 in o["slot"] and plain.drop[0] == 0


def test_letterbox_first_row_and_death():
    """The band's first row, and max_dropouts refusals in a row kill the feature."""
    img = _spots([(8, 11, 255)])  # detection at (8, 12)
    p = R.params(max_dropouts=1)
    ref = R.FrontEndRef(48, 36, K_SMALL, 32, 2)
    ref.set_gates(letterbox=True)
    ref.track(p, img, 0, R.pose(), True)
    assert (ref.u[0], ref.v[0]) == (8, 12)
    o = ref.track(p, img, 1, R.pose((0.0, 0.02, 0.0)), False)   # 11.5
    assert ref.refused == 1 and ref.drop[0] == 1 and ref.alive[0] and len(o["slot"]) == 0
    o = ref.track(p, img, 2, R.pose((0.0, 0.02, 0.0)), False)
    assert ref.refused == 1 and not ref.alive[0] and ref.status[0] == R.DIED and ref.counts[R.DIED] == 1


# ---- 4. the height band ----

def test_height_holder_leaves_the_emission_to_the_other_feature():
    c, p, plain, out_plain, (cell, win, lose), h = G.colliding_runs()
    assert win in out_plain["slot"] and lose not in out_plain["slot"]
    ref = R.FrontEndRef(FC.W, FC.H, c.K, FC.SLOTS, FC.RING)
    for call in c.calls[:2]:
        ref.track(p, call[1], call[4], call[2], call[3])
    ref.set_gates(min_height=h[lose], max_height=h[lose], up=(0, 1, 0))  # min_height == max_height: a band of one value
    _, img, T, is_pf, img_id = c.calls[2]
    out = ref.track(p, img, img_id, T, is_pf)
    assert win in ref.held_slots and lose in out["slot"] and win not in out["slot"]
    assert ref.held == len(ref.held_slots) >= 2 and ref.held + len(out["slot"]) <= len(ref.proj_all)
    assert all(h[s] == h[lose] for s in out["slot"])  # nothing else gets through a band of one value
    # a held feature keeps everything the tracker did: the whole state equals the ungated run's
    assert same_bits(ref.state(), plain.state())
    assert any(ref.status[s] == R.OK and ref.drop[s] == 0 for s in ref.held_slots)  # fused, counter cleared, and held
    # frame 3, a pose frame at the same pose: a cell whose only projections are held gets no detection
    _, img, T, is_pf, img_id = c.calls[3]
    assert is_pf
    out = ref.track(p, img, img_id, T, is_pf)
    dws, ncx = p["detection_win_size"], (FC.W + p["detection_win_size"] - 1) // p["detection_win_size"]
    emit_cells = {(int(y) // dws) * ncx + int(x) // dws for x, y in out["vtx"]}
    lone = ref._held_cells - emit_cells
    g2, thr, m = R.g2_image(img), R.g2_threshold(p["min_grad_mag"]), p["win_size"] // 2 + 1
    blocked = 0
    for cell in lone:
        ccx, ccy = cell % ncx, cell // ncx
        sub = g2[max(ccy * dws, m):min(ccy * dws + dws, FC.H - m), max(ccx * dws, m):min(ccx * dws + dws, FC.W - m)]
        blocked += int(sub.size > 0 and sub.max() >= thr)  # the detector would have planted a feature here
    assert blocked >= 5
    new_cells = {(int(y) // dws) * ncx + int(x) // dws for (x, y), st in zip(out["vtx"], out["status"]) if st == R.NEW}
    assert not (new_cells & ref._held_cells)


def test_nan_height_is_held():
    """idepth_init = 0 and no motion: a new feature keeps mu = 0 (NO_PARALLAX), so its inverse depth in the frame is 0; at the
    principal point's row hr . b is 0 as well and the height is 0 / 0.  It is held under the widest band there is; with a prior of
    0.5 the same feature passes."""
    img = _spots([(8, 19, 255)])  # detection at (8, 18); cy = 18
    for init, held in ((0.0, True), (0.5, False)):
        p = R.params(idepth_init=init)
        ref = R.FrontEndRef(48, 36, K_SMALL, 32, 2)
        ref.set_gates(min_height=-G.BIG, max_height=G.BIG, up=(0, 1, 0))
        ref.track(p, img, 0, R.pose(), True)
        assert (ref.u[0], ref.v[0]) == (8, 18)
        o = ref.track(p, img, 1, R.pose(), False)
        px, py, xc, _ = ref.proj_all[0]
        with np.errstate(all="ignore"):
            hgt = G.height32(ref.K4, *G.gate_record(R.pose(), (0, 1, 0)), px, py, xc)
        assert bool(np.isnan(hgt)) == held
        assert (ref.held_slots == [0] and len(o["slot"]) == 0) if held else (ref.held == 0 and list(o["slot"]) == [0])
        assert ref.status[0] == R.NO_PARALLAX and ref.drop[0] == 0


def test_no_gate_is_the_base_class():
    """Never set, set and cleared, and set with nothing switched on: FrontEndRef's results."""
    fr = SC.scene("diagonal_roll", 1)
    p = R.params()
    base = R.FrontEndRef(SC.W, SC.H, SC.K, 256, 4)
    a, b = R.FrontEndRef(SC.W, SC.H, SC.K, 256, 4), R.FrontEndRef(SC.W, SC.H, SC.K, 256, 4)
    b.set_gates(letterbox=True, max_height=0.0)
    b.set_gates()
    for k, (img, T) in enumerate(fr):
        want = base.track(p, img, k, T, k == 0)
        assert same_bits(want, a.track(p, img, k, T, k == 0)) and same_bits(want, b.track(p, img, k, T, k == 0))
        assert same_bits(base.state(), a.state()) and same_bits(base.state(), b.state())
    for bad in (dict(min_height=1.0, max_height=0.0), dict(min_height=0.0, up=(0, 0, 0)), dict(max_height=float("nan")),
                dict(min_height=0.0, up=(0, float("inf"), 0))):
        with pytest.raises(ValueError):
            a.set_gates(**bad)


# ---- 5. the float32 height against the float64 geometry ----

def test_height_arithmetic_against_float64():
    """height = n . (R K^-1 (px, py, 1) / xi + t) in float64 from the pose, against the float32 expression on the rounded record.
    Rounding count along the longest path, the one of hr0 bx: hr0 rounded from double (1), px - cx (1), / fx (1), the product (1),
    the two sums (2), the quotient (1), + h0 (1) = 8; the paths of hr2 (4) and h0 (2) are shorter.  So the error is at most
    8 x 2^-24 x M to first order, M = (|hr0 bx| + |hr1 by| + |hr2|) / |xi| + |h0|; the factor 1 + 2^-20 covers the second order
    ((1 + 2^-24)^8 - 1 < 8 x 2^-24 (1 + 2^-21))."""
    rng = np.random.default_rng(5)
    fx, fy, cx, cy = SC.K4
    K4 = tuple(F(a) for a in SC.K4)
    worst = 0.0
    for _ in range(3000):
        Rm = SC.rotation(*rng.uniform(-0.6, 0.6, 3))
        t = rng.uniform(-2, 2, 3)
        n = rng.uniform(-1, 1, 3).astype(np.float32)
        px, py = F(rng.uniform(0, SC.W - 1)), F(rng.uniform(0, SC.H - 1))
        xi = F(rng.uniform(0.02, 3.0))
        T = np.concatenate([Rm, t[:, None]], axis=1)
        hr, h0 = G.gate_record(T, n)
        got = float(G.height32(K4, hr, h0, px, py, xi))
        b = np.array([(float(px) - cx) / fx, (float(py) - cy) / fy, 1.0])
        nd = n.astype(np.float64)
        want = float(nd @ (Rm @ b / float(xi) + t))
        hrd = nd @ Rm
        M = (abs(hrd[0] * b[0]) + abs(hrd[1] * b[1]) + abs(hrd[2])) / float(xi) + abs(float(nd @ t))
        bound = 8.0 * 2.0 ** -24 * M * (1.0 + 2.0 ** -20)
        assert abs(got - want) <= bound, (got, want, bound)
        worst = max(worst, abs(got - want) / bound)
    assert 0.05 < worst <= 1.0  # (the bound is not vacuous either)


# ---- 6. ground truth ----

CONVERGED = 0.01  # Flame's variance gate (idepth_var_max_graph)


@pytest.mark.parametrize("name", list(G.BANDS))
def test_height_band_against_ground_truth(name):
    """up = (0, 1, 0): height is the world y of the plane's point.  For every converged feature (var_cur < 0.01) with an acceptable
    projection, the TRUE world point at its pixel decides what must happen, with a margin of 3 |d height / d xi| sqrt(var_cur)
    around each band edge inside which nothing is asserted."""
    lo, hi = G.BANDS[name]
    frames = SC.scene(name, 1)
    p = R.params()
    ref = R.FrontEndRef(SC.W, SC.H, SC.K, 256, 4)
    ref.set_gates(min_height=lo, max_height=hi, up=(0, 1, 0))
    lo, hi = -np.inf if lo is None else lo, np.inf if hi is None else hi
    n_conv = n_margin = n_out_held = n_in_emitted = 0
    for k, (img, T) in enumerate(frames):
        out = ref.track(p, img, k, T, k == 0)
        if k == 0:
            continue
        emitted, held = set(int(s) for s in out["slot"]), set(ref.held_slots)
        hrd = np.array([0.0, 1.0, 0.0]) @ T[:, :3]
        for s, (px, py, xc, vc) in ref.proj_all.items():
            if not ref.alive[s] or not vc < CONVERGED:
                continue
            n_conv += 1
            _, X = SC.plane_idepth(SC.K4, T, np.array(float(px)), np.array(float(py)))
            true_h = float(X[1])
            b = np.array([(float(px) - SC.K4[2]) / SC.K4[0], (float(py) - SC.K4[3]) / SC.K4[1], 1.0])
            margin = 3.0 * abs(float(hrd @ b)) / float(xc) ** 2 * math.sqrt(float(vc))
            if abs(true_h - lo) <= margin or abs(true_h - hi) <= margin:
                n_margin += 1
                continue
            if lo <= true_h <= hi:
                assert s not in held, (k, s, true_h)
                n_in_emitted += int(s in emitted)
            else:
                assert s not in emitted and s in held, (k, s, true_h)
                n_out_held += 1
            if s in emitted:
                assert lo - margin <= true_h <= hi + margin
    print("%s: converged %d, in the margin %d, outside and held %d, inside and emitted %d" % (name, n_conv, n_margin, n_out_held, n_in_emitted))
    assert n_margin <= FC.CAP * n_conv
    assert n_conv >= 100 and n_out_held >= 20 and n_in_emitted >= 20


# ---- 7. the ABI surface, on a handle without a device ----

def test_abi_surface_without_a_device():
    L = lib.load()
    assert hasattr(L, "flame_hip_frontend_set_gates")
    assert L.flame_hip_version() >= 408
    from flame_ros_amd import frontend as FE
    assert callable(FE.GpuFrontEnd.set_gates)
    W, H = 48, 36
    h = C.c_void_p()
    assert L.flame_hip_frontend_create(C.byref(h), -1, W, H, K_SMALL.ctypes.data_as(C.c_void_p), 64, 2) == 0
    try:
        def info(key):
            v = C.c_int64(-7)
            assert L.flame_hip_frontend_info(h, key, C.byref(v)) == 0
            return v.value

        def gates(letterbox=0, height=0, lo=0.0, hi=0.0, up=(0.0, -1.0, 0.0)):
            return FE.Gates(letterbox, height, lo, hi, (C.c_float * 3)(*up))
        sg = L.flame_hip_frontend_set_gates
        assert sg(None, C.byref(gates())) == lib.ERR_ARG
        assert info(b"gates") == 0 and info(b"held_height") == 0 and info(b"refused_letterbox") == 0
        assert sg(h, C.byref(gates(1, 0))) == 0 and info(b"gates") == 1
        assert sg(h, C.byref(gates(0, 1, -1.0, 2.0))) == 0 and info(b"gates") == 2
        assert sg(h, C.byref(gates(1, 1, 0.5, 0.5))) == 0 and info(b"gates") == 3
        # a refused record leaves the gates as they were
        assert sg(h, C.byref(gates(0, 1, 1.0, 0.0))) == lib.ERR_ARG
        assert sg(h, C.byref(gates(0, 1, 0.0, 1.0, (0.0, 0.0, 0.0)))) == lib.ERR_ARG
        for bad in (gates(0, 1, float("nan"), 1.0), gates(0, 1, 0.0, float("inf")), gates(1, 1, 0.0, 1.0, (0.0, float("nan"), 0.0)),
                    gates(0, 1, float("-inf"), 1.0)):
            assert sg(h, C.byref(bad)) == lib.ERR_NAN
        assert info(b"gates") == 3
        # with the height gate off its fields are not read
        assert sg(h, C.byref(gates(1, 0, float("nan"), float("nan"), (0.0, 0.0, 0.0)))) == 0 and info(b"gates") == 1
        assert sg(h, C.byref(gates(0, 0))) == 0 and info(b"gates") == 0
        assert sg(h, C.byref(gates(1, 1, 0.0, 1.0))) == 0 and sg(h, None) == 0 and info(b"gates") == 0
        # the letterbox on 48 x 36 passes the band check (NODEVICE comes after it)
        p = FE.default_frontend_params()
        img, T, n = np.zeros((H, W), np.uint8), np.ascontiguousarray(R.pose().reshape(-1)), C.c_int32()
        track = lambda: L.flame_hip_frontend_track(h, C.byref(p), img.ctypes.data_as(C.c_void_p), W, 0,  # noqa: E731
                                                   T.ctypes.data_as(C.c_void_p), 1, C.byref(n))
        assert sg(h, C.byref(gates(1, 0))) == 0 and track() == lib.ERR_NODEVICE
    finally:
        L.flame_hip_frontend_destroy(h)
    # H = 8: a band of four rows is refused at the next _track, where win is known -- and only with the letterbox on
    K8 = np.array([50, 0, 24, 0, 50, 4, 0, 0, 1], np.float32)
    with FE.GpuFrontEnd(48, 8, K8, 64, 2, device=-1) as fe:
        p, img = FE.default_frontend_params(), np.zeros((8, 48), np.uint8)
        fe.set_gates(letterbox=True)
        assert fe.info("gates") == 1
        with pytest.raises(FE.FlameHipError) as e:
            fe.track(p, img, 0, R.pose(), True)
        assert e.value.code == lib.ERR_ARG
        fe.set_gates(min_height=0.0)
        assert fe.info("gates") == 2
        with pytest.raises(FE.FlameHipError) as e:
            fe.track(p, img, 0, R.pose(), True)
        assert e.value.code == lib.ERR_NODEVICE
        fe.set_gates()
        assert fe.info("gates") == 0
        for kw, code in ((dict(min_height=1.0, max_height=0.0), lib.ERR_ARG), (dict(max_height=1.0, up=(0, 0, 0)), lib.ERR_ARG),
                         (dict(min_height=float("nan")), lib.ERR_NAN)):
            with pytest.raises(FE.FlameHipError) as e:
                fe.set_gates(**kw)
            assert e.value.code == code
