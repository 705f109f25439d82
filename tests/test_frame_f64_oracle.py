"""CPU: the C oracle's frame-results stage (rows a6, a8, a9, f1, f2, coverage) against the independent
float64 statement oracle/frame_f64.py on the adversarial corpus of tests/frame_corpus.py.  This pins the
oracle's post-solve stage as K9 (tests/test_oracle_kat.py) pins its solver; the HIP path equals the oracle
bit for bit (tests/test_gpu_parity.py) and is held against frame_f64 directly by tests/test_gpu_frame_f64.py."""
import numpy as np
import pytest

from oracle import COracle
from oracle.cbind import TriParams, coverage, depthmaps, default_params, mesh, triangles
from oracle import frame_f64 as F
from tests import frame_checks as chk
from tests.frame_corpus import corpus, filter_cases

CASES = corpus()


@pytest.fixture(scope="module")
def cases(oracle_built):
    return CASES


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_frame_stage(cases, name):
    c = cases[name]
    tp = TriParams(*c["tp"])
    x = c["x"]
    tn, tv, vn = triangles(tp, c["Kinv"], c["pos"], x, c["tris"])
    TR = chk.check_triangles(c, x, tn, tv, vn, name)
    for filtered in (False, True):
        what = "%s %s" % (name, "filtered" if filtered else "unfiltered")
        idm, dm, cl = depthmaps(c["W"], c["H"], c["pos"], x, c["tris"], tv, filtered, c["Kinv"], c["min_depth"], c["max_depth"])
        R = chk.check_raster(c, x, idm, tv.astype(bool) if filtered else None, what)
        chk.check_depth(idm, dm, what)
        chk.check_cloud(c, dm, cl, what)
        if filtered:
            chk.check_coverage(R, coverage(idm), what)
    if c["W"] >= 2 and c["H"] >= 2:
        pts, faces = mesh(c["Kinv"], c["pos"], x, vn, c["tris"], tv, c["W"], c["H"])
        chk.check_mesh(c, x, TR, pts, faces, tv, name)


@pytest.mark.parametrize("name", ["random_640x480_sparse", "idepth_specials_96x64", "offset_2m20_1241x376"])
def test_oracle_costs(cases, name):
    c = cases[name]
    rng = np.random.default_rng(3)
    V, E = len(c["x"]), len(c["edges"])
    z = np.nan_to_num(c["x"], nan=0.5, posinf=2.0).clip(-1, 2).astype(np.float32)
    x = (z + rng.normal(0, 0.05, V)).astype(np.float32)
    w1, w2 = (rng.normal(0, 1e-3, V).astype(np.float32) for _ in range(2))
    alpha, beta = rng.uniform(0.05, 1, E).astype(np.float32), rng.uniform(0.05, 1, E).astype(np.float32)
    wgt = rng.uniform(0, 3, V).astype(np.float32)
    o = COracle(c["pos"], c["edges"], alpha, beta, z, wgt)
    o.set_state(x=x, w1=w1, w2=w2)
    p = default_params()
    chk.check_costs(o.costs(p), F.costs(c["pos"], c["edges"], alpha, beta, x, w1, w2, z, wgt, p.data_factor), name)


@pytest.mark.parametrize("case", filter_cases(), ids=lambda c: c[0])
@pytest.mark.parametrize("kind", [0, 1])
def test_oracle_graph_filter(oracle_built, case, kind):
    name, x, edges = case
    V = len(x)
    o = COracle(np.zeros((V, 2)), edges, np.ones(len(edges)), np.ones(len(edges)), np.ones(V), np.ones(V))
    o.set_state(x=x)
    o.graph_filter(kind)
    chk.check_filter(x, edges, kind, o.x, "%s kind %d" % (name, kind))


def test_far_quad_is_drawn(cases):
    """Beyond 2^31 px the bounding box must still be clamped in float: the whole image is covered."""
    c = cases["far_quad_beyond_2p31"]
    tv = np.ones(2, np.uint8)
    idm = depthmaps(c["W"], c["H"], c["pos"], c["x"], c["tris"], tv, False, c["Kinv"], 0.1, 100.0)[0]
    assert not np.isnan(idm).any() and np.all(idm == np.float32(0.5))


def test_corpus_reaches_what_it_claims(cases):
    """Mean triangle area on both sides of 64 px; an 8-lane group of six > 256 px triangles; exact zeros."""
    areas = {n: c["W"] * c["H"] / len(c["tris"]) for n, c in cases.items()}
    assert min(areas.values()) < 64 <= max(areas.values())
    c = cases["lattice_37x1001_slivers"]
    T = len(c["tris"])
    box = np.ptp(c["pos"][c["tris"][T - 6:]], axis=1).prod(1)
    assert (T - 6) % 8 == 0 and np.all(box > 256)
    R = F.raster(c["W"], c["H"], c["pos"], c["x"], c["tris"])
    assert (R.margin == 0).sum() > 1000  # pixel centres exactly on edges
