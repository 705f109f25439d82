"""-m gpu: the HIP frame-results stage held DIRECTLY against the independent float64 statement
oracle/frame_f64.py (not against the C oracle, whose operation order the kernels share: a mistake made in
both would pass tests/test_gpu_parity.py).  Every case of tests/frame_corpus.py through the standalone
entry points (triangles, mesh, depthmaps filtered and unfiltered, graph_filter, costs, costs_masked) and
the fused frame_results (scale_back != 1, with_coverage)."""
import numpy as np
import pytest

from flame_ros_amd.regularizer import GraphRegularizer, default_params
from flame_ros_amd.lib import TriParams
from oracle import frame_f64 as F
from tests import frame_checks as chk
from tests.frame_corpus import corpus, filter_cases

pytestmark = pytest.mark.gpu

CASES = corpus()
OPTS = dict(path=1)  # the frame stage does not depend on the solver path


def handle(c, x, **kw):
    E = len(c["edges"])
    z = np.full(len(x), 0.5, np.float32)  # (upload wants finite data; the state is set right after)
    r = GraphRegularizer(c["pos"], c["edges"], np.ones(E), np.ones(E), z, np.ones(len(x)), tris=c["tris"], **OPTS, **kw)
    r.set_state(x=x, xb=x)
    return r


@pytest.mark.parametrize("name", list(CASES))
def test_frame_stage_vs_float64(gpu, name):
    c = CASES[name]
    x = c["x"]
    tp = TriParams(*c["tp"])
    with handle(c, x) as r:
        tn, tv, vn = r.triangles(c["Kinv"], tp)
        TR = chk.check_triangles(c, x, tn, tv, vn, name)
        for filtered in (False, True):
            what = "%s %s" % (name, "filtered" if filtered else "unfiltered")
            idm, dm, cl = r.depthmaps(c["Kinv"], tp, filtered=filtered, min_depth=c["min_depth"], max_depth=c["max_depth"])
            chk.check_raster(c, x, idm, tv.astype(bool) if filtered else None, what)
            chk.check_depth(idm, dm, what)
            chk.check_cloud(c, dm, cl, what)
        if c["W"] >= 2 and c["H"] >= 2:
            pts, faces = r.mesh(c["Kinv"], tp)
            chk.check_mesh(c, x, TR, pts, faces, tv, name)


def random_state(c, seed):
    rng = np.random.default_rng(seed)
    V, E = len(c["x"]), len(c["edges"])
    z = np.nan_to_num(c["x"], nan=0.5, posinf=2.0, neginf=-1.0).clip(-1, 2).astype(np.float32)
    z[np.abs(z) < 1e-30] = 0.0
    x = (z + rng.normal(0, 0.05, V)).astype(np.float32)
    w1, w2 = (rng.normal(0, 1e-3, V).astype(np.float32) for _ in range(2))
    alpha, beta = rng.uniform(0.05, 1, E).astype(np.float32), rng.uniform(0.05, 1, E).astype(np.float32)
    wgt = rng.uniform(0, 3, V).astype(np.float32)
    return z, x, w1, w2, alpha, beta, wgt


@pytest.mark.parametrize("name", ["random_752x480_dense", "offset_2m20_1241x376", "lattice_37x1001_slivers"])
def test_costs_vs_float64(gpu, name):
    c = CASES[name]
    z, x, w1, w2, alpha, beta, wgt = random_state(c, 5)
    p = default_params()
    rng = np.random.default_rng(6)
    vm, em = rng.random(len(x)) < 0.5, rng.random(len(alpha)) < 0.3
    with GraphRegularizer(c["pos"], c["edges"], alpha, beta, z, wgt, tris=c["tris"], **OPTS) as r:
        r.set_state(x=x, w1=w1, w2=w2)
        args = (c["pos"], c["edges"], alpha, beta, x, w1, w2, z, wgt, p.data_factor)
        chk.check_costs(r.costs(p), F.costs(*args), name)
        chk.check_costs(r.costs_masked(p, vmask=vm, emask=em), F.costs(*args, emask=em, vmask=vm), name + " masked")
        chk.check_costs(r.costs_masked(p, vmask=vm), F.costs(*args, vmask=vm), name + " vertex-masked")


@pytest.mark.parametrize("name", ["random_640x480_sparse", "random_752x480_dense", "lattice_752x480_backslash",
                                  "idepth_specials_96x64", "outside_1e4"])
@pytest.mark.parametrize("scale_back", [1.0, 1.25])
def test_frame_results_vs_float64(gpu, name, scale_back):
    """The fused launches (k_frame_a: triangle stage + costs + owner clear, k_frame_b: vertex normals + owner
    raster, k_raster_fill) in one call: costs before the state is scaled back, then everything after."""
    c = CASES[name]
    z, x, w1, w2, alpha, beta, wgt = random_state(c, 7)
    x = np.where(np.isfinite(c["x"]), c["x"], x).astype(np.float32) if name == "idepth_specials_96x64" else x
    p = default_params()
    tp = TriParams(*c["tp"])
    with GraphRegularizer(c["pos"], c["edges"], alpha, beta, z, wgt, tris=c["tris"], **OPTS) as r:
        r.set_state(x=x, w1=w1, w2=w2)
        s, d, xs, vn, tv, _, cov = r.frame_results(p, c["Kinv"], tp, scale_back=scale_back, with_coverage=True)
        what = "%s frame_results(scale_back=%g)" % (name, scale_back)
        chk.check_costs((s, d), F.costs(c["pos"], c["edges"], alpha, beta, x, w1, w2, z, wgt, p.data_factor), what)
        want_x = x.astype(np.float64) * scale_back
        assert np.all(chk.close(xs, want_x, F.U32 * np.abs(want_x) + 2.0 ** -150)), what + ": x times scale_back"
        tn = np.zeros((len(c["tris"]), 3), np.float32)  # (frame_results hands out no triangle normals)
        R = F.triangles(c["Kinv"], c["pos"], xs, c["tris"], chk._TP(*c["tp"]))
        tn[R["ok"]] = R["normal"][R["ok"]]
        chk.check_triangles(c, xs, tn, tv, vn, what)
        idm = r.depthmaps(c["Kinv"], tp, filtered=True, cloud=False)[0]
        Rr = chk.check_raster(c, xs, idm, tv.astype(bool), what + " filtered map")
        chk.check_coverage(Rr, cov, what)


@pytest.mark.parametrize("case", filter_cases(), ids=lambda c: c[0])
@pytest.mark.parametrize("kind", [0, 1])
def test_graph_filter_vs_float64(gpu, case, kind):
    name, x, edges = case
    V, E = len(x), len(edges)
    rng = np.random.default_rng(V)
    with GraphRegularizer(rng.uniform(0, 100, (V, 2)), edges, np.ones(E), np.ones(E), np.full(V, 0.5), np.ones(V), **OPTS) as r:
        r.set_state(x=x, xb=x)
        r.graph_filter(kind)
        got, gotb = r.download()[0], r.download_bar()[0]
    chk.check_filter(x, edges, kind, got, "%s kind %d" % (name, kind))
    assert np.array_equal(got.view(np.uint32), gotb.view(np.uint32)), name + ": x_bar is set to the filtered x"
