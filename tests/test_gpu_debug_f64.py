"""-m gpu: the four mesh debug images of flame_hip_debug_image (k_dbg_lines, k_dbg_wire_color, k_dbg_feat_mark,
k_dbg_feat_color, k_dbg_idm_color, k_dbg_normals) held DIRECTLY against the independent statement oracle/debug_f64.py
on the corpus of tests/debug_corpus.py -- not against the C oracle, whose expressions the kernels share
(tests/test_gpu_debug_images.py keeps that byte comparison).  The checks take the handle's own tri_valid, vertex
normals and filtered dense map; each image is rendered twice and must repeat byte for byte, and the dense map must
read the same afterwards."""
import numpy as np
import pytest

from flame_ros_amd import lib
from flame_ros_amd.lib import TriParams
from flame_ros_amd.regularizer import GraphRegularizer
from tests import frame_checks as chk
from tests.debug_corpus import corpus

pytestmark = pytest.mark.gpu

CASES = corpus()
OPTS = dict(path=1)  # as tests/test_gpu_frame_f64.py: the frame stage does not depend on the solver path
KIND_IDS = dict(wireframe=lib.IMG_WIREFRAME, features=lib.IMG_FEATURES, normals=lib.IMG_NORMALS, idepthmap=lib.IMG_IDEPTHMAP)
_RENDERED = {}


def rendered(name):
    """The device's triangle stage, filtered map and four images of a case (each rendered twice), once per session."""
    if name in _RENDERED:
        return _RENDERED[name]
    c = CASES[name]
    x, E = c["x"], len(c["edges"])
    tp = TriParams(*c["tp"])
    z = np.full(len(x), 0.5, np.float32)  # (upload wants finite data; the state is set right after)
    with GraphRegularizer(c["pos"], c["edges"], np.ones(E), np.ones(E), z, np.ones(len(x)), tris=c["tris"], **OPTS) as r:
        r.set_state(x=x, xb=x)
        _, tv, vn = r.triangles(c["Kinv"], tp)
        idm = r.depthmaps(c["Kinv"], tp, filtered=True, cloud=False)[0]
        imgs = {}
        for k, kind in KIND_IDS.items():
            imgs[k] = r.debug_image(kind, c["Kinv"], tp, c["scale"], c["feat_pos"], c["feat_mu"])
            again = r.debug_image(kind, c["Kinv"], tp, c["scale"], c["feat_pos"], c["feat_mu"])
            assert np.array_equal(imgs[k], again), "%s %s: the second render differs from the first" % (name, k)
        idm2 = r.depthmaps(c["Kinv"], tp, filtered=True, cloud=False)[0]
        assert np.array_equal(idm.view(np.uint32), idm2.view(np.uint32)), name + ": the dense map changed under the images"
    _RENDERED[name] = (tv, vn, idm, imgs)
    return _RENDERED[name]


@pytest.mark.parametrize("name", list(CASES))
def test_debug_images_vs_statement(gpu, name):
    c = CASES[name]
    tv, vn, idm, imgs = rendered(name)
    R = chk.check_raster(c, c["x"], idm, tv.astype(bool), name + " filtered map")  # (the map the images are judged with)
    chk.check_debug_images(c, c["x"], tv, vn, idm, imgs, name, R=R)


def test_reach_and_edges_read_as_stated(gpu):
    """The named read-offs of tests/test_debug_f64_oracle.py, on the device's images."""
    chk.check_read_offs(CASES, lambda name: rendered(name)[3])
