"""-m gpu: a dataset-format sequence through image -> GPU tracker -> mesh: tools/flame_offline_lite.cc with --gpu-frontend
(the features come from flame::GpuFrontEnd instead of the depth stand-in) and --debug-images (the Detections / Matches pictures
of every frame as PPM files).  The ten-frame "sideways" scene is written as a TUM-format sequence (8-bit grey PNGs, 16-bit depth
PNGs of the plane, frame RDF); the restatement (tests/fe_debug_ref.py) is fed the same pixels and the poses read back from the
frame lines, and must give the frame line's feature counts and, byte for byte, the pictures."""
import os
import subprocess

import numpy as np
import pytest

from tests import fe_debug_ref as D
from tests import frontend_ref as R
from tests import frontend_scenes as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, ITERS, VAR_MAX = 10, 20, 0.01  # (0.01: Params::idepth_var_max_graph, cfg/flame_offline_tum.yaml:92)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("folf") / "flame_offline_lite")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "flame_offline_lite.cc"), "-o", out,
                           "-L" + os.path.join(ROOT, "flame_ros_amd"), "-lflame_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "flame_ros_amd"), "-pthread"])
    return out


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    PIL = pytest.importorskip("PIL.Image")
    seq = tmp_path_factory.mktemp("seq")
    (seq / "rgb").mkdir()
    (seq / "depth").mkdir()
    yy, xx = np.mgrid[0:SC.H, 0:SC.W].astype(np.float64)
    lines = ["# the sideways scene"]
    frames = SC.scene("sideways", 1, frames=FRAMES)
    for k, (img, T) in enumerate(frames):
        idepth, _ = SC.plane_idepth(SC.K4, T, xx, yy)
        PIL.fromarray(np.ascontiguousarray(img), mode="L").save(str(seq / "rgb" / ("%d.png" % k)))  # (toGray8 passes 8-bit grey through)
        PIL.fromarray(np.round(5000.0 / idepth).astype(np.uint16)).save(str(seq / "depth" / ("%d.png" % k)))
        yaw = np.arctan2(T[0, 2], T[0, 0])  # the scene's poses are yaw about y + translation
        t = 1305031102.175304 + 0.033 * k
        lines.append("%.6f %.12f %.12f %.12f 0 %.12f 0 %.12f %.6f rgb/%d.png %.6f depth/%d.png" % (
            t, T[0, 3], T[1, 3], T[2, 3], np.sin(yaw / 2), np.cos(yaw / 2), t, k, t, k))
    (seq / "index.txt").write_text("\n".join(lines) + "\n")
    return seq, frames


def rows_of(stdout):
    out = []
    for l in stdout.splitlines():
        if not l.startswith("frame "):
            continue
        tok = l.split()
        i, j = tok.index("pose_t"), tok.index("pose_q")
        r = dict(zip(tok[0:i:2], tok[1:i:2]))
        r["pose_t"] = [float(x) for x in tok[i + 1:i + 4]]
        r["pose_q"] = [float(x) for x in tok[j + 1:j + 5]]
        out.append(r)
    return out


def args(seq):
    return [str(seq / "index.txt"), "RDF"] + [str(a) for a in SC.K4] + [str(ITERS)]


def read_ppm(path):
    raw = open(path, "rb").read()
    head = raw.split(b"\n", 3)
    assert head[0] == b"P6" and head[2] == b"255", head[:3]
    w, h = (int(a) for a in head[1].split())
    assert len(head[3]) == 3 * w * h
    return np.frombuffer(head[3], np.uint8).reshape(h, w, 3)


def test_sequence_through_the_gpu_tracker(gpu, exe, sequence, tmp_path):
    seq, frames = sequence
    dbg = tmp_path / "dbg"
    dbg.mkdir()
    p = subprocess.run([exe] + args(seq) + ["--gpu-frontend", "--debug-images", str(dbg)], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 3, (p.returncode, p.stdout, p.stderr)  # (the first frames fail: nothing is under the variance gate yet)
    rows = rows_of(p.stdout)
    assert len(rows) == FRAMES
    ref = R.FrontEndRef(SC.W, SC.H, np.array(SC.K, np.float32), 4096, 16)  # flame::GpuFrontEnd's slots and ring
    pr = R.params()
    oks = []
    for k, (r, (img, _)) in enumerate(zip(rows, frames)):
        assert int(r["frame"]) == k
        T = R.quat_pose(r["pose_q"], r["pose_t"])  # (printed with %.9g: the float32 pose update() got)
        o = ref.track(pr, img, k, T, k % 10 == 0)
        gated = int((o["idepth_var"] < np.float32(VAR_MAX)).sum())
        assert int(r["feats"]) == len(o["slot"]), (k, r)
        assert int(r["ok"]) == int(gated >= 3), (k, r, gated)
        if int(r["ok"]):
            assert int(r["vtx"]) == gated and int(r["hip_error"]) == 0 and int(r["tris"]) > gated, (k, r)
            assert 0.0 < float(r["rms_vs_truth"]) < 0.2, (k, r)  # (the depth image scores the mesh: every gated feature claims sigma < 0.1)
        oks.append(int(r["ok"]))
        for kind, name in ((D.IMG_MATCHES, "matches"), (D.IMG_DETECTIONS, "detections")):
            got = read_ppm(str(dbg / ("%s_%d.ppm" % (name, k))))
            want = ref.debug_image(kind)[:, :, ::-1]  # BGR -> RGB
            assert got.shape == want.shape and np.array_equal(got, want), "frame %d %s: %d pixels differ" % (
                k, name, (got != want).any(axis=2).sum())
        if k >= 1:
            assert (ref.debug_image(D.IMG_MATCHES) == np.array(D.GREEN, np.uint8)).all(axis=2).sum() >= 100
    assert oks[0] == 0 and oks[-1] == 1 and sum(oks) >= 3, oks  # (re-derived above, not vacuous: both kinds of frame occur)


def test_without_the_flag_the_depth_stand_in_runs_as_before(gpu, exe, sequence):
    seq, _ = sequence
    runs = []
    for _ in range(2):
        p = subprocess.run([exe] + args(seq), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
        rows = rows_of(p.stdout)
        assert len(rows) == FRAMES
        for r in rows:  # one feature per 16 x 16 cell with a depth measurement: every cell here, all through the gate
            assert r["ok"] == "1" and int(r["feats"]) == int(r["vtx"]) == (SC.W // 16) * (SC.H // 16), r
            assert float(r["rms_vs_truth"]) < 0.03 and "photo_total" not in r, r
            r.pop("update_ms")
        runs.append(rows)
    assert runs[0] == runs[1]


def test_usage_errors(gpu, exe, sequence, tmp_path):
    seq, _ = sequence
    for flags in (["--debug-images", str(tmp_path)], ["--gpu-frontend", "--dump", str(tmp_path)]):
        p = subprocess.run([exe] + args(seq) + flags, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "usage" in p.stderr and p.stdout == "", (flags, p.returncode, p.stderr)
