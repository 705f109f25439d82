"""flame::GpuFrontEnd (include/flame/gpu_frontend.h) behind flame::Flame::update(time, id, pose, img, is_poseframe), compiled
like tests/test_facade.py's programs (g++ -std=c++11 -Wall -Wextra -Werror) with the fallback types and with the cv:: / Eigen:: /
Sophus:: stand-ins.  CPU: it compiles, the header is self-contained, and without a GPU every update fails cleanly.  GPU: the
slanted-plane scene of tests/frontend_ref.py runs through the plain update() overload and what Flame hands out equals the
restatement bit for bit."""
import os
import struct
import subprocess

import numpy as np
import pytest

from flame_ros_amd import lib
from tests import frontend_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror"]
LINK = ["-L" + os.path.join(ROOT, "flame_ros_amd"), "-lflame_hip", "-Wl,-rpath," + os.path.join(ROOT, "flame_ros_amd"), "-pthread"]
STANDINS = ["-I" + os.path.join(ROOT, "tests", "cpp", "standins")]
ITERS = 20


def have_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.fixture(scope="module", params=["fallback", "standins"])
def exe(request, tmp_path_factory):
    lib.load()
    out = str(tmp_path_factory.mktemp("gpu_frontend") / ("gpu_frontend_" + request.param))
    subprocess.check_call(CXX + (STANDINS if request.param == "standins" else []) +
                          ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "gpu_frontend.cc"), "-o", out] + LINK)
    return out


def scene():
    """Scene (b) with the poses as float32 quaternion + translation (what SE3f carries)."""
    frames = []
    for k, (img, _) in enumerate(R.plane_scene(1)):
        q = np.array([0.0, np.sin(0.002 * k), 0.0, np.cos(0.002 * k)], np.float32)  # yaw 0.004 k about y
        t = np.array([0.03 * k, 0.0, 0.0], np.float32)
        frames.append((img, q, t))
    return frames


def write_input(path, frames, device=0):
    with open(path, "wb") as f:
        f.write(struct.pack("<5i", R.SCENE_W, R.SCENE_H, len(frames), device, ITERS))
        f.write(np.array([R.SCENE_K[0], R.SCENE_K[4], R.SCENE_K[2], R.SCENE_K[5]], np.float32).tobytes())
        for k, (img, q, t) in enumerate(frames):
            f.write(struct.pack("<2i", 40 + k, int(k == 0)))
            f.write(q.tobytes() + t.tobytes() + img.tobytes())


def test_header_is_self_contained(tmp_path):
    src = tmp_path / "t.cc"
    src.write_text("#include <flame/gpu_frontend.h>\nint main() { return 0; }\n")
    for extra in ([], STANDINS):
        subprocess.check_call(CXX + extra + ["-I" + os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])


def test_fails_cleanly_without_gpu(exe, tmp_path):
    if have_gpu():
        pytest.skip("GPU present: covered by the gpu test")
    inp = str(tmp_path / "in.bin")
    write_input(inp, scene()[:2])
    p = subprocess.run([exe, inp, str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert p.returncode == 3, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.count("update=0 hip_error=%d" % lib.ERR_NODEVICE) == 2, p.stdout


@pytest.fixture(scope="module")
def restated():
    """The restatement over the scene with the facade's defaults (4 096 slots, ring of 16), once for both builds."""
    fe = R.FrontEndRef(R.SCENE_W, R.SCENE_H, R.SCENE_K, 4096, 16)
    return [fe.track(R.params(), img, 40 + k, R.quat_pose(q, t), k == 0) for k, (img, q, t) in enumerate(scene())]


@pytest.mark.gpu
def test_update_from_images_matches_the_restatement(gpu, exe, restated, tmp_path):
    frames = scene()
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_input(inp, frames)
    p = subprocess.run([exe, inp, outp], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    lines = p.stdout.strip().splitlines()
    assert len(lines) == len(frames)
    raw = open(outp, "rb").read()
    off, seen_true = 0, False
    for k, want in enumerate(restated):
        gate = want["idepth_var"] < np.float32(0.01)
        expect = len(want["slot"]) >= 3 and int(gate.sum()) >= 3
        # the first frames may fail: every feature is above the variance gate; from the frame at which three or more pass
        # the update succeeds
        assert ("update=%d" % int(expect)) in lines[k], (k, lines[k], int(gate.sum()))
        if not expect:
            assert not seen_true
            continue
        seen_true = True
        fk, n_raw, n_vtx = struct.unpack_from("<3i", raw, off)
        off += 12
        assert (fk, n_raw, n_vtx) == (k, len(want["slot"]), int(gate.sum()))
        take = lambda n: np.frombuffer(raw, np.float32, n, off)  # noqa: E731
        rv = take(2 * n_raw).reshape(-1, 2); off += 8 * n_raw
        mu = take(n_raw); off += 4 * n_raw
        var = take(n_raw); off += 4 * n_raw
        vtx = take(2 * n_vtx).reshape(-1, 2); off += 8 * n_vtx
        idepths = take(n_vtx); off += 4 * n_vtx
        for name, g, w in (("raw vtx", rv, want["vtx"]), ("raw mu", mu, want["idepth_mu"]), ("raw var", var, want["idepth_var"]),
                           ("mesh vtx", vtx, want["vtx"][gate])):
            assert np.array_equal(g.view(np.uint32), np.ascontiguousarray(w).view(np.uint32)), (k, name)
        assert np.isfinite(idepths).all() and "tris=0" not in lines[k]  # getInverseDepthMesh is non-empty
    assert seen_true and off == len(raw)
