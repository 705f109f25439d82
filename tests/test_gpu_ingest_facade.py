"""flame::GpuFrontEnd::setCamera (include/flame/gpu_frontend.h) behind flame::Flame::update(): tests/cpp/ingest_facade.cc runs
two Flame + GpuFrontEnd pairs over one sequence of raw (distorted) grey frames -- one with setCamera on the raw frames, one on
frames rectified on the host by include/flame_ros/image_io.h -- and compares everything Flame hands out bit for bit, the photo
keys of Params::photo_error included (FrontEnd::rectified).  Compiled like tests/test_gpu_frontend_facade.py's program
(g++ -std=c++11 -Wall -Wextra -Werror, fallback types and the stand-ins).  CPU: it compiles with both type sets and without a
device every update fails cleanly."""
import os
import struct
import subprocess

import numpy as np
import pytest

from flame_ros_amd import lib
from tests import frontend_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror"]
LINK = ["-L" + os.path.join(ROOT, "flame_ros_amd"), "-lflame_hip", "-Wl,-rpath," + os.path.join(ROOT, "flame_ros_amd"), "-pthread"]
STANDINS = ["-I" + os.path.join(ROOT, "tests", "cpp", "standins")]
ITERS = 20
D = (-0.28, 0.07, 0.0002, 0.00002, 0.0)
VAR_MAX = 1e6  # every emitted feature passes the variance gate: the first (pose) frame already commits a mesh


@pytest.fixture(scope="module", params=["fallback", "standins"])
def exe(request, tmp_path_factory):
    lib.load()
    out = str(tmp_path_factory.mktemp("ingest_facade") / ("ingest_facade_" + request.param))
    subprocess.check_call(CXX + (STANDINS if request.param == "standins" else []) +
                          ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "ingest_facade.cc"), "-o", out] + LINK)
    return out


def run(exe, tmp_path, device, photo_error, tag):
    inp = str(tmp_path / ("in_%s.bin" % tag))
    frames = SC.scene("sideways", 1)
    with open(inp, "wb") as f:
        f.write(struct.pack("<6i", SC.W, SC.H, len(frames), device, ITERS, int(photo_error)))
        f.write(np.array(list(SC.K4) + [VAR_MAX] + list(D), np.float32).tobytes())
        for k, (img, T) in enumerate(frames):
            # the scene's poses are yaw about y + translation: as the float32 quaternion SE3f carries
            yaw = np.arctan2(T[0, 2], T[0, 0])
            q = np.array([0.0, np.sin(yaw / 2), 0.0, np.cos(yaw / 2)], np.float32)
            f.write(struct.pack("<2i", 40 + k, int(k % 2 == 0)))
            f.write(q.tobytes() + T[:, 3].astype(np.float32).tobytes() + np.ascontiguousarray(img).tobytes())
    p = subprocess.run([exe, inp], capture_output=True, text=True)
    rows = [dict(kv.split("=") for kv in l.split()) for l in p.stdout.splitlines() if l.startswith("frame=")]
    return p, rows


def test_fails_cleanly_without_a_device(exe, tmp_path):
    """(device 99 exists on no machine: the same on a GPU box)"""
    p, rows = run(exe, tmp_path, 99, True, "nodev")
    assert p.returncode == 3, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.count("update=0/0 hip_error=%d" % lib.ERR_NODEVICE) == 6, p.stdout
    assert "camera=0" in p.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("photo_error", [False, True])
def test_raw_frames_give_what_host_rectified_frames_give(gpu, exe, tmp_path, photo_error):
    p, rows = run(exe, tmp_path, 0, photo_error, "photo%d" % photo_error)
    print(p.stdout)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert "camera=1 rectified_bound=1/0" in p.stdout
    assert len(rows) == 6
    for k, r in enumerate(rows):
        assert r["update"] == "1/1" and r["same"] == "1" and r["photo_same"] == "1", (k, r)
        assert int(r["vtx"]) >= 30 and int(r["valid"]) >= 10, (k, r)  # (not vacuous)
        if photo_error and k >= 1:  # from the second frame on there is a comparison frame
            assert int(r["photo_pixels"]) > 1000 and float(r["photo_total"]) > 0.0, (k, r)
        if not photo_error:
            assert int(r["photo_pixels"]) == 0
