"""flame::Flame::getDebugImageDetections() / getDebugImageMatches() behind flame::GpuFrontEnd (FrontEnd::debugImage,
include/flame/flame.h, gpu_frontend.h): tests/cpp/fe_debug_facade.cc runs four Flame + GpuFrontEnd pairs over the six-frame
"sideways" scene -- flags on (the callback wrapped in a counter), flags on + debug_flip_images, flags off, flags on without the
callback -- and compares the getters with flame_hip_frontend_debug_image called directly on the handle.  Compiled like
tests/test_gpu_ingest_facade.py's program (g++ -std=c++11 -Wall -Wextra -Werror, fallback types and the stand-ins).  CPU: it
compiles with both type sets, and without a device every update fails cleanly and the pictures stay black."""
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


@pytest.fixture(scope="module", params=["fallback", "standins"])
def exe(request, tmp_path_factory):
    lib.load()
    out = str(tmp_path_factory.mktemp("fe_debug_facade") / ("fe_debug_facade_" + request.param))
    subprocess.check_call(CXX + (STANDINS if request.param == "standins" else []) +
                          ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "fe_debug_facade.cc"), "-o", out] + LINK)
    return out


def run(exe, tmp_path, device):
    inp = str(tmp_path / "in.bin")
    frames = SC.scene("sideways", 1)
    with open(inp, "wb") as f:
        f.write(struct.pack("<5i", SC.W, SC.H, len(frames), device, ITERS))
        f.write(np.array(list(SC.K4), np.float32).tobytes())
        for k, (img, T) in enumerate(frames):
            yaw = np.arctan2(T[0, 2], T[0, 0])  # the scene's poses are yaw about y + translation
            q = np.array([0.0, np.sin(yaw / 2), 0.0, np.cos(yaw / 2)], np.float32)
            f.write(struct.pack("<2i", 40 + k, int(k == 0)))
            f.write(q.tobytes() + T[:, 3].astype(np.float32).tobytes() + np.ascontiguousarray(img).tobytes())
    p = subprocess.run([exe, inp], capture_output=True, text=True)
    rows = [dict(kv.split("=") for kv in l.split()) for l in p.stdout.splitlines() if l.startswith("frame=")]
    return p, rows


def test_fails_cleanly_without_a_device(exe, tmp_path):
    """(device 99 exists on no machine: the same on a GPU box)"""
    p, rows = run(exe, tmp_path, 99)
    assert p.returncode == 3, (p.returncode, p.stdout, p.stderr)
    assert "callback_bound=1" in p.stdout and "before=1" in p.stdout
    assert len(rows) == 6
    for r in rows:
        assert r["update"] == "0" and int(r["hip_error"]) == lib.ERR_NODEVICE and r["direct"] == "0", r
        assert r["black_a"] == r["black_off"] == r["black_nocb"] == "1", r


@pytest.mark.gpu
def test_getters_equal_the_library_call(gpu, exe, tmp_path):
    p, rows = run(exe, tmp_path, 0)
    print(p.stdout)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert "callback_bound=1" in p.stdout and "before=1" in p.stdout
    assert len(rows) == 6
    for k, r in enumerate(rows):
        assert r["direct"] == r["matches_same"] == r["detections_same"] == r["cached"] == r["flip_same"] == "1", (k, r)
        assert r["renders"] == "2" and r["black_off"] == r["black_nocb"] == "1" and r["black_a"] == "0", (k, r)
        # frames 0-3 fail at the default variance gate and are drawn all the same (frame 0, the pose frame, searched nothing)
        assert r["update"] == ("0" if k < 4 else "1"), (k, r)
        assert int(r["coloured_detections"]) >= 9 * 30 and (int(r["coloured_matches"]) >= 100) == (k > 0), (k, r)
    assert int(rows[-1]["vtx"]) >= 30
