"""The front end's gates behind flame::GpuFrontEnd (include/flame/gpu_frontend.h: Params::do_letterbox, min_height / max_height,
setUpAxis / setGates): tests/cpp/fe_gates_facade.cc runs three Flame + front-end pairs over the ten-frame "sideways" scene -- gated
(letterbox + a finite min_height), ungated, and ungated through a `track` written on the bare C ABI, a pair built without any call
of the gates.  Compiled like tests/test_gpu_fe_debug_facade.py's program (g++ -std=c++11 -Wall -Wextra -Werror, fallback types and
the stand-ins).  CPU: it compiles with both type sets, a refused gate record lands in lastError() and fails track() on a handle
without a device, and without a device every update fails cleanly."""
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
FRAMES = 10
MIN_HEIGHT = -0.05  # up = (0, -1, 0): the world points with y <= 0.05 stay, the lower half of the plane's image is held


@pytest.fixture(scope="module", params=["fallback", "standins"])
def exe(request, tmp_path_factory):
    lib.load()
    out = str(tmp_path_factory.mktemp("fe_gates_facade") / ("fe_gates_facade_" + request.param))
    subprocess.check_call(CXX + (STANDINS if request.param == "standins" else []) +
                          ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "fe_gates_facade.cc"), "-o", out] + LINK)
    return out


def run(exe, tmp_path, device):
    inp = str(tmp_path / "in.bin")
    frames = SC.scene("sideways", 1, frames=FRAMES)
    with open(inp, "wb") as f:
        f.write(struct.pack("<5i", SC.W, SC.H, len(frames), device, ITERS))
        f.write(np.array(list(SC.K4) + [MIN_HEIGHT], np.float32).tobytes())
        for k, (img, T) in enumerate(frames):
            yaw = np.arctan2(T[0, 2], T[0, 0])  # the scene's poses are yaw about y + translation
            q = np.array([0.0, np.sin(yaw / 2), 0.0, np.cos(yaw / 2)], np.float32)
            f.write(struct.pack("<2i", 40 + k, int(k in (0, 5))))
            f.write(q.tobytes() + T[:, 3].astype(np.float32).tobytes() + np.ascontiguousarray(img).tobytes())
    p = subprocess.run([exe, inp], capture_output=True, text=True)
    rows = [dict(kv.split("=") for kv in l.split()) for l in p.stdout.splitlines() if l.startswith("frame=")]
    return p, rows


def test_refused_record_and_clean_failure_without_a_device(exe, tmp_path):
    """(device 99 exists on no machine: the same on a GPU box)"""
    p, rows = run(exe, tmp_path, 99)
    assert p.returncode == 3, (p.returncode, p.stdout, p.stderr)
    assert "refused=1" in p.stdout, p.stdout
    assert len(rows) == FRAMES
    for r in rows:
        assert r["update_g"] == r["update_u"] == r["update_p"] == "0" and int(r["hip_error"]) == lib.ERR_NODEVICE, r
        assert r["vtx_g"] == r["vtx_u"] == "0" and r["mesh_same"] == "1", r


@pytest.mark.gpu
def test_gated_mesh_lies_in_the_band_and_ungated_mesh_is_unchanged(gpu, exe, tmp_path):
    p, rows = run(exe, tmp_path, 0)
    print(p.stdout)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert "refused=1" in p.stdout and "gates_g=3 gates_u=0" in p.stdout
    assert len(rows) == FRAMES
    for k, r in enumerate(rows):
        assert r["in_band"] == "1" and r["mesh_same"] == "1" and r["held_u"] == "0", (k, r)
        assert r["update_u"] == r["update_p"], (k, r)
    good = [r for r in rows if r["update_g"] == "1" and r["update_u"] == "1"]
    assert len(good) >= 3
    for r in good:
        assert 3 <= int(r["vtx_g"]) < int(r["vtx_u"]) and r["u_outside"] == "1", r
    assert max(int(r["held"]) for r in rows) > 0 and int(rows[-1]["held"]) > 0
