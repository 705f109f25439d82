"""The gain-invariant matching cost behind flame::GpuFrontEnd (include/flame/gpu_frontend.h: Params::gain_invariant_matching,
setGainInvariant): tests/cpp/fe_gi_facade.cc runs six Flame + front-end pairs over the ten-frame halved "sideways" scene
(tests/fe_gi_scenes.py) and its gained copy (2 v + b on every frame that is no pose frame, v + |b| on the pose frames) -- the
gain-invariant cost on both, the zero-mean cost alone on both, the defaults, and the defaults through a `track` written on the bare
C ABI, a pair built without any call of a matching cost.  Compiled like tests/test_gpu_fe_zm_facade.py's program (g++ -std=c++11
-Wall -Wextra -Werror, fallback types and the stand-ins).  CPU: it compiles with both type sets, the switch works on a handle
without a device, and without a device every update fails cleanly."""
import os
import struct
import subprocess

import numpy as np
import pytest

from flame_ros_amd import lib
from tests import fe_gi_scenes as GS
from tests import fe_zm_scenes as ZS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror"]
LINK = ["-L" + os.path.join(ROOT, "flame_ros_amd"), "-lflame_hip", "-Wl,-rpath," + os.path.join(ROOT, "flame_ros_amd"), "-pthread"]
STANDINS = ["-I" + os.path.join(ROOT, "tests", "cpp", "standins")]
ITERS, FRAMES, WIN, POSEFRAMES = 20, 10, 7, (0, 5)


@pytest.fixture(scope="module", params=["fallback", "standins"])
def exe(request, tmp_path_factory):
    lib.load()
    out = str(tmp_path_factory.mktemp("fe_gi_facade") / ("fe_gi_facade_" + request.param))
    subprocess.check_call(CXX + (STANDINS if request.param == "standins" else []) +
                          ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "fe_gi_facade.cc"), "-o", out] + LINK)
    return out


def run(exe, tmp_path, device):
    inp = str(tmp_path / "in.bin")
    offsets = ZS.random_offsets(11, FRAMES)
    with open(inp, "wb") as f:
        f.write(struct.pack("<6i", ZS.W, ZS.H, FRAMES, device, ITERS, WIN))
        f.write(np.array(ZS.K4, np.float32).tobytes())
        for frames in (GS.halved("sideways", frames=FRAMES), GS.gained("sideways", frames=FRAMES, poseframes=POSEFRAMES, offsets=offsets)[0]):
            for k, (img, T) in enumerate(frames):
                yaw = np.arctan2(T[0, 2], T[0, 0])  # the scene's poses are yaw about y + translation
                q = np.array([0.0, np.sin(yaw / 2), 0.0, np.cos(yaw / 2)], np.float32)
                f.write(struct.pack("<2i", 40 + k, int(k in POSEFRAMES)))
                f.write(q.tobytes() + T[:, 3].astype(np.float32).tobytes() + np.ascontiguousarray(img).tobytes())
    p = subprocess.run([exe, inp], capture_output=True, text=True)
    rows = [dict(kv.split("=") for kv in l.split()) for l in p.stdout.splitlines() if l.startswith("frame=")]
    return p, rows


def test_the_switch_and_clean_failure_without_a_device(exe, tmp_path):
    """(device 99 exists on no machine: the same on a GPU box)"""
    p, rows = run(exe, tmp_path, 99)
    assert p.returncode == 3, (p.returncode, p.stdout, p.stderr)
    assert "surface=1" in p.stdout, p.stdout
    assert len(rows) == FRAMES
    for r in rows:
        assert r["update_g0"] == r["update_g1"] == r["update_z0"] == r["update_s0"] == r["update_p"] == "0", r
        assert int(r["hip_error"]) == lib.ERR_NODEVICE, r
        assert r["vtx_g0"] == r["vtx_s0"] == "0" and r["gi_same"] == r["plain_same"] == "1" and r["images_differ"] == "1", r


@pytest.mark.gpu
def test_gained_copy_gives_the_same_mesh_with_the_switch_and_another_with_zero_mean_alone(gpu, exe, tmp_path):
    p, rows = run(exe, tmp_path, 0)
    print(p.stdout)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert "surface=1" in p.stdout and "gi_g=1 gi_z=0 gi_s=0 cost_g=0 cost_z=1" in p.stdout and "zssd_moved=1" in p.stdout
    assert len(rows) == FRAMES
    for k, r in enumerate(rows):
        assert r["gi_same"] == "1" and r["plain_same"] == "1" and r["images_differ"] == "1", (k, r)
        assert r["update_g0"] == r["update_g1"] and r["update_s0"] == r["update_p"], (k, r)
    good = [r for r in rows if r["update_g0"] == "1"]
    assert len(good) >= 3 and all(int(r["vtx_g0"]) >= 3 for r in good)
    assert any(r["zssd_same"] == "0" for r in rows)
