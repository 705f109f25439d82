"""The reference-patch gradient gate behind flame::GpuFrontEnd (include/flame/gpu_frontend.h: Params::min_epipolar_grad, setRefGrad):
tests/cpp/fe_rg_facade.cc runs three Flame + front-end pairs through flame::Flame::update() over the ten-frame half-striped
"sideways" scene (tests/fe_rg_ref.py) -- the gate at 5, the defaults, and the defaults through a `track` written on the bare C ABI,
a pair built without any call of the gate.  Compiled like tests/test_gpu_fe_zm_facade.py's program (g++ -std=c++11 -Wall -Wextra
-Werror, fallback types and the stand-ins).  CPU: it compiles with both type sets, the switch works on a handle without a device,
and without a device every update fails cleanly."""
import os
import struct
import subprocess

import numpy as np
import pytest

from flame_ros_amd import lib
from tests import fe_rg_ref as RG
from tests import fe_zm_scenes as ZS
from tests import frontend_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror"]
LINK = ["-L" + os.path.join(ROOT, "flame_ros_amd"), "-lflame_hip", "-Wl,-rpath," + os.path.join(ROOT, "flame_ros_amd"), "-pthread"]
STANDINS = ["-I" + os.path.join(ROOT, "tests", "cpp", "standins")]
ITERS, FRAMES, WIN, MIN_GRAD = 20, 10, 7, 5.0
OFF = 0.10  # the line between the gated and the ungated population (tests/test_fe_rg_ref.py)


@pytest.fixture(scope="module", params=["fallback", "standins"])
def exe(request, tmp_path_factory):
    lib.load()
    out = str(tmp_path_factory.mktemp("fe_rg_facade") / ("fe_rg_facade_" + request.param))
    subprocess.check_call(CXX + (STANDINS if request.param == "standins" else []) +
                          ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "fe_rg_facade.cc"), "-o", out] + LINK)
    return out


def run(exe, tmp_path, device):
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    frames = RG.half_striped("sideways", frames=FRAMES)
    with open(inp, "wb") as f:
        f.write(struct.pack("<6i", ZS.W, ZS.H, FRAMES, device, ITERS, WIN))
        f.write(np.array(ZS.K4 + (MIN_GRAD,), np.float32).tobytes())
        for k, (img, T) in enumerate(frames):
            yaw = np.arctan2(T[0, 2], T[0, 0])  # the scene's poses are yaw about y + translation
            q = np.array([0.0, np.sin(yaw / 2), 0.0, np.cos(yaw / 2)], np.float32)
            f.write(struct.pack("<2i", 40 + k, int(k in (0, 5))))
            f.write(q.tobytes() + T[:, 3].astype(np.float32).tobytes() + np.ascontiguousarray(img).tobytes())
    p = subprocess.run([exe, inp, outp], capture_output=True, text=True)
    rows = [dict(kv.split("=") for kv in l.split()) for l in p.stdout.splitlines() if l.startswith("frame=")]
    meshes = []
    if os.path.exists(outp):
        raw = open(outp, "rb").read()
        pos = 0
        while pos < len(raw):
            n, = struct.unpack_from("<i", raw, pos)
            meshes.append(np.frombuffer(raw, np.float32, 3 * n, pos + 4).reshape(n, 3))
            pos += 4 + 12 * n
    return p, rows, list(zip(meshes[0::2], meshes[1::2])), frames


def test_the_switch_and_clean_failure_without_a_device(exe, tmp_path):
    """(device 99 exists on no machine: the same on a GPU box)"""
    p, rows, meshes, _ = run(exe, tmp_path, 99)
    assert p.returncode == 3, (p.returncode, p.stdout, p.stderr)
    assert "surface=1" in p.stdout, p.stdout
    assert len(rows) == FRAMES == len(meshes)
    for r in rows:
        assert r["update_g"] == r["update_d"] == r["update_p"] == "0" and int(r["hip_error"]) == lib.ERR_NODEVICE, r
        assert r["vtx_g"] == r["vtx_d"] == "0" and r["plain_same"] == "1" and r["fail_g"] == r["fail_d"] == "-1", r


def off_plane(mesh, T):
    truth, _ = SC.plane_idepth(ZS.K4, T, mesh[:, 0].astype(np.float64), mesh[:, 1].astype(np.float64))
    return np.abs(mesh[:, 2].astype(np.float64) - truth) / truth


@pytest.mark.gpu
def test_gated_mesh_lies_on_the_plane_and_the_default_is_the_bare_abi(gpu, exe, tmp_path):
    p, rows, meshes, frames = run(exe, tmp_path, 0)
    print(p.stdout)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert "surface=1" in p.stdout and "gate_g=1 gate_d=0" in p.stdout
    assert len(rows) == FRAMES == len(meshes)
    for k, r in enumerate(rows):
        assert r["plain_same"] == "1" and r["fail_d"] == "-1" and r["update_d"] == r["update_p"], (k, r)  # the default: key unset, the bare ABI's mesh
        if r["update_g"] == "1":
            assert int(r["fail_g"]) == int(r["info_g"]) >= 0, (k, r)
    good = [k for k, r in enumerate(rows) if r["update_g"] == "1"]
    assert len(good) >= 3 and rows[-1]["update_g"] == "1"
    assert sum(int(rows[k]["fail_g"]) for k in good) > 0 and int(rows[-1]["fail_g"]) > 0
    worst_g = worst_d = 0.0
    for k in good:
        mg, md = meshes[k]
        assert len(mg) == int(rows[k]["vtx_g"]) >= 3
        err = off_plane(mg, frames[k][1])
        worst_g = max(worst_g, float(err.max()))
        assert (err <= OFF).all(), (k, float(err.max()))
        if len(md):
            worst_d = max(worst_d, float(off_plane(md, frames[k][1]).max()))
    print("worst relative error of a mesh vertex: gated %.4f, default %.4f" % (worst_g, worst_d))
