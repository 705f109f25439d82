"""The warped matching window behind flame::GpuFrontEnd (include/flame/gpu_frontend.h: Params::warp_matching_window, setWarp):
tests/cpp/fe_warp_facade.cc runs three Flame + front-end pairs through flame::Flame::update() over the eight-frame roll-30 scene
(tests/fe_warp_scenes.py) -- the switch on, the defaults, and the switch on through a `track` written on the bare C ABI.  Compiled like
tests/test_gpu_fe_rg_facade.py's program (g++ -std=c++11 -Wall -Wextra -Werror, fallback types and the stand-ins).  CPU: it compiles
with both type sets, the switch works on a handle without a device, and without a device every update fails cleanly."""
import os
import struct
import subprocess

import numpy as np
import pytest

from flame_ros_amd import lib
from tests import fe_warp_scenes as WS
from tests import frontend_ref as R
from tests import frontend_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror"]
LINK = ["-L" + os.path.join(ROOT, "flame_ros_amd"), "-lflame_hip", "-Wl,-rpath," + os.path.join(ROOT, "flame_ros_amd"), "-pthread"]
STANDINS = ["-I" + os.path.join(ROOT, "tests", "cpp", "standins")]
ITERS, WIN, VAR_MAX = 20, 5, 0.01  # (Params::idepth_var_max_graph: what Flame lets into the mesh)


def quaternion(Rm):
    """(x, y, z, w) of a rotation matrix whose angle is below pi (w > 0: every pose of the scene)."""
    w = 0.5 * np.sqrt(1.0 + Rm[0, 0] + Rm[1, 1] + Rm[2, 2])
    return np.array([(Rm[2, 1] - Rm[1, 2]) / (4 * w), (Rm[0, 2] - Rm[2, 0]) / (4 * w), (Rm[1, 0] - Rm[0, 1]) / (4 * w), w], np.float32)


def sequence():
    """[(image, float32 quaternion, float32 translation, the [R|t] the facade forms from them)]"""
    out = []
    for img, T in WS.scene("roll30"):
        q, t = quaternion(T[:, :3]), T[:, 3].astype(np.float32)
        out.append((img, q, t, R.quat_pose(q, t)))
    return out


@pytest.fixture(scope="module", params=["fallback", "standins"])
def exe(request, tmp_path_factory):
    lib.load()
    out = str(tmp_path_factory.mktemp("fe_warp_facade") / ("fe_warp_facade_" + request.param))
    subprocess.check_call(CXX + (STANDINS if request.param == "standins" else []) +
                          ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "fe_warp_facade.cc"), "-o", out] + LINK)
    return out


def run(exe, tmp_path, device):
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    frames = sequence()
    with open(inp, "wb") as f:
        f.write(struct.pack("<6i", WS.W, WS.H, len(frames), device, ITERS, WIN))
        f.write(np.array(WS.K4, np.float32).tobytes())
        for k, (img, q, t, _) in enumerate(frames):
            f.write(struct.pack("<2i", 40 + k, int(k == 0)))
            f.write(q.tobytes() + t.tobytes() + np.ascontiguousarray(img).tobytes())
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
    p, rows, meshes, frames = run(exe, tmp_path, 99)
    assert p.returncode == 3, (p.returncode, p.stdout, p.stderr)
    assert "surface=1" in p.stdout, p.stdout
    assert len(rows) == len(frames) == len(meshes)
    for r in rows:
        assert r["update_w"] == r["update_d"] == r["update_p"] == "0" and int(r["hip_error"]) == lib.ERR_NODEVICE, r
        assert r["vtx_w"] == r["vtx_d"] == "0" and r["abi_same"] == "1" and r["fail_w"] == r["fail_d"] == "-1", r


@pytest.mark.gpu
def test_warped_mesh_is_the_library_calls_and_the_restatements(gpu, exe, tmp_path):
    p, rows, meshes, frames = run(exe, tmp_path, 0)
    print(p.stdout)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert "surface=1" in p.stdout and "warp_w=1 warp_d=0" in p.stdout
    assert len(rows) == len(frames) == len(meshes)
    # the restatement over the poses the facade forms, switch on and off
    want = {}
    for warp in (True, False):
        fe = R.FrontEndRef(WS.W, WS.H, WS.K, 4096, 16)
        fe.set_warp(warp)
        pr = R.params(win_size=WIN)
        want[warp] = [fe.track(pr, img, 40 + k, T, k == 0) for k, (img, _, _, T) in enumerate(frames)]
    for k, r in enumerate(rows):
        assert r["abi_same"] == "1" and r["fail_d"] == "-1" and r["update_w"] == r["update_p"], (k, r)  # W is the bare ABI's; D: key unset
        if r["update_w"] == "1":
            assert int(r["fail_w"]) == int(r["info_w"]) == 0, (k, r)  # (present while the switch is on; nothing is refused here)
            conv = want[True][k]["idepth_var"] < np.float32(VAR_MAX)
            mw = meshes[k][0]
            assert len(mw) == int(r["vtx_w"]) == int(conv.sum()), (k, r)
            rows_of = lambda a: sorted(map(tuple, np.ascontiguousarray(a, np.float32).view(np.uint32).tolist()))  # noqa: E731
            assert rows_of(mw[:, :2]) == rows_of(want[True][k]["vtx"][conv]), k  # the same vertices, bit for bit
    assert rows[-1]["update_w"] == "1"
    n_on, n_off = int(rows[-1]["vtx_w"]), int(rows[-1]["vtx_d"])
    off_conv = int((want[False][-1]["idepth_var"] < np.float32(VAR_MAX)).sum())
    print("last frame: %d vertices with the switch on, %d with it off (restatement: %d)" % (n_on, n_off, off_conv))
    assert n_on >= 25 and n_off < n_on
    if rows[-1]["update_d"] == "1":
        assert n_off == off_conv
    mw = meshes[-1][0]
    truth, _ = SC.plane_idepth(WS.K4, frames[-1][3], mw[:, 0].astype(np.float64), mw[:, 1].astype(np.float64))
    err = np.abs(mw[:, 2].astype(np.float64) - truth) / truth
    print("worst relative error of a mesh vertex: %.4f" % err.max())
    assert (err <= 0.10).all()
