"""The hand-over behind flame::GpuFrontEnd (include/flame/gpu_frontend.h: Params::carry_features, setCarry):
tests/cpp/fe_carry_facade.cc runs three Flame + front-end pairs with a pose-frame ring of 2 through flame::Flame::update() over
twenty frames of the hovering sequence (tests/fe_carry_ref.py), a pose frame every 3rd frame -- the switch on, the defaults, and the
switch on through a `track` written on the bare C ABI.  Compiled like tests/test_gpu_fe_warp_facade.py's program (g++ -std=c++11
-Wall -Wextra -Werror, fallback types and the stand-ins).  CPU: it compiles with both type sets, the switch works on a handle
without a device, and without a device every update fails cleanly."""
import os
import struct
import subprocess

import numpy as np
import pytest

from flame_ros_amd import lib
from tests import fe_carry_ref as CR
from tests import frontend_ref as R
from tests.test_gpu_fe_warp_facade import CXX, LINK, ROOT, STANDINS, quaternion

ITERS, RING, EVERY, FRAMES = 20, 2, 3, 20
K4 = (float(R.SCENE_K[0]), float(R.SCENE_K[4]), float(R.SCENE_K[2]), float(R.SCENE_K[5]))


def sequence():
    """[(image, float32 quaternion, float32 translation, the [R|t] the facade forms from them)]"""
    out = []
    for img, T in CR.hover_scene(1, FRAMES):
        q, t = quaternion(T[:, :3]), T[:, 3].astype(np.float32)
        out.append((img, q, t, R.quat_pose(q, t)))
    return out


@pytest.fixture(scope="module", params=["fallback", "standins"])
def exe(request, tmp_path_factory):
    lib.load()
    out = str(tmp_path_factory.mktemp("fe_carry_facade") / ("fe_carry_facade_" + request.param))
    subprocess.check_call(CXX + (STANDINS if request.param == "standins" else []) +
                          ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "fe_carry_facade.cc"), "-o", out] + LINK)
    return out


def run(exe, tmp_path, device):
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    frames = sequence()
    with open(inp, "wb") as f:
        f.write(struct.pack("<6i", R.SCENE_W, R.SCENE_H, len(frames), device, ITERS, RING))
        f.write(np.array(K4, np.float32).tobytes())
        for k, (img, q, t, _) in enumerate(frames):
            f.write(struct.pack("<2i", 40 + k, int(k % EVERY == 0)))
            f.write(q.tobytes() + t.tobytes() + np.ascontiguousarray(img).tobytes())
    p = subprocess.run([exe, inp, outp], capture_output=True, text=True)
    rows = [dict(kv.split("=") for kv in l.split()) for l in p.stdout.splitlines() if l.startswith("frame=")]
    return p, rows, frames


def test_the_switch_and_clean_failure_without_a_device(exe, tmp_path):
    """(device 99 exists on no machine: the same on a GPU box)"""
    p, rows, frames = run(exe, tmp_path, 99)
    assert p.returncode == 3, (p.returncode, p.stdout, p.stderr)
    assert "surface=1" in p.stdout, p.stdout
    assert len(rows) == len(frames)
    for r in rows:
        assert r["update_c"] == r["update_d"] == r["update_p"] == "0" and int(r["hip_error"]) == lib.ERR_NODEVICE, r
        assert r["vtx_c"] == r["vtx_d"] == "0" and r["abi_same"] == "1", r
        assert r["carried_c"] == r["lost_c"] == r["carried_d"] == r["lost_d"] == "-1", r


@pytest.mark.gpu
def test_the_mesh_survives_the_evictions(gpu, exe, tmp_path):
    p, rows, frames = run(exe, tmp_path, 0)
    print(p.stdout)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert "surface=1" in p.stdout and "carry_c=1 carry_d=0" in p.stdout
    assert len(rows) == len(frames)
    # the restatement over the poses the facade forms, switch on and off
    want = {}
    for on in (True, False):
        fe = CR.CarryRef(R.SCENE_W, R.SCENE_H, R.SCENE_K, 256, RING)
        fe.set_carry(on)
        want[on] = []
        for k, (img, _, _, T) in enumerate(frames):
            out = fe.track(R.params(), img, 40 + k, T, k % EVERY == 0)
            want[on].append((int((out["idepth_var"] < np.float32(CR.GRAPH_VAR)).sum()), fe.carried, fe.carry_lost))
    for k, r in enumerate(rows):
        assert r["abi_same"] == "1" and r["update_c"] == r["update_p"], (k, r)  # C is the bare ABI's
        assert r["carried_d"] == r["lost_d"] == "-1", (k, r)                      # D: the keys stay unset
        n_on, carried, lost = want[True][k]
        if r["update_c"] == "1":
            assert int(r["graph_c"]) == int(r["vtx_c"]) == n_on, (k, r)
            assert int(r["carried_c"]) == int(r["info_carried"]) == carried and int(r["lost_c"]) == int(r["info_lost"]) == lost, (k, r)
        if r["update_d"] == "1":
            assert int(r["graph_d"]) == int(r["vtx_d"]) == want[False][k][0], (k, r)
    evicting = [k for k in range(FRAMES) if k % EVERY == 0 and k // EVERY >= RING]
    assert sum(want[True][k][1] for k in evicting) >= 100
    for k in (6, 18):  # the well-populated pose frame is evicted: the switch-off graph is empty and the frame's update fails
        assert want[False][k][0] == 0 and rows[k]["graph_d"] == "0" and rows[k]["update_d"] == "0", rows[k]
    for k in range(3, FRAMES):  # never a collapse with the switch on
        assert rows[k]["update_c"] == "1" and int(rows[k]["vtx_c"]) >= 0.8 * 44, rows[k]
