"""flame::Flame::update() with flame::GpuFrontEnd and Params::photo_error (include/flame/flame.h): the evaluate stage behind the
facade.  tests/cpp/eval_facade.cc is compiled like tests/test_gpu_frontend_facade.py's program (g++ -std=c++11 -Wall -Wextra
-Werror, fallback types and the stand-ins).  CPU: it compiles with both type sets and without a device every update fails
cleanly.  GPU: three frames of the slanted-plane scene; the photo keys equal what the C call gives for the same image, pose
and committed map, the num_* keys equal the front end's counts, getTruthStats equals the C call, and with the Param off the
photo keys are absent and the frames' outputs are bit-identical."""
import os
import struct
import subprocess

import numpy as np
import pytest

from flame_ros_amd import lib
from flame_ros_amd.regularizer import GraphRegularizer, default_tri_params
from tests import eval_ref as ER
from tests import frontend_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror"]
LINK = ["-L" + os.path.join(ROOT, "flame_ros_amd"), "-lflame_hip", "-Wl,-rpath," + os.path.join(ROOT, "flame_ros_amd"), "-pthread"]
STANDINS = ["-I" + os.path.join(ROOT, "tests", "cpp", "standins")]
ITERS = 20
W, H = R.SCENE_W, R.SCENE_H
VAR_MAX = 1e6  # every emitted feature passes the variance gate, so the first (pose) frame already commits a mesh
U32 = np.uint32


@pytest.fixture(scope="module", params=["fallback", "standins"])
def exe(request, tmp_path_factory):
    lib.load()
    out = str(tmp_path_factory.mktemp("eval_facade") / ("eval_facade_" + request.param))
    subprocess.check_call(CXX + (STANDINS if request.param == "standins" else []) +
                          ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "eval_facade.cc"), "-o", out] + LINK)
    return out


def scene():
    """Three frames of scene (b), poses as float32 quaternion + translation (what SE3f carries); frames 0 and 1 are pose
    frames; the true depth has a band without truth."""
    frames = []
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    for k, (img, _) in enumerate(R.plane_scene(1)[:3]):
        q = np.array([0.0, np.sin(0.002 * k), 0.0, np.cos(0.002 * k)], np.float32)
        t = np.array([0.03 * k, 0.0, 0.0], np.float32)
        T = R.quat_pose(q, t)
        depth = (1.0 / R.plane_idepth(T, xx, yy)[0]).astype(np.float32)
        depth[100:, :] = 0.0
        frames.append(dict(img=img, q=q, t=t, T=T, depth=depth, is_poseframe=k < 2))
    return frames


def write_input(path, frames, device, photo_error):
    with open(path, "wb") as f:
        f.write(struct.pack("<6i", W, H, len(frames), device, ITERS, int(photo_error)))
        f.write(np.array([R.SCENE_K[0], R.SCENE_K[4], R.SCENE_K[2], R.SCENE_K[5], VAR_MAX], np.float32).tobytes())
        for k, d in enumerate(frames):
            f.write(struct.pack("<2i", 40 + k, int(d["is_poseframe"])))
            f.write(d["q"].tobytes() + d["t"].tobytes() + d["img"].tobytes() + d["depth"].tobytes())


def read_output(path):
    raw, off, out = open(path, "rb").read(), 0, []
    while off < len(raw):
        k, ok, stat_bits, timing_bits, nv, truth_ok = struct.unpack_from("<6i", raw, off); off += 24
        d = dict(frame=k, ok=bool(ok), stat_bits=stat_bits, timing_bits=timing_bits, truth_ok=bool(truth_ok))
        d["photo"] = struct.unpack_from("<3d", raw, off); off += 24
        d["num"] = struct.unpack_from("<6q", raw, off); off += 48
        d["info"] = struct.unpack_from("<4q", raw, off); off += 32
        d["conf"] = struct.unpack_from("<4q", raw, off); off += 32
        d["total_error"] = struct.unpack_from("<d", raw, off)[0]; off += 8
        d["derived"] = np.frombuffer(raw, np.float32, 3, off); off += 12
        if ok:
            d["idepths"] = np.frombuffer(raw, np.float32, nv, off); off += 4 * nv
            d["map"] = np.frombuffer(raw, np.float32, W * H, off).reshape(H, W); off += 4 * W * H
            d["err"] = np.frombuffer(raw, np.float32, W * H, off).reshape(H, W); off += 4 * W * H
        out.append(d)
    return out


def run(exe, tmp_path, device=0, photo_error=True, tag="on"):
    inp, outp = str(tmp_path / ("in_%s.bin" % tag)), str(tmp_path / ("out_%s.bin" % tag))
    write_input(inp, scene(), device, photo_error)
    p = subprocess.run([exe, inp, outp], capture_output=True, text=True)
    return p, outp


def test_fails_cleanly_without_a_device(exe, tmp_path):
    """(device 99 exists on no machine: the same on a GPU box)"""
    p, outp = run(exe, tmp_path, device=99)
    assert p.returncode == 3, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.count("update=0 hip_error=%d" % lib.ERR_NODEVICE) == 3, p.stdout
    for d in read_output(outp):
        assert not d["ok"] and d["stat_bits"] == 0 and not d["truth_ok"]


def same_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = np.flatnonzero(np.ascontiguousarray(got).view(U32).ravel() != np.ascontiguousarray(want).view(U32).ravel())
    assert bad.size == 0, (what, bad.size, bad[:5])


@pytest.mark.gpu
def test_photo_keys_truth_stats_and_tracking_keys(gpu, exe, tmp_path):
    fr = scene()
    p, outp = run(exe, tmp_path)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    print(p.stdout)
    out = read_output(outp)
    assert len(out) == 3 and all(d["ok"] for d in out)
    K = np.array(R.SCENE_K, np.float32)
    tp = default_tri_params(W, H)
    # frame 0: no comparison frame yet -- the keys are there and read 0
    assert out[0]["stat_bits"] == 7 and out[0]["photo"] == (0.0, 0.0, 0.0) and out[0]["timing_bits"] == 0
    with GraphRegularizer.empty() as r:
        for k in (1, 2):  # against the most recent pose frame before: frame 0, then frame 1 (promoted inside the library)
            d = out[k]
            r.photo_reference(fr[k - 1]["img"], fr[k - 1]["T"])
            total256, counts = r.photo_error(fr[k]["img"], fr[k]["T"], K, None, tp, idepthmap=d["map"])
            assert d["stat_bits"] == 7 and d["timing_bits"] == 3
            assert counts[0] > 1000, counts  # (not vacuous)
            assert d["photo"] == (total256 / 256.0, total256 / 256.0 / counts[0], float(counts[0])), (k, d["photo"], total256, counts)
        for k, d in enumerate(out):
            # the tracking keys are the front end's counts of that frame; the gate let everything through
            assert d["num"][:4] == d["info"] and min(d["info"]) >= 0, (k, d["num"], d["info"])
            assert d["num"][4] == 0 and d["num"][5] == -1  # num_fail_max_var; num_fail_ref_patch_grad stays unset
            # getTruthStats = the C call on the committed filtered map
            conf, total, err = r.truth_stats(fr[k]["depth"], None, tp, idepthmap=d["map"], want_map=True)
            assert d["truth_ok"] and d["conf"] == conf and sum(conf) == W * H
            assert np.float64(d["total_error"]).view(np.uint64) == np.float64(total).view(np.uint64)
            same_bits(d["err"], err, "truth error map")
            same_bits(d["derived"], np.array(ER.derived(conf, total), np.float32), "avg_error, precision, recall")
            assert conf[0] > 1000 and conf[2] > 100  # estimates with truth, and in the band without
    assert out[2]["num"][0] > 0  # features were updated by frame 2


@pytest.mark.gpu
def test_switched_off_it_is_todays_behaviour(gpu, exe, tmp_path):
    p_on, out_on = run(exe, tmp_path, tag="on")
    p_off, out_off = run(exe, tmp_path, photo_error=False, tag="off")
    assert p_on.returncode == 0 and p_off.returncode == 0, (p_on.stdout, p_off.stdout, p_off.stderr)
    for a, b in zip(read_output(out_on), read_output(out_off)):
        assert b["ok"] and b["stat_bits"] == 0 and b["timing_bits"] == 0  # none of the photo keys
        assert b["num"] == a["num"] and b["num"][:4] == b["info"]         # the num_* keys are there either way
        same_bits(a["idepths"], b["idepths"], "mesh idepths")
        same_bits(a["map"], b["map"], "filtered idepth map")
        assert a["conf"] == b["conf"]
