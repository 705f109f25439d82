"""flame::Flame::update() with Params::project_graph (include/flame/flame.h): the previous frame's mesh, warped into the new
view by the library's prediction stage, becomes the x0 of the new frame.  tests/cpp/predict_facade.cc is compiled like
tests/test_gpu_frontend_facade.py's program (g++ -std=c++11 -Wall -Wextra -Werror, fallback types and the stand-ins); a
registered FrontEnd::track feeds synthetic plane features, do_nltgv2 = false, so the mesh hands out x0.  CPU: it compiles with
both type sets and without a device every update fails cleanly.  GPU: frame 2's mesh equals the restatement's predictions
bit for bit where finite and mu elsewhere; with the switch off, or without init_with_prediction, it equals mu."""
import os
import struct
import subprocess

import numpy as np
import pytest

from flame_ros_amd import lib
from tests import frontend_ref as FR
from tests import frontend_scenes as S
from tests import predict_cases as PC
from tests import predict_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror"]
LINK = ["-L" + os.path.join(ROOT, "flame_ros_amd"), "-lflame_hip", "-Wl,-rpath," + os.path.join(ROOT, "flame_ros_amd"), "-pthread"]
STANDINS = ["-I" + os.path.join(ROOT, "tests", "cpp", "standins")]
W, H, K4 = S.W, S.H, S.K4
U32 = np.uint32


@pytest.fixture(scope="module", params=["fallback", "standins"])
def exe(request, tmp_path_factory):
    lib.load()
    out = str(tmp_path_factory.mktemp("predict_facade") / ("predict_facade_" + request.param))
    subprocess.check_call(CXX + (STANDINS if request.param == "standins" else []) +
                          ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "predict_facade.cc"), "-o", out] + LINK)
    return out


def frames():
    """Two views of the plane of tests/frontend_scenes.py, poses as float32 quaternion + translation (what SE3f carries);
    frame 1 carries the exact idepths, frame 2 -- other features, another pose -- 1.2 x the truth; variances below the gate."""
    out = []
    for k, (q, t, gain) in enumerate((((0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0), 1.0),
                                      ((0.0, np.sin(0.004), 0.0, np.cos(0.004)), (0.06, 0.01, 0.05), 1.2))):
        q, t = np.array(q, np.float32), np.array(t, np.float32)
        T = FR.quat_pose(q, t)
        pos = PC.lattice(seed=20 + k)
        truth = S.plane_idepth(K4, T, pos[:, 0].astype(np.float64), pos[:, 1].astype(np.float64))[0]
        mu = (gain * truth).astype(np.float32)
        out.append(dict(q=q, t=t, T=T, pos=pos, mu=mu, var=np.full(len(mu), 1e-4, np.float32)))
    return out


def write_input(path, fr, device, project_graph, init_with_prediction):
    with open(path, "wb") as f:
        f.write(struct.pack("<6i", W, H, len(fr), device, int(project_graph), int(init_with_prediction)))
        f.write(np.array(K4, np.float32).tobytes())
        for d in fr:
            f.write(d["q"].tobytes() + d["t"].tobytes() + struct.pack("<i", len(d["mu"])))
            f.write(np.column_stack([d["pos"], d["mu"], d["var"]]).astype(np.float32).tobytes())


def read_output(path):
    raw, off, out = open(path, "rb").read(), 0, []
    while off < len(raw):
        k, nv, nt, predicted, has_map = struct.unpack_from("<5i", raw, off)
        off += 20
        d = dict(frame=k, predicted=predicted)
        d["vtx"] = np.frombuffer(raw, np.float32, 2 * nv, off).reshape(-1, 2); off += 8 * nv
        d["idepths"] = np.frombuffer(raw, np.float32, nv, off); off += 4 * nv
        d["tris"] = np.frombuffer(raw, np.int32, 3 * nt, off).reshape(-1, 3); off += 12 * nt
        d["valid"] = np.frombuffer(raw, np.uint8, nt, off); off += nt
        d["map"] = None
        if has_map:
            d["map"] = np.frombuffer(raw, np.float32, W * H, off).reshape(H, W); off += 4 * W * H
        out.append(d)
    return out


def run(exe, tmp_path, device=0, project_graph=True, init_with_prediction=True):
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_input(inp, frames(), device, project_graph, init_with_prediction)
    p = subprocess.run([exe, inp, outp], capture_output=True, text=True)
    return p, outp


def test_fails_cleanly_without_a_device(exe, tmp_path):
    """(device 99 exists on no machine: the same on a GPU box)"""
    p, _ = run(exe, tmp_path, device=99)
    assert p.returncode == 3, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.count("update=0 hip_error=%d" % lib.ERR_NODEVICE) == 2, p.stdout


def same_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = np.flatnonzero(np.ascontiguousarray(got).view(U32).ravel() != np.ascontiguousarray(want).view(U32).ravel())
    assert bad.size == 0, (what, bad.size, bad[:5])


@pytest.mark.gpu
def test_the_previous_mesh_becomes_x0(gpu, exe, tmp_path):
    fr = frames()
    p, outp = run(exe, tmp_path)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    lines = p.stdout.strip().splitlines()
    f1, f2 = read_output(outp)
    # frame 1: nothing to warp from -- the stage does not run, the mesh is the features' own idepths
    assert "project_graph=0 predicted=-1" in lines[0] and f1["map"] is None
    same_bits(f1["vtx"], fr[0]["pos"], "frame 1 vtx")
    same_bits(f1["idepths"], fr[0]["mu"], "frame 1 idepths")
    assert f1["valid"].sum() > 0.8 * len(f1["valid"])
    # frame 2: the restatement over frame 1's mesh as the facade handed it out
    pred, dense, _ = R.predict(K4, W, H, fr[0]["T"], fr[1]["T"], f1["vtx"], f1["idepths"], f1["tris"], f1["valid"], fr[1]["pos"])
    fin = np.isfinite(pred)
    assert fin.sum() > 0.6 * len(pred) and (~fin).sum() > 0  # (both branches are exercised)
    same_bits(f2["vtx"], fr[1]["pos"], "frame 2 vtx")
    same_bits(f2["idepths"], np.where(fin, pred, fr[1]["mu"]), "frame 2 idepths")
    assert "project_graph=1 predicted=%d" % int(fin.sum()) in lines[1], lines[1]
    assert f2["predicted"] == int(fin.sum())
    same_bits(f2["map"], dense, "predicted map")
    # ... and the prediction is the plane, not the 1.2 x of the features
    truth = fr[1]["mu"].astype(np.float64) / 1.2
    assert (np.abs(f2["idepths"][fin] / truth[fin] - 1.0) < 1e-5).all()  # (a check of meaning: mu is 2e-1 off; precision is tests/test_predict_ref.py's)


@pytest.mark.gpu
@pytest.mark.parametrize("project_graph,init_with_prediction", [(False, True), (True, False)])
def test_switched_off_it_is_todays_behaviour(gpu, exe, tmp_path, project_graph, init_with_prediction):
    fr = frames()
    p, outp = run(exe, tmp_path, project_graph=project_graph, init_with_prediction=init_with_prediction)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    for line in p.stdout.strip().splitlines():
        assert "project_graph=0 predicted=-1" in line, line
    for d, want in zip(read_output(outp), fr):
        same_bits(d["idepths"], want["mu"], "idepths")
        assert d["map"] is None
