"""-m gpu: tools/flame_offline_lite.cc asl --gpu-rectify on a generated ASL sequence (the folders of
tests/test_dataset_streams.py write_asl: EuRoC's 752 x 480 camera with its radial-tangential distortion): the grey image is
rectified by the library's ingest stage on the GPU instead of by include/flame_ros/image_io.h on the host, and the frame lines
are the same.  The features of this tool come from the depth image, so the runs carry --photo-error: the evaluate stage reads
the rectified image, and its three fields differ as soon as one rectified pixel does."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_dataset_streams import write_asl

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 752, 480


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fol_rectify") / "flame_offline_lite")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "flame_offline_lite.cc"), "-o", out,
                           "-L" + os.path.join(ROOT, "flame_ros_amd"), "-lflame_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "flame_ros_amd"), "-pthread"])
    return out


def test_gpu_rectify_prints_the_same_frame_lines(gpu, exe, tmp_path):
    PIL = pytest.importorskip("PIL.Image")
    root = tmp_path / "asl"
    root.mkdir()
    pose_t, rgb_t, _ = write_asl(root, True)
    # a camera at rest (write_asl's poses are random: no two frames would see the same surface)
    with open(root / "pose" / "data.csv", "w") as f:
        f.write("#timestamp [ns],p_x,p_y,p_z,q_w,q_x,q_y,q_z\n")
        for t in pose_t:
            f.write("%d,0.5,-0.25,1.0,0.8,0.0,0.6,0.0\n" % t)
    rng = np.random.default_rng(2)
    vv, uu = np.mgrid[0:H, 0:W]
    idepth = 0.45 + 0.0004 * uu - 0.0002 * vv + 0.25 * (uu > W // 2)
    base = 127.5 + 60.0 * np.sin(uu / 9.0) * np.cos(vv / 7.0) + 0.1 * uu
    for name in ("cam0", "depth0"):
        (root / name / "data").mkdir()
    for t in rgb_t[:3]:
        grey = np.clip(base + rng.normal(0, 4, (H, W)), 0, 255).astype(np.uint8)
        PIL.fromarray(grey).save(str(root / "cam0" / "data" / ("%d.png" % t)))
        PIL.fromarray(np.round(1000.0 / idepth).astype(np.uint16)).save(str(root / "depth0" / "data" / ("%d.png" % t)))
    args = [exe, "asl", str(root / "pose"), str(root / "cam0"), str(root / "depth0"), "FLU", "20", "--photo-error"]
    host = subprocess.run(args, capture_output=True, text=True, timeout=120)
    dev = subprocess.run(args + ["--gpu-rectify"], capture_output=True, text=True, timeout=120)
    assert host.returncode == 0 and dev.returncode == 0, (host.stdout, host.stderr, dev.stdout, dev.stderr)
    frames = lambda out: [l.split() for l in out.splitlines() if l.startswith("frame")]  # noqa: E731
    rows_host, rows_dev = frames(host.stdout), frames(dev.stdout)
    print(dev.stdout)
    assert len(rows_host) == len(rows_dev) == 2  # (the first image has no depth, the fourth no pose)
    for k, (a, b) in enumerate(zip(rows_host, rows_dev)):
        ms = a.index("update_ms") + 1  # (the wall time differs)
        assert a[a.index("ok") + 1] == "1" and a[:ms] == b[:ms] and a[ms + 1:] == b[ms + 1:], (a, b)
    # not vacuous: the second frame was scored against the first, pixel by pixel of the rectified images
    last = rows_dev[-1]
    field = lambda name: last[last.index(name) + 1]  # noqa: E731
    assert int(field("photo_pixels")) > 0.3 * W * H and float(field("photo_total")) > 0.0, last
