"""-m gpu: tools/flame_offline_lite.cc --photo-error on a short TUM-format sequence (the scene and the parsing of
tests/test_gpu_offline_lite.py): the flag appends `photo_total ... photo_avg ... photo_pixels ...` at the END of the frame
line and changes nothing in front of it; without the flag the line carries none of the three."""
import os
import subprocess

import numpy as np
import pytest

from tests import test_gpu_offline_lite as OL

pytestmark = pytest.mark.gpu
ROOT = OL.ROOT
W, H = OL.W, OL.H


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fol_photo") / "flame_offline_lite")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "flame_offline_lite.cc"), "-o", out,
                           "-L" + os.path.join(ROOT, "flame_ros_amd"), "-lflame_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "flame_ros_amd"), "-pthread"])
    return out


def test_photo_error_flag(gpu, exe, tmp_path):
    PIL = pytest.importorskip("PIL.Image")
    seq = tmp_path / "seq"
    (seq / "rgb").mkdir(parents=True)
    (seq / "depth").mkdir()
    rng = np.random.default_rng(0)
    lines = ["# synthetic sequence, a camera at rest"]
    for k in range(3):
        idepth, rgb, _ = OL.scene(0, rng)  # the same surface every frame, fresh image noise
        raw = np.round(5000.0 / idepth).astype(np.uint16)
        PIL.fromarray(rgb).save(str(seq / "rgb" / ("%d.png" % k)))
        PIL.fromarray(raw).save(str(seq / "depth" / ("%d.png" % k)))
        t = 1305031102.175304 + 0.033 * k
        lines.append("%.6f 1.34 0.62 1.65 0.6574 0.6126 -0.2949 -0.3248 %.6f rgb/%d.png %.6f depth/%d.png" % (t, t, k, t, k))
    (seq / "index.txt").write_text("\n".join(lines) + "\n")
    args = [exe, str(seq / "index.txt"), "RDF", "525.0", "525.0", "319.5", "239.5", "20"]
    off = subprocess.run(args, capture_output=True, text=True, timeout=120)
    on = subprocess.run(args + ["--photo-error"], capture_output=True, text=True, timeout=120)
    assert off.returncode == 0 and on.returncode == 0, (off.stdout, off.stderr, on.stdout, on.stderr)
    frames = lambda out: [l.split() for l in out.splitlines() if l.startswith("frame")]  # noqa: E731
    rows_off, rows_on = frames(off.stdout), frames(on.stdout)
    assert len(rows_off) == len(rows_on) == 3
    for k, (a, t) in enumerate(zip(rows_off, rows_on)):
        assert a[a.index("ok") + 1] == "1" and "photo_total" not in a
        # the line in front of the appended fields is the line without the flag (but for the wall time)
        skip = a.index("update_ms") + 1
        assert len(t) == len(a) + 6 and t[:skip] == a[:skip] and t[skip + 1:len(a)] == a[skip + 1:], (a, t)
        assert t[len(a)::2] == ["photo_total", "photo_avg", "photo_pixels"]
        b = dict(zip(t[len(a)::2], t[len(a) + 1::2]))
        if k == 0:  # frame 0 is the first pose frame: nothing to compare with yet
            assert (float(b["photo_total"]), float(b["photo_avg"]), int(b["photo_pixels"])) == (0.0, 0.0, 0)
        else:
            # a camera at rest looking at the same surface: what is left is the image noise.  sigma 6 per colour channel is
            # ~4.0 in the grey image (weights 0.299 / 0.587 / 0.114), 5.7 in the difference of two frames, mean |.| ~4.5
            n = int(b["photo_pixels"])
            assert n > 0.5 * W * H and abs(float(b["photo_avg"]) - float(b["photo_total"]) / n) < 1e-5
            assert 1.0 < float(b["photo_avg"]) < 15.0, b
