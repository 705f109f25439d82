"""-m gpu: a TUM-format sequence through tools/flame_offline_lite.cc --gpu-frontend --zero-mean --win-size 7
(Params::zero_mean_matching into flame::GpuFrontEnd), in the style of tests/test_gpu_offline_lite_frontend.py: the ten-frame
"sideways" exposure scene (tests/fe_zm_scenes.py) as 8-bit grey PNGs, once plain and once with a grey offset per frame.  The
restatement (tests/fe_zm_ref.py) is fed the same pixels and the poses read back from the frame lines and must give the frame line's
feature counts; the two sequences must give the same frame lines, and without --zero-mean they must not."""
import subprocess

import numpy as np
import pytest

from tests import fe_zm_scenes as ZS
from tests import frontend_ref as R
from tests import frontend_scenes as SC
from tests.test_gpu_offline_lite_frontend import FRAMES, VAR_MAX, args, exe, rows_of  # noqa: F401  (exe: a fixture)

pytestmark = pytest.mark.gpu
WIN = 7


def write_sequence(seq, frames):
    PIL = pytest.importorskip("PIL.Image")
    (seq / "rgb").mkdir()
    (seq / "depth").mkdir()
    yy, xx = np.mgrid[0:ZS.H, 0:ZS.W].astype(np.float64)
    lines = ["# the sideways exposure scene"]
    for k, (img, T) in enumerate(frames):
        idepth, _ = SC.plane_idepth(ZS.K4, T, xx, yy)
        PIL.fromarray(np.ascontiguousarray(img), mode="L").save(str(seq / "rgb" / ("%d.png" % k)))
        PIL.fromarray(np.round(5000.0 / idepth).astype(np.uint16)).save(str(seq / "depth" / ("%d.png" % k)))
        yaw = np.arctan2(T[0, 2], T[0, 0])  # the scene's poses are yaw about y + translation
        t = 1305031102.175304 + 0.033 * k
        lines.append("%.6f %.12f %.12f %.12f 0 %.12f 0 %.12f %.6f rgb/%d.png %.6f depth/%d.png" % (
            t, T[0, 3], T[1, 3], T[2, 3], np.sin(yaw / 2), np.cos(yaw / 2), t, k, t, k))
    (seq / "index.txt").write_text("\n".join(lines) + "\n")
    return seq


@pytest.fixture(scope="module")
def sequences(tmp_path_factory):
    plain = ZS.scene("sideways", 1, frames=FRAMES)
    shifted = ZS.scene("sideways", 1, ZS.random_offsets(11, FRAMES), frames=FRAMES)
    return (write_sequence(tmp_path_factory.mktemp("seq_plain"), plain), plain), (write_sequence(tmp_path_factory.mktemp("seq_offset"), shifted), shifted)


def cost_modes(stdout):
    out = []
    for l in stdout.splitlines():
        if l.startswith("frame "):
            tok = l.split()
            out.append(int(tok[tok.index("cost_mode") + 1]) if "cost_mode" in tok else None)
    return out


def lines_without_time(rows):
    return [{k: v for k, v in r.items() if k != "update_ms"} for r in rows]


def test_sequence_with_zero_mean(gpu, exe, sequences):  # noqa: F811
    runs = []
    for seq, frames in sequences:
        p = subprocess.run([exe] + args(seq) + ["--gpu-frontend", "--zero-mean", "--win-size", str(WIN)], capture_output=True, text=True, timeout=300)
        print(p.stdout)
        assert p.returncode == 3, (p.returncode, p.stdout, p.stderr)  # (the first frames fail: nothing is under the variance gate yet)
        rows = rows_of(p.stdout)
        assert len(rows) == FRAMES and cost_modes(p.stdout) == [1] * FRAMES
        ref = R.FrontEndRef(ZS.W, ZS.H, np.array(ZS.K, np.float32), 4096, 16)  # flame::GpuFrontEnd's slots and ring
        ref.set_cost()
        pr = R.params(win_size=WIN)
        oks = []
        for k, (r, (img, _)) in enumerate(zip(rows, frames)):
            T = R.quat_pose(r["pose_q"], r["pose_t"])
            o = ref.track(pr, img, k, T, k % 10 == 0)
            gated = int((o["idepth_var"] < np.float32(VAR_MAX)).sum())
            assert int(r["feats"]) == len(o["slot"]) and int(r["ok"]) == int(gated >= 3), (k, r, gated)
            if int(r["ok"]):
                assert int(r["vtx"]) == gated and int(r["hip_error"]) == 0, (k, r)
                assert 0.0 < float(r["rms_vs_truth"]) < 0.2, (k, r)
            oks.append(int(r["ok"]))
        assert oks[0] == 0 and oks[-1] == 1 and sum(oks) >= 3, oks
        runs.append(lines_without_time(rows))
    assert runs[0] == runs[1]  # the mesh and its score against the depth images: the offsets change nothing


def test_without_the_flag_the_offsets_show_and_the_frame_line_is_what_it_was(gpu, exe, sequences):  # noqa: F811
    runs = []
    for seq, _ in sequences:
        p = subprocess.run([exe] + args(seq) + ["--gpu-frontend", "--win-size", str(WIN)], capture_output=True, text=True, timeout=300)
        assert p.returncode in (0, 3) and cost_modes(p.stdout) == [None] * FRAMES, (p.returncode, p.stderr)
        runs.append(lines_without_time(rows_of(p.stdout)))
    assert len(runs[0]) == len(runs[1]) == FRAMES and runs[0] != runs[1]


def test_usage(gpu, exe, sequences):  # noqa: F811
    seq = sequences[0][0]
    for flags in (["--zero-mean"], ["--win-size", "7"]):
        p = subprocess.run([exe] + args(seq) + flags, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "usage" in p.stderr and "--zero-mean" in p.stderr and p.stdout == "", (flags, p.returncode, p.stderr)
