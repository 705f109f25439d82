"""-m gpu: a TUM-format sequence through tools/flame_offline_lite.cc --gpu-frontend --gain-invariant --win-size 7
(Params::gain_invariant_matching into flame::GpuFrontEnd), in the style of tests/test_gpu_offline_lite_zm.py: the ten-frame halved
"sideways" scene (tests/fe_gi_scenes.py) as 8-bit grey PNGs, once plain and once gained (frame 0, the tool's pose frame, v + |b|; every
other frame 2 v + b).  The restatement (tests/fe_gi_ref.py) is fed the same pixels and the poses read back from the frame lines and
must give the frame line's feature counts; the two sequences must give the same frame lines, and with --zero-mean in the flag's
place they must not."""
import subprocess

import numpy as np
import pytest

from tests import fe_gi_scenes as GS
from tests import fe_zm_scenes as ZS
from tests import frontend_ref as R
from tests.test_gpu_offline_lite_frontend import FRAMES, VAR_MAX, args, exe, rows_of  # noqa: F401  (exe: a fixture)
from tests.test_gpu_offline_lite_zm import lines_without_time, write_sequence

pytestmark = pytest.mark.gpu
WIN = 7


@pytest.fixture(scope="module")
def sequences(tmp_path_factory):
    plain = GS.halved("sideways", frames=FRAMES)
    gained, _ = GS.gained("sideways", frames=FRAMES, poseframes=(0,), offsets=ZS.random_offsets(11, FRAMES))
    return (write_sequence(tmp_path_factory.mktemp("seq_plain"), plain), plain), (write_sequence(tmp_path_factory.mktemp("seq_gained"), gained), gained)


def switches(stdout):
    out = []
    for l in stdout.splitlines():
        if l.startswith("frame "):
            tok = l.split()
            out.append(int(tok[tok.index("gain_invariant") + 1]) if "gain_invariant" in tok else None)
    return out


def test_sequence_with_the_flag(gpu, exe, sequences):  # noqa: F811
    runs = []
    for seq, frames in sequences:
        p = subprocess.run([exe] + args(seq) + ["--gpu-frontend", "--gain-invariant", "--win-size", str(WIN)], capture_output=True, text=True,
                           timeout=300)
        print(p.stdout)
        assert p.returncode == 3, (p.returncode, p.stdout, p.stderr)  # (the first frames fail: nothing is under the variance gate yet)
        rows = rows_of(p.stdout)
        assert len(rows) == FRAMES and switches(p.stdout) == [1] * FRAMES
        assert all(l.split()[-2:] == ["gain_invariant", "1"] for l in p.stdout.splitlines() if l.startswith("frame "))  # (appended)
        ref = R.FrontEndRef(ZS.W, ZS.H, np.array(ZS.K, np.float32), 4096, 16)  # flame::GpuFrontEnd's slots and ring
        ref.set_gain_invariant()
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
    assert runs[0] == runs[1]  # the mesh and its score against the depth images: gain and offsets change nothing


def test_with_zero_mean_alone_the_gain_shows_and_the_frame_line_is_what_it_was(gpu, exe, sequences):  # noqa: F811
    runs = []
    for seq, _ in sequences:
        p = subprocess.run([exe] + args(seq) + ["--gpu-frontend", "--zero-mean", "--win-size", str(WIN)], capture_output=True, text=True, timeout=300)
        assert p.returncode in (0, 3) and switches(p.stdout) == [None] * FRAMES, (p.returncode, p.stderr)
        runs.append(lines_without_time(rows_of(p.stdout)))
    assert len(runs[0]) == len(runs[1]) == FRAMES and runs[0] != runs[1]


def test_usage(gpu, exe, sequences):  # noqa: F811
    seq = sequences[0][0]
    p = subprocess.run([exe] + args(seq) + ["--gain-invariant"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "usage" in p.stderr and "--gain-invariant" in p.stderr and p.stdout == "", (p.returncode, p.stderr)
