"""-m gpu: a TUM-format sequence through tools/flame_offline_lite.cc --gpu-frontend --min-epipolar-grad 5 --win-size 7
(Params::min_epipolar_grad into flame::GpuFrontEnd), in the style of tests/test_gpu_offline_lite_zm.py: the ten-frame half-striped
"sideways" scene (tests/fe_rg_ref.py) as 8-bit grey PNGs.  The restatement is fed the same pixels and the poses read back from the
frame lines and must give the frame line's feature counts and its `fail_ref_grad`; without the flag the frame line is what it was
and the mesh scores worse against the depth images."""
import subprocess

import numpy as np
import pytest

from tests import fe_rg_ref as RG
from tests import fe_zm_scenes as ZS
from tests import frontend_ref as R
from tests.test_gpu_offline_lite_frontend import FRAMES, VAR_MAX, args, exe, rows_of  # noqa: F401  (exe: a fixture)
from tests.test_gpu_offline_lite_zm import write_sequence

pytestmark = pytest.mark.gpu
WIN, MIN_GRAD = 7, 5.0


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    frames = RG.half_striped("sideways", frames=FRAMES)
    return write_sequence(tmp_path_factory.mktemp("seq_striped"), frames), frames


def fail_ref_grad(stdout):
    out = []
    for l in stdout.splitlines():
        if l.startswith("frame "):
            tok = l.split()
            out.append(int(tok[tok.index("fail_ref_grad") + 1]) if "fail_ref_grad" in tok else None)
    return out


def test_sequence_with_the_gate(gpu, exe, sequence):  # noqa: F811
    seq, frames = sequence
    p = subprocess.run([exe] + args(seq) + ["--gpu-frontend", "--min-epipolar-grad", str(MIN_GRAD), "--win-size", str(WIN)],
                       capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 3, (p.returncode, p.stdout, p.stderr)  # (the first frames fail: nothing is under the variance gate yet)
    rows, fails = rows_of(p.stdout), fail_ref_grad(p.stdout)
    assert len(rows) == FRAMES == len(fails)
    ref = R.FrontEndRef(ZS.W, ZS.H, np.array(ZS.K, np.float32), 4096, 16)  # flame::GpuFrontEnd's slots and ring
    ref.set_ref_grad(MIN_GRAD)
    pr = R.params(win_size=WIN)
    oks, want = [], []
    for k, (r, (img, _)) in enumerate(zip(rows, frames)):
        T = R.quat_pose(r["pose_q"], r["pose_t"])
        o = ref.track(pr, img, k, T, k % 10 == 0)
        gated = int((o["idepth_var"] < np.float32(VAR_MAX)).sum())
        assert int(r["feats"]) == len(o["slot"]) and int(r["ok"]) == int(gated >= 3), (k, r, gated)
        want.append(ref.counts.get(RG.REF_GRAD, 0))
        if int(r["ok"]):
            assert int(r["vtx"]) == gated and int(r["hip_error"]) == 0, (k, r)
            assert 0.0 < float(r["rms_vs_truth"]) < 0.2, (k, r)
        oks.append(int(r["ok"]))
    # (reportStats runs behind every track() that emitted >= 3 features: every frame here)
    assert fails == want and max(want) >= 25, (fails, want)
    assert oks[0] == 0 and oks[-1] == 1 and sum(oks) >= 3, oks
    # without the flag: the frame line carries no such field, and the striped half drags the mesh off the depth images
    q = subprocess.run([exe] + args(seq) + ["--gpu-frontend", "--win-size", str(WIN)], capture_output=True, text=True, timeout=300)
    assert q.returncode in (0, 3) and fail_ref_grad(q.stdout) == [None] * FRAMES, (q.returncode, q.stderr)
    plain = rows_of(q.stdout)
    print("rms_vs_truth of the last frame: gated %s, ungated %s" % (rows[-1]["rms_vs_truth"], plain[-1]["rms_vs_truth"]))
    assert int(plain[-1]["ok"]) == 1 and float(plain[-1]["rms_vs_truth"]) > float(rows[-1]["rms_vs_truth"])


def test_usage(gpu, exe, sequence):  # noqa: F811
    p = subprocess.run([exe] + args(sequence[0]) + ["--min-epipolar-grad", "5"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "usage" in p.stderr and "--min-epipolar-grad" in p.stderr and p.stdout == "", (p.returncode, p.stderr)
