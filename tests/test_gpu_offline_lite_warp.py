"""-m gpu: a TUM-format sequence through tools/flame_offline_lite.cc --gpu-frontend --warp-window (Params::warp_matching_window
into flame::GpuFrontEnd), in the style of tests/test_gpu_offline_lite_rg.py: the eight-frame roll-30 scene (tests/fe_warp_scenes.py)
as 8-bit grey PNGs with full quaternions.  The restatement is fed the same pixels and the poses read back from the frame lines and
must give the frame line's feature counts and its `fail_warp`; without the flag the frame line is what it was and the roll loses
the features."""
import subprocess

import numpy as np
import pytest

from tests import fe_warp_scenes as WS
from tests import frontend_ref as R
from tests import frontend_scenes as SC
from tests.test_gpu_fe_warp_facade import quaternion
from tests.test_gpu_offline_lite_frontend import VAR_MAX, args, exe, rows_of  # noqa: F401  (exe: a fixture)

pytestmark = pytest.mark.gpu
WIN = 5


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    PIL = pytest.importorskip("PIL.Image")
    seq = tmp_path_factory.mktemp("seq_roll30")
    frames = WS.scene("roll30")
    (seq / "rgb").mkdir()
    (seq / "depth").mkdir()
    yy, xx = np.mgrid[0:WS.H, 0:WS.W].astype(np.float64)
    lines = ["# the roll-30 scene"]
    for k, (img, T) in enumerate(frames):
        idepth, _ = SC.plane_idepth(WS.K4, T, xx, yy)
        PIL.fromarray(np.ascontiguousarray(img), mode="L").save(str(seq / "rgb" / ("%d.png" % k)))
        PIL.fromarray(np.round(5000.0 / idepth).astype(np.uint16)).save(str(seq / "depth" / ("%d.png" % k)))
        q = quaternion(T[:, :3]).astype(np.float64)
        t = 1305031102.175304 + 0.033 * k
        lines.append("%.6f %.12f %.12f %.12f %.12f %.12f %.12f %.12f %.6f rgb/%d.png %.6f depth/%d.png" % (
            t, T[0, 3], T[1, 3], T[2, 3], q[0], q[1], q[2], q[3], t, k, t, k))
    (seq / "index.txt").write_text("\n".join(lines) + "\n")
    return seq, frames


def fail_warp(stdout):
    out = []
    for l in stdout.splitlines():
        if l.startswith("frame "):
            tok = l.split()
            out.append(int(tok[tok.index("fail_warp") + 1]) if "fail_warp" in tok else None)
    return out


def restatement(rows, frames, warp):
    ref = R.FrontEndRef(WS.W, WS.H, np.array(WS.K, np.float32), 4096, 16)  # flame::GpuFrontEnd's slots and ring
    ref.set_warp(warp)
    pr = R.params(win_size=WIN)
    out = []
    for k, (r, (img, _)) in enumerate(zip(rows, frames)):
        o = ref.track(pr, img, k, R.quat_pose(r["pose_q"], r["pose_t"]), k % 10 == 0)
        out.append((len(o["slot"]), int((o["idepth_var"] < np.float32(VAR_MAX)).sum()), ref.warp_refused()))
    return out


def test_sequence_with_the_warped_window(gpu, exe, sequence):  # noqa: F811
    seq, frames = sequence
    p = subprocess.run([exe] + args(seq) + ["--gpu-frontend", "--warp-window", "--win-size", str(WIN)], capture_output=True, text=True,
                       timeout=300)
    print(p.stdout)
    assert p.returncode in (0, 3), (p.returncode, p.stdout, p.stderr)  # (the first frames fail: nothing is under the variance gate yet)
    rows, fails = rows_of(p.stdout), fail_warp(p.stdout)
    assert len(rows) == len(frames) == len(fails)
    oks = []
    for k, (r, (feats, gated, refused)) in enumerate(zip(rows, restatement(rows, frames, True))):
        assert int(r["feats"]) == feats and int(r["ok"]) == int(gated >= 3), (k, r, gated)
        assert fails[k] == refused == 0, (k, fails)  # (reportStats runs behind every track() that emitted >= 3 features: every frame here)
        if int(r["ok"]):
            assert int(r["vtx"]) == gated and int(r["hip_error"]) == 0, (k, r)
            assert 0.0 < float(r["rms_vs_truth"]) < 0.2, (k, r)
        oks.append(int(r["ok"]))
    assert oks[0] == 0 and oks[-1] == 1 and sum(oks) >= 3 and int(rows[-1]["vtx"]) >= 25, (oks, rows[-1])
    # without the flag: the frame line carries no such field, and the roll loses the features
    q = subprocess.run([exe] + args(seq) + ["--gpu-frontend", "--win-size", str(WIN)], capture_output=True, text=True, timeout=300)
    assert q.returncode in (0, 3) and fail_warp(q.stdout) == [None] * len(frames), (q.returncode, q.stderr)
    plain = rows_of(q.stdout)
    for k, (r, (feats, gated, _)) in enumerate(zip(plain, restatement(plain, frames, False))):
        assert int(r["feats"]) == feats and int(r["ok"]) == int(gated >= 3), (k, r, gated)
    last = restatement(plain, frames, False)[-1]
    print("last frame: %s vertices with the flag, %d converged features without" % (rows[-1]["vtx"], last[1]))
    assert last[1] < int(rows[-1]["vtx"]) // 2


def test_usage(gpu, exe, sequence):  # noqa: F811
    p = subprocess.run([exe] + args(sequence[0]) + ["--warp-window"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "usage" in p.stderr and "--warp-window" in p.stderr and p.stdout == "", (p.returncode, p.stderr)
