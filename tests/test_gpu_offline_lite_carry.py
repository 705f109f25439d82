"""-m gpu: a TUM-format sequence through tools/flame_offline_lite.cc --gpu-frontend --carry-features --max-poseframes 1
(Params::carry_features into flame::GpuFrontEnd), in the style of tests/test_gpu_offline_lite_warp.py: 24 frames of the hovering
sequence (tests/fe_carry_ref.py) as 8-bit grey PNGs with full quaternions; the tool takes a pose frame every 10th frame, so with a
ring of 1 the frames 10 and 20 evict.  The restatement is fed the same pixels and the poses read back from the frame lines and must
give the frame line's feature counts and its `carried` / `carry_lost`; without the flag the frame line is what it was and the
evictions empty the graph."""
import subprocess

import numpy as np
import pytest

from tests import fe_carry_ref as CR
from tests import frontend_ref as R
from tests.test_gpu_fe_warp_facade import quaternion
from tests.test_gpu_offline_lite_frontend import VAR_MAX, exe, rows_of  # noqa: F401  (exe: a fixture)

pytestmark = pytest.mark.gpu
FRAMES, ITERS = 24, 20


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    PIL = pytest.importorskip("PIL.Image")
    seq = tmp_path_factory.mktemp("seq_hover")
    frames = CR.hover_scene(1, FRAMES)
    (seq / "rgb").mkdir()
    (seq / "depth").mkdir()
    yy, xx = np.mgrid[0:R.SCENE_H, 0:R.SCENE_W].astype(np.float64)
    lines = ["# the hovering sequence"]
    for k, (img, T) in enumerate(frames):
        idepth, _ = R.plane_idepth(T, xx, yy)
        PIL.fromarray(np.ascontiguousarray(img), mode="L").save(str(seq / "rgb" / ("%d.png" % k)))
        PIL.fromarray(np.round(5000.0 / idepth).astype(np.uint16)).save(str(seq / "depth" / ("%d.png" % k)))
        q = quaternion(T[:, :3]).astype(np.float64)
        t = 1305031102.175304 + 0.033 * k
        lines.append("%.6f %.12f %.12f %.12f %.12f %.12f %.12f %.12f %.6f rgb/%d.png %.6f depth/%d.png" % (
            t, T[0, 3], T[1, 3], T[2, 3], q[0], q[1], q[2], q[3], t, k, t, k))
    (seq / "index.txt").write_text("\n".join(lines) + "\n")
    return seq, frames


def args(seq):
    return [str(seq / "index.txt"), "RDF"] + [str(float(a)) for a in (R.SCENE_K[0], R.SCENE_K[4], R.SCENE_K[2], R.SCENE_K[5])] + [str(ITERS)]


def carried(stdout):
    out = []
    for l in stdout.splitlines():
        if l.startswith("frame "):
            tok = l.split()
            out.append((int(tok[tok.index("carried") + 1]), int(tok[tok.index("carry_lost") + 1])) if "carried" in tok else None)
    return out


def restatement(rows, frames, on):
    ref = CR.CarryRef(R.SCENE_W, R.SCENE_H, R.SCENE_K, 4096, 1)  # flame::GpuFrontEnd's slots, --max-poseframes 1
    ref.set_carry(on)
    out = []
    for k, (r, (img, _)) in enumerate(zip(rows, frames)):
        o = ref.track(R.params(), img, k, R.quat_pose(r["pose_q"], r["pose_t"]), k % 10 == 0)
        out.append((len(o["slot"]), int((o["idepth_var"] < np.float32(VAR_MAX)).sum()), ref.carried, ref.carry_lost))
    return out


def test_sequence_with_the_hand_over(gpu, exe, sequence):  # noqa: F811
    seq, frames = sequence
    p = subprocess.run([exe] + args(seq) + ["--gpu-frontend", "--carry-features", "--max-poseframes", "1"], capture_output=True, text=True,
                       timeout=300)
    print(p.stdout)
    assert p.returncode in (0, 3), (p.returncode, p.stdout, p.stderr)  # (the first frames fail: nothing is under the variance gate yet)
    rows, got = rows_of(p.stdout), carried(p.stdout)
    assert len(rows) == len(frames) == len(got)
    want = restatement(rows, frames, True)
    for k, (r, (feats, gated, n_carried, n_lost)) in enumerate(zip(rows, want)):
        assert int(r["feats"]) == feats and int(r["ok"]) == int(gated >= 3), (k, r, gated)
        assert got[k] == (n_carried, n_lost), (k, got[k])  # (reportStats runs behind every track() that emitted >= 3 features: every frame here)
        if int(r["ok"]):
            assert int(r["vtx"]) == gated and int(r["hip_error"]) == 0, (k, r)
            assert 0.0 < float(r["rms_vs_truth"]) < 0.2, (k, r)
    assert [k for k, c in enumerate(got) if c != (0, 0)] == [10, 20] and got[10][0] >= 30 and got[20][0] >= 30, got
    assert all(int(r["ok"]) == 1 and int(r["vtx"]) >= 0.8 * 44 for r in rows[3:]), [r["vtx"] for r in rows]
    # without the flag: the frame line carries no such fields, and the evicting frames and the ones behind them have no graph
    q = subprocess.run([exe] + args(seq) + ["--gpu-frontend", "--max-poseframes", "1"], capture_output=True, text=True, timeout=300)
    assert q.returncode in (0, 3) and carried(q.stdout) == [None] * len(frames), (q.returncode, q.stderr)
    plain = rows_of(q.stdout)
    for k, (r, (feats, gated, _, _)) in enumerate(zip(plain, restatement(plain, frames, False))):
        assert int(r["feats"]) == feats and int(r["ok"]) == int(gated >= 3), (k, r, gated)
    assert [int(plain[k]["ok"]) for k in (10, 11, 20, 21)] == [0, 0, 0, 0]


def test_usage(gpu, exe, sequence):  # noqa: F811
    for flags in (["--carry-features"], ["--max-poseframes", "2"], ["--gpu-frontend", "--max-poseframes", "0"],
                  ["--gpu-frontend", "--max-poseframes", "65"]):
        p = subprocess.run([exe] + args(sequence[0]) + flags, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "usage" in p.stderr and "--carry-features" in p.stderr and p.stdout == "", (flags, p.returncode, p.stderr)
