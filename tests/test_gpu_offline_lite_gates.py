"""-m gpu: a TUM-format sequence through tools/flame_offline_lite.cc --gpu-frontend with the gate flags (--letterbox, --min-height,
--max-height, --up-axis: Params::do_letterbox / min_height / max_height into flame::GpuFrontEnd), in the style of
tests/test_gpu_offline_lite_frontend.py: the ten-frame "sideways" scene as 8-bit grey PNGs; the restatement
(tests/fe_gates_ref.py) is fed the same pixels and the poses read back from the frame lines, and must give the frame line's
feature counts and both gate counters."""
import os
import subprocess

import numpy as np
import pytest

from tests import fe_gates_ref as G
from tests import frontend_ref as R
from tests import frontend_scenes as SC
from tests.test_gpu_offline_lite_frontend import FRAMES, VAR_MAX, args, exe, rows_of, sequence  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
MAX_HEIGHT = 0.05  # up = (0, -1, 0): the world points with y >= -0.05 stay


def gate_counts(stdout):
    out = []
    for l in stdout.splitlines():
        if l.startswith("frame "):
            tok = l.split()
            out.append((int(tok[tok.index("held_height") + 1]), int(tok[tok.index("refused_letterbox") + 1])) if "held_height" in tok else None)
    return out


@pytest.mark.parametrize("flags,kw", [
    (["--letterbox", "--max-height", str(MAX_HEIGHT)], dict(letterbox=True, max_height=MAX_HEIGHT)),
    (["--min-height", "-0.05", "--up-axis", "0,1,0"], dict(min_height=-0.05, up=(0, 1, 0))),
])
def test_sequence_with_gates(gpu, exe, sequence, flags, kw):  # noqa: F811
    seq, frames = sequence
    p = subprocess.run([exe] + args(seq) + ["--gpu-frontend"] + flags, capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 3, (p.returncode, p.stdout, p.stderr)  # (the first frames fail: nothing is under the variance gate yet)
    rows, counts = rows_of(p.stdout), gate_counts(p.stdout)
    assert len(rows) == FRAMES and None not in counts
    ref = R.FrontEndRef(SC.W, SC.H, np.array(SC.K, np.float32), 4096, 16)  # flame::GpuFrontEnd's slots and ring
    ref.set_gates(**kw)
    pr = R.params()
    oks, held = [], 0
    y_lo, y_hi = G.band(SC.H)
    for k, (r, (img, _)) in enumerate(zip(rows, frames)):
        T = R.quat_pose(r["pose_q"], r["pose_t"])
        o = ref.track(pr, img, k, T, k % 10 == 0)
        gated = int((o["idepth_var"] < np.float32(VAR_MAX)).sum())
        assert int(r["feats"]) == len(o["slot"]) and counts[k] == (ref.held, ref.refused), (k, r, counts[k], ref.held, ref.refused)
        assert int(r["ok"]) == int(gated >= 3), (k, r, gated)
        if int(r["ok"]):
            assert int(r["vtx"]) == gated and int(r["hip_error"]) == 0, (k, r)
        if kw.get("letterbox"):
            assert (o["vtx"][:, 1] >= y_lo).all() and (o["vtx"][:, 1] <= y_hi - 1).all()
        oks.append(int(r["ok"]))
        held += ref.held
    assert oks[0] == 0 and oks[-1] == 1 and sum(oks) >= 3 and held >= 50, (oks, held)


def test_without_the_flags_the_frame_line_is_what_it_was(gpu, exe, sequence):  # noqa: F811
    seq, _ = sequence
    p = subprocess.run([exe] + args(seq) + ["--gpu-frontend"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 3 and gate_counts(p.stdout) == [None] * FRAMES, (p.returncode, p.stderr)


def test_usage_and_refused_band(gpu, exe, sequence):  # noqa: F811
    seq, _ = sequence
    for flags in (["--letterbox"], ["--max-height", "1"], ["--gpu-frontend", "--up-axis", "0,1"]):
        p = subprocess.run([exe] + args(seq) + flags, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "usage" in p.stderr and p.stdout == "", (flags, p.returncode, p.stderr)
    for flags in (["--min-height", "1", "--max-height", "0"], ["--letterbox", "--max-height", "1", "--up-axis", "0,0,0"]):
        p = subprocess.run([exe] + args(seq) + ["--gpu-frontend"] + flags, capture_output=True, text=True, timeout=60)
        assert p.returncode == 5 and "gates: hip_error" in p.stderr and p.stdout == "", (flags, p.returncode, p.stderr)
