"""GPU: the feature front end (flame_hip_frontend_*, csrc/frontend.hip) held DIRECTLY against the float64 statement written
from the geometry (oracle/frontend_f64.py) -- not through the float32 restatement, so a slip the kernel and the restatement
share (tests/test_gpu_frontend.py is bit parity between those two) shows on the device.  Same corpus and the same checks as
tests/test_frontend_f64.py: before every track() the device's own state is the pre-state, after it the device's state, its
emitted features and its info() counters must be admissible; the cap on uncertain features holds per case."""
import pytest

from oracle import frontend_f64 as F64
from tests import frontend_corpus as C

pytestmark = pytest.mark.gpu

KEYS = {F64.OK: "ok", F64.NO_PARALLAX: "no_parallax", F64.OUTSIDE: "outside", F64.BAD_MATCH: "bad_match",
        F64.AMBIGUOUS: "ambiguous", F64.NEW: "new", F64.DIED: "died", "dropped": "detections_dropped", "emitted": "emitted"}


def gpu_info(fe):
    return {k: fe.info(key) for k, key in KEYS.items()}


@pytest.mark.parametrize("name", C.NAMES)
def test_gpu_is_admissible(gpu, name):
    from flame_ros_amd.frontend import GpuFrontEnd, default_frontend_params
    c = C.case(name)
    with GpuFrontEnd(C.W, C.H, c.K, C.SLOTS, C.RING) as fe:
        reps = C.drive(c, fe, default_frontend_params(**c.kw), gpu_info)
    tracked = [r for r in reps if r["tracked"]]
    assert reps[0]["new"] >= 28 and len(tracked) == len(reps) - 1
    for k, r in enumerate(reps):
        print("%s frame %d: tracked %d uncertain %d certain %s new %d ratios meas %.3f proj %.3f" % (
            name, k, r["tracked"], r["uncertain"], sorted(r["certain"].items()), r["new"], r["ratio"]["meas"], r["ratio"]["proj"]))
    if name.startswith("scene_"):
        assert all(r["certain"].get(F64.OK, 0) >= 30 for r in tracked)
    if name == "checkerboard_noise":
        assert tracked[0]["certain"].get(F64.AMBIGUOUS, 0) >= 20
    if name == "border_windows":
        assert tracked[0]["certain"].get(F64.OUTSIDE, 0) >= 5
