"""CPU: the float32 restatement of the feature front end (tests/frontend_ref.py) against the float64 statement written from
the geometry (oracle/frontend_f64.py), feature by feature and frame by frame over tests/frontend_corpus.py: every post-state
and every emitted list must be ADMISSIBLE -- status and k* among the admissible branches, mu' and var' inside that branch's
rounding band, projection, dropouts, death, the cell's winner, the detections and the untouched state as the contract says.
The statement shares no arithmetic with the restatement (no A = K R, no float32), so a slip they cannot share shows here;
the ground-truth runs on the same scenes are tests/test_frontend_ref.py::test_general_motion_plane_converges.

Floors keep the checks from passing on emptiness (unmutated run: >= 56 certain OK per tracking frame of the six scenes, 33
certain AMBIGUOUS on the checkerboard, 7 certain OUTSIDE in the border case's first tracking frame); the cap on uncertain
features (frontend_corpus.CAP, 15 %) is asserted per case (unmutated run: at most 7 of 80 in a frame, 3.4 % of a case)."""
import pytest

from oracle import frontend_f64 as F64
from tests import frontend_corpus as C
from tests import frontend_ref as R


def ref_info(fe):
    d = dict(fe.counts)
    d["dropped"] = fe.dropped
    return d


@pytest.mark.parametrize("name", C.NAMES)
def test_restatement_is_admissible(name):
    c = C.case(name)
    fe = R.FrontEndRef(C.W, C.H, c.K, C.SLOTS, C.RING)
    reps = C.drive(c, fe, R.params(**c.kw), ref_info)
    tracked = [r for r in reps if r["tracked"]]
    assert reps[0]["new"] >= 28 and len(tracked) == len(reps) - 1
    for k, r in enumerate(reps):
        print("%s frame %d: tracked %d uncertain %d certain %s new %d ratios meas %.3f proj %.3f" % (
            name, k, r["tracked"], r["uncertain"], sorted(r["certain"].items()), r["new"], r["ratio"]["meas"], r["ratio"]["proj"]))
        # the band constants are 4 x these ratios' worst: a run that exceeds what the constants were taken from says so
        assert 4.0 * r["ratio"]["meas"] <= F64.BAND["meas"] * 1.01 and 4.0 * r["ratio"]["proj"] <= F64.BAND["proj"] * 1.01
    if name.startswith("scene_"):
        assert all(r["certain"].get(F64.OK, 0) >= 30 for r in tracked)
    if name == "checkerboard_noise":
        assert tracked[0]["certain"].get(F64.AMBIGUOUS, 0) >= 20
    if name == "border_windows":
        assert tracked[0]["certain"].get(F64.OUTSIDE, 0) >= 5
    if name in ("two_poseframes", "set_poses_and_prune"):
        assert any(r["new"] for r in reps[1:]) and fe.pf_added == 2  # features of two ring slots were tracked


def test_outcome_level_projection_intervals():
    """feature_outcomes: the projection propagated from an outcome's own (mu', var') interval (no observed value used) holds
    the restatement's emitted pixel, xi_cur and var_cur, its dropout count and its death -- frame 3 of the roll scene."""
    from tests import frontend_scenes as SC
    frames = SC.scene("diagonal_roll", 1)
    fe = R.FrontEndRef(C.W, C.H, SC.K, C.SLOTS, C.RING)
    p = R.params()
    for k in range(3):
        fe.track(p, frames[k][0], k, frames[k][1], k == 0)
    pre = fe.state()
    o = fe.track(p, frames[3][0], 3, frames[3][1], False)
    post = fe.state()
    img, ref = frames[3][0].astype("int64"), frames[0][0].astype("int64")
    assert len(o["slot"]) >= 40  # (52 in the unmutated run)
    for i, s in enumerate(o["slot"]):
        feat = {k: pre[k][s] for k in ("u", "v", "mu", "var", "drop")}
        outs = F64.feature_outcomes(p, SC.K4, C.W, C.H, img, frames[3][1], ref, frames[0][1], feat)
        fits = [q for q in outs if q["status"] == post["status"][s] and q["kstar"] == post["kstar"][s] and q["proj"] is not None
                and True in q["pok"] and int(post["drop"][s]) in q["drop"] and False in q["dies"]
                and q["mu"][0] <= post["mu"][s] <= q["mu"][1] and q["var"][0] <= post["var"][s] <= q["var"][1]
                and q["proj"]["px"][0] <= o["vtx"][i][0] <= q["proj"]["px"][1] and q["proj"]["py"][0] <= o["vtx"][i][1] <= q["proj"]["py"][1]
                and q["proj"]["xi"][0] <= o["idepth_mu"][i] <= q["proj"]["xi"][1]
                and q["proj"]["vc"][0] <= o["idepth_var"][i] <= q["proj"]["vc"][1]]
        assert fits, (s, outs)
        assert all(q["proj"]["vc"][1] - q["proj"]["vc"][0] <= 1e-3 * q["proj"]["vc"][1] for q in fits)  # and the intervals are tight


def test_statement_is_independent():
    """The float64 statement imports neither the restatement nor the package."""
    import ast
    import inspect
    mods = set()
    for node in ast.walk(ast.parse(inspect.getsource(F64))):
        if isinstance(node, ast.Import):
            mods.update(a.name.split(".")[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            mods.add((node.module or "").split(".")[0])
    assert mods <= {"math", "numpy"}, mods
