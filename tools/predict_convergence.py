"""What the warm start buys: the regulariser's total cost (smoothness + data) after 10 / 25 / 50 / 100 / 200 iterations with
x0 = the previous frame's mesh warped into the view (GraphRegularizer.predict, Params::project_graph in the facade) against
x0 = the frame's own noisy idepths, on a stream of plane frames (the scenes of tests/frontend_scenes.py, a new jittered feature
lattice per frame, idepth_mu = truth x (1 + noise)), and the iteration count at which the warm-started solve reaches the cold
solve's 200-iteration cost.  Measured, recorded in DESIGN.md 6, not gated.

  python tools/predict_convergence.py [--scene forward] [--noise 0.05] [--step 12] [--size 160x120]

Prints one JSON line per frame and a summary line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flame_ros_amd.regularizer import GraphRegularizer, default_params, default_sync_params, default_tri_params  # noqa: E402
from tests import frontend_scenes as S  # noqa: E402

CHECK = (10, 25, 50, 100, 200)
STRIDE = 5


def features(k, step, noise, W, H):
    rng = np.random.default_rng(100 + k)
    xs, ys = np.meshgrid(np.arange(step / 2, W, step), np.arange(step / 2, H, step))
    pos = (np.stack([xs.ravel(), ys.ravel()], -1) + rng.uniform(-step / 4, step / 4, (xs.size, 2))).astype(np.float32)
    return pos, rng.normal(0.0, noise, len(pos))


def curve(r, params):
    """total cost every STRIDE iterations up to 200: {iterations: cost}"""
    out = {0: sum(r.costs(params))}
    for it in range(STRIDE, CHECK[-1] + 1, STRIDE):
        r.step(params, STRIDE)
        out[it] = sum(r.costs(params))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="forward", choices=S.NAMES)
    ap.add_argument("--noise", type=float, default=0.05, help="relative sigma of idepth_mu")
    ap.add_argument("--step", type=float, default=12.0, help="feature lattice pitch in px")
    ap.add_argument("--size", default="160x120")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split("x"))
    s = W / S.W  # the scenes' camera scaled with the image
    K4 = tuple(s * k for k in S.K4)
    K = np.array([K4[0], 0, K4[2], 0, K4[1], K4[3], 0, 0, 1], np.float32)
    Kinv = np.linalg.inv(K.reshape(3, 3).astype(np.float64)).astype(np.float32)
    p, tp = default_params(), default_tri_params(W, H)
    sp = default_sync_params()
    var_of = lambda n: np.full(n, 1e-4, np.float32)  # noqa: E731
    warm, cold = GraphRegularizer.empty(), GraphRegularizer.empty()
    reach = []
    T_prev = None
    for k in range(S.FRAMES):
        T = S.scene_pose(a.scene, k)
        pos, eps = features(k, a.step, a.noise, W, H)
        truth = S.plane_idepth(K4, T, pos[:, 0].astype(np.float64), pos[:, 1].astype(np.float64))[0]
        mu = (truth * (1.0 + eps)).astype(np.float32)
        tris = warm.delaunay(pos)
        pred = None
        if T_prev is not None:  # the previous frame, solved and behind its triangle stage, still lies in `warm`
            pred = warm.predict(W, H, K, T_prev, T, pos)
        warm.sync_features(pos, mu, var_of(len(mu)), tris, sp, prediction=pred)
        cw = curve(warm, p)
        x = warm.frame_results(p, Kinv, tp)[2]
        row = {"frame": k, "V": len(mu), "rms_rel_error_after_200": float(np.sqrt(np.mean((x / truth - 1.0) ** 2)))}
        if pred is not None:
            cold.sync_features(pos, mu, var_of(len(mu)), tris, sp)
            cc = curve(cold, p)
            hit = next((it for it in sorted(cw) if cw[it] <= cc[CHECK[-1]]), None)
            reach.append(hit)
            row.update(predicted=int(np.isfinite(pred).sum()), cost_cold={str(i): cc[i] for i in (0,) + CHECK},
                       cost_warm={str(i): cw[i] for i in (0,) + CHECK}, warm_reaches_cold_200_at=hit)
        print(json.dumps(row))
        T_prev = T
    print(json.dumps({"scene": a.scene, "noise": a.noise, "size": a.size, "stride": STRIDE, "warm_reaches_cold_200_at": reach}))
    warm.close()
    cold.close()


if __name__ == "__main__":
    main()
