"""Cost of the feature front end per frame: microseconds per flame_hip_frontend_track at 640x480 with ~1 200 live features,
for a tracking frame and for a pose frame.  Recorded beside the from-features frame time of bench.py, not part of it.

A ring of ONE pose frame makes every pose-frame call start from scratch (the features of the overwritten pose frame die, every
cell detects again), so the two calls of a pair do the same work every time: the pose frame = upload + detection in all 1 200
cells + slot assignment + compaction; the tracking frame = upload + 1 200 searches with the widest prior a feature ever has
(var_init: ~16 samples of 5x5 pixels each) + projection + compaction.  Both are upper bounds of a running sequence, where
most priors are narrower.  Times: HIP events around the call's device work (image upload to counts download) and the host's
wall time of the whole call, median over the pairs after a warm-up.

--gates: the same pairs with both gates on (GpuFrontEnd.set_gates: the letterbox and a height band of +-0.15 about the camera
along the default up axis, which holds about half of the features the letterbox leaves; only a third of the cells detect, so
fewer features live) -- what the compares, the height and the held-cell flag cost where they act.

--zero-mean: the same pairs with the ZSSD matching cost (GpuFrontEnd.set_cost: k_fe_track<true>, one more integer sum per window
pixel and a 64-bit multiply-subtract per sample).  --repeat N: N runs in one process, every run's tracking-frame device time,
their median and their spread -- what DESIGN.md 6 compares between two trees.  --win-size N: the matching window (5; ZSSD wants 7).

--gain-invariant: the same pairs with the gain-invariant matching cost (GpuFrontEnd.set_gain_invariant: the third cost of
k_fe_track -- three integer sums per window pixel and a double multiply, divide and subtract per sample).

--warp: the same pairs with the warped matching window (GpuFrontEnd.set_warp: the warped instantiation of k_fe_track -- four byte
loads instead of two and two integer multiply-adds per window pixel; under this sequence's sideways translation the map is the
identity and the features are the same bits).

--min-epipolar-grad G: the same pairs with the reference-patch gradient gate (GpuFrontEnd.set_ref_grad: the gated instantiation of
k_fe_track -- 2 x 3 byte loads per lane and three wave sums in front of every search; a refused feature skips its search).

--carry: the device time of an EVICTING pose frame with the hand-over (GpuFrontEnd.set_carry) on against the same frame with it
off.  The pairs alternate -- (pose frame a, tracking b), (pose frame b, tracking a) -- so that every pose frame sees the features of
the pose frame it evicts `shift` pixels away: with the switch off they are killed and every cell detects again, as above; with it on
they are searched against the new image once more (the work of a tracking frame inside the pose frame), k_fe_carry runs behind the
compaction and the image is copied into the ring slot (W x H bytes, device to device).  Each of --repeat N runs is one off run and
one on run; the medians of the runs' medians are reported side by side.

    python tools/frontend_bench.py [--frames 100] [--warmup 10] [--gates] [--zero-mean] [--gain-invariant] [--warp] [--carry] [--win-size 7] [--min-epipolar-grad 5] [--repeat 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def texture(h, w, seed=5, factor=8):
    rng = np.random.default_rng(seed)
    low = rng.integers(0, 256, (h // factor + 3, w // factor + 3)).astype(np.float32)
    ys, xs = np.arange(h) / factor, np.arange(w) / factor
    y0, x0 = ys.astype(int), xs.astype(int)
    fy, fx = (ys - y0)[:, None], (xs - x0)[None, :]
    up = (1 - fy) * (1 - fx) * low[y0][:, x0] + (1 - fy) * fx * low[y0][:, x0 + 1] + fy * (1 - fx) * low[y0 + 1][:, x0] + \
        fy * fx * low[y0 + 1][:, x0 + 1]
    return np.floor(up + 0.5).astype(np.uint8)


def run(frames=100, warmup=10, W=640, H=480, shift=6, gates=False, zero_mean=False, win_size=5, min_epipolar_grad=0.0, gain_invariant=False, warp=False, carry=None):
    from flame_ros_amd.frontend import GpuFrontEnd, default_frontend_params
    K = np.array([525, 0, 319.5, 0, 525, 239.5, 0, 0, 1], np.float32)
    big = texture(H, W + shift)
    a, b = np.ascontiguousarray(big[:, :W]), np.ascontiguousarray(big[:, shift:])
    Ta = np.hstack([np.eye(3), np.zeros((3, 1))])
    Tb = Ta.copy()
    Tb[0, 3] = shift * 2.0 / 525.0  # the plane at depth 2 moved `shift` pixels
    p = default_frontend_params(win_size=win_size)
    t = {"poseframe": {"device": [], "host": []}, "tracking": {"device": [], "host": []}}
    with GpuFrontEnd(W, H, K, max_features=2048, max_poseframes=1) as fe:
        live = ok = held = refused = fail_rg = carried = carry_lost = 0
        if gates:
            fe.set_gates(letterbox=True, min_height=-0.15, max_height=0.15)
        if zero_mean:
            fe.set_cost(zero_mean=True)
        if gain_invariant:
            fe.set_gain_invariant(True)
        if warp:
            fe.set_warp(True)
        if min_epipolar_grad > 0:
            fe.set_ref_grad(min_epipolar_grad)
        if carry is not None:
            fe.set_carry(carry)
        for i in range(warmup + frames):
            swap = carry is not None and i % 2 == 1  # --carry: the pairs alternate, every pose frame evicts one `shift` pixels away
            for kind, img, T, pf in (("poseframe", b if swap else a, Tb if swap else Ta, True), ("tracking", a if swap else b, Ta if swap else Tb, False)):
                fe.track(p, img, 2 * i + (not pf), T, pf)
                if pf and carry:
                    carried, carry_lost = fe.info("carried"), fe.info("carry_lost")
                if i >= warmup:
                    t[kind]["device"].append(fe.info("track_device_us"))
                    t[kind]["host"].append(fe.info("track_us"))
            live, ok, fail_rg = fe.info("live"), fe.info("ok"), fe.info("fail_ref_grad")
            if gates:
                held, refused = fe.info("held_height"), fe.info("refused_letterbox")
    res = {"width": W, "height": H, "live_features": live, "matched_ok": ok, "pairs": frames}
    if gates:
        res.update(gates=3, held_height=held, refused_letterbox=refused)
    if zero_mean:
        res.update(cost_mode=1)
    if gain_invariant:
        res.update(gain_invariant=1)
    if warp:
        res.update(warp=1)
    if carry is not None:
        res.update(carry=int(carry), carried=carried, carry_lost=carry_lost)
    if min_epipolar_grad > 0:
        res.update(min_epipolar_grad=min_epipolar_grad, fail_ref_grad=fail_rg)
    if win_size != 5:
        res.update(win_size=win_size)
    for kind in t:
        res[kind + "_device_us"] = float(np.median(t[kind]["device"]))
        res[kind + "_host_us"] = float(np.median(t[kind]["host"]))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--gates", action="store_true")
    ap.add_argument("--zero-mean", action="store_true")
    ap.add_argument("--gain-invariant", action="store_true")
    ap.add_argument("--warp", action="store_true")
    ap.add_argument("--carry", action="store_true")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--win-size", type=int, default=5)
    ap.add_argument("--min-epipolar-grad", type=float, default=0.0)
    a = ap.parse_args()
    kw = dict(gates=a.gates, zero_mean=a.zero_mean, win_size=a.win_size, min_epipolar_grad=a.min_epipolar_grad, gain_invariant=a.gain_invariant, warp=a.warp)
    if a.carry:  # off and on alternate; every run is a handle of its own
        off, on = [], []
        for _ in range(max(a.repeat, 1)):
            off.append(run(max(a.frames, 50), a.warmup, carry=False, **kw))
            on.append(run(max(a.frames, 50), a.warmup, carry=True, **kw))
        res = on[-1]
        for name, rs in (("off", off), ("on", on)):
            for kind in ("poseframe", "tracking"):
                t = [r[kind + "_device_us"] for r in rs]
                res["%s_device_us_carry_%s" % (kind, name)] = float(np.median(t))
                res["%s_device_us_carry_%s_runs" % (kind, name)] = t
        print(json.dumps({"frontend_track": res}))
        sys.exit(0)
    runs = [run(max(a.frames, 50), a.warmup, **kw) for _ in range(max(a.repeat, 1))]
    res = runs[-1]
    if a.repeat > 1:
        t = [r["tracking_device_us"] for r in runs]
        res.update(tracking_device_us_runs=t, tracking_device_us=float(np.median(t)), tracking_device_us_spread=[min(t), max(t)])
    print(json.dumps({"frontend_track": res}))
