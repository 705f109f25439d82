"""What the ingest stage costs and what it replaces, on one MI355X and one host thread of the same machine.  Two cases:
752x480 GRAY8 with EuRoC cam0's K and D (the remap kernel alone), and 640x480 BGR8 with TUM's kinect camera (D = 0: the
grey kernel alone), resize factor 1.  Per case:

  (a) host_undistort_us / host_gray_us: include/flame_ros/image_io.h undistort<uint8_t> / toGray8 on one host thread
      (tools/ingest_bench.cc, g++ -O2), median per frame;
  (b) ingest_device_us: HIP events around the raw upload and the stage (info key of the same name), median;
  (c) track_raw_host_us against track_host_us: the host's wall time of flame_hip_frontend_track_raw on the raw image and of
      flame_hip_frontend_track on the image rectified beforehand, on two handles fed the same frames in turn, tracking
      frames with ~1 200 live features (the pairs of tools/frontend_bench.py), median; raw_minus_rectified_us is what the
      stage adds to a frame on the host's clock.
The stage earns its place when raw_minus_rectified_us is smaller than (a).  Recorded in DESIGN.md 6, not part of bench.py.

    python tools/ingest_bench.py [--frames 100] [--warmup 10]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.frontend_bench import texture  # noqa: E402

CASES = {
    "euroc_752x480_gray8": dict(W=752, H=480, fmt=0, K4=(458.654, 457.296, 367.215, 248.375),
                                D=(-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0)),
    "tum_640x480_bgr8": dict(W=640, H=480, fmt=1, K4=(525.0, 525.0, 319.5, 239.5), D=(0.0, 0.0, 0.0, 0.0, 0.0)),
}


def host_times(case, reps):
    """(a): the header on one thread."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "ingest_bench")
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tools", "ingest_bench.cc"), "-o", exe])
        args = [exe, str(case["W"]), str(case["H"]), str(3 if case["fmt"] else 1), str(reps)]
        args += [repr(float(x)) for x in case["K4"] + case["D"]]
        tok = subprocess.run(args, capture_output=True, text=True, check=True).stdout.split()
    return float(tok[tok.index("gray_us") + 1]), float(tok[tok.index("undistort_us") + 1])


def device_times(case, frames, warmup, shift=6):
    """(b) and (c)."""
    from flame_ros_amd.frontend import GpuFrontEnd, default_frontend_params
    W, H, fmt = case["W"], case["H"], case["fmt"]
    fx, fy, cx, cy = case["K4"]
    K = np.array([fx, 0, cx, 0, fy, cy, 0, 0, 1], np.float32)
    big = texture(H, W + shift)
    grey = [np.ascontiguousarray(big[:, :W]), np.ascontiguousarray(big[:, shift:])]
    raws = grey if fmt == 0 else [np.ascontiguousarray(np.repeat(g[..., None], 3, axis=2)) for g in grey]
    Ta = np.hstack([np.eye(3), np.zeros((3, 1))])
    Tb = Ta.copy()
    Tb[0, 3] = shift * 2.0 / fx
    p = default_frontend_params()
    t = {"raw": [], "rect": [], "ingest": []}
    with GpuFrontEnd(W, H, K, max_features=2048, max_poseframes=1) as fa, GpuFrontEnd(W, H, K, max_features=2048, max_poseframes=1) as fb:
        fa.set_camera(W, H, case["D"], format=fmt)
        rects = [fa.rectify(r) for r in raws]  # (what a host that rectifies itself would hand to track)
        for i in range(warmup + frames):
            for k, (T, pf) in enumerate(((Ta, True), (Tb, False))):
                fa.track_raw(p, raws[k], 2 * i + k, T, pf)
                fb.track(p, rects[k], 2 * i + k, T, pf)
                if i >= warmup and not pf:
                    t["raw"].append(fa.info("track_us"))
                    t["rect"].append(fb.info("track_us"))
                    t["ingest"].append(fa.info("ingest_device_us"))
        live, ok = fa.info("live"), fa.info("ok")
        assert (live, ok) == (fb.info("live"), fb.info("ok"))
    med = {k: float(np.median(v)) for k, v in t.items()}
    return dict(live_features=live, matched_ok=ok, frames=frames, ingest_device_us=med["ingest"], track_raw_host_us=med["raw"],
                track_host_us=med["rect"], raw_minus_rectified_us=med["raw"] - med["rect"],
                raw_minus_rectified_us_spread=[float(np.percentile(np.array(t["raw"]) - np.array(t["rect"]), q)) for q in (10, 90)])


def run(frames=100, warmup=10):
    import torch
    assert torch.cuda.is_available(), "ingest_bench needs a GPU: there is no CPU path to time"
    out = {}
    for name, case in CASES.items():
        g, u = host_times(case, max(frames, 20))
        res = dict(host_gray_us=g if case["fmt"] else 0.0, host_undistort_us=u if any(case["D"]) else 0.0)
        res.update(device_times(case, frames, warmup))
        res["host_replaced_us"] = res["host_gray_us"] + res["host_undistort_us"]
        out[name] = res
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    print(json.dumps({"ingest": run(max(a.frames, 50), a.warmup)}))
