"""-m gpu: a plain `bench.py` run -- the headline line only, exactly --steps timed steps -- and what --dump-outputs writes: the
state of the timed handle after its last step, bit for bit the oracle's after as many iterations."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import COracle
from oracle.cbind import default_params as oracle_params
from tests.util import graphgen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(gpu, tmp_path):
    steps, warmup = 3, 1
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--workload", "5k", "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == steps and d["warmup"] == warmup and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "PD iterations/s" and "iterations/sec" in d["metric"]
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - d["config"]["iters_per_step"]) <= 1e-6 * d["config"]["iters_per_step"]
    assert not {"roofline", "repeats", "cpu_baseline", "facade_frame_ms"} & set(d), sorted(d)
    # bench.py solves twice before the warm-up (hipGraph capture), then warm-up and timed steps on the same state
    g, iters = graphgen.named("5k", seed=0)
    o = COracle(g.pos, g.edges, g.alpha, g.beta, g.z, g.wgt)
    o.solve(oracle_params(), (2 + warmup + steps) * iters)
    for name, want in (("x", o.x), ("w1", o.w1), ("w2", o.w2), ("q", o.q)):
        got = np.load(str(tmp_path / (name + ".npy")))
        assert got.dtype == np.float32 and got.shape == want.shape, (name, got.dtype, got.shape)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
