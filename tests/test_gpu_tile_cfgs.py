"""-m gpu: every instantiated tile-kernel configuration (flame_ros_amd/csrc/tile_cfgs.h) run on the device, one case of
tests/tile_cfg_cases.py per test, so that a failure names its kernel: k_tile<nt, ept, vpt> by launches, k_tile_persist<nt,
ept, vpt> resident, and the four fat resident variants.  tests/test_tile_cfg_cases.py shows on the CPU that the table covers
all of them; tests/solver_corpus.py only reaches (256 | 512 | 1024, 2 | 3, 1).

Per case: the handle reports the target configuration with the default (device) plan builder and with plan_device = 0; from
the case's start state the device's own successive states S_n, n in {0, 1, 2, D - 1, D, D + 1, D + 2} (D = the plan's halo
depth, 4 for an isolated tile) and one ragged split of two solves satisfy check_step -- the loop of
tests/test_gpu_solver_f64.py test_kernel_steps_against_f64 -- and every S_n equals the C oracle's bits on x, w1, w2, q and
the bars.  No tolerance of its own: the bands are oracle/nltgv2_np.py's, the bits the oracle's."""
import pytest

from flame_ros_amd.regularizer import GraphRegularizer, default_params
from tests.solver_corpus import STATE, check_step, state_of
from tests.tile_cfg_cases import config_cases, oracle_of
from tests.util import assert_bit_equal, settle_lease

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in config_cases()}
INFO = ("tile_threads", "tile_ept", "tile_vpt", "tile_slot12", "tile_fat")


def download_all(r):
    x, w1, w2, q = r.download()
    xb, w1b, w2b = r.download_bar()
    return dict(x=x, w1=w1, w2=w2, xb=xb, w1b=w1b, w2b=w2b, q=q)


def solve_from(r, st, P, chunks):
    r.set_state(**st)
    for n in chunks:
        if n:
            r.step(P, n)
    return download_all(r)


def oracle_states(c, upto):
    """{n: the C oracle's state after n iterations from the case's start state}, n = 0 .. upto."""
    o, p = oracle_of(c)
    out = {0: state_of(o)}
    for n in range(1, upto + 1):
        o.solve(p, 1)
        out[n] = state_of(o)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_configuration_against_f64_and_oracle(gpu, name):
    c = CASES[name]
    kind = c["target"][5]
    p = c["p"]
    P = default_params(p["lam"], p["tau"], p["sigma"], p["theta"], p["x_min"], p["x_max"])
    if kind != "launches":
        settle_lease()  # (resident sizing and persist_used are statements about a free lease)
    want, first_on_device = None, None
    for builder in ("device", "host"):
        opts = dict(c["tile"], **({"plan_device": 0} if builder == "host" else {}))
        what = "%s (%s plan builder)" % (name, builder)
        with GraphRegularizer(c["pos"], c["edges"], c["alpha"], c["beta"], c["z"], c["wgt"], device=0, d_sign=c["d_sign"],
                              **opts) as r:
            assert r.info("path") == 2 and tuple(r.info(k) for k in INFO) == c["target"][:5], \
                (what, r.info("path"), [r.info(k) for k in INFO], r.info("num_tiles"), r.info("tile_depth"))
            on_device = r.info("plan_on_device")
            assert builder == "device" or on_device == 0, what
            if builder == "device":
                first_on_device = on_device
            elif not first_on_device:
                continue  # (an isolated tile, a smaller lds_bytes: the default builder WAS the host's -- the same plan again)
            D = r.info("tile_depth") or 4
            tiles = r.info("num_tiles")
            if want is None:
                want = oracle_states(c, 2 * D + 2)
            S = {}
            for n in sorted({0, 1, 2, max(D - 1, 0), D, D + 1, D + 2}):
                S[n] = solve_from(r, c["st"], P, [n])
                if n > D:  # (up to D iterations are one launch either way)
                    assert r.info("persist_used") == (0 if kind == "launches" else 1), (what, n, D, tiles)
                for k in STATE:
                    assert_bit_equal(S[n][k], want[n][k], "%s: %s after %d iterations (D = %d)" % (what, k, n, D))
            for n in sorted({0, 1, max(D - 1, 0), D, D + 1}):
                check_step(c, S[n], S[n + 1], "%s: step %d (D = %d)" % (what, n + 1, D))
            a = solve_from(r, c["st"], P, [D + 2, D - 1])
            b = solve_from(r, c["st"], P, [D + 2, D])
            check_step(c, a, b, "%s: step %d after a ragged split (D = %d)" % (what, 2 * D + 2, D))
            for k in STATE:
                assert_bit_equal(a[k], want[2 * D + 1][k], "%s: %s after %d + %d iterations" % (what, k, D + 2, D - 1))
                assert_bit_equal(b[k], want[2 * D + 2][k], "%s: %s after %d + %d iterations" % (what, k, D + 2, D))
            if kind != "launches":
                assert tiles >= 2 and r.info("persist_recovered") == 0, (what, tiles)  # (the resident kernel's own result)
