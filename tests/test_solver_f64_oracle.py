"""CPU: the C oracle's PD step (oracle/nltgv2_oracle.c) and the graph sync (row a7) of the
oracle and of the library's host path, held against the independent float64 statements of oracle/nltgv2_np.py.

Every GPU solver test compares the kernels with the C oracle bit for bit, so a slip shared by both (beta read as alpha,
the prox without its weight) would pass them all.  Here the oracle is stepped through tests/solver_corpus.py -- alpha and
beta independent, wide and zero data weights, ties, clamps, saturated duals, hubs, cancelling w d terms -- and every
step is checked against the float64 step from the oracle's own previous state, within float32 bands."""
import numpy as np
import pytest

from flame_ros_amd.regularizer import GraphRegularizer, default_sync_params
from oracle import COracle
from oracle import nltgv2_np as N
from oracle.cbind import OracleParams, SyncParams as OSync, graph_sync as oracle_sync
from tests.solver_corpus import check_step, check_sync, corpus, reached, state_of
from tests.test_graph_sync import features

CASES = {c["name"]: c for c in corpus()}
STEPS = 40


def oracle_of(case):
    """The oracle has no d_sign: it sees pos * d_sign (it uses pos only through d = pos_i - pos_j)."""
    c = case
    o = COracle(c["pos"] * np.float32(c["d_sign"]), c["edges"], c["alpha"], c["beta"], c["z"], c["wgt"])
    o.set_state(**c["st"])
    p = c["p"]
    return o, OracleParams(p["lam"], p["tau"], p["sigma"], p["theta"], p["x_min"], p["x_max"])


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_steps_against_f64(oracle_built, name):
    case = CASES[name]
    o, p = oracle_of(case)
    for n in range(STEPS):
        prev = state_of(o)
        o.solve(p, 1)
        check_step(case, prev, state_of(o), "%s step %d" % (name, n + 1))


def test_corpus_reaches_what_it_claims():
    missed = []
    for name, c in CASES.items():
        facts = reached(c)
        for claim in c["claims"]:
            if claim.startswith("tiles:"):
                with GraphRegularizer(c["pos"], c["edges"], c["alpha"], c["beta"], c["z"], c["wgt"], device=-1,
                                      d_sign=c["d_sign"], **c["tile"]) as r:
                    got = r.info("num_tiles")
                    ok = got == int(claim[6:]) and r.info("path") == 2
                if not ok:
                    missed.append((name, claim, got))
            elif not facts[claim]:
                missed.append((name, claim))
    assert not missed, missed
    covered = {k for c in CASES.values() for k in c["claims"]}
    assert covered >= {"beta_ratio", "beta_ne_alpha", "alpha_zero", "beta_zero", "wgt_wide", "snap", "tie", "clamp_min", "clamp_max",
                       "pinch", "z_outside", "dual_unit", "dual_sat", "neg_zero", "unstable", "hub", "parallel",
                       "reversed", "components", "two_vertices", "long_short", "cancel", "d_sign", "fat", "tiles:1",
                       "tiles:2", "tiles:32", "tiles:33", "tiles:256"}
    assert {c["p"]["theta"] for c in CASES.values()} >= {0.0, 1.0, 0.3}


# ---- row a7: the graph sync ----
def host_sync(sp_args, pos, mu, var, tris, pred):
    """The library's host sync on a plan-only handle."""
    with GraphRegularizer.empty(device=-1) as r:
        scale = r.sync_features(pos, mu, var, tris, default_sync_params(*sp_args), prediction=pred)
        return dict(edges=r.edges(), alpha=r.plan_array("sync_alpha", np.float32),
                    beta=r.plan_array("sync_beta", np.float32), z=r.plan_array("sync_z", np.float32),
                    wgt=r.plan_array("sync_wgt", np.float32), x0=r.plan_array("sync_x0", np.float32), scale=scale)


SYNC_SWITCHES = [(0, 0, 1, 0, 0.0, 0.0), (1, 0, 0, 0, 0.0, 0.0), (0, 1, 1, 0, 0.0, 0.0), (1, 1, 1, 0, 0.0, 0.0),
                 (0, 1, 1, 1, 2.5, 0.75), (1, 1, 1, 2, 0.5, 3.0), (0, 0, 1, 3, 1.5, 0.25), (1, 1, 0, 2, 0.0, 0.0),
                 (0, 1, 1, 3, 0.0, 2.0)]


@pytest.mark.parametrize("adaptive,rescale,init_pred,rule,ag,bg", SYNC_SWITCHES)
@pytest.mark.parametrize("V,seed", [(3000, 11), (9000, 12)])
def test_sync_against_f64(oracle_built, adaptive, rescale, init_pred, rule, ag, bg, V, seed):
    g, var, pred = features(V, seed)
    mu = g.z * np.float32(3.7)  # a mean far from 1: the rescale does something
    args = (adaptive, rescale, init_pred, 0.01, rule, ag, bg)
    o = oracle_sync(OSync(*args), g.pos, mu, var, g.tris, pred)
    check_sync(o, g.pos, mu, var, g.tris, pred, adaptive, rescale, init_pred, rule, ag, bg, "oracle")
    h = host_sync(args, g.pos, mu, var, g.tris, pred)
    check_sync(h, g.pos, mu, var, g.tris, pred, adaptive, rescale, init_pred, rule, ag, bg, "library host sync")


def test_sync_scale_edge_cases(oracle_built):
    """A mean that is exactly a float32, a mean that is not > 0 (reads 1), and a single feature."""
    pos = np.float32([[1, 2], [30, 40], [50, 5], [9, 33]])
    tris = np.int32([[0, 1, 2], [0, 2, 3]])
    var = np.float32([1e-4] * 4)
    for mu in (np.float32([0.5, 0.25, 0.75, 0.5]), np.float32([-0.5, 0.25, 0.125, 0.0]), np.float32([0, 0, 0, 0]),
               np.float32([1e-3, 3e-3, 7e-3, 0.2])):
        for impl in ("oracle", "host"):
            args = (1, 1, 1, 0.01, 0, 0.0, 0.0)
            got = oracle_sync(OSync(*args), pos, mu, var, tris) if impl == "oracle" else host_sync(args, pos, mu, var, tris, None)
            check_sync(got, pos, mu, var, tris, None, 1, 1, 1, what="%s mu=%s" % (impl, mu.tolist()))
