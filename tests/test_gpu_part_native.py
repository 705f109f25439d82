"""-m gpu: the library's own partition mode (csrc/part.cpp) on the ONE GPU of the test box: a communicator that owns
an ncclComm_t of world size 1, the graph cut into parts_per_rank subdomains all held by rank 0, so every halo record
travels through ncclGroupStart / ncclSend + ncclRecv to the own rank / ncclGroupEnd on the solve stream, between
flame_hip_halo_pack and flame_hip_halo_unpack, with no host synchronisation inside a solve; costs through
ncclAllReduce.  No torch.distributed, no Python in the data path.  Bit-exact against the oracle.  (A process of its own:
the RCCL copy it loads is the library's, not one torch initialised.)"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
from flame_ros_amd import graphgen, partition
from flame_ros_amd.regularizer import default_params
from oracle import COracle
from oracle.cbind import default_params as oparams
from tests.util import decoupled
assert partition.rccl_available()
uid = partition.unique_id()
total_recovered = 0
with partition.Communicator(0, 0, 1, uid) as comm:
    for V, k, depth, iters, pipe, dec in ((6000, 2, 8, 50, 1, 0), (6000, 2, 8, 50, 0, 0), (9000, 3, 4, 23, 1, 0), (50000, 2, 16, 100, 1, 0),
                                          (7000, 3, 5, 31, 1, 1)):
        g = graphgen.synthetic(V, seed=5)
        if dec:  # beta independent of alpha, non-uniform data weights with zeros
            g = decoupled(g, V)
        with partition.Partition(comm, g.pos, g.edges, g.alpha, g.beta, g.z, g.wgt, parts_per_rank=k, halo_depth=depth) as ps:
            p = default_params()
            ps.set_option("pipeline", pipe)  # (forced either way; the default is on from 4 parts per rank.  r05: the records of part i travel while part i + 1 iterates; same bits)
            ps.step(p, iters // 2)
            ps.step(p, iters - iters // 2)
            was_resident = int(all(ps.info("persist_launches", i) > 0 for i in range(k)))  # (parts of one rank queue behind
            assert was_resident == int(any(ps.info("persist_launches", i) > 0 for i in range(k)))  # each other on ONE stream)
            assert ps.info("p2p_ops") >= 2 * k and ps.info("exchanges") == (iters - 1) // depth, (ps.info("p2p_ops"), ps.info("exchanges"))
            assert (ps.info("exchanges_pipelined") > 0) == bool(pipe), (ps.info("exchanges_pipelined"), pipe)
            x, w1, w2, q = ps.gather_solution()
            assert ps.info("recovered") == (EXPECT_RECOVERED if was_resident else 0), (ps.info("recovered"), was_resident)
            sm, da = ps.costs(p)
            o = COracle(g.pos, g.edges, g.alpha, g.beta, g.z, g.wgt)
            o.solve(oparams(), iters)
            for name, got, want in (("x", x, o.x), ("w1", w1, o.w1), ("w2", w2, o.w2), ("q", q, o.q)):
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (V, k, name)
            so, do = o.costs(oparams())
            assert abs(sm - so) <= 1e-9 * so and abs(da - do) <= 1e-9 * do, (sm, so, da, do)
            if V == 6000 and pipe:  # a second frame on the same topology: new data terms, state reset
                z2 = (g.z * 1.07 + 0.01).astype(np.float32)
                ps.update_data(z2, g.wgt)
                ps.step(p, 33)
                o2 = COracle(g.pos, g.edges, g.alpha, g.beta, z2, g.wgt); o2.solve(oparams(), 33)
                assert np.array_equal(ps.gather_solution()[0].view(np.uint32), o2.x.view(np.uint32)), "update_data"
            if V == 50000 and EXPECT_RECOVERED == 0:  # (after a give-up the process sits out resident tiles for a while)
                assert was_resident == 1, "resident tiles in partition mode, on every part of the rank"
            total_recovered += ps.info("recovered")
            print("V %%d, %%d parts on rank 0, depth %%d: %%d P2P ops per exchange, %%d exchanges, resident tiles: %%d, "
                  "solves repeated after a give-up: %%d, bit-exact" %% (
                V, k, depth, ps.info("p2p_ops"), ps.info("exchanges"), was_resident, ps.info("recovered")))
    assert comm.info("rccl_ranks") == 1 and comm.info("world") == 1 and comm.info("shared_gpu") == 0
print("native partition ok, solves repeated in all: %%d" %% total_recovered)
''' % ROOT


def test_native_rccl_partition_with_itself(gpu):
    out = subprocess.run([sys.executable, "-c", CODE.replace("EXPECT_RECOVERED", "0")], cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "native partition ok" in out.stdout, out.stdout[-3000:] + out.stderr[-5000:]


def test_native_partition_repeats_a_give_up(gpu):
    """VERDICT r04 item 4 / ADVICE r04: a launch of resident tiles that gives up inside a partitioned solve used to be
    FLAME_HIP_ERR_STATE (the halo unpack had rewritten the state, the peers held records of the unfinished solve).  Now
    flame_hip_part_sync rolls every part back to the snapshot in front of the queued solves and repeats them by launches:
    the hooks library's persist_fail makes every resident launch report a give-up; every result must still be the oracle's."""
    from tests.util import hooks_env, with_hooks
    out = subprocess.run([sys.executable, "-c", with_hooks(CODE.replace("EXPECT_RECOVERED", "2"), persist_fail=1)], cwd=ROOT,
                         capture_output=True, text=True, timeout=900, env=hooks_env())
    assert out.returncode == 0 and "native partition ok" in out.stdout, out.stdout[-3000:] + out.stderr[-5000:]
    import re
    n = int(re.search(r"solves repeated in all: (\d+)", out.stdout).group(1))
    assert n >= 2, out.stdout[-3000:]  # (the 6 k graph's first two solves and its second frame; later graphs sit out the back-off)


@pytest.mark.parametrize("parts,depth,iters,V,peer", [(2, 8, 60, 8000, 0), (3, 4, 25, 12000, 0), (3, 4, 25, 12000, 1)])
def test_partitioned_graph_from_cpp(gpu, tmp_path, parts, depth, iters, V, peer):
    """tests/cpp/part_native.cc: the C++ mirror (flame::optimizers::nltgv2_l1_graph_regularizer::Communicator /
    PartitionedGraph / step / costs) against a single Graph handle on the same random Delaunay graph -- every bit."""
    exe = str(tmp_path / "part_native")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "part_native.cc"), "-o", exe,
                           "-L" + os.path.join(ROOT, "flame_ros_amd"), "-lflame_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "flame_ros_amd"), "-pthread"])
    p = subprocess.run([exe, "0", str(parts), str(depth), str(iters), str(V), str(peer)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "bit_exact 1 costs_ok 1" in p.stdout, (p.returncode, p.stdout, p.stderr)
