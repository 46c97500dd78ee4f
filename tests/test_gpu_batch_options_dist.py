"""Batched right-hand sides with chained preconditioner cycles (precond_steps = 2) on the row-distributed solver: K systems in
lockstep on every rank, each stage of a step -- cycle, residual, cycle, operator -- with the exchange of ONE system.  The yardstick
is the same distributed solver's one-at-a-time solves: bits per column, and the collectives of a lockstep step counted against
those of a single solve's step (e exchanges, a allreduces).  Ranks share the one GPU of the test box (gloo + host staging, or the
library's file transport); 40 x 46 x 20 in latitude bands."""
import json
import os
import subprocess
import sys

import pytest

from test_dist_gloo import free_port

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = 2


def launch(world, out, cases, extra=(), env_extra=None):
    port = free_port()
    procs = []
    args = ["--out", out, "--cases", cases, "--opts", json.dumps({"precond_steps": STEPS}), *extra]
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0", **(env_extra or {}))
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dist_batch_options_worker.py"), *args],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=600)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log
    res = [json.load(open(f"{out}.{r}")) for r in range(world)]
    assert all(not r["comm_errors"] for r in res), res
    for r in res:
        assert r["guards"]["equil"] == 0 and r["guards"]["precond_steps"] == STEPS, r["guards"]
    return res


def assert_bits(res, nrhs_list):
    for r in res:
        for nrhs in nrhs_list:
            got = r["bits"][str(nrhs)]
            assert len(got["columns"]) == nrhs
            for c, col in enumerate(got["columns"]):
                assert col["x_equal"], (r["rank"], nrhs, c, col)
                assert col["iters"] == col["iters_single"] and col["relres_equal"] and col["berr_equal"], (r["rank"], nrhs, c, col)
            assert got["delta"]["batch_steps"] > 0, (r["rank"], nrhs, got["delta"])
    for nrhs in nrhs_list:                                # every rank took the same global decisions
        assert len({tuple(col["iters"] for col in r["bits"][str(nrhs)]["columns"]) for r in res}) == 1


def assert_counts(res, e, a):
    """The identities of tests/test_gpu_batch_dist.py: e exchanges and a allreduces per Krylov step of ONE system, whatever the
    number of systems in the group.  What a solve spends outside its steps (restarts, verdicts) is per system in both."""
    for r in res:
        S = [s["delta"]["dist_alltoallv_calls"] for s in r["single"][:4]]
        R = [s["delta"]["dist_allreduce_calls"] for s in r["single"][:4]]
        I = [s["iters"] for s in r["single"][:4]]
        for c in range(4):
            assert I[c] > 0 and S[c] >= e * I[c] and R[c] >= a * I[c], (r["rank"], c, S[c], R[c], I[c], e, a)
            assert S[c] < (e + 1) * I[c], (r["rank"], c, S[c], I[c], e)          # e is the count per step, not a lower bound of it
        b = r["counts"]
        Sb, Rb, Tb = b["delta"]["dist_alltoallv_calls"], b["delta"]["dist_allreduce_calls"], b["delta"]["batch_steps"]
        print(f"rank {r['rank']}: I={I} S={S} R={R}  batched: steps={Tb} alltoallv={Sb} allreduce={Rb}")
        assert max(I) <= Tb < sum(I), (Tb, I)
        assert Sb <= sum(S[c] - e * I[c] for c in range(4)) + e * Tb, (Sb, S, I, Tb)
        assert Rb <= sum(R[c] - a * I[c] for c in range(4)) + a * Tb, (Rb, R, I, Tb)
        assert b["batch_width"] == 4
        for c, col in enumerate(b["columns"]):
            assert col["x_equal"] and col["iters"] == I[c], (r["rank"], c, col)


def test_two_ranks_gloo(tmp_path):
    res = launch(2, str(tmp_path / "r"), "bits,counts")
    assert_bits(res, (2, 3, 4, 5))
    assert all(r["guards"]["ras"] == 1 and r["guards"]["ras_rows"] > 0 and r["guards"]["overlap"] == 1 for r in res), res
    assert_counts(res, e=2 * STEPS, a=2)


def test_three_ranks_file_transport(tmp_path):
    comm_dir = tmp_path / "comm"
    comm_dir.mkdir()
    res = launch(3, str(tmp_path / "r"), "bits,counts", extra=("--comm", "file", "--file-dir", str(comm_dir), "--nrhs", "3,4"),
                 env_extra={"NKP_COMM_TIMEOUT": "120"})
    assert_bits(res, (3, 4))
    assert_counts(res, e=2 * STEPS, a=2)


@pytest.mark.parametrize("name,env,e", [("no_ras", {"NKP_DIST_RAS": "0"}, STEPS), ("two_rings", {"NKP_DIST_RAS_RINGS": "2"}, 2 * STEPS)])
def test_two_ranks_other_overlaps(tmp_path, name, env, e):
    res = launch(2, str(tmp_path / "r"), "bits,counts", extra=("--nrhs", "3,4"), env_extra=env)
    assert_bits(res, (3, 4))
    assert all(r["guards"]["ras"] == (0 if name == "no_ras" else 1) for r in res), res
    assert_counts(res, e, a=2)
