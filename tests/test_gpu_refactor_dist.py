"""nkp_refactor_dist: new values on a row-distributed solver.  Ranks share the one GPU of the test box (gloo + host staging of
the collectives).  On every rank the refactored solver is bit for bit a fresh nkp_create_dist of the new values: every array of
every hierarchy level, the SpMV, the preconditioner, the solution slice and the iteration count."""
import json
import os
import subprocess
import sys

import pytest

from test_dist_gloo import free_port

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL_LEVELS = {"NKP_ML_DEVICE_MIN": "0", "NKP_ML_COARSEST_ROWS": "300"}     # setup kernels and the dense inverse exercised


def launch(world, out, extra=(), env_extra=None):
    port = free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0", **SMALL_LEVELS, **(env_extra or {}))
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dist_refactor_worker.py"), "--out", out, *extra],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=600)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log
    return [json.load(open(f"{out}.{r}")) for r in range(world)]


def assert_fresh(res, case):
    """every rank equals its fresh nkp_create_dist and the refactored solve converged the same way everywhere"""
    rows = [r[case] for r in res]
    for r in rows:
        assert r["hier_diff"] == [], (case, r)
        assert r["spmv_equal"] and r["precond_equal"] and r["x_equal"], (case, r)
        assert r["iters"] == r["iters_fresh"], (case, r)
        assert r["status"] == 0 and r["relres"] <= 1e-10, (case, r)
    assert len({r["iters"] for r in rows}) == 1, (case, rows)
    assert all(not r["comm_errors"] for r in res), res


@pytest.fixture(scope="module", params=[2, 3])
def bands(request, tmp_path_factory):
    world = request.param
    out = str(tmp_path_factory.mktemp(f"bands{world}") / "r")
    return launch(world, out, ("--cases", "same,device,mixed,rebuild,drift,refuse"))


def test_same_cells_host_and_device_values(bands):
    for case in ("same", "device"):
        assert_fresh(bands, case)
        for r in bands:
            c = r[case]
            assert c["rebuilt"] == 0 and c["count"] == 1 and c["refactor_us"] > 0, c
            assert c["ras"] == 1, c
            if c["ras_rows"] > 0:
                assert c["halo_values"] > 0, c


def test_the_exchange_is_real(bands):
    """only rank 0 passes new values: rank 1's hierarchy changes through its overlap rows alone"""
    assert_fresh(bands, "mixed")
    assert bands[1]["mixed"]["level0_changed"], bands[1]["mixed"]


def test_rebuild_flag_gives_the_fresh_hierarchy(bands):
    assert_fresh(bands, "rebuild")
    assert all(r["rebuild"]["rebuilt"] == 1 for r in bands)


def test_drift_rebuilds_only_the_ranks_that_see_it(bands):
    for case in ("drift_own", "drift_overlap"):
        assert_fresh(bands, case)
        assert all(r[case]["candidates"] > 0 for r in bands)
        assert [r[case]["rebuilt"] for r in bands] == [r[case]["expect_rebuilt"] for r in bands], [r[case] for r in bands]
    assert [r["drift_own"]["rebuilt"] for r in bands] == [int(k == 1) for k in range(len(bands))]
    assert bands[1]["drift_overlap"]["rebuilt"] == 1            # rank 1's own values did not change


def test_refusal_is_collective(bands):
    for r in bands:
        c = r["refuse"]
        if r["rank"] == 1:
            assert c["code"] == -4, c
        else:
            assert c["code"] == -5 and "rank 1" in c["message"], c
        assert c["unchanged"] and c["count"] == 0, c
    assert_fresh([dict(r, after=r["refuse"]["after"]) for r in bands], "after")


@pytest.mark.parametrize("layout", ["no_overlap", "tracers", "column_jacobi"])
def test_other_layouts(tmp_path, layout):
    extra, env = ["--cases", "same"], None
    if layout == "no_overlap":
        env = {"NKP_DIST_RAS": "0"}
    elif layout == "tracers":
        extra += ["--partition", "tracers"]
    else:
        extra += ["--precond", "column"]
    res = launch(2, str(tmp_path / "r"), extra, env)
    assert_fresh(res, "same")
    for r in res:
        assert r["same"]["ras"] == 0 and r["same"]["halo_values"] == 0, r
        assert r["same"]["rebuilt"] == 0 and r["same"]["count"] == 1, r


def test_one_rank_forced_distributed(tmp_path):
    res = launch(1, str(tmp_path / "r"), ["--cases", "same,rebuild"], {"NKP_FORCE_DIST": "1"})
    assert_fresh(res, "same")
    assert_fresh(res, "rebuild")
    assert res[0]["same"]["rebuilt"] == 0 and res[0]["same"]["halo_values"] == 0
