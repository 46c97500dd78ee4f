"""nkp_values_product* and nkp_solve_tangent_device on row-distributed solvers: 2 and 3 processes on the one GPU of the test box
over the library's file transport.  Every rank's slice of y has the bits of the numpy restatement on its local CSR -- the halo rows
of x arrive in ONE alltoallv per product whatever nrhs is -- the tangent solve is the composition it is documented to be on every
rank, and a rank with a bad argument, or one that alone passes no d_dval, makes every rank leave together."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def launch(world, tmp):
    out = str(tmp / "r")
    comm_dir = tmp / "comm"
    comm_dir.mkdir()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), OMP_NUM_THREADS="2", NKP_COMM_TIMEOUT="120", NKP_ML_DEVICE_MIN="0",
                   NKP_ML_COARSEST_ROWS="300")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dist_values_product_worker.py"), "--out", out, "--file-dir", str(comm_dir)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=600)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log
    res = [json.load(open(f"{out}.{r}")) for r in range(world)]
    assert all(not r["comm_errors"] for r in res), res
    return res


@pytest.fixture(scope="module", params=[2, 3])
def bands(request, tmp_path_factory):
    return launch(request.param, tmp_path_factory.mktemp(f"vp{request.param}"))


def test_every_rank_has_the_bits_of_the_restatement_on_its_local_rows(bands):
    assert sum(r["m_loc"] for r in bands) > 0 and all(r["halo_rows"] > 0 for r in bands)
    for r in bands:
        for K in ("1", "3", "4"):
            c = r["bits"][K]
            assert c["equal"] and c["tail"] and c["host_equal"], (K, c)
            assert c["alltoallv"] == 1 and c["host_alltoallv"] == 1 and c["calls"] == 1, (K, c)      # one exchange per product, for any nrhs


def test_tangent_solve_is_the_composition_on_every_rank(bands):
    for r in bands:
        for K in ("1", "3", "4"):
            c = r["tangent"][K]
            assert c["equal"] and c["infos_equal"] and all(st == 0 for st in c["status"]), (K, c)
            assert c["product_calls"] == 1 and c["tangent_calls"] == 1, (K, c)
            assert c["no_dval_equal"] and c["no_dval_same_exchanges"], (K, c)                        # without d_dval: no product exchange


def test_a_bad_argument_on_one_rank_is_told_to_all(bands):
    for r in bands:
        c = r["refuse"]
        if c["bad"]:
            assert c["code"] == -1 and "nrhs" in c["message"], c
        else:
            assert c["code"] == -5 and f"rank {c['bad_rank']}" in c["message"], c
        assert c["calls_unchanged"] and c["next_solve_equal"], c


def test_a_rank_that_alone_passes_no_dval_makes_every_rank_return(bands):
    for r in bands:
        c = r["mismatch"]
        assert c["code"] == -1 and f"rank {c['bad_rank']}" in c["message"] and "d_dval" in c["message"], c
        assert c["next_solve_equal"], c
