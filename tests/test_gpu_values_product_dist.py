"""nkp_values_product* and nkp_solve_tangent_device on row-distributed solvers: 2 and 3 processes on the one GPU of the test box
over the library's file transport.  Every rank's slice of y has the bits of the numpy restatement on its local CSR -- the halo rows
of x arrive in ONE alltoallv per product whatever nrhs is -- the tangent solve is the composition it is documented to be on every
rank, and a rank with a bad argument, or one that alone passes no d_dval, makes every rank leave together."""
import json
import os
import subprocess
import sys

import pytest

from comm_trace import AGREE, GOOD_CALL, REFUSED_CALL

pytestmark = pytest.mark.gpu
# what nkp_solve_batch_device calls first, by nrhs (recorded from the library before the envelope of these calls was shared)
TANGENT_SOLVE_FIRST = {1: ["allreduce sum 1"], 3: [AGREE]}

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


def _assert_refused(c, output):
    if c["bad"]:
        assert c["code"] == -1 and "nrhs" in c["message"], c
    else:
        assert c["code"] == -5 and f"rank {c['bad_rank']}" in c["message"], c
    assert c["trace"] == REFUSED_CALL, c["trace"]                              # the first agreement, made by the failing rank too
    assert c["counters"] == dict(alltoallv=0, allreduce=0, calls=0), c["counters"]
    assert c[output], c


def test_the_callbacks_are_agreement_exchange_agreement(bands):
    """nrhs = 1, the solver's first call at width 4 (which makes the K-wide exchange buffers) and the host flavour make the same
    three calls; a rank with nine vectors makes the first agreement and every rank leaves after it, nothing written or counted"""
    for r in bands:
        t = r["trace"]
        for key in ("device1", "device3", "host3"):
            assert t[key]["trace"] == GOOD_CALL, (key, t[key])
            assert t[key]["counters"] == dict(alltoallv=1, allreduce=0, calls=1), (key, t[key])
        assert t["host3"]["equal"], t["host3"]
        _assert_refused(t["refuse"], "y_untouched")
        assert t["refuse"]["next_equal"], t["refuse"]


def test_the_tangent_solve_makes_the_products_calls_then_the_batched_solves(bands):
    """its own first agreement, the product's exchange and second agreement, then the first callback of nkp_solve_batch_device: at
    nrhs = 1 the reduction of the first norms, at the first width 4 the agreement on the interleave width"""
    for r in bands:
        t = r["trace"]
        assert t["tangent1"] == dict(trace=GOOD_CALL + TANGENT_SOLVE_FIRST[1], calls=1), t["tangent1"]
        assert t["tangent3"] == dict(trace=GOOD_CALL + TANGENT_SOLVE_FIRST[3], calls=1), t["tangent3"]
        _assert_refused(t["tangent_refuse"], "y_untouched")


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
