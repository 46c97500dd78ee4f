"""nkp_set_solve_controls and nkp_solve_batch_device_ex on a row-distributed solver: two processes on the one GPU of the test box
over the library's file transport.  The worker (tests/dist_solve_controls_worker.py) runs once; the tests read what it recorded.
Every comparison is equality of bits, against solvers created with the values or against single solves."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GATHER = "allgather_i64_host"


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("controls")
    comm_dir = tmp / "comm"
    comm_dir.mkdir()
    out = str(tmp / "r")
    procs = []
    for r in range(2):
        env = dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0", NKP_COMM_TIMEOUT="60")
        # every process under a time limit of its own; a rank that dies ends its peer through the transport's deadline
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(HERE, "dist_solve_controls_worker.py"), "--out", out,
                                       "--rank", str(r), "--world", "2", "--file-dir", str(comm_dir)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate()[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log
    res = [json.load(open(f"{out}.{r}")) for r in range(2)]
    assert all(not r["comm_errors"] for r in res), res
    for r in res:                                            # really two ranks with a halo and a hierarchy of several levels
        assert r["dist_on"]["halo"] > 0 and r["dist_on"]["levels"] >= 3, r["dist_on"]
    return res


def test_equal_values_give_the_bits_of_solvers_created_with_them(ranks):
    for r in ranks:
        got = r["setter"]
        assert got["set_controls"] == dict(rtol=1e-3, atol=0.0, max_iters=200)
        assert got["set"] == got["created_with"], r["rank"]
        assert got["set"] != got["untouched"]
        assert got["reset_controls"] == got["created"] == dict(rtol=1e-10, atol=0.0, max_iters=300)
        assert got["reset"] == got["untouched"], r["rank"]


def test_setter_makes_three_allgathers_whatever_happens_locally(ranks):
    for r in ranks:
        got = r["setter"]
        for key in ("set_calls", "mismatch_calls", "mismatch_iters_calls", "local_calls", "reset_calls"):
            assert got[key] == [GATHER] * 3, (r["rank"], key, got[key])


def test_different_values_are_refused_on_both_ranks_and_change_nothing(ranks):
    for r in ranks:
        got = r["setter"]
        assert got["mismatch"]["code"] == -1 and "rank 1" in got["mismatch"]["message"] and "rtol" in got["mismatch"]["message"], got["mismatch"]
        assert got["mismatch_iters"]["code"] == -1 and "rank 1" in got["mismatch_iters"]["message"] and "max_iters" in got["mismatch_iters"]["message"]
        assert got["local_code"] == -1 and "rank 1" in got["local_message"], got["local_message"]
        assert got["mismatch_controls"] == got["set_controls"] == got["after_refusals_controls"]
        assert got["after_refusals"] == got["set"], r["rank"]
    assert "NaN" in ranks[1]["setter"]["local_message"]          # the rank that failed says why


def test_ex_columns_have_the_bits_of_their_single_solves(ranks):
    for r in ranks:
        got = r["ex"]
        for nrhs in (5, 2):
            ex = got[f"ex{nrhs}"]
            assert ex["columns"] == got["single"][:nrhs], (r["rank"], nrhs, [c["infos"] for c in ex["columns"]], [c["infos"] for c in got["single"][:nrhs]])
            assert ex["first_call"] == GATHER and ex["batch_steps"] > 0
            assert ex["controls"] == dict(rtol=1e-10, atol=0.0, max_iters=300)
        assert all(c["infos"][0][0] == 0 for c in got["single"])
        assert len({c["infos"][0][1] for c in got["single"]}) > 1        # the tolerances were read: different iteration counts
    assert [c["infos"] for c in ranks[0]["ex"]["single"]] == [c["infos"] for c in ranks[1]["ex"]["single"]]


def test_mismatching_arrays_are_refused_before_any_exchange(ranks):
    for r in ranks:
        got = r["ex"]
        for key in ("mismatch", "mismatch_null"):
            assert got[key]["code"] == -1 and "rank 1" in got[key]["message"] and "nothing solved" in got[key]["message"], got[key]
            assert got[key + "_calls"] == [GATHER], (r["rank"], key, got[key + "_calls"])
        assert got["mismatch_alltoallv"] == 0
        assert got["after_mismatch"] == got["single"][:2]
