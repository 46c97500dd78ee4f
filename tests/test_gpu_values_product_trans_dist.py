"""nkp_values_product_trans_dist* on row-distributed solvers: 2 and 3 processes on the one GPU of the test box over the library's
file transport.  Every rank's slice of y = alpha G^T x has the bits of the numpy restatement on the GLOBAL transposed pattern -- the
bits of the single-GPU product, whatever the number of ranks -- with one alltoallv per call; the index is built once and kept; the
product is the adjoint of nkp_values_product; a column longer than 2048 entries assembled from every rank takes the SpMV's tree; a
rank with a bad argument makes every rank leave together; the handles that are refused are refused without a collective."""
import json
import os
import subprocess
import sys

import pytest

from comm_trace import AGREE, GOOD_CALL, REFUSED_CALL

pytestmark = pytest.mark.gpu
# the call that builds the transposed index (recorded from the library before the envelope of these calls was shared)
BUILDING_CALL = [AGREE, "alltoallv_i32_host", AGREE] + GOOD_CALL[1:]

HERE = os.path.dirname(os.path.abspath(__file__))


def launch(world, tmp):
    out = str(tmp / "r")
    comm_dir = tmp / "comm"
    comm_dir.mkdir()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), OMP_NUM_THREADS="2", NKP_COMM_TIMEOUT="120", NKP_ML_DEVICE_MIN="0",
                   NKP_ML_COARSEST_ROWS="300")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dist_values_product_trans_worker.py"), "--out", out, "--file-dir", str(comm_dir)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=600)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log
    res = [json.load(open(f"{out}.{r}")) for r in range(world)]
    assert all(not r["comm_errors"] for r in res), res
    return res


@pytest.fixture(scope="module", params=[2, 3])
def bands(request, tmp_path_factory):
    return launch(request.param, tmp_path_factory.mktemp(f"vpt{request.param}"))


def _assert_bits(c, where):
    assert c["acc_equal"] and c["tail"] and c["x_untouched"], (where, c)        # alpha = 0.37 added to a seeded y, sentinel tails, poisoned x tails
    assert c["write_equal"] and c["write_tail"], (where, c)                     # alpha = -1 written over NaN
    assert c["alltoallv"] == 1 and c["calls"] == 1, (where, c)                  # one exchange per product, for any nrhs


def test_device_flavour_has_the_bits_of_the_global_restatement_on_every_rank(bands):
    assert sum(r["m_loc"] for r in bands) > 0
    for r in bands:
        for K in ("1", "3", "4", "8"):
            _assert_bits(r["bits"][K], (r["rank"], K))


def test_host_flavour_has_the_bits_of_the_global_restatement(bands):
    for r in bands:
        c = r["host"]
        assert c["acc_equal"] and c["write_equal"] and c["alltoallv"] == 1 and c["calls"] == 1, c


def test_index_is_built_once_kept_and_counted(bands):
    assert all(r["halo_rows"] > 0 for r in bands)
    for r in bands:
        assert r["index_bytes_at_start"] == 0 and r["bits"]["1"]["index_before"] == 0
        idx = r["bits"]["1"]["index_after"]
        assert idx > 0
        assert all(r["bits"][K]["index_before"] == idx and r["bits"][K]["index_after"] == idx for K in ("3", "4", "8"))
        c = r["after_refactor"]                                                 # refactor_dist with new values: the pattern is kept
        assert c["index_kept"] and c["index_before"] == idx and c["index_after"] == idx
        _assert_bits(c, (r["rank"], "after refactor"))
    assert sum(r["sent_entries"] for r in bands) == sum(r["recv_entries"] for r in bands)
    assert any(r["sent_entries"] > 0 for r in bands)


def test_the_callbacks_of_the_building_call_and_of_the_steady_state(bands):
    """the first call agrees, exchanges the entry counts of the index on the host, agrees that every rank built its part, and goes on
    as every later call does, device or host flavour and whatever nrhs is: agreement, ONE exchange, agreement"""
    for r in bands:
        assert r["bits"]["1"]["trace"] == BUILDING_CALL, r["bits"]["1"]["trace"]
        assert r["bits"]["1"]["write_trace"] == GOOD_CALL, r["bits"]["1"]["write_trace"]
        for K in ("3", "4", "8"):
            assert r["bits"][K]["trace"] == GOOD_CALL and r["bits"][K]["write_trace"] == GOOD_CALL, (K, r["bits"][K])
        assert all(r["bits"][K]["allreduce"] == 0 for K in ("1", "3", "4", "8")), r["bits"]
        assert r["host"]["trace"] == GOOD_CALL, r["host"]["trace"]


def test_adjoint_of_the_values_product(bands):
    """<G^T x, z> and <x, G z> are sums of the same nnz products val[e] x[i] z[j] in different orders: they differ by a few thousand
    roundings of 1e-16 at the most"""
    lhs, rhs = sum(r["adjoint"]["gtx_z"] for r in bands), sum(r["adjoint"]["x_gz"] for r in bands)
    assert lhs != 0.0 and abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (lhs, rhs)


def test_long_column_from_every_rank_and_noncanonical_rows(bands):
    for r in bands:
        c = r["long"]
        assert c["long_rows"] == [c["jstar"]] and c["column_entries"] > 2048 and all(k > 0 for k in c["per_rank"]), c
        assert c["descending"] and c["repeated"], c
        for K in ("1", "4"):
            _assert_bits(c["bits"][K], (r["rank"], "long", K))
    assert sum(r["long"]["owner"] for r in bands) == 1


def test_a_bad_argument_on_one_rank_is_told_to_all(bands):
    for r in bands:
        assert r["multilevel_equal"]
        for c in r["refuse"]:                                                   # once before the index exists, once after
            assert c["had_index"] == c["want_index"], c
            if c["bad"]:
                assert c["code"] == -1 and "nrhs" in c["message"], c
            else:
                assert c["code"] == -5 and f"rank {c['bad_rank']}" in c["message"], c
            assert c["calls_unchanged"] and c["index_unchanged"] and c["next_solve_equal"], c
            assert c["trace"] == REFUSED_CALL and c["exchanges"] == 0, c        # the first agreement, made by the failing rank too
            assert c["y_untouched"] and c["next_equal"], c
            assert c["next_trace"] == (GOOD_CALL if c["want_index"] else BUILDING_CALL), c


def test_transposed_handle_is_refused_without_a_collective(bands):
    for r in bands:
        c = r["handle"]
        assert c["code"] == -1 and "nkp_values_product_trans_dist_device" in c["message"] and "owner" in c["message"], c
        assert c["y_untouched"] and c["files_unchanged"] and c["counters_unchanged"], c


def test_force_dist_on_one_rank_has_the_single_gpu_bits(bands):
    c = bands[0]["solo"]
    assert c["distributed"] and c["index"] and c["sent"] == 0 and c["recv"] == 0, c
    assert c["equal_plain"] and c["equal_reference"], c
    assert c["plain_equal"] and c["plain_calls"] == 2, c                        # on a plain solver the call is nkp_values_product_trans_device
