"""nkp_residual_batch* on row-distributed solvers: 2 and 3 processes on the one GPU of the test box over the library's file
transport, nrhs 1, 3 and 8.  Every rank's slice of R and the global berr have the bits of the single-GPU call on the whole matrix
(a maximum is order-free); rnorm and bnorm lie within the relative n 2^-52 of the exact values (tests/test_gpu_residual_batch.py
derives it: n rounded squares, n - 1 additions of non-negative terms in any order -- the ranks' partial sums and their allreduce are
one such order -- one square root) and are identical on all ranks.  The transport's callbacks are wrapped and recorded: a call is
exactly allgather, alltoallv, allreduce (sum, 2 K), allreduce (max, K), allgather.  A rank that passes a bad ldx still makes the
first agreement; every rank returns after it -- that rank NKP_EINVAL, the others NKP_ECOMM naming it -- and nothing else is
exchanged: an exchange between ranks that have not agreed on their arguments and buffers would not be safe to make."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -52


def launch(world, tmp):
    out = str(tmp / "r")
    comm_dir = tmp / "comm"
    comm_dir.mkdir()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), OMP_NUM_THREADS="2", NKP_COMM_TIMEOUT="120")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dist_residual_batch_worker.py"), "--out", out, "--file-dir", str(comm_dir)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=600)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log
    res = [json.load(open(f"{out}.{r}")) for r in range(world)]
    assert all(not r["comm_errors"] for r in res), res
    return res


@pytest.fixture(scope="module", params=[2, 3])
def bands(request, tmp_path_factory):
    return launch(request.param, tmp_path_factory.mktemp(f"rb{request.param}"))


def sequence(K):
    return ["allgather_i64_host", "alltoallv", f"allreduce sum {2 * K}", f"allreduce max {K}", "allgather_i64_host"]


@pytest.mark.parametrize("nrhs", [1, 3, 8])
def test_every_rank_has_the_bits_of_the_single_gpu_call(bands, nrhs):
    assert sum(r["m_loc"] for r in bands) == bands[0]["n"] and all(r["halo_rows"] > 0 for r in bands)
    for r in bands:
        c = r["good"][str(nrhs)]
        assert c["r_equal"] and c["sentinels"] and c["b_untouched"] and c["x_untouched"], c
        assert c["berr_equal"], c


@pytest.mark.parametrize("nrhs", [1, 3, 8])
def test_norms_are_global_identical_on_all_ranks_and_within_the_bound(bands, nrhs):
    n = bands[0]["n"]
    first = bands[0]["good"][str(nrhs)]
    for r in bands[1:]:
        c = r["good"][str(nrhs)]
        assert c["rnorm"] == first["rnorm"] and c["bnorm"] == first["bnorm"], (c, first)
    exact = bands[0]["exact"]
    for name in ("rnorm", "bnorm"):
        for k in range(nrhs):
            got, ref, one = float.fromhex(first[name][k]), float.fromhex(exact[name][k]), float.fromhex(first[name + "_single"][k])
            print(f"{name}[{k}]: distributed {got!r}, single-GPU {one!r}, exact {ref!r}: relative {abs(got - ref) / ref:.3e}, bound {n * U:.3e}")
            assert abs(got - ref) <= n * U * ref and abs(one - ref) <= n * U * ref


@pytest.mark.parametrize("nrhs", [1, 3, 8])
def test_the_callbacks_are_the_five_calls_in_order(bands, nrhs):
    K = 1 if nrhs == 1 else 4 if nrhs == 3 else 8
    for r in bands:
        c = r["good"][str(nrhs)]
        assert c["trace"] == sequence(K), c["trace"]
        assert c["counters"] == dict(alltoallv=1, allreduce=2, calls=1), c["counters"]
        if nrhs == 3:
            assert c["host_trace"] == sequence(K), c["host_trace"]
            assert c["host_r_equal"] and c["host_numbers_equal"], c


def test_a_bad_ldx_on_one_rank_is_told_to_all_and_nothing_else_is_exchanged(bands):
    for r in bands:
        c = r["refuse"]
        if c["bad"]:
            assert c["code"] == -1 and "ldx" in c["message"], c
        else:
            assert c["code"] == -5 and f"rank {c['bad_rank']}" in c["message"], c
        assert c["trace"] == ["allgather_i64_host"], c["trace"]             # the first agreement, made by the failing rank too
        assert c["counters"] == dict(alltoallv=0, allreduce=0, calls=0), c["counters"]
        assert c["r_untouched"] and c["next_equal"], c
