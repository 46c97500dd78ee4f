"""nkp_value_gradient on row-distributed solvers: 2 and 3 processes on the one GPU of the test box over the library's file
transport.  Every rank's values have the bits of its slice of the numpy formula on the GLOBAL matrix -- the halo rows of x
arrive in ONE alltoallv per call whatever K is -- also on the handle of nkp_transpose_dist, and a rank with a bad argument makes
every rank leave together."""
import json
import os
import subprocess
import sys

import pytest

from comm_trace import GOOD_CALL, REFUSED_CALL

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def launch(world, tmp, extra=(), env_extra=None):
    out = str(tmp / "r")
    comm_dir = tmp / "comm"
    comm_dir.mkdir()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), OMP_NUM_THREADS="2", NKP_COMM_TIMEOUT="120", NKP_ML_DEVICE_MIN="0",
                   NKP_ML_COARSEST_ROWS="300", **(env_extra or {}))
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dist_value_gradient_worker.py"), "--out", out, "--file-dir", str(comm_dir), *extra],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=600)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log
    res = [json.load(open(f"{out}.{r}")) for r in range(world)]
    assert all(not r["comm_errors"] for r in res), res
    return res


def assert_case(c, nnz):
    for key in ("host1", "host4", "device4"):
        assert c[key]["equal"], (key, c)
        assert c[key]["alltoallv"] == 1, (key, c)                  # exactly one exchange per call, for either K
    assert c["host1"]["size"] == c["host4"]["size"] == nnz, c
    assert c["calls"] == 3, c


@pytest.fixture(scope="module", params=[2, 3])
def bands(request, tmp_path_factory):
    return launch(request.param, tmp_path_factory.mktemp(f"vg{request.param}"))


def test_every_rank_has_the_bits_of_its_slice_of_the_global_formula(bands):
    assert sum(r["m_loc"] for r in bands) > 0 and all(r["bits"]["halo_rows"] > 0 for r in bands)
    for r in bands:
        assert_case(r["bits"], r["nnz_loc"])


def test_transposed_dist_handle(bands):
    for r in bands:
        assert r["transposed"]["nnz_equal"] and r["transposed"]["halo_rows"] > 0, r
        assert_case(r["transposed"], r["transposed"]["host1"]["size"])


def test_a_bad_argument_on_one_rank_is_told_to_all(bands):
    for r in bands:
        c = r["refuse"]
        if c["bad"]:
            assert c["code"] == -1 and "nrhs" in c["message"], c
        else:
            assert c["code"] == -5 and f"rank {c['bad_rank']}" in c["message"], c
        assert c["calls_unchanged"] and c["next_equal"], c


def test_the_callbacks_are_agreement_exchange_agreement(bands):
    """K = 1, the first call at K = 4 (which makes the K-wide exchange buffers) and the host flavour make the same three calls; a
    rank with nine pairs makes the first agreement and every rank leaves after it, with nothing written and nothing counted"""
    for r in bands:
        t = r["trace"]
        for key in ("device1", "device3", "host3"):
            assert t[key]["trace"] == GOOD_CALL, (key, t[key])
            assert t[key]["counters"] == dict(alltoallv=1, allreduce=0, calls=1) and t[key]["equal"], (key, t[key])
        c = t["refuse"]
        if c["bad"]:
            assert c["code"] == -1 and "nrhs" in c["message"], c
        else:
            assert c["code"] == -5 and f"rank {c['bad_rank']}" in c["message"], c
        assert c["trace"] == REFUSED_CALL, c["trace"]
        assert c["counters"] == dict(alltoallv=0, allreduce=0, calls=0), c["counters"]
        assert c["g_untouched"] and c["next_equal"], c


def test_multilevel_solver_with_overlap(tmp_path):
    """the hierarchy's overlap changes the halo plan (whole water columns) and the K-wide buffers (shared with the batched solve)"""
    res = launch(2, tmp_path, ("--precond", "multilevel", "--cases", "bits"))
    for r in res:
        assert_case(r["bits"], r["nnz_loc"])


def test_one_rank_forced_distributed(tmp_path):
    res = launch(1, tmp_path, ("--cases", "bits",), {"NKP_FORCE_DIST": "1"})
    c = res[0]["bits"]
    assert c["halo_rows"] == 0
    assert_case(c, res[0]["nnz_loc"])
