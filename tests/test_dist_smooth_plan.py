"""The lists of the fine-level exchange (tuning dist_smooth_exchange) in the host plan of nkp_create_dist: nkp_dist_overlap_plan_host
on CPU over gloo, latitude bands of 40x46x20 (seed 5), worlds 2, 3 and 8, one and two rings.  Per colour c = (i + j) % 2 of the
water columns: the rows a rank expects are exactly its overlap rows of that colour, each once, in hierarchy order; what rank p
sends to q is what q expects from p (checked on the gathered lists and by running the exchange); every sent row is an own row of
the sender; the counts agree both ways.  The planner also runs alone, all ranks as threads of the stand-alone program
tests/dist_smooth_plan_main.cpp built with the address and undefined-behaviour sanitizers, and must give the same lists."""
import json
import os
import subprocess
import sys

import pytest

from test_dist_gloo import free_port

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "nk_ocn_tracer_jacobian_precond_amd", "csrc")
LISTS = ("smooth_send_rows0", "smooth_send_rows1", "smooth_recv_rows0", "smooth_recv_rows1", "smooth_give0", "smooth_give1", "smooth_need0", "smooth_need1")


def launch(world, mode, out, extra=()):
    port = free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2",
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        for k in ("NKP_DIST_RAS_RINGS", "NKP_DIST_RAS", "NKP_DIST_SMOOTH_EXCHANGE"):
            env.pop(k, None)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dist_smooth_worker.py"), "--mode", mode, "--out", out, *extra],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=600)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log
    return [json.load(open(f"{out}.{r}")) for r in range(world)]


def check_lists(res, world, rings):
    for r in res:
        print(r["rank"], "ring columns", r["ring_cols"], "overlap rows", r["n_sel"], "give", r["give0"], r["give1"], "need", r["need0"], r["need1"])
    assert all(r["ras"] == 1 and r["smooth_exchange"] == 1 and r["ras_rings"] == rings for r in res), res
    for r in res:
        assert r["n_sel"] == r["n_sel_expected"] > 0, r["rank"]
        for c in (0, 1):
            for k in ("recv_rows_ok", "need_ok", "send_own_ok", "send_sorted_ok", "exchange_ok"):
                assert r[f"{k}{c}"], (r["rank"], k, c)
            # both colours together are all the overlap rows
        assert sum(r["need0"]) + sum(r["need1"]) == r["n_sel"], r["rank"]
    for c in (0, 1):
        for p in range(world):
            for q in range(world):
                assert res[p][f"give{c}"][q] == res[q][f"need{c}"][p], (c, p, q)               # the counts agree both ways
                assert res[p][f"sent{c}"][q] == res[q][f"expected{c}"][p], (c, p, q)           # what p sends q is what q expects from p
                if p == q:
                    assert res[p][f"give{c}"][q] == 0
    # both colours carry rows somewhere: the split is not trivially one-sided
    assert all(any(sum(r[f"need{c}"]) > 0 for r in res) for c in (0, 1))


@pytest.mark.parametrize("rings", [1, 2])
@pytest.mark.parametrize("world", [2, 3, 8])
def test_smooth_lists_over_gloo(tmp_path, world, rings):
    res = launch(world, "plan", str(tmp_path / "p"), extra=("--rings", str(rings)))
    check_lists(res, world, rings)


@pytest.mark.parametrize("world,ask_all", [(2, 1), (3, 1), (3, 0)])
def test_knob_zero_on_any_rank_leaves_every_list_empty(tmp_path, world, ask_all):
    """Rank 0 asks for 1 and the others for 0 (ask_all = 0: nobody asks): the smallest value holds."""
    res = launch(world, "off", str(tmp_path / "o"), extra=("--ask-all", str(ask_all)))
    assert [r["asked"] for r in res] == [ask_all] + [0] * (world - 1)
    for r in res:
        assert r["ras"] == 1 and r["smooth_exchange"] == 0, r
        assert all(v == 0 for v in r["sizes"].values()), r


@pytest.mark.parametrize("value,bad_rank", [(2, -1), (-1, -1), (2, 1), (7, 0)])
def test_out_of_range_value_is_refused_on_every_rank(tmp_path, value, bad_rank):
    res = launch(2, "refuse", str(tmp_path / "x"), extra=("--value", str(value), "--bad-rank", str(bad_rank)))
    for r in res:
        if r["bad"]:
            assert r["code"] == -1 and "dist_smooth_exchange" in r["message"], r        # NKP_EINVAL naming the field
        else:
            assert r["code"] == -5 and "failed its checks" in r["message"], r           # NKP_ECOMM naming the failing rank


def test_tuning_field_and_environment(monkeypatch):
    from nk_ocn_tracer_jacobian_precond_amd import solver
    monkeypatch.delenv("NKP_DIST_SMOOTH_EXCHANGE", raising=False)
    assert solver.default_tuning().dist_smooth_exchange == 0
    assert solver.default_tuning(dist_smooth_exchange=1).dist_smooth_exchange == 1
    monkeypatch.setenv("NKP_DIST_SMOOTH_EXCHANGE", "1")
    assert solver.default_tuning().dist_smooth_exchange == 1


# ---------------------------------------------------------------- the planner alone, under the sanitizers
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
STATIC_RUNTIME = ["-static-libasan", "-static-libubsan"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("dist_smooth_asan")
    probe = d / "probe.cpp"
    probe.write_text("int main () { return 0; }\n")
    if subprocess.run(["g++", "-fsanitize=address", *STATIC_RUNTIME, str(probe), "-o", str(d / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler cannot link -fsanitize=address")
    exe = str(d / "dist_smooth_plan_main")
    cxx = ["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", *SANITIZE]
    units = [os.path.join(HERE, "dist_smooth_plan_main.cpp"), os.path.join(CSRC, "dist_plan.cpp"), os.path.join(CSRC, "tuning.cpp")]
    objs = [str(d / (os.path.basename(u) + ".o")) for u in units]
    jobs = [subprocess.Popen([*cxx, "-c", u, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for u, o in zip(units, objs)]
    for j in jobs:                                   # any warning fails the build
        out = j.communicate()[0]
        assert j.returncode == 0 and not out.strip(), out
    r = subprocess.run([*cxx, *STATIC_RUNTIME, *objs, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    return exe


def test_planner_alone_under_the_sanitizers_gives_the_same_lists(tmp_path, program):
    """World 3, two rings: the lists of the gloo run against those of the same planner run as three threads of one sanitized
    process (no Python in it)."""
    case = str(tmp_path / "case.txt")
    res = launch(3, "plan", str(tmp_path / "p"), extra=("--rings", "2", "--dump", case))
    r = subprocess.run([program, case], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    got = {}
    for ln in r.stdout.splitlines():
        rank, name, *vals = ln.split()
        got[(int(rank), name)] = [int(v) for v in vals]
    for q in range(3):
        assert got[(q, "smooth_exchange")] == [1]
        for k in LISTS:
            assert got[(q, k)] == res[q]["lists"][k], (q, k)
