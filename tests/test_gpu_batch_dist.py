"""Batched right-hand sides on the row-distributed solver (nkp_solve with nrhs >= 2 / nkp_solve_batch_device on a solver made by
nkp_create_dist with more than one rank): K systems in lockstep on every rank with the collectives of ONE system per Krylov
step.  The yardstick throughout is the same distributed solver's one-at-a-time solves; for accuracy the CPU oracle's SpMV.
Ranks share the one GPU of the test box (gloo + host staging, or the library's file transport)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from test_dist_gloo import free_port

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def launch(world, out, cases, extra=(), env_extra=None, opts=None):
    port = free_port()
    procs = []
    args = ["--out", out, "--cases", cases, "--opts", json.dumps(opts or {}), *extra]
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0", **(env_extra or {}))
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dist_batch_worker.py"), *args],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=600)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log
    res = [json.load(open(f"{out}.{r}")) for r in range(world)]
    assert all(not r["comm_errors"] for r in res), res
    return res


def assert_batched_path(res):
    """none of the cases below may pass through a silent fallback"""
    for r in res:
        assert r["guards"]["equil"] == 0 and r["guards"]["precond_steps"] == 1, r["guards"]


def assert_bits(res, key, nrhs_list):
    assert_batched_path(res)
    for r in res:
        for nrhs in nrhs_list:
            got = r[key][str(nrhs)]
            assert len(got["columns"]) == nrhs
            for c, col in enumerate(got["columns"]):
                assert col["x_equal"], (key, r["rank"], nrhs, c, col)
                assert col["iters"] == col["iters_single"] and col["relres_equal"] and col["berr_equal"], (key, r["rank"], nrhs, c, col)
            assert got["delta"]["batch_steps"] > 0, (key, r["rank"], nrhs, got["delta"])
    for nrhs in nrhs_list:                                # every rank took the same global decisions
        assert len({tuple(col["iters"] for col in r[key][str(nrhs)]["columns"]) for r in res}) == 1


def assert_counts(res, e, a):
    """Collectives do not grow with K: identities of the lockstep structure (e exchanges and a allreduces per Krylov step of
    ONE system, whatever the number of systems in the group)."""
    assert_batched_path(res)
    for r in res:
        S = [s["delta"]["dist_alltoallv_calls"] for s in r["single"][:4]]
        R = [s["delta"]["dist_allreduce_calls"] for s in r["single"][:4]]
        I = [s["iters"] for s in r["single"][:4]]
        for c in range(4):
            assert I[c] > 0 and S[c] >= e * I[c] and R[c] >= a * I[c], (r["rank"], c, S[c], R[c], I[c], e, a)
        b = r["counts"]
        Sb, Rb, Tb = b["delta"]["dist_alltoallv_calls"], b["delta"]["dist_allreduce_calls"], b["delta"]["batch_steps"]
        print(f"rank {r['rank']}: I={I} S={S} R={R}  batched: steps={Tb} alltoallv={Sb} allreduce={Rb}")
        assert max(I) <= Tb < sum(I), (Tb, I)
        assert Sb <= sum(S[c] - e * I[c] for c in range(4)) + e * Tb, (Sb, S, I, Tb)
        assert Rb <= sum(R[c] - a * I[c] for c in range(4)) + a * Tb, (Rb, R, I, Tb)
        assert b["batch_width"] == 4
        for c, col in enumerate(b["columns"]):
            assert col["x_equal"] and col["iters"] == I[c], (r["rank"], c, col)


# ---------------------------------------------------------------- 1, 4, 6: two ranks over gloo
@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("two") / "r")
    return launch(2, out, "bits,counts,zero,refactor")


def test_bits_two_ranks(two_ranks):
    assert_bits(two_ranks, "bits", (2, 3, 4, 5))
    assert all(r["guards"]["ras"] == 1 and r["guards"]["ras_rows"] > 0 and r["guards"]["overlap"] == 1 for r in two_ranks), two_ranks


def test_collectives_do_not_grow_with_K(two_ranks):
    assert_counts(two_ranks, e=2, a=2)


def test_zero_and_mixed_right_hand_sides(two_ranks):
    for r in two_ranks:
        cols = r["zero"]["columns"]
        assert cols[1]["iters"] == 0 and cols[1]["zero_x"] and cols[1]["status"] == 0, cols[1]
        for c in (0, 2):
            assert cols[c]["x_equal"] and cols[c]["iters"] == cols[c]["iters_single"] and cols[c]["relres_equal"], (r["rank"], c, cols[c])
        assert r["zero"]["delta"]["batch_steps"] > 0


def test_batched_call_after_refactor_dist_sees_the_new_values(two_ranks):
    for r in two_ranks:
        got = r["refactor"]
        assert got["refactor_count"] == 1 and got["batch_steps"] > 0, got
        for c, col in enumerate(got["columns"]):
            assert col["x_equal"] and col["iters"] == col["iters_single"] and col["relres_equal"] and col["status"] == 0, (r["rank"], c, col)
            assert col["differs_from_old"], (r["rank"], c)


@pytest.mark.parametrize("name,env,opts,e,a", [("ml_f64", {"NKP_ML_F32": "0"}, {}, 2, 2), ("no_ras", {"NKP_DIST_RAS": "0"}, {}, 1, 2),
                                               ("one_reduce", {"NKP_DIST_ONE_REDUCE": "1"}, {}, 2, 1), ("reorth", {}, {"reorth": 1}, 2, 3)])      # reorth: two multi-dot passes and the norm
def test_bits_two_ranks_variants(tmp_path, name, env, opts, e, a):
    res = launch(2, str(tmp_path / "r"), "bits,counts", env_extra=env, opts=opts)
    assert_bits(res, "bits", (2, 3, 4, 5))
    if name == "no_ras":
        assert all(r["guards"]["ras"] == 0 for r in res)
    assert_counts(res, e, a)


def test_bits_eight_per_sweep(tmp_path):
    res = launch(2, str(tmp_path / "r"), "bits", extra=("--nvec", "9", "--nrhs", "9"), opts={"tuning": {"rhs_batch": 8}})
    assert_bits(res, "bits", (9,))
    assert all(r["bits"]["9"]["batch_width"] == 8 for r in res)


def test_width_narrows_on_a_live_solver(tmp_path):
    """Groups of 8, 2 and 4 right-hand sides and then a solve alone on ONE solver, two rings of overlap and the fine-level exchange
    in force: the SpMV halo, the overlap residual's own exchange and both colours of the fine-level exchange go from 8-wide rows
    to 2-wide, 4-wide and single rows.  Every column has the bits of its single solve, and a lockstep step makes the exchanges of
    one system at every width: the SpMV's, the overlap residual's and the 11 of a V(3, 3) cycle."""
    tuning = {"rhs_batch": 8, "dist_ras_rings": 2, "dist_smooth_exchange": 1, "ml_coarsest_rows": 4000}      # (level 0 smooths on every rank)
    res = launch(2, str(tmp_path / "r"), "narrow", extra=("--nvec", "8"), opts={"tuning": tuning})
    assert_batched_path(res)
    e, a = 1 + 1 + 11, 2
    for r in res:
        assert r["guards"]["ras"] == 1 and r["guards"]["rings"] == 2 and r["guards"]["smooth"] == 1 and r["guards"]["ras_rows"] > 0, r["guards"]
        S = [s["delta"]["dist_alltoallv_calls"] for s in r["single"]]
        R = [s["delta"]["dist_allreduce_calls"] for s in r["single"]]
        I = [s["iters"] for s in r["single"]]
        assert list(r["narrow"]["groups"]) == ["8", "2", "4"]
        assert all(v > 0 for v in r["narrow"]["smooth_rows"].values()), (r["rank"], r["narrow"]["smooth_rows"])      # both colours carry rows, both ways
        for k, got in ((int(key), val) for key, val in r["narrow"]["groups"].items()):
            assert len(got["columns"]) == k and got["batch_width"] == k
            for c, col in enumerate(got["columns"]):
                assert col["x_equal"] and col["iters"] == I[c] and col["relres_equal"] and col["berr_equal"], (r["rank"], k, c, col)
                assert I[c] > 0 and S[c] >= e * I[c] and R[c] >= a * I[c], (r["rank"], c, S[c], R[c], I[c])
            Sb, Rb, Tb = got["delta"]["dist_alltoallv_calls"], got["delta"]["dist_allreduce_calls"], got["delta"]["batch_steps"]
            print(f"rank {r['rank']} group of {k}: I={I[:k]} S={S[:k]} R={R[:k]}  batched: steps={Tb} alltoallv={Sb} allreduce={Rb}")
            assert max(I[:k]) <= Tb < sum(I[:k]), (k, Tb, I)
            assert e * Tb <= Sb <= sum(S[c] - e * I[c] for c in range(k)) + e * Tb, (k, Sb, S, I, Tb)
            assert Rb <= sum(R[c] - a * I[c] for c in range(k)) + a * Tb, (k, Rb, R, I, Tb)
        again = r["narrow"]["again"]
        assert again["x_equal"] and again["iters"] == I[1], (r["rank"], again)
        assert again["delta"]["dist_alltoallv_calls"] == S[1] and again["delta"]["dist_allreduce_calls"] == R[1] and again["delta"]["batch_steps"] == 0, (r["rank"], again, S[1], R[1])
    for k in ("8", "2", "4"):                             # every rank took the same global decisions
        assert len({tuple(col["iters"] for col in r["narrow"]["groups"][k]["columns"]) for r in res}) == 1


def test_bits_two_tracers_cell_major(tmp_path):
    res = launch(2, str(tmp_path / "r"), "bits", extra=("--partition", "cells", "--nrhs", "3,4"))
    assert_bits(res, "bits", (3, 4))


# ---------------------------------------------------------------- 2: three ranks over the file transport
def test_bits_three_ranks_file_transport(tmp_path):
    comm_dir = tmp_path / "comm"
    comm_dir.mkdir()
    res = launch(3, str(tmp_path / "r"), "bits,counts", extra=("--comm", "file", "--file-dir", str(comm_dir), "--nrhs", "3,4"),
                 env_extra={"NKP_COMM_TIMEOUT": "120"})
    assert_bits(res, "bits", (3, 4))
    assert_counts(res, e=2, a=2)


# ---------------------------------------------------------------- 3: three ranks over gloo
def test_three_ranks_gloo_converge(tmp_path):
    res = launch(3, str(tmp_path / "r"), "accuracy")
    assert_batched_path(res)
    for r in res:
        for col in r["accuracy"]["columns"]:
            assert col["status"] == 0 and col["relres"] <= 1e-10, (r["rank"], col)
        assert r["accuracy"]["delta"]["batch_steps"] > 0
    assert len({tuple(col["iters"] for col in r["accuracy"]["columns"]) for r in res}) == 1
    checked = res[0]["accuracy"]["relres_checked"]
    assert len(checked) == 4 and all(v <= 1.1e-10 for v in checked), checked


# ---------------------------------------------------------------- 5: one tracer per rank
def test_bits_one_tracer_per_rank(tmp_path):
    res = launch(2, str(tmp_path / "r"), "bits,counts", extra=("--partition", "tracers", "--nrhs", "4"))
    assert_bits(res, "bits", (4,))
    assert all(r["guards"]["ras"] == 0 and r["guards"]["overlap"] == 0 for r in res), res
    assert_counts(res, e=1, a=2)


# ---------------------------------------------------------------- 7: fallbacks stay collective
def test_fallbacks_stay_collective(tmp_path):
    res = launch(2, str(tmp_path / "r"), "fallback_equil,fallback_rhs_batch0")
    for r in res:
        assert r["fallback_equil"]["equil"] == 1
        for key in ("fallback_equil", "fallback_rhs_batch0"):
            got = r[key]
            assert got["delta"]["batch_steps"] == 0, (key, got["delta"])
            for col in got["columns"]:
                assert col["x_equal"] and col["iters"] == col["iters_single"] and col["relres_equal"], (key, r["rank"], col)


# ---------------------------------------------------------------- 8: a failing collective
def test_failing_allreduce_ends_the_batched_call_on_every_rank(tmp_path):
    res = launch(2, str(tmp_path / "r"), "broken")
    for r in res:
        got = r["broken"]
        assert got["code"] == -5 and "collective" in got["message"], got          # NKP_ECOMM
        assert got["single_after"]["status"] == 0 and got["single_after"]["relres"] <= 1e-10, got


# ---------------------------------------------------------------- 9: the executable
def _run_solve_ABdist(tmp_path, g, tag, env_extra):
    exe = os.path.join(ROOT, "nk_ocn_tracer_jacobian_precond_amd", "bin", "solve_ABdist")
    dst = str(tmp_path / f"B_{tag}.nc")
    shutil.copy(g.tracer_path, dst)
    comm_dir = tmp_path / f"comm_{tag}"
    comm_dir.mkdir()
    procs = []
    for r in range(2):
        env = dict(os.environ, NKP_COMM="file", NKP_COMM_DIR=str(comm_dir), NKP_COMM_TIMEOUT="60", NKP_RTOL="1e-12", RANK=str(r),
                   WORLD_SIZE="2", LOCAL_RANK=str(r), **env_extra)
        if "NKP_RHS_BLOCK" not in env_extra:
            env.pop("NKP_RHS_BLOCK", None)
        procs.append(subprocess.Popen([exe, "-D1", "-n", "1", "-v", ",".join(g.varnames), g.matrix_path, dst], stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True, env=env))
    outs = [p.communicate(timeout=240) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se + so
    assert not list(comm_dir.iterdir())
    return dst, [so for so, _ in outs]


def test_solve_ABdist_cli_rhs_block(tmp_path, golden_by_name):
    from nk_ocn_tracer_jacobian_precond_amd import nc3
    g = golden_by_name("penta_12x10x6")
    blocked, logs = _run_solve_ABdist(tmp_path, g, "block", {"NKP_RHS_BLOCK": "2"})
    for rank, so in enumerate(logs):
        assert f"({rank}) calling nkp_solve for 2 right-hand sides, 2 per call" in so, so
    out = nc3.NcFile(blocked)
    for v in g.varnames:
        x = out.get(v)[g.ind_k, g.ind_j, g.ind_i]
        ref = g.gold["x_" + v]
        assert np.linalg.norm(x - ref) / np.linalg.norm(ref) <= 1e-7, v
    plain, _ = _run_solve_ABdist(tmp_path, g, "plain", {})
    assert open(blocked, "rb").read() == open(plain, "rb").read()
