"""The Krylov drivers on a row-distributed solver against the drivers restated in tests/krylov_reference.py (see
tests/test_gpu_krylov.py for the single-GPU part and the tolerances).  Ranks share the one GPU of the test box.

One rank forced distributed walks the allreduce points of the driver; with one reduction per step it is the only place where
finish_column_pythagoras_kernel (csrc/blas1.hip:438-462) and the weak_norm mark of fg_post_step run, and the restatement is
taken with its pythagoras epilogue.  Two ranks show that every rank's partial dots are the true local contributions: the
gathered x_k is the x_k of the single-process restatement on the global matrix."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import krylov_cases as kc
import krylov_reference as kr
from nk_ocn_tracer_jacobian_precond_amd import solver
from test_dist_gloo import free_port

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def launch(world, mode, out, env_extra=None):
    port = free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0", **(env_extra or {}))
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dist_krylov_worker.py"), "--mode", mode, "--out", out],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=600)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log
    res = [json.load(open(f"{out}.{r}")) for r in range(world)]
    assert all(not r["comm_errors"] for r in res), res
    return res


@pytest.fixture(scope="module", params=["two_reductions", "one_reduction"])
def one_rank(request, tmp_path_factory):
    env = {"NKP_FORCE_DIST": "1", "NKP_DIST_ONE_REDUCE": "1" if request.param == "one_reduction" else "0"}
    res = launch(1, "one", str(tmp_path_factory.mktemp(request.param) / "r"), env)[0]
    assert res["one_reduce"] == (request.param == "one_reduction")
    return res


def test_one_rank_against_the_restatement(one_rank):
    for run in kc.dist_one_rank_runs():
        r = one_rank["runs"][run.id]
        print(f"{run.id} one_reduce {one_rank['one_reduce']}: iters {r['iters']} / {r['ref_iters']}, dx {r['dx']:.2e} (tol {r['tol']:.1e}), "
              f"relres {r['relres']:.6e} / {r['ref_relres']:.6e} (bound {r['relres_bound']:.2e}), allreduces {r['allreduce_calls']}")
        assert not r["stagnated"]
        assert r["iters"] == r["ref_iters"] and r["status"] == r["ref_status"], (run, r)
        assert r["dx"] <= r["tol"], (run, r)
        assert abs(r["relres"] - r["ref_relres"]) <= r["relres_bound"], (run, r)
        if run.k is None:
            assert r["status"] == kr.OK and r["closest_decision"] >= 1000.0 * r["tol"], (run, r)
        else:
            assert r["iters"] == run.k


def test_one_reduction_takes_one_allreduce_per_step(one_rank):
    """the pythagoras epilogue is what ran: a step of one Gram-Schmidt pass costs one allreduce, not two"""
    run = next(r for r in kc.dist_one_rank_runs() if r.k == 9 and not r.reorth)
    r = one_rank["runs"][run.id]
    fixed = 4                                           # ||b||, the true residual of the two restarts, the backward error
    assert r["allreduce_calls"] == fixed + 9 * (1 if one_rank["one_reduce"] else 2), r


def test_lucky_breakdown(one_rank):
    """the Krylov space closes at step 3: with one reduction the weak mark ends the cycle there; x is the exact solution"""
    run = next(r for r in kc.dist_one_rank_runs() if r.case == "lucky513")
    r = one_rank["runs"][run.id]
    assert r["iters"] == 3 and r["status"] == kr.OK and r["error"] <= 64 * 2.0 ** -52, r
    if one_rank["one_reduce"]:
        assert [t for _, t in r["weak"]] == [False, False, True], r


def test_two_ranks_against_the_global_restatement(tmp_path):
    out = str(tmp_path / "r")
    res = launch(2, "two", out)
    for run in kc.dist_two_rank_runs():
        c = kc.case(run.case)
        parts = [res[r]["runs"][run.id] for r in range(2)]
        assert [p["fst_row"] for p in parts] == [0, parts[0]["m_loc"]] and sum(p["m_loc"] for p in parts) == c.n and min(p["m_loc"] for p in parts) > 0
        x = np.concatenate([np.load(f"{out}.{r}.{run.id}.npy") for r in range(2)])
        with solver.NkpSolver(c.rowptr, c.colind, c.val, c.blk, **run.options()) as s:
            ref = kc.reference(run, s.spmv, s.precond_apply)
        tol = kc.TOL[run.cls][1]
        dx = float(np.linalg.norm(x - ref.x) / np.linalg.norm(ref.x))
        print(f"{run.id}: iters {parts[0]['iters']} / {ref.iters}, dx {dx:.2e} (tol {tol:.1e})")
        for p in parts:
            assert p["iters"] == ref.iters == 9 and p["status"] == ref.status, (run, p)
            assert abs(p["relres"] - ref.relres) <= c.relres_bound(ref.x, ref.relres, tol), (run, p)
        assert dx <= tol, (run, dx, tol)


def test_two_ranks_refuse_together(tmp_path):
    """a NaN in a row that rank 1 owns, and b 2^-600 (include/nkp.h at nkp_solve): ||b||^2 is global, so both ranks count their
    entries, add the counts and return NKP_BREAKDOWN with iters 0 and every own row NaN -- rank 0 too, whose rows hold no NaN.
    A clean solve afterwards has the bits of the one before.  (berr is left out: what the max-allreduce makes of a NaN is the
    transport's business.)  The file transport of the library carries the collectives."""
    res = launch(2, "refuse", str(tmp_path / "r"), {"NKP_COMM_TIMEOUT": "60"})
    assert [r["fst_row"] for r in res] == [0, res[0]["m_loc"]] and min(r["m_loc"] for r in res) > 5
    assert res[0]["clean"]["status"] == kr.OK and res[0]["clean"]["iters"] > 0
    assert [res[r]["refused"]["nan_on_rank_1"]["holds_nan"] for r in range(2)] == [False, True]
    for r in res:
        for what, got in r["refused"].items():
            assert got["status"] == kr.BREAKDOWN and got["iters"] == 0 and got["relres_is_nan"] and got["rows_nan"] == r["m_loc"], (r["rank"], what, got)
        assert r["clean_again"], r
