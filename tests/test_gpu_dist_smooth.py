"""The fine-level exchange of the row-distributed cycle (tuning dist_smooth_exchange) on the GPU: 2 and 3 ranks share the one GPU
of the test box over the library's file transport; latitude bands of 40x46x20 (upwind3 + isop, seed 5).  One launch per world runs
all cases (tests/dist_smooth_gpu_worker.py).  The exchange follows the half sweeps of level 0, so the cases stop coarsening at
4000 rows (tuning ml_coarsest_rows): with the default 8000 the smallest of three bands of this grid is one dense level, which has
no half sweeps, and the ranks then agree to leave the exchange out -- the "default" solves show that, too."""
import json
import os
import subprocess
import sys

import pytest

from test_dist_gloo import free_port

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NU = 3                               # nkp_options.ml_smooth, the level-0 sweeps before and after the coarse correction
PER_CYCLE = 2 * (NU + NU) - 1        # exchanges the knob adds to one cycle: every level-0 half sweep but the last


def launch(world, tmp, cases):
    port = free_port()
    comm_dir = tmp / "comm"
    comm_dir.mkdir()
    out = str(tmp / "r")
    procs = []
    for r in range(world):
        # a mismatch in the collectives ends in the transport's deadline, well inside the launch's own time limit
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0", NKP_COMM_TIMEOUT="60")
        for k in ("NKP_DIST_RAS_RINGS", "NKP_DIST_RAS", "NKP_DIST_SMOOTH_EXCHANGE", "NKP_ML_OMEGA", "NKP_ML_WAVE_FUSED", "NKP_ML_LANE_FUSED"):
            env.pop(k, None)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dist_smooth_gpu_worker.py"), "--out", out, "--cases", cases,
                                       "--file-dir", str(comm_dir)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=480)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log
    return [json.load(open(f"{out}.{r}")) for r in range(world)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return {w: launch(w, tmp_path_factory.mktemp(f"w{w}"), "sweep,solve,batch,refactor,transpose,agree") for w in (2, 3)}


@pytest.mark.parametrize("case", ["ring1", "ring2", "two_kernel"])
def test_the_sweep_is_the_global_sweep(runs, case):
    """One cycle with ml_omega = 1e-300 (no coarse correction to speak of) on a random r: with the knob on, every rank's z is the
    matching slice of the same cycle on a single-GPU solver of the whole matrix, max |z_d - z_s| <= 1e-10 max |z_s| -- not bit for
    bit, a row's columns are renumbered [own | halo] and summed in another order.  With the knob off the cut shows: the
    difference must exceed 1e-8 max |z_s|, so a cycle that ignores the knob cannot pass.  One ring, two rings, and the two-kernel
    half sweeps (ml_wave_fused = ml_lane_fused = 0).

    The two values the 1e-10 line separates, as measured on an MI355X (max |z_d - z_s| / max |z_s| over the ranks of worlds 2 and
    3, the same in the fused and the two-kernel case): knob on 1.9e-18 .. 7.5e-18 (a few last-bit differences in rows whose z is
    small), knob off 3.5e-3 .. 1.5e-2 with one ring and 2.3e-3 .. 9.2e-3 with two -- seven orders of magnitude on either side."""
    for w, res in runs.items():
        for r in res:
            s = r["sweep"][case]
            on, off = s["on"]["diff"] / s["zs_max"], s["off"]["diff"] / s["zs_max"]
            print(f"world {w} rank {r['rank']} {case}: max|z_d - z_s| / max|z_s| = {on:.3e} (knob on), {off:.3e} (knob off); overlap rows {s['on']['ras_rows']}, "
                  f"alltoallv per cycle {s['on']['alltoallv']} / {s['off']['alltoallv']}")
            assert s["on"]["in_force"] == 1 and s["off"]["in_force"] == 0, (w, r["rank"], s)
            assert s["on"]["rings"] == s["off"]["rings"] == (2 if case == "ring2" else 1), s
            assert s["on"]["smooth_rows"] == s["on"]["ras_rows"] > 0 and s["off"]["smooth_rows"] == 0, s
            assert on <= 1e-10, (w, r["rank"], case, on)
            assert off > 1e-8, (w, r["rank"], case, off)
            assert s["on"]["alltoallv"] == 1 + PER_CYCLE and s["off"]["alltoallv"] == 1, s


def test_solves_converge_in_no_more_iterations(runs):
    """Knob on: status 0, relres <= 1e-10 (host-checked <= 1.1e-10), the same iterations on every rank, and no more of them than
    with the knob off, at both worlds."""
    for w, res in runs.items():
        for tname in ("smoothed", "default"):
            rec = res[0]["solve"][tname]
            off, on = rec["off"], rec["on"]
            print(f"world {w} ({tname} tuning, {on['levels']} levels on rank 0, in force: {on['in_force']}): iterations {rec['single_iters']} (one rank), "
                  f"{off['iters']} (knob off) -> {on['iters']} (knob on); relres checked {off['relres_checked']:.2e} / {on['relres_checked']:.2e}")
            # with the default tuning the exchange is in force only where every rank smooths its level 0 (see the worker); the
            # agreement is the same on every rank either way
            assert len({r["solve"][tname]["on"]["in_force"] for r in res}) == 1, (w, tname)
            assert on["in_force"] == 1 or tname == "default", (w, tname)
            for r in res:
                s = r["solve"][tname]["on"]
                assert r["solve"][tname]["off"]["in_force"] == 0, (w, r["rank"])
                assert s["status"] == 0 and s["relres"] <= 1e-10, (w, r["rank"], s)
                assert s["iters"] == on["iters"] and r["solve"][tname]["off"]["iters"] == off["iters"]
            assert on["relres_checked"] <= 1.1e-10, (w, on)
            assert on["iters"] <= off["iters"], (w, tname, off["iters"], on["iters"])


def test_counters(runs):
    """One nkp_precond_apply makes the overlap residual's exchange and, with the knob on, 11 more (V(3, 3)); a solve makes those 12
    and the SpMV's one per iteration, plus the true residuals of its restart cycles and the backward error (no cycle in them)."""
    restart = 60
    for w, res in runs.items():
        for r in res:
            on, off = r["solve"]["smoothed"]["on"], r["solve"]["smoothed"]["off"]
            assert on["apply_delta"]["dist_alltoallv_calls"] == 1 + PER_CYCLE and off["apply_delta"]["dist_alltoallv_calls"] == 1, (w, r["rank"], on, off)
            assert on["apply_delta"]["dist_allreduce_calls"] == off["apply_delta"]["dist_allreduce_calls"] == 0
            for s, per in ((on, 1 + PER_CYCLE + 1), (off, 2)):
                extra = s["solve_delta"]["dist_alltoallv_calls"] - per * s["iters"]
                cycles = -(-s["iters"] // restart)
                print(f"world {w} rank {r['rank']}: {s['iters']} iterations, {s['solve_delta']['dist_alltoallv_calls']} alltoallv = {per} per iteration + {extra}")
                assert 0 < extra <= 2 * (cycles + 1) + 2, (w, r["rank"], per, s)


@pytest.mark.parametrize("name,steps", [("steps1", 1), ("steps2", 2)])
def test_batched_solves_keep_the_bits_and_make_the_exchanges_of_one_system(runs, name, steps):
    """nrhs = 4, knob on: every column has the bits, iterations, relres and berr of its own single solve on the same solver, and a
    lockstep step costs the exchanges of one system: per cycle 1 + 11, per operator 1 (with precond_steps = 2: two cycles and one
    more operator in the chain)."""
    e = steps * (1 + PER_CYCLE) + (steps - 1) + 1
    for w, res in runs.items():
        for r in res:
            b = r["batch"][name]
            assert b["in_force"] == 1 and b["equil"] == 0 and b["precond_steps"] == steps, b
            for c, col in enumerate(b["columns"]):
                assert col["x_equal"] and col["iters"] == col["iters_single"] and col["relres_equal"] and col["berr_equal"] and col["status"] == 0, (w, r["rank"], c, col)
            assert b["delta"]["batch_steps"] > 0 and b["batch_width"] == 4, b
            S = [s["delta"]["dist_alltoallv_calls"] for s in b["single"]]
            I = [s["iters"] for s in b["single"]]
            Sb, Tb = b["delta"]["dist_alltoallv_calls"], b["delta"]["batch_steps"]
            print(f"world {w} rank {r['rank']} {name}: I={I} S={S} batched: steps={Tb} alltoallv={Sb}")
            for c in range(4):
                assert I[c] > 0 and S[c] >= e * I[c], (c, S[c], I[c])
            assert max(I) <= Tb < sum(I), (Tb, I)
            assert e * Tb <= Sb <= sum(S[c] - e * I[c] for c in range(4)) + e * Tb, (Sb, S, I, Tb)


def test_refactor_dist_device_matches_a_fresh_create(runs):
    for w, res in runs.items():
        for r in res:
            for name in ("kept", "rebuild"):
                got = r["refactor"][name]
                print(f"world {w} rank {r['rank']} {name}: {got}")
                assert got["in_force"] == got["in_force_fresh"] == 1, got
                assert got["x_equal"] and got["iters"] == got["iters_fresh"] and got["relres"] == got["relres_fresh"] and got["status"] == 0, (w, r["rank"], name, got)
            assert r["refactor"]["kept"]["rebuilt"] == 0 and r["refactor"]["rebuild"]["rebuilt"] == 1, (w, r["rank"], r["refactor"])


def test_transposed_solver_inherits_the_exchange(runs):
    for w, res in runs.items():
        for r in res:
            t = r["transpose"]
            print(f"world {w} rank {r['rank']}: {t}")
            assert t["is_transpose"] == 1 and t["in_force"] == t["in_force_source"] == 1, t
            assert t["apply_alltoallv"] == 1 + PER_CYCLE, t
            assert t["status"] == 0 and t["relres"] <= 1e-10, t
        assert res[0]["transpose"]["relres_checked"] <= 1.1e-10, res[0]["transpose"]


def test_agreement_and_default(runs):
    """Rank 0 asks for 1 and the others for 0: nobody gets it, and the solution has the bits of a solver that never set the field;
    so has an explicit 0."""
    for w, res in runs.items():
        for r in res:
            g = r["agree"]
            assert g["mixed"]["in_force"] == g["unset"]["in_force"] == g["zero"]["in_force"] == 0, (w, r["rank"], g)
            assert g["x_equal_mixed_unset"] and g["x_equal_zero_unset"], (w, r["rank"])
            assert g["mixed"]["iters"] == g["unset"]["iters"] == g["zero"]["iters"] and g["mixed"]["alltoallv"] == g["unset"]["alltoallv"] == g["zero"]["alltoallv"], g
