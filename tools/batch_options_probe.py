"""Batched right-hand sides under row equilibration and chained preconditioner cycles against the same calls one at a time
(DESIGN.md 8b).

The bench's synthetic 1 degree x 60 matrix, four device-resident right-hand sides solved to 1e-10 by solve_batch_device with

  steps in {1, 2}    preconditioner cycles per Krylov iteration (precond_steps)
  equil in {0, 1}    row equilibration
  K     in {1, 4}    rhs_batch = 0 (one at a time) or the default (groups of four in lockstep)

Host wall clock around calls that synchronise, one warm-up call (code objects, the group's work vectors), then the median of
--reps calls.  Reported per configuration: ms per solve (median, min, max of the calls), iterations per column, batch_steps of
a call (0 = the call went one at a time, whatever K asked for), device memory of the solver after the calls (its own and that of
the group's further sets of work vectors; a library without the batch_member_bytes key reports 0 for those), and whether the
K = 4 solutions have the bits of the K = 1 ones.  --restarts adds the K = 4 cases without equilibration at other restart lengths
(the Krylov bases are most of a group's memory, and half the iterations allow half the restart length).  One JSON line per
configuration.  --lib measures another build of the library (an earlier commit's, where some of these calls fall back) through the same script; compare runs of the same session.

    python tools/batch_options_probe.py [--grid 320x384x60] [--reps 5] [--restart 200] [--restarts 60,30] [--lib PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="320x384x60")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nrhs", type=int, default=4)
    ap.add_argument("--restart", type=int, default=200)
    ap.add_argument("--restarts", default="", help="restart lengths for the extra two-cycle K = 4 runs, e.g. 60,30")
    ap.add_argument("--lib", default="", help="measure this libnkp_hip.so instead of the tree's")
    a = ap.parse_args()
    import torch
    from nk_ocn_tracer_jacobian_precond_amd import solver, synth

    if a.lib:
        solver._lib = solver.load_library(os.path.abspath(a.lib))
    if solver.device_count() < 1:
        sys.exit("batch_options_probe: no HIP device visible (a timing needs the GPU)")
    imt, jmt, km = (int(t) for t in a.grid.split("x"))
    p = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=0, isop_k33=True)
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    n, K = p.flat_len, a.nrhs
    dB = torch.from_numpy(np.random.default_rng(1).standard_normal((K, n))).cuda()
    dX = torch.empty_like(dB)
    torch.cuda.synchronize()

    def run(steps, equil, batch, restart):
        with solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, col_i=ci, col_j=cj, rtol=1e-10, restart=restart, precond_steps=steps,
                              equil=1 if equil else -1, tuning=dict(rhs_batch=1 if batch else 0)) as s:
            def call():
                t0 = time.perf_counter()
                infos = s.solve_batch_device(dB.data_ptr(), dX.data_ptr(), K, n, raise_on_fail=False)       # synchronises before it returns
                return time.perf_counter() - t0, infos
            call()
            b0 = s.get_int("batch_steps")
            runs = [call() for _ in range(a.reps)]
            t = np.array([r[0] for r in runs]) / K * 1e3
            out = dict(lib=a.lib or "this build", grid=a.grid, steps=steps, equil=equil, K=4 if batch else 1, restart=restart,
                       ms_per_solve=float(np.median(t)), ms_min=float(t.min()), ms_max=float(t.max()), iters=[i["iters"] for i in runs[-1][1]],
                       status=[i["status"] for i in runs[-1][1]], relres_max=max(i["relres"] for i in runs[-1][1]),
                       batch_steps_per_call=(s.get_int("batch_steps") - b0) / a.reps, batch_width=s.get_int("batch_width"),
                       device_MB=s.get_int("device_bytes") / 1e6, member_MB=max(s.get_int("batch_member_bytes"), 0) / 1e6)
            torch.cuda.synchronize()
            return out, dX.cpu().numpy().copy()

    for steps in (1, 2):
        for equil in (0, 1):
            one, x1 = run(steps, equil, False, a.restart)
            print(json.dumps(one), flush=True)
            four, x4 = run(steps, equil, True, a.restart)
            four["same_bits_as_K1"] = bool(np.array_equal(x1, x4))
            four["per_solve_speedup_over_K1"] = one["ms_per_solve"] / four["ms_per_solve"]
            print(json.dumps(four), flush=True)
    for restart in (int(t) for t in a.restarts.split(",") if t):
        for steps in (1, 2):
            out, _ = run(steps, 0, True, restart)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
