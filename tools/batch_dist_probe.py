"""Batched right-hand sides on the row-distributed solver against the same systems one at a time.

Two ranks share ONE GPU through TorchComm over gloo: every collective is staged through host memory.  The numbers are those of a
host-staged transport with ranks sharing a GPU, not a multi-GPU result.  The bench's synthetic 1 degree x 60 matrix is cut
into two latitude bands; four right-hand sides are solved to 1e-10

  one_at_a_time   by a solver with rhs_batch = 0 (nkp_solve takes them one after the other: the path without this feature)
  batched         by a solver with the default rhs_batch (K = 4 in lockstep, the collectives of one system per Krylov step)

with device-resident vectors (solve_batch_device), host wall clock around calls that synchronise, median of --reps calls after
a warm-up call.  Reported per rank: time per solve, the four counters of one call (dist_alltoallv_calls, dist_allreduce_calls,
batch_steps, batch_width), device memory of the solver, and whether the two paths returned the same bits.  One JSON line per
rank.  --lib measures another build of the library (e.g. an earlier commit's) through the same script.

    python tools/batch_dist_probe.py [--grid 320x384x60] [--reps 5] [--ranks 2] [--modes one_at_a_time,batched] [--lib PATH]
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTERS = ("dist_alltoallv_calls", "dist_allreduce_calls", "batch_steps", "batch_width")


def spawn(a):
    """one child process per rank (the parent never opens the GPU)"""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(a.ranks):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(a.ranks), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="4")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env))
    return max(p.wait() for p in procs)


def rank_main(a):
    import torch
    import torch.distributed as dist
    from nk_ocn_tracer_jacobian_precond_amd import dist as nd
    from nk_ocn_tracer_jacobian_precond_amd import solver, synth

    if a.lib:
        solver._lib = solver.load_library(os.path.abspath(a.lib))
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    imt, jmt, km = (int(t) for t in a.grid.split("x"))
    p = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=0, isop_k33=True)
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    starts = nd.snap_partition(blk, world)
    loc = nd.local_slice(p.rowptr, p.colind, p.nzval, blk, starts, rank, ci, cj)
    n, f, m = p.flat_len, int(loc["fst_row"]), int(loc["m_loc"])
    K = a.nrhs
    B = np.ascontiguousarray(np.random.default_rng(1).standard_normal((K, n))[:, f:f + m])
    dB = torch.from_numpy(B).cuda()
    dX = torch.empty_like(dB)
    torch.cuda.synchronize()
    comm = nd.TorchComm()
    kw = dict(precond=solver.PRECOND_MULTILEVEL, restart=200, ml_smooth=a.ml_smooth, rtol=1e-10)
    out = dict(grid=a.grid, ranks=world, rank=rank, m_loc=m, nrhs=K, lib=a.lib or "this build", transport="gloo, host-staged; ranks share one GPU")
    sols = {}
    for mode in a.modes.split(","):
        s = nd.NkpDistSolver(loc, n, comm, tuning=dict(rhs_batch=0 if mode == "one_at_a_time" else 1), **kw)
        mem0 = s.get_int("device_bytes")
        get = lambda: {k: s.get_int(k) for k in COUNTERS}

        def call():
            dist.barrier()
            t0 = time.perf_counter()
            infos = s.solve_batch_device(dB.data_ptr(), dX.data_ptr(), K, m)
            return time.perf_counter() - t0, infos
        call()                                         # warm-up: code objects, the batch's work vectors
        c0 = get()
        runs = [call() for _ in range(a.reps)]
        c1 = get()
        t = np.array([r[0] for r in runs])
        torch.cuda.synchronize()
        sols[mode] = dX.cpu().numpy().copy()
        out[mode] = dict(ms_per_solve=float(np.median(t)) / K * 1e3, ms_per_solve_min=float(t.min()) / K * 1e3, ms_per_solve_max=float(t.max()) / K * 1e3,
                         iters=[i["iters"] for i in runs[-1][1]], relres_max=max(i["relres"] for i in runs[-1][1]),
                         alltoallv_per_call=(c1[COUNTERS[0]] - c0[COUNTERS[0]]) / a.reps if c1[COUNTERS[0]] >= 0 else None,
                         allreduce_per_call=(c1[COUNTERS[1]] - c0[COUNTERS[1]]) / a.reps if c1[COUNTERS[1]] >= 0 else None,
                         batch_steps_per_call=(c1[COUNTERS[2]] - c0[COUNTERS[2]]) / a.reps if c1[COUNTERS[2]] >= 0 else None,
                         batch_width=c1[COUNTERS[3]], device_MB_created=mem0 / 1e6, device_MB_after=s.get_int("device_bytes") / 1e6)
        s.close()
    if len(sols) == 2:
        x, y = sols.values()
        out["same_bits"] = bool(np.array_equal(x, y))
        ms = [out[k]["ms_per_solve"] for k in sols]
        out["speedup_batched"] = ms[0] / ms[1]
    out["comm_errors"] = comm.errors
    print(json.dumps(out), flush=True)
    dist.barrier()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="320x384x60")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--nrhs", type=int, default=4)
    ap.add_argument("--ml-smooth", type=int, default=3)
    ap.add_argument("--modes", default="one_at_a_time,batched")
    ap.add_argument("--lib", default="", help="measure this libnkp_hip.so instead of the tree's")
    a = ap.parse_args()
    if "RANK" not in os.environ:
        sys.exit(spawn(a))
    rank_main(a)


if __name__ == "__main__":
    main()
