"""nkp_refactor_dist against nkp_create_dist on the bench's synthetic matrix cut into latitude bands ("New values on
the same pattern", distributed subsection).

Two ranks share ONE GPU through TorchComm over gloo: every collective is staged through host memory.  The numbers are those of a
host-staged transport with ranks sharing a GPU, not a multi-GPU result.  Each rank creates a solver for day_cnt = 365, refactors
it to the day_cnt = 180 Jacobian (same pattern) and back, with host (nkp_refactor_dist) and device (nkp_refactor_dist_device)
values: host wall clock around calls that synchronise, median of --reps after the first call, and the time spent inside the
alltoallv callback of each call (the overlap exchange).  One JSON line per rank.

    python tools/refactor_dist_probe.py [--grid 320x384x60] [--reps 5] [--ranks 2]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/refactor_dist_probe.py --reps 2     (per-kernel times, separate run)
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

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    imt, jmt, km = (int(t) for t in a.grid.split("x"))
    p = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=0, isop_k33=True)
    q = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=0, isop_k33=True, day_cnt=180.0)
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    starts = nd.snap_partition(blk, world)
    lp = nd.local_slice(p.rowptr, p.colind, p.nzval, blk, starts, rank, ci, cj)
    lq = nd.local_slice(q.rowptr, q.colind, q.nzval, blk, starts, rank, ci, cj)
    comm = nd.TorchComm()
    xchg = []                                  # seconds inside alltoallv during the current refactor call
    inner = comm._alltoallv

    def timed_alltoallv(*args):
        t0 = time.perf_counter()
        rc = inner(*args)
        xchg.append(time.perf_counter() - t0)
        return rc
    comm._fns = (comm._fns[0], solver._ALLTOALLV_FN(timed_alltoallv), comm._fns[2], comm._fns[3])
    comm.ops.alltoallv = comm._fns[1]
    n = p.flat_len
    kw = dict(precond=solver.PRECOND_MULTILEVEL, restart=200, ml_smooth=a.ml_smooth, rtol=1e-10)
    mk = lambda loc: nd.NkpDistSolver(loc, n, comm, **kw)
    mk(lp).close()                             # warm-up: code objects, allocator
    dist.barrier()
    t0 = time.perf_counter()
    s = mk(lp)
    out = dict(grid=a.grid, ranks=world, rank=rank, m_loc=lp["m_loc"], nnz_loc=int(lp["colind"].size), ras_rows=s.get_int("dist_ras_rows"),
               transport="gloo, host-staged; ranks share one GPU", create_dist_us=(time.perf_counter() - t0) * 1e6, create_lib_us=s.get_int("create_us"),
               device_MB_create=s.get_int("device_bytes") / 1e6)

    def timed(fn):
        xchg.clear()
        dist.barrier()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e6, sum(xchg) * 1e6

    vals = (lq["val"], lp["val"])
    first, first_x = timed(lambda: s.refactor_dist(vals[0]))
    out.update(refactor_first_us=first, refactor_first_exchange_us=first_x, rebuilt_first=s.get_int("refactor_rebuilt"),
               halo_values=s.get_int("refactor_halo_values"))
    host = [timed(lambda k=k: s.refactor_dist(vals[(k + 1) % 2])) for k in range(a.reps)]
    out["refactor_host_us"] = float(np.median([h[0] for h in host]))
    out["refactor_host_exchange_us"] = float(np.median([h[1] for h in host]))
    dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in vals]
    torch.cuda.synchronize()
    devt = [timed(lambda k=k: s.refactor_dist_device(dev[k % 2].data_ptr())) for k in range(a.reps)]
    out["refactor_device_us"] = float(np.median([d[0] for d in devt]))
    out["refactor_device_exchange_us"] = float(np.median([d[1] for d in devt]))
    out["refactor_lib_us"] = s.get_int("refactor_us")
    out["rebuilt_steady"] = s.get_int("refactor_rebuilt")
    out["device_MB_after"] = s.get_int("device_bytes") / 1e6
    b = np.random.default_rng(1).standard_normal(n)[lp["fst_row"]:lp["fst_row"] + lp["m_loc"]]
    s.refactor_dist(lq["val"])
    x, info = s.solve(b)
    t = mk(lq)
    x2, _ = t.solve(b)
    out["solve_bitwise_equal_to_create"] = bool(np.array_equal(x, x2))
    out["iters"] = info["iters"]
    out["ratio_device_to_create"] = out["refactor_device_us"] / max(1.0, out["create_dist_us"])
    out["comm_errors"] = comm.errors
    s.close()
    t.close()
    print(json.dumps(out), flush=True)
    dist.barrier()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="320x384x60")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--ml-smooth", type=int, default=3)
    a = ap.parse_args()
    if "RANK" not in os.environ:
        sys.exit(spawn(a))
    rank_main(a)


if __name__ == "__main__":
    main()
