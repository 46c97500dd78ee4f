"""Depth of the overlap of the row-distributed solver's hierarchies (tuning dist_ras_rings; DESIGN.md section 7, "rings").

Ranks share ONE GPU through TorchComm over gloo: every collective is staged through host memory, so times say nothing about a
multi-GPU node; the iteration counts and sizes are what this probe is for.  The bench's synthetic 1 degree x 60 matrix
(upwind3 + isop with K33, seed 0) is cut into --ranks latitude bands and solved to 1e-10 with FGMRES(200) and a V(3,3) cycle
(the recipe of the band counts in DESIGN.md section 7), once per depth in --rings.  Reported per rank and depth: iterations,
relres, overlap rows of the rank's hierarchy, rows received per preconditioner application (the whole SpMV halo with one ring,
the overlap rows alone with more), SpMV halo rows, device memory, create_us (the library's clock) and the wall time of the
collective create (barrier to barrier).  One JSON line per rank and depth.

    python tools/ras_rings_probe.py [--grid 320x384x60] [--ranks 2] [--rings 1,2,3]
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
        env.pop("NKP_DIST_RAS_RINGS", None)
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
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    starts = nd.snap_partition(blk, world)
    loc = nd.local_slice(p.rowptr, p.colind, p.nzval, blk, starts, rank, ci, cj)
    n, f, m = p.flat_len, int(loc["fst_row"]), int(loc["m_loc"])
    b = np.ascontiguousarray(np.random.default_rng(1).standard_normal(n)[f:f + m])
    comm = nd.TorchComm()
    kw = dict(precond=solver.PRECOND_MULTILEVEL, restart=200, ml_smooth=3, rtol=1e-10, max_iters=2000)
    for depth in (int(t) for t in a.rings.split(",")):
        dist.barrier()
        t0 = time.perf_counter()
        s = nd.NkpDistSolver(loc, n, comm, tuning=dict(dist_ras_rings=depth), **kw)
        dist.barrier()
        wall = time.perf_counter() - t0
        x, info = s.solve(b, raise_on_fail=False)
        out = dict(grid=a.grid, ranks=world, rank=rank, m_loc=m, rings_asked=depth, rings=s.get_int("dist_ras_rings"),
                   iters=info["iters"], relres=info["relres"], status=info["status"], overlap_rows=s.get_int("dist_ras_rows"),
                   overlap_pct_of_own=100.0 * s.get_int("dist_ras_rows") / m, recv_rows_per_precond=s.get_int("dist_ras_recv_rows"),
                   halo_rows=s.get_int("dist_halo_rows"), device_MB=s.get_int("device_bytes") / 1e6, create_us=s.get_int("create_us"),
                   create_wall_s=wall, transport="gloo, host-staged; ranks share one GPU", comm_errors=list(comm.errors))
        print(json.dumps(out), flush=True)
        s.close()
    dist.barrier()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="320x384x60")
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--rings", default="1,2,3")
    a = ap.parse_args()
    if "RANK" not in os.environ:
        sys.exit(spawn(a))
    rank_main(a)


if __name__ == "__main__":
    main()
