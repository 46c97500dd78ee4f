"""What nkp_transpose_dist costs on the bench's synthetic matrix cut into latitude bands.

Two ranks share ONE GPU through TorchComm over gloo: every collective is staged through host memory.  The numbers are those of a
host-staged transport with ranks sharing a GPU, not a multi-GPU result.  Each rank creates a solver and reports -- medians of
--reps runs after one warm-up each, host wall clock around calls that synchronise -- the time of nkp_transpose_dist and its
device part next to the wall time of nkp_create_dist, the entries shipped and received, the device bytes of the transposed solver
next to the source's, one transposed solve against the forward solve on the same right-hand side, and nkp_refactor_dist_device
with and without a transposed solver attached.  One JSON line per rank.

    python tools/probe_transpose_dist.py [--grid 320x384x60] [--reps 5] [--ranks 2]
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
    n = p.flat_len
    kw = dict(precond=solver.PRECOND_MULTILEVEL, restart=200, ml_smooth=a.ml_smooth, rtol=1e-10)
    med = lambda v: float(np.median(v))

    def timed(fn):
        dist.barrier()
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e6, r

    nd.NkpDistSolver(lp, n, comm, **kw).close()                  # warm-up: code objects, allocator
    create_us, s = timed(lambda: nd.NkpDistSolver(lp, n, comm, **kw))
    out = dict(grid=a.grid, ranks=world, rank=rank, m_loc=lp["m_loc"], nnz_loc=int(lp["colind"].size), transport="gloo, host-staged; ranks share one GPU",
               create_dist_us=create_us, create_lib_us=s.get_int("create_us"), device_bytes=s.get_int("device_bytes"), ras_rows=s.get_int("dist_ras_rows"))
    dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (lq["val"], lp["val"])]
    torch.cuda.synchronize()

    # nkp_refactor_dist_device without a transposed solver (the first call builds the value maps)
    s.refactor_dist_device(dev[0].data_ptr())
    out["refactor_device_us"] = med([timed(lambda k=k: s.refactor_dist_device(dev[(k + 1) % 2].data_ptr()))[0] for k in range(a.reps)])
    s.refactor_dist_device(dev[1].data_ptr())                    # back to the first matrix

    # nkp_transpose_dist: build, read the counters, detach on every rank, again
    s.transposed_dist().close()                                  # warm-up
    wall, tot, ker = [], [], []
    for _ in range(a.reps):
        w, t = timed(s.transposed_dist)
        wall.append(w)
        tot.append(s.get_int("trans_us"))
        ker.append(s.get_int("trans_kernel_us"))
        t.close()
    out.update(trans_wall_us=med(wall), trans_us=med(tot), trans_kernel_us=med(ker))
    t = s.transposed_dist()
    out.update(trans_device_bytes=s.get_int("trans_device_bytes"), trans_sent_entries=s.get_int("trans_sent_entries"), trans_recv_entries=s.get_int("trans_recv_entries"),
               trans_nnz_loc=t.nnz, trans_ras_rows=t.get_int("dist_ras_rows"), trans_levels=t.get_int("levels"), levels=s.get_int("levels"))

    # one solve each on the same right-hand side
    b = np.random.default_rng(1).standard_normal(n)[lp["fst_row"]:lp["fst_row"] + lp["m_loc"]]
    for name, h in (("solve", s), ("trans_solve", t)):
        h.solve(b)
        runs = [timed(lambda: h.solve(b)) for _ in range(a.reps)]
        out[name + "_us"], out[name + "_iters"], out[name + "_relres"] = med([r[0] for r in runs]), runs[0][1][1]["iters"], runs[0][1][1]["relres"]

    # nkp_refactor_dist_device with the transposed solver attached (the first call builds its buffers and the transposed solver's maps)
    s.refactor_dist_device(dev[0].data_ptr())
    out["refactor_device_with_transposed_us"] = med([timed(lambda k=k: s.refactor_dist_device(dev[(k + 1) % 2].data_ptr()))[0] for k in range(a.reps)])
    out["trans_device_bytes_after_refactor"] = s.get_int("trans_device_bytes")
    out["transposed_still_attached"] = bool(s.transposed_dist() is t and t.get_int("refactor_count") == a.reps + 1)
    out["comm_errors"] = comm.errors
    s.close()
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
