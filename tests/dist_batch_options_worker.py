"""Worker of tests/test_gpu_batch_options_dist.py, one process per rank, all ranks on the test box's one GPU.

A row-distributed solver with chained preconditioner cycles (--opts '{"precond_steps": 2}'): every case compares a batched solve
(NkpDistSolver.solve_many, nkp_solve with nrhs >= 2) with the SAME distributed solver's one-at-a-time solves of the same
right-hand sides.  All ranks run the same cases in the same order (the calls are collective).

  --comm gloo   collectives over torch.distributed (gloo, host staging)
  --comm file   the library's file transport (nkp_comm_file_init), wired up through ctypes
"""
import argparse
import ctypes as C
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

COUNTERS = ("dist_alltoallv_calls", "dist_allreduce_calls", "batch_steps", "batch_width")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", required=True)
    ap.add_argument("--comm", default="gloo")
    ap.add_argument("--file-dir", default="")
    ap.add_argument("--grid", default="40x46x20")
    ap.add_argument("--opts", default="{}", help="JSON: options of NkpDistSolver on top of rtol / restart / max_iters")
    ap.add_argument("--nrhs", default="2,3,4,5")
    ap.add_argument("--nvec", type=int, default=5)
    a = ap.parse_args()
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from nk_ocn_tracer_jacobian_precond_amd import dist as nd
    from nk_ocn_tracer_jacobian_precond_amd import solver, synth
    torch.cuda.set_device(0)
    lib = solver.load_library()

    imt, jmt, km = (int(t) for t in a.grid.split("x"))
    p = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=5)
    n = p.flat_len
    cnt = 1
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    starts = nd.snap_partition(blk, world)                  # latitude bands
    loc = nd.local_slice(p.rowptr, p.colind, p.nzval, blk, starts, rank, ci, cj)
    f, m = int(loc["fst_row"]), int(loc["m_loc"])
    Bg = np.random.default_rng(11).standard_normal((a.nvec, n))
    Bg[2] *= 1e-3                                       # the systems of a group leave the interleave at different steps
    B = np.ascontiguousarray(Bg[:, f:f + m])

    if a.comm == "file":
        lib.nkp_comm_file_init.argtypes = [C.POINTER(solver.NkpCommOps), C.c_char_p, C.c_int, C.c_int]
        lib.nkp_comm_file_free.argtypes = [C.POINTER(solver.NkpCommOps)]
        lib.nkp_comm_file_free.restype = None
        ops = solver.NkpCommOps()
        assert lib.nkp_comm_file_init(C.byref(ops), a.file_dir.encode(), rank, world) == 0
        comm = types.SimpleNamespace(ops=ops, errors=[])
    else:
        comm = nd.TorchComm()

    base = dict(rtol=1e-10, restart=60, max_iters=3000)
    opts = dict(base, **json.loads(a.opts))

    def make(transport=comm, **over):
        return nd.NkpDistSolver(loc, n, transport, coupled_tracer_cnt=cnt, **dict(opts, **over))

    def counters(s):
        return {k: s.get_int(k) for k in COUNTERS}

    def delta(after, before):
        return {k: after[k] - before[k] for k in COUNTERS[:3]}

    def singles(s, cols):
        out = []
        for c in cols:
            c0 = counters(s)
            x, info = s.solve(B[c], raise_on_fail=False)
            out.append(dict(x=x, info=info, delta=delta(counters(s), c0)))
        return out

    def batched(s, cols, single):
        """one solve_many of B[cols] against the single solves: per column bit equality of the solution, iters, relres, berr"""
        c0 = counters(s)
        X, infos = s.solve_many(B[cols], raise_on_fail=False)
        c1 = counters(s)
        col = []
        for q, c in enumerate(cols):
            one = single[c]
            col.append(dict(x_equal=bool(np.array_equal(X[q], one["x"])), iters=infos[q]["iters"], iters_single=one["info"]["iters"],
                            relres_equal=bool(infos[q]["relres"] == one["info"]["relres"]), berr_equal=bool(infos[q]["berr"] == one["info"]["berr"]),
                            relres=infos[q]["relres"], status=infos[q]["status"], status_single=one["info"]["status"],
                            zero_x=bool(not X[q].any())))
        return dict(columns=col, delta=delta(c1, c0), batch_width=c1["batch_width"]), X

    def guards(s):
        return dict(equil=s.get_int("equil"), precond_steps=s.get_int("precond_steps"), ras=s.get_int("dist_ras"), ras_rows=s.get_int("dist_ras_rows"),
                    overlap=s.get_int("dist_overlap"))

    res = dict(rank=rank, m_loc=m)
    cases = a.cases.split(",")
    nrhs_list = [int(t) for t in a.nrhs.split(",")]
    s = make()
    res["guards"] = guards(s)
    single = {c: one for c, one in enumerate(singles(s, range(a.nvec)))}
    res["single"] = [dict(one["info"], delta=one["delta"]) for one in single.values()]
    if "bits" in cases:
        res["bits"] = {str(k): batched(s, list(range(k)), single)[0] for k in nrhs_list}
    if "counts" in cases:
        res["counts"] = batched(s, [0, 1, 2, 3], single)[0]
    s.close()
    res["comm_errors"] = list(comm.errors)
    if a.comm == "file":
        lib.nkp_comm_file_free(C.byref(comm.ops))
    with open(f"{a.out}.{rank}", "w") as fh:
        json.dump(res, fh)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
