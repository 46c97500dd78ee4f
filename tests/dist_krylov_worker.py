"""Worker of tests/test_gpu_krylov_dist.py, one process per rank, all ranks on the test box's one GPU (gloo + host staging).

  --mode one   one rank forced distributed (NKP_FORCE_DIST=1), with or without NKP_DIST_ONE_REDUCE=1: the worker runs the
               restated driver of tests/krylov_reference.py itself on the solver's own spmv and precond_apply (with the
               pythagoras epilogue under one reduction) and writes, per run, the relative difference in x, the iterations, the
               status and the residuals of both sides
  --mode two   latitude bands of n2001 on two ranks: every rank writes its slice of x_k; the test gathers them and compares
               with the single-process restatement on the global matrix
  --mode refuse  two ranks on the library's file transport (directory <out>.comm): a right-hand side with a NaN in a row of rank 1,
               and b 2^-600, are refused on BOTH ranks (the counts of classify_rhs are added across them), and a clean solve
               afterwards has the bits of the one before
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--mode", required=True)
    a = ap.parse_args()
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import krylov_cases as kc
    import krylov_reference as kr
    from nk_ocn_tracer_jacobian_precond_amd import dist as nd

    torch.cuda.set_device(0)
    comm = nd.TorchComm()
    one_reduce = os.environ.get("NKP_DIST_ONE_REDUCE", "0") == "1"
    res = dict(rank=rank, one_reduce=one_reduce, runs={})

    def local(c):
        starts = nd.snap_partition(c.blk, world)
        loc = nd.local_slice(c.rowptr, c.colind, c.val, c.blk, starts, rank)
        return loc, int(loc["fst_row"]), int(loc["m_loc"])

    if a.mode == "refuse":
        from nk_ocn_tracer_jacobian_precond_amd import solver
        lib = solver.load_library()
        lib.nkp_comm_file_init.argtypes = [C.POINTER(solver.NkpCommOps), C.c_char_p, C.c_int, C.c_int]
        lib.nkp_comm_file_free.argtypes = [C.POINTER(solver.NkpCommOps)]
        lib.nkp_comm_file_free.restype = None
        os.makedirs(a.out + ".comm", exist_ok=True)
        dist.barrier()
        ops = solver.NkpCommOps()
        assert lib.nkp_comm_file_init(C.byref(ops), (a.out + ".comm").encode(), rank, world) == 0
        fcomm = types.SimpleNamespace(ops=ops, errors=[])
        run = kc.Run("n2001", kc.JACOBI, None, restart=8)
        c = kc.case(run.case)
        loc, f, m = local(c)
        s = nd.NkpDistSolver(loc, c.n, fcomm, **run.options())
        x0, info0 = s.solve(c.b[f:f + m], raise_on_fail=False)
        res.update(m_loc=m, fst_row=f, clean=info0, refused={})
        nan = c.b.copy()
        nan[c.n - 5] = np.nan                                # a row of the last rank
        for what, b in (("nan_on_rank_1", nan), ("down600", kc.bad_rhs(c.b, "down600"))):
            x, info = s.solve(b[f:f + m], raise_on_fail=False)
            res["refused"][what] = dict(status=info["status"], iters=info["iters"], relres_is_nan=bool(info["relres"] != info["relres"]),
                                        rows_nan=int(np.isnan(x).sum()), holds_nan=bool(np.isnan(b[f:f + m]).any()))
        x1, info1 = s.solve(c.b[f:f + m], raise_on_fail=False)
        res["clean_again"] = bool(kc.same_bits(x1, x0) and info1 == info0)
        s.close()
        res["comm_errors"] = list(fcomm.errors)
        lib.nkp_comm_file_free(C.byref(ops))
        with open(f"{a.out}.{rank}", "w") as fh:
            json.dump(res, fh)
        dist.barrier()
        dist.destroy_process_group()
        return

    for run in (kc.dist_one_rank_runs() if a.mode == "one" else kc.dist_two_rank_runs()):
        c = kc.case(run.case)
        loc, f, m = local(c)
        s = nd.NkpDistSolver(loc, c.n, comm, **run.options())
        calls = s.get_int("dist_allreduce_calls")
        x, info = s.solve(c.b[f:f + m], raise_on_fail=False)
        out = dict(info, allreduce_calls=s.get_int("dist_allreduce_calls") - calls, m_loc=m, fst_row=f)
        if a.mode == "one":
            ref = kc.reference(run, s.spmv, s.precond_apply, pythagoras=one_reduce and not run.reorth)
            tol = kc.TOL[run.cls][1]
            out.update(dx=float(np.linalg.norm(x - ref.x) / np.linalg.norm(ref.x)), tol=tol, ref_iters=ref.iters, ref_status=ref.status,
                       ref_relres=ref.relres, relres_bound=c.relres_bound(ref.x, ref.relres, tol), stagnated=ref.stagnated,
                       weak=[[d.its, d.taken] for d in ref.log if d.kind == "weak"],
                       closest_decision=min(d.dist for d in ref.log))
            if c.exact is not None:
                out["error"] = float(np.linalg.norm(x - c.exact) / np.linalg.norm(c.exact))
        else:
            np.save(f"{a.out}.{rank}.{run.id}.npy", x)
        s.close()
        res["runs"][run.id] = out
    res["comm_errors"] = list(comm.errors)
    with open(f"{a.out}.{rank}", "w") as fh:
        json.dump(res, fh)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
