"""Worker of tests/test_gpu_batch_dist.py, one process per rank, all ranks on the test box's one GPU.

Every case compares a batched solve (NkpDistSolver.solve_many, nkp_solve with nrhs >= 2) with the SAME distributed solver's
one-at-a-time solves of the same right-hand sides.  All ranks run the same cases in the same order (the calls are collective).

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
    ap.add_argument("--partition", default="bands")
    ap.add_argument("--opts", default="{}", help="JSON: options of NkpDistSolver on top of rtol / restart / max_iters")
    ap.add_argument("--nrhs", default="2,3,4,5")
    ap.add_argument("--nvec", type=int, default=5)
    a = ap.parse_args()
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import oracle_binding as ora
    from nk_ocn_tracer_jacobian_precond_amd import dist as nd
    from nk_ocn_tracer_jacobian_precond_amd import solver, synth
    torch.cuda.set_device(0)
    lib = solver.load_library()

    imt, jmt, km = (int(t) for t in a.grid.split("x"))
    p = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=5)
    n = p.flat_len
    cnt = 1
    glob = None                                         # the global matrix, where the oracle checks against it
    if a.partition == "tracers":
        loc, starts, n = nd.tracer_slice(p, rank, world)
    elif a.partition == "cells":
        cnt = 2
        p2 = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=5, coupled_tracer_cnt=cnt)
        blk2 = solver.column_blocks(p2.col_start(), p2.tracer_state_len, cnt)
        ci2, cj2 = solver.column_coords(p2.ind_i, p2.ind_j, p2.col_start(), cnt)
        loc, starts, perm = nd.cell_major_slice(p2.rowptr, p2.colind, p2.nzval, blk2, cnt, world, rank, ci2, cj2)
        n = p2.flat_len
    else:
        blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
        ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
        starts = nd.snap_partition(blk, world)
        loc = nd.local_slice(p.rowptr, p.colind, p.nzval, blk, starts, rank, ci, cj)
        glob = p
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
                    overlap=s.get_int("dist_overlap"), rings=s.get_int("dist_ras_rings"), smooth=s.get_int("dist_smooth_exchange"))

    res = dict(rank=rank, m_loc=m)
    cases = a.cases.split(",")
    nrhs_list = [int(t) for t in a.nrhs.split(",")]
    s = make()
    res["guards"] = guards(s)
    single = {}
    if any(c in cases for c in ("bits", "counts", "accuracy", "refactor", "narrow")):
        for c, one in enumerate(singles(s, range(a.nvec))):
            single[c] = one
        res["single"] = [dict(one["info"], delta=one["delta"]) for one in single.values()]
    if "bits" in cases:
        res["bits"] = {str(k): batched(s, list(range(k)), single)[0] for k in nrhs_list}
    if "narrow" in cases:
        # ONE solver through groups of 8, 2 and 4 right-hand sides, then a solve alone: the interleave narrows on live exchanges
        groups = {str(k): batched(s, list(range(k)), single)[0] for k in (8, 2, 4)}
        again = singles(s, (1,))[0]
        # the host plan of the same create: the rows this rank sends and receives per colour of the fine-level exchange
        pl = nd.overlap_plan_host(loc, n, comm, cnt, tuning=dict(opts["tuning"]))
        rows = {k: int(pl[k].size) for k in ("smooth_send_rows0", "smooth_send_rows1", "smooth_recv_rows0", "smooth_recv_rows1")}
        res["narrow"] = dict(groups=groups, smooth_rows=rows, again=dict(x_equal=bool(np.array_equal(again["x"], single[1]["x"])), iters=again["info"]["iters"], delta=again["delta"]))
    if "counts" in cases:
        res["counts"] = batched(s, [0, 1, 2, 3], single)[0]
    if "accuracy" in cases:
        out, X = batched(s, [0, 1, 2, 3], single)
        checked = []
        for q in range(4):
            xg = np.zeros(n if rank == 0 else 1)
            x_loc = np.ascontiguousarray(X[q])
            rc = lib.nkp_gather_root(s._h, solver._p(x_loc, C.c_double), solver._p(xg, C.c_double))
            assert rc == 0, lib.nkp_last_error().decode()
            if rank == 0:
                r = Bg[q] - ora.spmv(glob.rowptr, glob.colind, glob.nzval, xg)
                checked.append(float(np.linalg.norm(r) / np.linalg.norm(Bg[q])))
        out["relres_checked"] = checked
        res["accuracy"] = out
    if "zero" in cases:
        keep = B[1].copy()
        one = {c: o for c, o in zip((0, 2), singles(s, (0, 2)))}
        B[1] = 0.0
        one[1] = singles(s, (1,))[0]
        res["zero"] = batched(s, [0, 1, 2], one)[0]
        B[1] = keep
    if "refactor" in cases:
        # members exist (the batched calls above, or this one); new values must reach them
        s.solve_many(B[:4], raise_on_fail=False)
        scale = 1.0 + 0.05 * np.random.default_rng(100 + rank).random(loc["val"].size)
        s.refactor_dist(loc["val"] * scale)
        c0 = counters(s)
        X, infos = s.solve_many(B[:4], raise_on_fail=False)
        moved = counters(s)["batch_steps"] - c0["batch_steps"]
        after = singles(s, range(4))
        res["refactor"] = dict(columns=[dict(x_equal=bool(np.array_equal(X[c], after[c]["x"])), iters=infos[c]["iters"], iters_single=after[c]["info"]["iters"],
                                             relres_equal=bool(infos[c]["relres"] == after[c]["info"]["relres"]), status=infos[c]["status"],
                                             differs_from_old=bool(not np.array_equal(X[c], single[c]["x"]))) for c in range(4)],
                               batch_steps=moved, refactor_count=s.get_int("refactor_count"))
    s.close()
    for name, over in (("fallback_equil", dict(equil=1)), ("fallback_rhs_batch0", dict(tuning=dict(rhs_batch=0)))):
        if name in cases:
            t = make(**over)
            one = {c: o for c, o in enumerate(singles(t, range(2)))}
            out = batched(t, [0, 1], one)[0]
            out["equil"] = t.get_int("equil")
            res[name] = out
            t.close()
    if "broken" in cases:
        # the allreduce of EVERY rank takes part in the real collective and reports failure from its n-th call on (armed after
        # the create): the batched call ends with NKP_ECOMM on every rank, nobody waits for anybody
        state = dict(armed=False, calls=0, after=7)

        def failing(ctx, buf, count, op, stream):
            rc = comm._allreduce(ctx, buf, count, op, stream)
            if state["armed"]:
                state["calls"] += 1
                if state["calls"] >= state["after"]:
                    return 1
            return rc
        fn = solver._ALLREDUCE_FN(failing)
        ops = solver.NkpCommOps()
        C.memmove(C.byref(ops), C.byref(comm.ops), C.sizeof(ops))
        ops.allreduce = fn
        bad = types.SimpleNamespace(ops=ops, errors=comm.errors)
        t = make(transport=bad)
        state["armed"] = True
        try:
            t.solve_many(B[:4], raise_on_fail=False)
            out = dict(code=0, message="")
        except solver.NkpError as exc:
            out = dict(code=exc.code, message=str(exc))
        out["failing_calls"] = state["calls"]
        state["armed"] = False
        t.close()
        u = make()
        x, info = u.solve(B[0], raise_on_fail=False)
        out["single_after"] = info
        u.close()
        res["broken"] = out
    res["comm_errors"] = list(comm.errors)
    if a.comm == "file":
        lib.nkp_comm_file_free(C.byref(comm.ops))
    with open(f"{a.out}.{rank}", "w") as fh:
        json.dump(res, fh)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
