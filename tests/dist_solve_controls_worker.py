"""Worker of tests/test_gpu_solve_controls_dist.py, one process per rank, all ranks on the test box's one GPU, collectives over
the library's file transport (nkp_comm_file_init), which promises a batched column the bits of its single solve.

Both ranks run the same calls in the same order (they are collective).  The transport is wrapped: every callback of
nkp_comm_ops appends its name to a log, so the test sees which collectives a call made and in which order.
One JSON file per rank."""
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

RTOL5 = [1e-3, 1e-10, 1e-6, 1e-12, 1e-4]
GUESS5 = [1, 0, 1, 0, 1]
BASE = dict(restart=5, rtol=1e-10, atol=0.0, max_iters=300, tuning=dict(ml_coarsest_rows=40))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--file-dir", required=True)
    a = ap.parse_args()
    rank, world = a.rank, a.world
    from nk_ocn_tracer_jacobian_precond_amd import dist as nd
    from nk_ocn_tracer_jacobian_precond_amd import solver, synth
    from test_gpu_solve_controls import Dev
    lib = solver.load_library()
    assert lib.nkp_set_device(0) == 0

    p = synth.generate(imt=12, jmt=10, km=10, adv="upwind3", hmix="isop", seed=36)
    n = p.flat_len
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    starts = nd.snap_partition(blk, world)
    loc = nd.local_slice(p.rowptr, p.colind, p.nzval, blk, starts, rank, ci, cj)
    f, m = int(loc["fst_row"]), int(loc["m_loc"])
    Bg = np.random.default_rng(30).standard_normal((5, n))
    Bg[2] *= 1e-3
    B = np.ascontiguousarray(Bg[:, f:f + m])
    xi = np.ascontiguousarray(np.random.default_rng(77).standard_normal((5, n))[:, f:f + m])

    lib.nkp_comm_file_init.argtypes = [C.POINTER(solver.NkpCommOps), C.c_char_p, C.c_int, C.c_int]
    lib.nkp_comm_file_free.argtypes = [C.POINTER(solver.NkpCommOps)]
    lib.nkp_comm_file_free.restype = None
    inner = solver.NkpCommOps()
    assert lib.nkp_comm_file_init(C.byref(inner), a.file_dir.encode(), rank, world) == 0

    log = []

    def allreduce(ctx, buf, count, op, stream):
        log.append("allreduce")
        return inner.allreduce(ctx, buf, count, op, stream)

    def alltoallv(ctx, send, scnt, recv, rcnt, stream):
        log.append("alltoallv")
        return inner.alltoallv(ctx, send, scnt, recv, rcnt, stream)

    def alltoallv_i32(ctx, send, scnt, recv, rcnt):
        log.append("alltoallv_i32_host")
        return inner.alltoallv_i32_host(ctx, send, scnt, recv, rcnt)

    def allgather(ctx, mine, out):
        log.append("allgather_i64_host")
        return inner.allgather_i64_host(ctx, mine, out)

    keep = (solver._ALLREDUCE_FN(allreduce), solver._ALLTOALLV_FN(alltoallv), solver._ALLTOALLV_I32_FN(alltoallv_i32), solver._ALLGATHER_I64_FN(allgather))
    ops = solver.NkpCommOps()
    C.memmove(C.byref(ops), C.byref(inner), C.sizeof(ops))
    ops.allreduce, ops.alltoallv, ops.alltoallv_i32_host, ops.allgather_i64_host = keep
    comm = types.SimpleNamespace(ops=ops, errors=[])

    def make(**over):
        return nd.NkpDistSolver(loc, n, comm, **dict(BASE, **over))

    def calls(fn):
        """(what fn returns or the NkpError it raises, the callbacks it reached)"""
        del log[:]
        try:
            out = fn()
        except solver.NkpError as exc:
            out = dict(code=exc.code, message=str(exc))
        return out, list(log)

    def pack(x, infos):
        return dict(x=np.asarray(x).tobytes().hex(), infos=[[i["status"], i["iters"], float(i["relres"]).hex(), float(i["berr"]).hex()] for i in infos])

    def every_call(s):
        x, info = s.solve(B[0], raise_on_fail=False)
        X, infos = s.solve_many(B[:3], raise_on_fail=False)
        return [pack(x, [info]), pack(X, infos)]

    res = dict(rank=rank, m_loc=m)
    s = make()
    res["dist_on"] = dict(ras=s.get_int("dist_ras"), halo=s.get_int("dist_halo_rows"), levels=s.get_int("levels"))
    created = s.get_solve_controls()

    # ---- the setter is collective
    out = {}
    t = make(rtol=1e-3, max_iters=200)
    out["created_with"] = every_call(t)
    t.close()
    out["untouched"] = every_call(s)
    _, out["set_calls"] = calls(lambda: s.set_solve_controls(rtol=1e-3, max_iters=200))
    out["set_controls"] = s.get_solve_controls()
    out["set"] = every_call(s)
    # different values on the ranks: refused everywhere, nothing changes
    out["mismatch"], out["mismatch_calls"] = calls(lambda: s.set_solve_controls(rtol=1e-4 if rank == 0 else 1e-5))
    out["mismatch_controls"] = s.get_solve_controls()
    out["mismatch_iters"], out["mismatch_iters_calls"] = calls(lambda: s.set_solve_controls(max_iters=40 + rank))
    # rank 1's own check fails (a NaN), rank 0's values are fine
    bad = solver.NkpSolveControls(C.sizeof(solver.NkpSolveControls), 0, float("nan") if rank == 1 else 1e-4, -1.0)
    del log[:]
    out["local_code"] = lib.nkp_set_solve_controls(s._h, C.byref(bad))
    out["local_message"], out["local_calls"] = solver.last_error(), list(log)
    out["after_refusals_controls"] = s.get_solve_controls()
    out["after_refusals"] = every_call(s)
    _, out["reset_calls"] = calls(s.reset_solve_controls)
    out["reset_controls"] = s.get_solve_controls()
    out["reset"] = every_call(s)
    out["created"] = created
    res["setter"] = out

    # ---- per-column controls and guesses on two ranks
    out = {}
    s.set_solve_controls(rtol=1e-12)
    exact = np.stack([s.solve(B[c])[0] for c in range(5)])
    s.reset_solve_controls()
    X0 = np.where(np.array(GUESS5)[:, None] != 0, exact * (1.0 + 1e-3 * xi), 0.0)
    single = []
    r = make()
    for c in range(5):
        r.set_solve_controls(rtol=RTOL5[c])
        with Dev(B[c]) as d_b, Dev(X0[c]) as d_x:
            info = r.solve_device(d_b.ptr, d_x.ptr, use_guess=bool(GUESS5[c]), raise_on_fail=False)
            single.append(pack(d_x.get(), [info]))
    r.close()
    out["single"] = single
    guesses = [X0[c] if GUESS5[c] else None for c in range(5)]
    for nrhs in (5, 2):
        steps = s.get_int("batch_steps")
        (X, infos), seen = calls(lambda: s.solve_many(B[:nrhs], raise_on_fail=False, X0=guesses[:nrhs], rtol=RTOL5[:nrhs]))
        out[f"ex{nrhs}"] = dict(columns=[pack(X[c], [infos[c]]) for c in range(nrhs)], first_call=seen[0], batch_steps=s.get_int("batch_steps") - steps,
                                controls=s.get_solve_controls())
    # the ranks pass different arrays: refused by the one allgather, before any exchange
    a2a = s.get_int("dist_alltoallv_calls")
    other = [RTOL5[0], RTOL5[1] * (1 if rank == 0 else 2)]
    out["mismatch"], out["mismatch_calls"] = calls(lambda: s.solve_many(B[:2], raise_on_fail=False, X0=guesses[:2], rtol=other))
    out["mismatch_null"], out["mismatch_null_calls"] = calls(lambda: s.solve_many(B[:2], raise_on_fail=False, X0=guesses[:2], rtol=RTOL5[:2] if rank == 0 else None))
    out["mismatch_alltoallv"] = s.get_int("dist_alltoallv_calls") - a2a
    (X, infos), _ = calls(lambda: s.solve_many(B[:2], raise_on_fail=False, X0=guesses[:2], rtol=RTOL5[:2]))
    out["after_mismatch"] = [pack(X[c], [infos[c]]) for c in range(2)]
    res["ex"] = out

    s.close()
    res["comm_errors"] = list(comm.errors)
    lib.nkp_comm_file_free(C.byref(inner))
    with open(f"{a.out}.{rank}", "w") as fh:
        json.dump(res, fh)


if __name__ == "__main__":
    main()
