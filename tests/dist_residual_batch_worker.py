"""Worker for tests/test_gpu_residual_batch_dist.py (launched once per rank; the library's file transport, all ranks share the one
GPU; no torch in the process).

Every rank builds a distributed solver on its latitude band of the synthetic 40x46x20 matrix, with every callback of the transport
wrapped so that the calls are recorded in order, and calls nkp_residual_batch* with its rows of seeded global B and X.  The reference
is the single-GPU call on the whole matrix, made here by every rank on a solver without preconditioner.  One JSON file per rank."""
import argparse
import ctypes as C
import json
import os
import sys
import types

import numpy as np

from comm_trace import traced
from dist_values_product_worker import GRID, Device, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--file-dir", required=True)
    a = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    from nk_ocn_tracer_jacobian_precond_amd import dist as nd
    from nk_ocn_tracer_jacobian_precond_amd import solver, synth

    lib = solver.load_library()
    assert lib.nkp_set_device(0) == 0
    lib.nkp_comm_file_init.argtypes = [C.POINTER(solver.NkpCommOps), C.c_char_p, C.c_int, C.c_int]
    lib.nkp_comm_file_free.argtypes = [C.POINTER(solver.NkpCommOps)]
    lib.nkp_comm_file_free.restype = None
    ops = solver.NkpCommOps()
    assert lib.nkp_comm_file_init(C.byref(ops), a.file_dir.encode(), rank, world) == 0
    log = []
    wrapped, orig = traced(solver, ops, log)
    comm = types.SimpleNamespace(ops=wrapped, errors=[], keep=orig)

    p = synth.generate(imt=GRID[0], jmt=GRID[1], km=GRID[2], adv="upwind3", hmix="isop", seed=2, u_scale=3.0, ah=4.0e6, isop_k33=True)
    n = p.flat_len
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    starts = nd.snap_partition(blk, world)
    loc = nd.local_slice(p.rowptr, p.colind, p.nzval, blk, starts, rank, ci, cj)
    f, m = int(loc["fst_row"]), int(loc["m_loc"])
    rng = np.random.default_rng(64)
    B, X = rng.standard_normal((8, n)), rng.standard_normal((8, n))
    X[:, 5::89] = -0.0
    ld = m + 3

    def rows(v):
        """this rank's rows of the vectors v, (K, ld) with a poisoned tail"""
        out = np.full((v.shape[0], ld), np.nan)
        out[:, :m] = v[:, f:f + m]
        return out

    # ---- the reference: the single-GPU call on the whole matrix
    single = {}
    with solver.NkpSolver(p.rowptr, p.colind, p.nzval, None, precond=solver.PRECOND_NONE, restart=4) as g:
        for K in (1, 3, 8):
            db, dx, dr = Device(B[:K]), Device(X[:K]), Device(np.full((K, n), np.nan))
            rn, bn, be = g.residual_batch_device(db.ptr, n, dx.ptr, n, K, dr.ptr, n)
            single[K] = dict(R=dr.get(), rnorm=rn.copy(), bnorm=bn.copy(), berr=be.copy())
            for d in (db, dx, dr):
                d.free()

    res = dict(rank=rank, m_loc=m, n=n)
    s = nd.NkpDistSolver(loc, n, comm, precond=solver.PRECOND_COLUMN_JACOBI, rtol=1e-10, restart=30, max_iters=3000)
    res["halo_rows"] = s.get_int("dist_halo_rows")

    def counters():
        return dict(alltoallv=s.get_int("dist_alltoallv_calls"), allreduce=s.get_int("dist_allreduce_calls"), calls=s.get_int("residual_batch_calls"))

    def delta(c0):
        c1 = counters()
        return {k: c1[k] - c0[k] for k in c0}

    # ---- bits, numbers, the trace and the counters of the device flavour; the host flavour for nrhs = 3
    res["good"] = {}
    for K in (1, 3, 8):
        db, dx, dr = Device(rows(B[:K])), Device(rows(X[:K])), Device(np.full((K + 1, ld), np.nan))
        c0 = counters()
        del log[:]
        rn, bn, be = s.residual_batch_device(db.ptr, ld, dx.ptr, ld, K, dr.ptr, ld)
        trace = list(log)
        got = dr.get()
        ref = single[K]
        out = dict(trace=trace, counters=delta(c0), r_equal=bits(got[:K, :m], ref["R"][:, f:f + m]),
                   sentinels=bool(np.all(np.isnan(got[:, m:])) and np.all(np.isnan(got[K:]))), berr_equal=bits(be, ref["berr"]),
                   rnorm=[v.hex() for v in rn.tolist()], bnorm=[v.hex() for v in bn.tolist()],
                   rnorm_single=[v.hex() for v in ref["rnorm"].tolist()], bnorm_single=[v.hex() for v in ref["bnorm"].tolist()],
                   b_untouched=bits(db.get()[:, :m], B[:K, f:f + m]), x_untouched=bits(dx.get()[:, :m], X[:K, f:f + m]))
        if K == 3:
            del log[:]
            h = s.residual_batch(np.ascontiguousarray(B[:K, f:f + m]), np.ascontiguousarray(X[:K, f:f + m]), want_residual=True)
            out.update(host_trace=list(log), host_r_equal=bits(h.R, got[:K, :m]),
                       host_numbers_equal=bits(h.rnorm, rn) and bits(h.bnorm, bn) and bits(h.berr, be))
        res["good"][str(K)] = out
        for d in (db, dx, dr):
            d.free()

    # ---- the exact norms of the single-GPU residuals (rank 0 computes them for the test's bound)
    if rank == 0:
        import math
        import spmv_shapes as sh

        def exact_norm(v):
            q, e = sh._two_prod(v, v)
            return math.sqrt(math.fsum(q.tolist() + e.tolist()))
        res["exact"] = dict(rnorm=[exact_norm(single[8]["R"][c]).hex() for c in range(8)], bnorm=[exact_norm(B[c]).hex() for c in range(8)])

    # ---- the last rank passes a bad ldx: every rank returns after the first agreement, nothing else is exchanged, and the next call
    # has the bits of the one before
    bad = rank == world - 1
    db, dx, dr = Device(rows(B[:3])), Device(rows(X[:3])), Device(np.full((3, ld), 2.5))
    c0 = counters()
    del log[:]
    try:
        s.residual_batch_device(db.ptr, ld, dx.ptr, m - 1 if bad else ld, 3, dr.ptr, ld)
        out = dict(code=0, message="")
    except solver.NkpError as exc:
        out = dict(code=exc.code, message=str(exc))
    out.update(bad=bad, bad_rank=world - 1, trace=list(log), counters=delta(c0), r_untouched=bool(np.all(dr.get() == 2.5)))
    rn, bn, be = s.residual_batch_device(db.ptr, ld, dx.ptr, ld, 3, dr.ptr, ld)
    out["next_equal"] = bits(dr.get()[:, :m], single[3]["R"][:, f:f + m]) and [v.hex() for v in rn.tolist()] == res["good"]["3"]["rnorm"] and bits(be, single[3]["berr"])
    res["refuse"] = out
    for d in (db, dx, dr):
        d.free()
    s.close()
    res["comm_errors"] = comm.errors
    with open(f"{a.out}.{rank}", "w") as fh:
        json.dump(res, fh)
    lib.nkp_comm_file_free(C.byref(ops))


if __name__ == "__main__":
    main()
