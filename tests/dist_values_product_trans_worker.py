"""Worker for tests/test_gpu_values_product_trans_dist.py (launched once per rank; the library's file transport, all ranks share the
one GPU; no torch in the process).

Every rank builds distributed solvers on its latitude band of the synthetic 40x46x20 matrix and calls
nkp_values_product_trans_dist* with its slices of seeded global values and vectors.  The reference is computed here, in numpy, from
the GLOBAL arrays: the stable host transpose of (pattern, dval), the restatement of its row sums with the global X (a row of more
than 2048 entries in the SpMV's tree), sliced to this rank's rows.  One JSON file per rank."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import types

import numpy as np

from comm_trace import traced
from dist_values_product_worker import GRID, SENTINEL, Device, bits, restate_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LDS_NNZ = 2048          # NKP_SPMV_LDS_NNZ: a row of more entries sits alone in its row block and is summed in the tree
LONG_ROWS = 2500


def host_transpose(rowptr, colind):
    """(rowptrT, rowT, src): row j of the transpose lists the entries of column j in ascending (row, stored position) order"""
    n, nnz = rowptr.size - 1, colind.size
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(rowptr, np.int64)))
    src = np.lexsort((np.arange(nnz), row, np.asarray(colind, np.int64)))
    rowptrT = np.concatenate([[0], np.cumsum(np.bincount(colind, minlength=n))]).astype(np.int64)
    return rowptrT, row[src], src


def tree_sum(prod):
    """the long row of the SpMV kernels: lane-strided partial sums over 256 lanes from +0.0, the 64-lane shuffle tree of every wave,
    then the 4 waves in order"""
    acc = np.zeros(256)
    for k in range(0, prod.size, 256):
        c = prod[k:k + 256]
        acc[:c.size] = acc[:c.size] + c
    a = acc.reshape(4, 64).copy()
    off = 32
    while off:
        a[:, :off] = a[:, :off] + a[:, off:2 * off]
        off >>= 1
    s = 0.0
    for w in range(4):
        s = s + a[w, 0]
    return s


def reference(rowptr, colind, dval, X):
    """t_c = (pattern with dval)^T x_c for every row of X, with the bits of the single-GPU kernel"""
    rowptrT, rowT, src = host_transpose(rowptr, colind)
    valT = dval[src]
    ln = np.diff(rowptrT)
    long_rows = np.flatnonzero(ln > LDS_NNZ)
    keep = np.ones(valT.size, bool)
    for j in long_rows:
        keep[rowptrT[j]:rowptrT[j + 1]] = False
    short_ptr = np.concatenate([[0], np.cumsum(np.where(ln > LDS_NNZ, 0, ln))])
    out = []
    for x in X:
        t = restate_rows(short_ptr, rowT[keep], valT[keep], x)
        for j in long_rows:
            a, z = rowptrT[j], rowptrT[j + 1]
            t[j] = tree_sum(valT[a:z] * x[rowT[a:z]])
        out.append(t)
    return np.stack(out), long_rows


def long_column_matrix(rowptr, colind, n):
    """the same pattern with one more entry in column j* in 2500 rows spread evenly over all rows, and a handful of rows stored in
    descending column order with their first column repeated"""
    jstar = n // 3
    extra = np.unique(np.linspace(0, n - 1, LONG_ROWS).astype(np.int64))
    flipped = {7, n // 4 + 1, n // 2, (3 * n) // 4 + 2, n - 5}
    has = np.zeros(n, bool)
    has[extra] = True
    rows = []
    for r in range(n):
        c = np.asarray(colind[rowptr[r]:rowptr[r + 1]], np.int64)
        if has[r]:
            c = np.concatenate([c, [jstar]])
        if r in flipped:
            c = np.sort(c)[::-1]
            c = np.concatenate([c, c[:1]])
        rows.append(c)
    rp = np.concatenate([[0], np.cumsum([c.size for c in rows])]).astype(np.int32)
    return rp, np.concatenate(rows).astype(np.int32), jstar, extra.size, sorted(flipped)


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
    e0, e1 = int(p.rowptr[f]), int(p.rowptr[f + m])
    rng = np.random.default_rng(62)
    dval = p.nzval * rng.standard_normal(p.nzval.size)
    dval[::53] = 0.0
    X, Y0, Z = rng.standard_normal((8, n)), rng.standard_normal((8, n)), rng.standard_normal((1, n))
    X[:, 5::89] = -0.0
    dval_loc = np.ascontiguousarray(dval[e0:e1])
    ld = m + 3
    T, long_rows = reference(p.rowptr, p.colind, dval, X)
    assert long_rows.size == 0

    def rows(v, fill=np.nan):
        """this rank's rows of the vectors v, (K, ld) with a poisoned tail"""
        out = np.full((v.shape[0], ld), fill)
        out[:, :m] = v[:, f:f + m]
        return out

    res = dict(rank=rank, m_loc=m, nnz_loc=e1 - e0)

    def code_of(fn):
        try:
            fn()
            return dict(code=0, message="")
        except solver.NkpError as exc:
            return dict(code=exc.code, message=str(exc))

    def counters(s):
        return dict(alltoallv=s.get_int("dist_alltoallv_calls"), allreduce=s.get_int("dist_allreduce_calls"), calls=s.get_int("values_product_trans_calls"),
                    index=s.get_int("trans_index_bytes"))

    def device_bits(s, dv, K, T_, out):
        """the two device calls of the issue: 0.37 accumulated on a seeded y with sentinel tails, -1 written over NaN"""
        dx, dy = Device(rows(X[:K])), Device(rows(Y0[:K], SENTINEL))
        c0 = counters(s)
        del log[:]
        s.values_product_trans_dist_device(dv.ptr, dx.ptr, K, ld, dy.ptr, ld, alpha=0.37, accumulate=True)
        out.update(trace=list(log))
        c1 = counters(s)
        got = dy.get()
        out.update(acc_equal=bits(got[:, :m], Y0[:K, f:f + m] + 0.37 * T_[:K, f:f + m]), tail=bool(np.all(got[:, m:] == SENTINEL)),
                   x_untouched=bits(dx.get()[:, :m], X[:K, f:f + m]) and bool(np.all(np.isnan(dx.get()[:, m:]))),
                   alltoallv=c1["alltoallv"] - c0["alltoallv"], allreduce=c1["allreduce"] - c0["allreduce"], calls=c1["calls"] - c0["calls"],
                   index_before=c0["index"], index_after=c1["index"])
        dn = Device(np.full((K, ld), np.nan))
        del log[:]
        s.values_product_trans_dist_device(dv.ptr, dx.ptr, K, ld, dn.ptr, ld, alpha=-1.0, accumulate=False)
        out.update(write_trace=list(log))
        got = dn.get()
        out.update(write_equal=bits(got[:, :m], -1.0 * T_[:K, f:f + m]), write_tail=bool(np.all(np.isnan(got[:, m:]))))
        for d in (dx, dy, dn):
            d.free()
        return out

    # ---- 1, 2, 3: bits of both flavours and the counters, on a solver that never solves
    s = nd.NkpDistSolver(loc, n, comm, precond=solver.PRECOND_COLUMN_JACOBI, rtol=1e-10, restart=60, max_iters=3000)
    res["halo_rows"] = s.get_int("dist_halo_rows")
    dv = Device(dval_loc)
    res["index_bytes_at_start"] = s.get_int("trans_index_bytes")
    res["bits"] = {str(K): device_bits(s, dv, K, T, {}) for K in (1, 3, 4, 8)}
    c0 = counters(s)
    del log[:]
    host = s.values_product_trans_dist(dval_loc, np.ascontiguousarray(X[:3, f:f + m]), alpha=0.37, Y=np.ascontiguousarray(Y0[:3, f:f + m]))
    host_trace = list(log)
    c1 = counters(s)
    host_w = s.values_product_trans_dist(dval_loc, np.ascontiguousarray(X[:3, f:f + m]), alpha=-1.0)
    res["host"] = dict(acc_equal=bits(host, Y0[:3, f:f + m] + 0.37 * T[:3, f:f + m]), write_equal=bits(host_w, -1.0 * T[:3, f:f + m]),
                       alltoallv=c1["alltoallv"] - c0["alltoallv"], calls=c1["calls"] - c0["calls"], trace=host_trace)
    res["sent_entries"], res["recv_entries"] = s.get_int("trans_index_sent_entries"), s.get_int("trans_index_recv_entries")
    idx = s.get_int("trans_index_bytes")
    s.refactor_dist(loc["val"] * 0.75)
    res["after_refactor"] = device_bits(s, dv, 3, T, dict(index_kept=s.get_int("trans_index_bytes") == idx))

    # ---- 4: <G^T x, z> = <x, G z>, this rank's part of both sums
    dx, dz, dy, dg = Device(rows(X[:1])), Device(rows(Z)), Device(np.zeros((1, ld))), Device(np.zeros((1, ld)))
    s.values_product_trans_dist_device(dv.ptr, dx.ptr, 1, ld, dy.ptr, ld)
    s.values_product_device(dv.ptr, dz.ptr, 1, ld, dg.ptr, ld)
    res["adjoint"] = dict(gtx_z=math.fsum(dy.get()[0, :m] * Z[0, f:f + m]), x_gz=math.fsum(X[0, f:f + m] * dg.get()[0, :m]))
    for d in (dx, dz, dy, dg):
        d.free()

    # ---- 7: the transposed handle is refused on the calling rank: no file of this rank appears in the transport's directory
    t = s.transposed_dist()
    mine = lambda: sorted(fn for fn in os.listdir(a.file_dir) if fn.endswith(f".{rank}"))
    files, c0 = mine(), counters(s)
    dx, dy = Device(rows(X[:2])), Device(np.full((2, ld), 2.5))
    out = code_of(lambda: t.values_product_trans_dist_device(dv.ptr, dx.ptr, 2, ld, dy.ptr, ld))
    out.update(y_untouched=bool(np.all(dy.get() == 2.5)), files_unchanged=mine() == files, counters_unchanged=counters(s) == c0)
    res["handle"] = out
    dx.free()
    dy.free()
    s.close()
    dv.free()

    # ---- 5: a column of more than 2048 entries from every rank, rows stored in descending order with a repeated column
    rpL, ciL, jstar, added, flipped = long_column_matrix(p.rowptr, p.colind, n)
    a0, a1 = int(rpL[f]), int(rpL[f + m])
    dvalL = np.random.default_rng(63).standard_normal(ciL.size)
    dvalL[::53] = 0.0
    TL, long_rows = reference(rpL, ciL, dvalL, X[:4])
    per_rank = [int(np.count_nonzero(ciL[rpL[starts[r]]:rpL[starts[r + 1]]] == jstar)) for r in range(world)]
    locL = dict(rowptr=(rpL[f:f + m + 1].astype(np.int64) - a0).astype(np.int32), colind=np.ascontiguousarray(ciL[a0:a1]), val=np.ones(a1 - a0),
                blk_start=np.arange(m + 1, dtype=np.int32), fst_row=f, m_loc=m)
    sl = nd.NkpDistSolver(locL, n, comm, precond=solver.PRECOND_NONE, restart=4)
    dv = Device(dvalL[a0:a1])
    res["long"] = dict(long_rows=long_rows.tolist(), jstar=jstar, column_entries=int(np.count_nonzero(ciL == jstar)), per_rank=per_rank, added=added,
                       descending=all(bool(np.any(np.diff(ciL[rpL[r]:rpL[r + 1]]) < 0)) for r in flipped),
                       repeated=all(np.unique(ciL[rpL[r]:rpL[r + 1]]).size < rpL[r + 1] - rpL[r] for r in flipped),
                       owner=bool(f <= jstar < f + m), bits={str(K): device_bits(sl, dv, K, TL, {}) for K in (1, 4)})
    sl.close()
    dv.free()

    # ---- 6: the last rank passes nine vectors, before the index exists and after: every rank returns, the next solve has its bits
    bad = rank == world - 1
    sm = nd.NkpDistSolver(loc, n, comm, rtol=1e-10, restart=60, max_iters=3000)
    dv, db, dx, dy = Device(dval_loc), Device(rows(Y0[:2])), Device(rows(np.vstack([X, X[:1]]))), Device(np.zeros((9, ld)))
    d1, d2, ys = Device(np.zeros((2, ld))), Device(np.zeros((2, ld))), Device(np.full((9, ld), 2.5))
    sm.solve_batch_device(db.ptr, d1.ptr, 2, ld, raise_on_fail=False)
    res["refuse"] = []
    for has_index in (False, True):
        c0 = counters(sm)
        del log[:]
        out = code_of(lambda: sm.values_product_trans_dist_device(dv.ptr, dx.ptr, 9 if bad else 4, ld, ys.ptr, ld))
        c1 = counters(sm)
        out.update(trace=list(log), exchanges=c1["alltoallv"] - c0["alltoallv"] + c1["allreduce"] - c0["allreduce"], y_untouched=bool(np.all(ys.get() == 2.5)))
        out.update(bad=bad, bad_rank=world - 1, calls_unchanged=c1["calls"] == c0["calls"], index_unchanged=c1["index"] == c0["index"],
                   had_index=c0["index"] > 0, want_index=has_index)
        sm.solve_batch_device(db.ptr, d2.ptr, 2, ld, raise_on_fail=False)
        out["next_solve_equal"] = bits(d1.get(), d2.get())
        res["refuse"].append(out)
        del log[:]
        sm.values_product_trans_dist_device(dv.ptr, dx.ptr, 4, ld, dy.ptr, ld)
        out.update(next_trace=list(log), next_equal=bits(dy.get()[:4, :m], T[:4, f:f + m]))
        if not has_index:
            res["multilevel_equal"] = out["next_equal"]
    for d in (dv, db, dx, dy, d1, d2, ys):
        d.free()
    sm.close()

    # ---- 7: force_dist on one rank (rank 0 alone, a communicator of its own): the distributed path with empty exchanges has the
    # bits of nkp_values_product_trans_device on a plain solver
    if rank == 0:
        solo_dir = a.file_dir + ".solo"
        os.makedirs(solo_dir)
        ops1 = solver.NkpCommOps()
        assert lib.nkp_comm_file_init(C.byref(ops1), solo_dir.encode(), 0, 1) == 0
        whole = nd.local_slice(p.rowptr, p.colind, p.nzval, blk, np.array([0, n]), 0, ci, cj)
        opts = dict(precond=solver.PRECOND_COLUMN_JACOBI, rtol=1e-10, restart=60, max_iters=3000)
        s1 = nd.NkpDistSolver(whole, n, types.SimpleNamespace(ops=ops1, errors=[]), tuning=dict(force_dist=1), **opts)
        s0 = solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, 1, **opts)
        dv, dx, y1, y0, y2 = Device(dval), Device(X[:3]), Device(np.full((3, n), np.nan)), Device(np.full((3, n), np.nan)), Device(np.full((3, n), np.nan))
        c0 = counters(s1)
        s1.values_product_trans_dist_device(dv.ptr, dx.ptr, 3, n, y1.ptr, n, alpha=0.37)
        c1 = counters(s1)
        s0.values_product_trans_device(dv.ptr, dx.ptr, 3, n, y0.ptr, n, alpha=0.37)
        nd.NkpDistSolver.values_product_trans_dist_device(s0, dv.ptr, dx.ptr, 3, n, y2.ptr, n, alpha=0.37)      # a plain solver: the call IS nkp_values_product_trans_device
        res["solo"] = dict(distributed=s1.get_int("dist_halo_rows") == 0 and c1["alltoallv"] - c0["alltoallv"] == 1 and c1["calls"] - c0["calls"] == 1,
                           equal_plain=bits(y1.get(), y0.get()), equal_reference=bits(y1.get(), 0.37 * T[:3]), sent=s1.get_int("trans_index_sent_entries"),
                           recv=s1.get_int("trans_index_recv_entries"), index=c1["index"] > 0, plain_equal=bits(y2.get(), y0.get()),
                           plain_calls=s0.get_int("values_product_trans_calls"))
        for d in (dv, dx, y1, y0, y2):
            d.free()
        s1.close()
        s0.close()
        lib.nkp_comm_file_free(C.byref(ops1))

    res["comm_errors"] = comm.errors
    with open(f"{a.out}.{rank}", "w") as fh:
        json.dump(res, fh)
    lib.nkp_comm_file_free(C.byref(ops))


if __name__ == "__main__":
    main()
