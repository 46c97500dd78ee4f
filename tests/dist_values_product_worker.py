"""Worker for tests/test_gpu_values_product_dist.py (launched once per rank; the library's file transport, all ranks share the
one GPU; no torch in the process).

Every rank builds a distributed solver on its latitude band of the synthetic 40x46x20 matrix and calls nkp_values_product* /
nkp_solve_tangent_device with its slices of seeded global values and vectors; the reference is the numpy restatement of the row
sums on the rank's local CSR, in the order it passed.  One JSON file per rank."""
import argparse
import ctypes as C
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GRID = (40, 46, 20)
SENTINEL = -7.25e77


def restate_rows(rowptr, colind, val, x):
    """+0.0, then every stored entry of the row in stored order, each product and each sum rounded (rows of fewer than 2048 entries)"""
    rowptr = np.asarray(rowptr, np.int64)
    ln = np.diff(rowptr)
    acc = np.zeros(ln.size)
    col = np.asarray(colind, np.int64)
    for k in range(int(ln.max(initial=0))):
        rows = np.flatnonzero(ln > k)
        e = rowptr[rows] + k
        acc[rows] = acc[rows] + val[e] * x[col[e]]
    return acc


def bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return bool(a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)))


class Device:
    def __init__(self, a):
        self.hip = C.CDLL("libamdhip64.so")
        a = np.ascontiguousarray(a, np.float64)
        self.shape, self.size, self.p = a.shape, a.size, C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(max(a.nbytes, 8))) == 0
        assert self.hip.hipMemcpy(self.p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
        self.ptr = self.p.value

    def get(self):
        out = np.empty(self.size)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(out.nbytes), 2) == 0
        return out.reshape(self.shape)

    def free(self):
        self.hip.hipFree(self.p)


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
    from comm_trace import Recorder, traced
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
    rowptr_loc, colind_glob = p.rowptr[f:f + m + 1].astype(np.int64) - e0, p.colind[e0:e1]
    rng = np.random.default_rng(62)
    dval = p.nzval * rng.standard_normal(p.nzval.size)
    dval[::53] = 0.0
    X, Y0, dB = rng.standard_normal((9, n)), rng.standard_normal((4, n)), rng.standard_normal((4, n))
    X[:, 5::89] = -0.0
    dval_loc = np.ascontiguousarray(dval[e0:e1])
    ld = m + 3

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

    s = nd.NkpDistSolver(loc, n, comm, rtol=1e-10, restart=60, max_iters=3000)
    res["halo_rows"] = s.get_int("dist_halo_rows")
    dv = Device(dval_loc)

    # ---- the order of the transport's callbacks and the counters, before anything else so that nrhs = 3 is the solver's first call
    # at width 4: the product in both flavours, a refused call, then the tangent solve up to the first callback of its batched solve
    rec, bad = Recorder(log, "values_product_calls"), rank == world - 1
    out = {}
    dx9, ys = Device(rows(X)), Device(np.full((9, ld), 2.5))
    for K in (1, 3):
        dy = Device(np.full((K, ld), np.nan))
        out[f"device{K}"], _ = rec.run(s, lambda: s.values_product_device(dv.ptr, dx9.ptr, K, ld, dy.ptr, ld, alpha=0.37))
        if K == 3:
            first = dy.get()
        dy.free()
    out["host3"], host = rec.run(s, lambda: s.values_product(dval_loc, np.ascontiguousarray(X[:3, f:f + m]), alpha=0.37))
    out["host3"]["equal"] = bits(host, first[:, :m])
    c, info = rec.run(s, lambda: code_of(lambda: s.values_product_device(dv.ptr, dx9.ptr, 9 if bad else 3, ld, ys.ptr, ld, alpha=0.37)))
    c.update(info, bad=bad, bad_rank=world - 1, y_untouched=bool(np.all(ys.get() == 2.5)))
    dy = Device(np.full((3, ld), np.nan))
    s.values_product_device(dv.ptr, dx9.ptr, 3, ld, dy.ptr, ld, alpha=0.37)
    c["next_equal"] = bits(dy.get()[:, :m], first[:, :m])
    out["refuse"] = c
    db = Device(rows(dB[:3]))
    for K in (1, 3):
        got, _ = rec.run(s, lambda: s.solve_tangent_device(dv.ptr, dx9.ptr, ld, db.ptr, dy.ptr, K, ld, raise_on_fail=False))
        out[f"tangent{K}"] = dict(trace=got["trace"][:4], calls=got["counters"]["calls"])
    c, info = rec.run(s, lambda: code_of(lambda: s.solve_tangent_device(dv.ptr, dx9.ptr, ld, db.ptr, ys.ptr, 9 if bad else 3, ld)))
    c.update(info, bad=bad, bad_rank=world - 1, y_untouched=bool(np.all(ys.get() == 2.5)))
    out["tangent_refuse"] = c
    res["trace"] = out
    for d in (dx9, ys, dy, db):
        d.free()

    # ---- bits: every rank's slice of y against the restatement on its local CSR, one alltoallv per product
    res["bits"] = {}
    for K in (1, 3, 4):
        T = np.stack([restate_rows(rowptr_loc, colind_glob, dval_loc, X[c]) for c in range(K)])
        dx, dy = Device(rows(X[:K])), Device(rows(Y0[:K], SENTINEL))
        c0, n0 = s.get_int("dist_alltoallv_calls"), s.get_int("values_product_calls")
        s.values_product_device(dv.ptr, dx.ptr, K, ld, dy.ptr, ld, alpha=0.37, accumulate=True)
        got = dy.get()
        out = dict(equal=bits(got[:, :m], Y0[:K, f:f + m] + 0.37 * T), tail=bool(np.all(got[:, m:] == SENTINEL)),
                   alltoallv=s.get_int("dist_alltoallv_calls") - c0, calls=s.get_int("values_product_calls") - n0)
        c0 = s.get_int("dist_alltoallv_calls")
        host = s.values_product(dval_loc, np.ascontiguousarray(X[:K, f:f + m]), alpha=-1.0)
        out.update(host_equal=bits(host, -1.0 * T), host_alltoallv=s.get_int("dist_alltoallv_calls") - c0)
        res["bits"][str(K)] = out
        dx.free()
        dy.free()

    # ---- the tangent solve against the composition it is documented to be, on every rank
    res["tangent"] = {}
    for K in (1, 3, 4):
        dx, db, dr = Device(rows(X[:K])), Device(rows(dB[:K], SENTINEL)), Device(rows(dB[:K], SENTINEL))
        dm, dt = Device(np.full((K, ld), SENTINEL)), Device(np.full((K, ld), SENTINEL))
        s.values_product_device(dv.ptr, dx.ptr, K, ld, dr.ptr, ld, alpha=-1.0, accumulate=True)
        info_m = s.solve_batch_device(dr.ptr, dm.ptr, K, ld, raise_on_fail=False)
        c0, t0 = s.get_int("values_product_calls"), s.get_int("tangent_calls")
        info_t = s.solve_tangent_device(dv.ptr, dx.ptr, ld, db.ptr, dt.ptr, K, ld, raise_on_fail=False)
        out = dict(equal=bits(dt.get(), dm.get()), infos_equal=info_t == info_m, status=[i["status"] for i in info_t],
                   product_calls=s.get_int("values_product_calls") - c0, tangent_calls=s.get_int("tangent_calls") - t0)
        a0 = s.get_int("dist_alltoallv_calls")
        s.solve_batch_device(db.ptr, dm.ptr, K, ld, raise_on_fail=False)
        a1 = s.get_int("dist_alltoallv_calls")
        s.solve_tangent_device(None, None, 0, db.ptr, dt.ptr, K, ld, raise_on_fail=False)
        out.update(no_dval_equal=bits(dt.get(), dm.get()), no_dval_same_exchanges=s.get_int("dist_alltoallv_calls") - a1 == a1 - a0)
        res["tangent"][str(K)] = out
        for d in (dx, db, dr, dm, dt):
            d.free()

    # ---- the last rank passes nine vectors: every rank returns, and the following collective solve has the bits of the one before
    bad = rank == world - 1
    db, d1, d2 = Device(rows(dB[:2])), Device(np.zeros((2, ld))), Device(np.zeros((2, ld)))
    s.solve_batch_device(db.ptr, d1.ptr, 2, ld, raise_on_fail=False)
    dx, dy = Device(rows(X)), Device(np.zeros((9, ld)))
    c0 = s.get_int("values_product_calls")
    out = code_of(lambda: s.values_product_device(dv.ptr, dx.ptr, 9 if bad else 4, ld, dy.ptr, ld))
    out.update(bad=bad, bad_rank=world - 1, calls_unchanged=s.get_int("values_product_calls") == c0)
    s.solve_batch_device(db.ptr, d2.ptr, 2, ld, raise_on_fail=False)
    out["next_solve_equal"] = bits(d1.get(), d2.get())
    res["refuse"] = out

    # ---- the last rank passes no d_dval to the tangent solve, the others do: every rank returns NKP_EINVAL, nobody waits
    out = code_of(lambda: s.solve_tangent_device(None if bad else dv.ptr, dx.ptr, ld, db.ptr, d2.ptr, 2, ld))
    out.update(bad_rank=world - 1)
    s.solve_batch_device(db.ptr, d2.ptr, 2, ld, raise_on_fail=False)
    out["next_solve_equal"] = bits(d1.get(), d2.get())
    res["mismatch"] = out
    for d in (db, d1, d2, dx, dy, dv):
        d.free()
    s.close()
    res["comm_errors"] = comm.errors
    with open(f"{a.out}.{rank}", "w") as fh:
        json.dump(res, fh)
    lib.nkp_comm_file_free(C.byref(ops))


if __name__ == "__main__":
    main()
