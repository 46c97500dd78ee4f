"""Worker for tests/test_gpu_value_gradient_dist.py (launched once per rank; the library's file transport, all ranks share the
one GPU; no torch in the process).

Every rank builds a distributed solver on its latitude band of the synthetic 40x46x20 matrix and calls nkp_value_gradient /
nkp_value_gradient_device with its slices of seeded global vectors; the reference is the numpy restatement of the formula on
the GLOBAL matrix, cut to the rank's entries.  One JSON file per rank."""
import argparse
import ctypes as C
import json
import os
import sys
import types

import numpy as np
import scipy.sparse as sp

from comm_trace import Recorder, traced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GRID = (40, 46, 20)


def restate(rowptr, colind, lam, x, alpha, g0=None):
    rowptr = np.asarray(rowptr, np.int64)
    row_of = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    col = np.asarray(colind, np.int64)
    s = lam[0][row_of] * x[0][col]
    for c in range(1, lam.shape[0]):
        s = s + lam[c][row_of] * x[c][col]
    v = alpha * s
    return v if g0 is None else g0 + v


def bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return bool(a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)))


class Device:
    def __init__(self, a):
        self.hip = C.CDLL("libamdhip64.so")
        a = np.ascontiguousarray(a, np.float64)
        self.size, self.p = a.size, C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(max(a.nbytes, 8))) == 0
        assert self.hip.hipMemcpy(self.p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
        self.ptr = self.p.value

    def get(self):
        out = np.empty(self.size)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self):
        self.hip.hipFree(self.p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--file-dir", required=True)
    ap.add_argument("--precond", default="none")
    ap.add_argument("--cases", default="bits,transposed,refuse,trace")
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
    comm = types.SimpleNamespace(ops=ops, errors=[])

    p = synth.generate(imt=GRID[0], jmt=GRID[1], km=GRID[2], adv="upwind3", hmix="isop", seed=2, u_scale=3.0, ah=4.0e6, isop_k33=True)
    n = p.flat_len
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    starts = nd.snap_partition(blk, world)
    loc = nd.local_slice(p.rowptr, p.colind, p.nzval, blk, starts, rank, ci, cj)
    f, m = int(loc["fst_row"]), int(loc["m_loc"])
    e0, e1 = int(p.rowptr[f]), int(p.rowptr[f + m])
    rng = np.random.default_rng(61)
    lam, x = rng.standard_normal((9, n)), rng.standard_normal((9, n))
    lam[:, ::97] = 0.0
    x[:, 5::89] = -0.0
    lam_loc, x_loc = np.ascontiguousarray(lam[:, f:f + m]), np.ascontiguousarray(x[:, f:f + m])
    opts = dict(rtol=1e-10, restart=60, max_iters=3000)
    if a.precond == "none":
        opts["precond"] = solver.PRECOND_NONE
    elif a.precond == "column":
        opts["precond"] = solver.PRECOND_COLUMN_JACOBI
    res = dict(rank=rank, m_loc=m, nnz_loc=e1 - e0)
    cases = a.cases.split(",")

    def code_of(fn):
        try:
            fn()
            return dict(code=0, message="")
        except solver.NkpError as exc:
            return dict(code=exc.code, message=str(exc))

    def check(h, rowptr, colind, lo, hi):
        """host flavour at K = 1 and 4, device flavour at K = 4 with ld = m + 3 and accumulation; one alltoallv per call"""
        out = dict(halo_rows=h.get_int("dist_halo_rows"))
        for K in (1, 4):
            want = restate(rowptr, colind, lam[:K], x[:K], -1.0)[lo:hi]
            c0 = h.get_int("dist_alltoallv_calls")
            got = h.value_gradient(lam_loc[:K], x_loc[:K])
            out[f"host{K}"] = dict(equal=bits(got, want), alltoallv=h.get_int("dist_alltoallv_calls") - c0, size=int(got.size))
        ld = m + 3
        L, X = np.full((4, ld), np.nan), np.full((4, ld), np.nan)
        L[:, :m], X[:, :m] = lam_loc[4:8], x_loc[4:8]
        g0 = restate(rowptr, colind, lam[:4], x[:4], -1.0)[lo:hi]
        want = restate(rowptr, colind, lam[4:8], x[4:8], 0.37)[lo:hi]
        dl, dx, dg = Device(L), Device(X), Device(g0)
        c0 = h.get_int("dist_alltoallv_calls")
        h.value_gradient_device(dl.ptr, dx.ptr, 4, ld, dg.ptr, alpha=0.37, accumulate=True)
        out["device4"] = dict(equal=bits(dg.get(), g0 + want), alltoallv=h.get_int("dist_alltoallv_calls") - c0)
        for d in (dl, dx, dg):
            d.free()
        out["calls"] = h.get_int("value_gradient_calls")
        return out

    s = nd.NkpDistSolver(loc, n, comm, **opts)
    if "bits" in cases:
        res["bits"] = check(s, p.rowptr, p.colind, e0, e1)
    if "transposed" in cases:
        T = sp.csr_matrix((p.nzval, p.colind, p.rowptr), shape=(n, n)).T.tocsr()
        T.sort_indices()
        t = s.transposed_dist()
        res["transposed"] = check(t, T.indptr, T.indices, int(T.indptr[f]), int(T.indptr[f + m]))
        res["transposed"]["nnz_equal"] = t.nnz == int(T.indptr[f + m] - T.indptr[f])
    if "refuse" in cases:
        # the last rank passes nine pairs: every rank returns non-zero, and the next valid call succeeds everywhere
        bad = rank == world - 1
        K = 9 if bad else 4
        c0 = s.get_int("value_gradient_calls")
        out = code_of(lambda: s.value_gradient(lam_loc[:K], x_loc[:K]))
        out.update(bad=bad, bad_rank=world - 1, calls_unchanged=s.get_int("value_gradient_calls") == c0)
        got = s.value_gradient(lam_loc[:4], x_loc[:4])
        out["next_equal"] = bits(got, restate(p.rowptr, p.colind, lam[:4], x[:4], -1.0)[e0:e1])
        res["refuse"] = out
    s.close()
    if "trace" in cases:
        # the order of the transport's callbacks and the counters, on a solver of its own whose first K = 4 call is the one recorded
        log = []
        wrapped, orig = traced(solver, ops, log)
        tcomm = types.SimpleNamespace(ops=wrapped, errors=comm.errors, keep=orig)
        rec = Recorder(log, "value_gradient_calls")
        ld, e = m + 3, e1 - e0
        bad = rank == world - 1

        def padded(v):
            out = np.full((v.shape[0], ld), np.nan)
            out[:, :m] = v
            return out

        with nd.NkpDistSolver(loc, n, tcomm, **opts) as h:
            out = {}
            dl, dx = Device(padded(lam_loc)), Device(padded(x_loc))
            for K in (1, 3):
                dg = Device(np.full(e, np.nan))
                out[f"device{K}"], _ = rec.run(h, lambda: h.value_gradient_device(dl.ptr, dx.ptr, K, ld, dg.ptr))
                out[f"device{K}"]["equal"] = bits(dg.get(), restate(p.rowptr, p.colind, lam[:K], x[:K], -1.0)[e0:e1])
                if K == 3:
                    first = dg.get()
                dg.free()
            out["host3"], got = rec.run(h, lambda: h.value_gradient(lam_loc[:3], x_loc[:3]))
            out["host3"]["equal"] = bits(got, first)
            dg = Device(np.full(e, 2.5))
            c, info = rec.run(h, lambda: code_of(lambda: h.value_gradient_device(dl.ptr, dx.ptr, 9 if bad else 3, ld, dg.ptr)))
            c.update(info, bad=bad, bad_rank=world - 1, g_untouched=bool(np.all(dg.get() == 2.5)))
            h.value_gradient_device(dl.ptr, dx.ptr, 3, ld, dg.ptr)
            c["next_equal"] = bits(dg.get(), first)
            out["refuse"] = c
            for d in (dl, dx, dg):
                d.free()
        res["trace"] = out
    res["comm_errors"] = comm.errors
    with open(f"{a.out}.{rank}", "w") as fh:
        json.dump(res, fh)
    lib.nkp_comm_file_free(C.byref(comm.ops))


if __name__ == "__main__":
    main()
