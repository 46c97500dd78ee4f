"""nkp_values_product_trans / nkp_values_product_trans_device on single-GPU solvers.

Column c of y has the bits of alpha * nkp_spmv_device of a throwaway PRECOND_NONE solver that STORES the host transpose of (A's
pattern, the caller's values) -- scipy's stable csr_matrix (...).T.tocsr (), checked here against a sort by (column, row, stored
position).  The parent's SpMV is the oracle, numpy adds one product and at most one sum.  Shapes: A = the transpose of the ragged row
blocks of tests/spmv_shapes.py (so A^T has rows and blocks at the 2048-entry and 256-row caps, a row over 2048 entries, empty rows and
a block of them), the ragged shapes themselves (empty columns), a one-row matrix, and the split_apart variant of
tests/noncanonical_cases.py (unsorted rows and a repeated column; the stored zeros are among the caller's values); for every nrhs,
with and without accumulation, three alphas, ldx, ldy > n with a NaN tail in x and a sentinel tail in y.  Then the host flavour, unit
vectors, the index and its accounting, the states a solver can be in, the refusals and the timing entry points."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import noncanonical_cases as nc
import spmv_shapes as sh
from nk_ocn_tracer_jacobian_precond_amd import solver
from test_gpu_values_product import SENTINEL, Device, assert_bits, expected, padded, spmv_oracle

pytestmark = pytest.mark.gpu

F64P = C.POINTER(C.c_double)
ALPHAS = (1.0, -1.0, 0.375)


# ---------------------------------------------------------------- helpers
def host_transpose(rowptr, colind):
    """(rowptrT, colindT, src): the pattern of A^T from scipy's stable transpose, entry p of it being entry src[p] of A -- ascending
    (row of A, stored position) inside every row of A^T"""
    n, nnz = rowptr.size - 1, colind.size
    tag = np.arange(1, nnz + 1, dtype=np.float64)
    T = sp.csr_matrix((tag, colind, rowptr), shape=(n, n)).T.tocsr()
    src = T.data.astype(np.int64) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    order = np.lexsort((np.arange(nnz), row, colind.astype(np.int64)))
    assert np.array_equal(src, order) and np.array_equal(T.indices, row[order])
    assert np.array_equal(T.indptr, np.concatenate([[0], np.cumsum(np.bincount(colind, minlength=n))]))
    return T.indptr.astype(np.int32), T.indices.astype(np.int32), src


class Case:
    """a pattern, caller's values with zeros, x with -0.0, y0, and the oracle's t for all eight vectors (computed once)"""

    def __init__(self, name, rowptr, colind, val, make_solver=True):
        self.name, self.rowptr, self.colind, self.val = name, np.asarray(rowptr, np.int32), np.asarray(colind, np.int32), np.asarray(val, np.float64)
        self.n, self.nnz = self.rowptr.size - 1, self.colind.size
        rng = np.random.default_rng(171)
        self.dval = rng.standard_normal(self.nnz)
        self.dval[::53] = 0.0
        self.X = rng.standard_normal((8, self.n))
        self.X[:, 5::89] = -0.0
        self.Y0 = rng.standard_normal((8, self.n))
        self.rowptrT, self.colindT, self.src = host_transpose(self.rowptr, self.colind)
        self.T = spmv_oracle(self.rowptrT, self.colindT, self.dval[self.src], self.X)
        self.h = solver.NkpSolver(self.rowptr, self.colind, self.val, None, precond=solver.PRECOND_NONE, restart=4) if make_solver else None

    def index_bytes(self):
        """4 (n + 1) + 4 nnz + 4 nnz + the row blocks of rowptrT (an array of no element holds one)"""
        return 4 * (self.n + 1) + 8 * max(self.nnz, 1) + 4 * sh.row_blocks(self.rowptrT).size


def _shape_case(name):
    if name == "one_row":
        return Case(name, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.0]))
    if name == "split_apart":
        v = nc.variant(name)
        assert np.any(np.diff(v.colind[v.rowptr[40]:v.rowptr[41]]) < 0)                       # unsorted rows
        assert any(np.unique(v.colind[v.rowptr[r]:v.rowptr[r + 1]]).size < v.len[r] for r in range(v.n))      # a repeated column
        return Case(name, v.rowptr, v.colind, v.val)
    s = getattr(sh, name.replace("T_", ""))()
    if name.startswith("T_"):
        rpT, ciT, src = host_transpose(s.rowptr, s.colind)
        c = Case(name, rpT, ciT, s.val[src])
        assert np.array_equal(c.rowptrT, s.rowptr)                  # A^T is the ragged shape: its rows and blocks sit at the caps
        assert np.diff(c.rowptrT.astype(np.int64)).max() > sh.LDS_NNZ
        assert np.any(np.diff(c.rowptrT) == 0) or name == "T_ragged_dd"      # empty rows of A^T (ragged_dd: the diagonal alone)
        return c
    c = Case(name, s.rowptr, s.colind, s.val)
    assert np.any(np.diff(c.rowptrT) == 0) or name == "ragged_dd"   # empty columns of A (ragged_dd: every column has its diagonal)
    return c


@pytest.fixture(scope="module", params=["T_ragged_empty", "T_ragged_dd", "ragged_empty", "ragged_dd", "one_row", "split_apart"])
def case(request):
    c = _shape_case(request.param)
    yield c
    c.h.close()


def product_trans(h, c, nrhs, alpha, accumulate, pad=5, extra_cols=0):
    """the device flavour with ldx, ldy > n, a NaN tail in x and a sentinel tail in y; returns the whole y buffer"""
    ldx, ldy = c.n + pad, c.n + pad + 2
    y0 = np.full((nrhs + extra_cols, ldy), SENTINEL)
    y0[:nrhs, :c.n] = c.Y0[:nrhs] if accumulate else np.nan         # without accumulation y may hold anything, NaN included
    with Device(c.dval) as dv, Device(padded(c.X[:nrhs], ldx)) as dx, Device(y0) as dy:
        h.values_product_trans_device(dv.ptr, dx.ptr, nrhs, ldx, dy.ptr, ldy, alpha=alpha, accumulate=accumulate)
        return dy.get()


# ---------------------------------------------------------------- bits
@pytest.mark.parametrize("nrhs", [1, 2, 3, 4, 5, 6, 7, 8])
def test_bits_of_alpha_times_the_spmv_of_a_solver_that_stores_the_host_transpose(case, nrhs):
    c = case
    for alpha in ALPHAS:
        for accumulate in (False, True):
            got = product_trans(c.h, c, nrhs, alpha, accumulate, extra_cols=1)
            assert_bits(got[:nrhs, :c.n], expected(c.T[:nrhs], alpha, c.Y0[:nrhs] if accumulate else None))
            assert np.all(got[:, c.n:] == SENTINEL) and np.all(got[nrhs:] == SENTINEL)      # no NaN of x's tail, the sentinel stays


def test_host_flavour_has_the_bits_of_the_device_flavour(case):
    c = case
    for K in (1, 3):
        X = c.X[:K] if K > 1 else c.X[0]
        dev = product_trans(c.h, c, K, 0.375, False)[:, :c.n]
        assert_bits(np.atleast_2d(c.h.values_product_trans(c.dval, X, alpha=0.375)), dev)
        Y0 = c.Y0[:K] if K > 1 else c.Y0[0]
        keep = Y0.copy()
        dev = product_trans(c.h, c, K, -1.0, True)[:, :c.n]
        assert_bits(np.atleast_2d(c.h.values_product_trans(c.dval, X, alpha=-1.0, Y=Y0)), dev)
        assert_bits(Y0, keep)                                       # the caller's Y is not modified
    ld = c.n + 4
    y = np.full((2, ld), SENTINEL)
    x = padded(c.X[:2], ld)
    assert c.h._lib.nkp_values_product_trans(c.h._h, 2, c.dval.ctypes.data_as(F64P), x.ctypes.data_as(F64P), ld, 1.0, 0, y.ctypes.data_as(F64P), ld) == 0, solver.last_error()
    assert_bits(y[:, :c.n], expected(c.T[:2], 1.0))
    assert np.all(y[:, c.n:] == SENTINEL)


def test_unit_vector_gives_a_row_of_the_values(case):
    """x = e_i, K = 1: y[j] is the sum of the values stored at (i, j), repeated entries in stored order -- every other product is a
    zero, and a zero added changes no sum"""
    c = case
    ln = np.diff(c.rowptr.astype(np.int64))
    rows = {0, c.n - 1, int(np.argmax(ln)), int(np.argmin(ln)), c.n // 2}
    if c.name == "split_apart":
        rows.add(next(r for r in range(c.n) if np.unique(c.colind[c.rowptr[r]:c.rowptr[r + 1]]).size < ln[r]))
    val = c.dval.copy()
    val[val == 0.0] = 0.5                                           # a row of V as stored, without the signs of zero
    for i in sorted(rows):
        x = np.zeros((1, c.n))
        x[0, i] = 1.0
        want = np.zeros(c.n)
        a, z = int(c.rowptr[i]), int(c.rowptr[i + 1])
        np.add.at(want, c.colind[a:z].astype(np.int64), val[a:z])
        with Device(val) as dv, Device(x) as dx, Device(np.full((1, c.n), np.nan)) as dy:
            c.h.values_product_trans_device(dv.ptr, dx.ptr, 1, c.n, dy.ptr, c.n)
            assert_bits(dy.get()[0], want)


# ---------------------------------------------------------------- the index and its accounting
def test_index_is_built_once_and_counted():
    s = sh.ragged_empty()
    c = Case("ragged_empty", s.rowptr, s.colind, s.val)
    h, n, nnz = c.h, c.n, c.nnz
    try:
        assert h.get_int("trans_index_bytes") == 0 and h.get_int("trans_index_us") == 0
        assert h.get_int("values_product_trans_calls") == 0 and h.get_int("values_product_trans_us") == 0
        b0 = h.get_int("device_bytes")
        product_trans(h, c, 1, 1.0, False)
        idx = h.get_int("trans_index_bytes")
        assert idx == c.index_bytes() > 0 and h.get_int("trans_index_us") > 0
        assert h.get_int("device_bytes") - b0 == idx                # K = 1 on device buffers: the index and no work space
        us = h.get_int("trans_index_us")
        product_trans(h, c, 3, 1.0, True)
        assert h.get_int("trans_index_bytes") == idx and h.get_int("trans_index_us") == us
        b1 = h.get_int("device_bytes")
        assert b1 - b0 == idx + 8 * 4 * n, (b0, b1)                 # the K = 4 interleaved copy of x
        h.values_product_trans(c.dval, c.X[:3])
        b2 = h.get_int("device_bytes")
        assert b2 - b1 == 8 * (nnz + 2 * 3 * n), (b1, b2)           # the staging of the host flavour: val, x and y
        h.values_product(c.dval, c.X[:3])                           # nkp_values_product shares the work space
        product_trans(h, c, 4, 1.0, False)
        assert h.get_int("device_bytes") == b2 and h.get_int("trans_index_bytes") == idx
        assert h.get_int("values_product_trans_calls") == 4 and h.get_int("values_product_trans_us") > 0
        assert h.get_int("values_product_calls") == 1 and h.get_int("trans_device_bytes") == 0
        with Device(c.dval) as dv, Device(c.X[:2]) as dx:
            with pytest.raises(solver.NkpError):
                h.values_product_trans_device(dv.ptr, dx.ptr, 2, n, dx.ptr, n)
        assert h.get_int("values_product_trans_calls") == 4         # successful calls only
    finally:
        h.close()


# ---------------------------------------------------------------- a multilevel solver: the hierarchy and spmv_diag play no part
def test_multilevel_solver_with_default_tuning(golden_by_name):
    g = golden_by_name("tri_12x10x6")
    ci, cj = solver.column_coords(g.ind_i, g.ind_j, g.col_start, g.cnt)
    c = Case(g.name, g.rowptr, g.colind, g.val, make_solver=False)
    with solver.NkpSolver(g.rowptr, g.colind, g.val, g.blk_start, g.cnt, col_i=ci, col_j=cj, rtol=1e-10, restart=150, max_iters=5000) as h:
        assert h.get_int("levels") >= 1
        for nrhs in (1, 2, 5, 8):
            got = product_trans(h, c, nrhs, 0.375, True)
            assert_bits(got[:, :c.n], expected(c.T[:nrhs], 0.375, c.Y0[:nrhs]))
        idx = h.get_int("trans_index_bytes")
        assert idx == c.index_bytes()
        want = expected(c.T[:3], -1.0, c.Y0[:3])
        assert_bits(product_trans(h, c, 3, -1.0, True)[:, :c.n], want)
        h.refactor(g.val * 0.75)                                    # flags 0, then NKP_REFACTOR_REBUILD: the pattern stays either way
        assert h.get_int("refactor_count") == 1
        assert_bits(product_trans(h, c, 3, -1.0, True)[:, :c.n], want)
        h.refactor(g.val, rebuild=True)
        assert h.get_int("refactor_count") == 2 and h.get_int("refactor_rebuilt") == 1 and h.get_int("trans_index_bytes") == idx
        assert_bits(product_trans(h, c, 3, -1.0, True)[:, :c.n], want)


# ---------------------------------------------------------------- states and refusals on a solver that solves
class Synth:
    def __init__(self):
        from test_gpu_transpose import _gen
        p = _gen()
        self.p = p
        self.blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
        self.case = Case("synth", p.rowptr, p.colind, p.nzval, make_solver=False)
        self.b = np.random.default_rng(5).standard_normal(p.flat_len)

    def make(self, **kw):
        p = self.p
        return solver.NkpSolver(p.rowptr, p.colind, p.nzval, self.blk, 1, precond=solver.PRECOND_COLUMN_JACOBI, rtol=1e-8, restart=60, max_iters=2000, **kw)


@pytest.fixture(scope="module")
def synth():
    return Synth()


def test_bits_are_the_same_in_every_state_of_the_solver(synth):
    c, p = synth.case, synth.p
    want = expected(c.T[:3], 0.375, c.Y0[:3])
    s = synth.make()
    try:
        assert_bits(product_trans(s, c, 3, 0.375, True)[:, :c.n], want)
        idx = s.get_int("trans_index_bytes")
        s.refactor(p.nzval * 0.75)
        assert s.get_int("refactor_count") == 1
        assert_bits(product_trans(s, c, 3, 0.375, True)[:, :c.n], want)
        s.refactor(p.nzval * 1.25, rebuild=True)
        assert s.get_int("refactor_count") == 2
        assert_bits(product_trans(s, c, 3, 0.375, True)[:, :c.n], want)
        t = s.transposed()                                          # a transposed handle alive: its own map, not the index
        assert s.get_int("trans_device_bytes") > 0 and s.get_int("trans_index_bytes") == idx
        assert_bits(product_trans(s, c, 3, 0.375, True)[:, :c.n], want)
        t.close()                                                   # ... and destroyed
        assert s.get_int("trans_device_bytes") == 0 and s.get_int("trans_index_bytes") == idx
        assert_bits(product_trans(s, c, 3, 0.375, True)[:, :c.n], want)

        # a refactor that fails after its commit point (test_gpu_refactor.py: a singular 2 x 2 corner of a water column)
        def at(r, j):
            q = np.nonzero(p.colind[p.rowptr[r]:p.rowptr[r + 1]] == j)[0]
            return p.rowptr[r] + q[0] if q.size else None

        blk = synth.blk
        r0 = next(int(blk[k]) for k in range(len(blk) - 1) if blk[k + 1] - blk[k] >= 2 and at(blk[k], blk[k] + 1) is not None)
        bad = p.nzval.copy()
        bad[[at(r0, r0), at(r0, r0 + 1), at(r0 + 1, r0), at(r0 + 1, r0 + 1)]] = (2.0, 2.0, 1.0, 1.0)
        with pytest.raises(solver.NkpError) as e:
            s.refactor(bad)
        assert e.value.code == -4
        with pytest.raises(solver.NkpError):
            s.solve(synth.b)
        assert_bits(product_trans(s, c, 3, 0.375, True)[:, :c.n], want)
        assert s.get_int("trans_index_bytes") == idx and s.get_int("values_product_trans_calls") == 6
    finally:
        s.close()


def test_refusals_leave_the_solver_as_it_was(synth):
    c, n = synth.case, synth.case.n
    s = synth.make()
    k = s.clone()
    t = s.transposed()
    try:
        x0, _ = s.solve(synth.b)
        product_trans(s, c, 4, 1.0, False)                          # index and work space of a valid call exist: no bad call may change them
        state = lambda: tuple(s.get_int(key) for key in ("device_bytes", "trans_index_bytes", "values_product_trans_calls", "values_product_calls"))
        before = state()
        with Device(c.dval) as dv, Device(np.vstack([c.X, c.X[:1]])) as dx, Device(np.full((9, n), 2.5)) as dy:
            for h, nrhs, ldx, ldy, y, what in ((s, 0, n, n, dy.ptr, "nrhs"), (s, 9, n, n, dy.ptr, "nrhs"), (s, 2, n - 1, n, dy.ptr, "ldx"), (s, 2, n, n - 1, dy.ptr, "ldy"),
                                               (s, 2, n, n, dx.ptr, "same buffer"), (k, 2, n, n, dy.ptr, "a clone shares its matrix; call it on the solver it was cloned from"),
                                               (t, 2, n, n, dy.ptr, "transposed handle; call it on the solver it was transposed from")):
                with pytest.raises(solver.NkpError) as e:
                    h.values_product_trans_device(dv.ptr, dx.ptr, nrhs, ldx, y, ldy)
                assert e.value.code == -1 and what in str(e.value) and "nkp_values_product_trans_device" in str(e.value), (nrhs, ldx, ldy, str(e.value))
            assert np.all(dy.get() == 2.5)
        for h in (k, t):
            with pytest.raises(solver.NkpError) as e:
                h.values_product_trans(c.dval, c.X[:2])
            assert e.value.code == -1
            assert h.get_int("trans_index_bytes") == 0 and h.get_int("values_product_trans_calls") == 0
        assert state() == before
        for h in (s, k):
            x1, _ = h.solve(synth.b)
            assert_bits(x1, x0)
    finally:
        k.close()
        s.close()


def test_row_distributed_solver_is_refused_without_a_collective(synth, tmp_path):
    """force_dist = 1 with the file transport, one rank: nkp_values_product_trans* and nkp_time_kernel 9 / 10 are NKP_EINVAL, and no
    collective callback is reached (the counters of the device collectives and the files of the transport stay as they were)"""
    import os
    p, c, n = synth.p, synth.case, synth.case.n
    lib = solver.load_library()
    lib.nkp_comm_file_init.argtypes = [C.POINTER(solver.NkpCommOps), C.c_char_p, C.c_int, C.c_int]
    lib.nkp_comm_file_free.argtypes = [C.POINTER(solver.NkpCommOps)]
    lib.nkp_comm_file_free.restype = None
    ops = solver.NkpCommOps()
    assert lib.nkp_comm_file_init(C.byref(ops), str(tmp_path).encode(), 0, 1) == 0
    opt = solver.default_options(precond=solver.PRECOND_COLUMN_JACOBI, rtol=1e-8, restart=60, max_iters=2000)
    tun = solver.default_tuning(force_dist=1)
    opt.tuning = C.pointer(tun)
    rp, ci, v = np.ascontiguousarray(p.rowptr, np.int32), np.ascontiguousarray(p.colind, np.int32), np.ascontiguousarray(p.nzval, np.float64)
    blk = np.ascontiguousarray(synth.blk, np.int32)
    h = C.c_void_p()
    rc = lib.nkp_create_dist(C.byref(h), C.byref(opt), n, 0, n, ci.size, solver._p(rp, C.c_int32), solver._p(ci, C.c_int32), solver._p(v, C.c_double),
                             solver._p(blk, C.c_int32), blk.size - 1, 1, C.byref(ops))
    assert rc == 0, lib.nkp_last_error().decode()
    s = solver.NkpSolver._from_handle(lib, h, n, ci.size, opt)
    try:
        x0, _ = s.solve(synth.b)
        files = sorted(os.listdir(tmp_path))
        calls = (s.get_int("dist_alltoallv_calls"), s.get_int("dist_allreduce_calls"), s.get_int("device_bytes"))
        with Device(c.dval) as dv, Device(c.X[:2]) as dx, Device(np.full((2, n), 2.5)) as dy:
            with pytest.raises(solver.NkpError) as e:
                s.values_product_trans_device(dv.ptr, dx.ptr, 2, n, dy.ptr, n)
            assert e.value.code == -1 and "row-distributed" in str(e.value)
            assert np.all(dy.get() == 2.5)
        with pytest.raises(solver.NkpError) as e:
            s.values_product_trans(c.dval, c.X[:2])
        assert e.value.code == -1 and "row-distributed" in str(e.value)
        for which in (9, 10):
            with pytest.raises(solver.NkpError) as e:
                s.time_kernel(which, reps=1, arg=2)
            assert e.value.code == -1 and "single-GPU" in str(e.value)
        assert (s.get_int("dist_alltoallv_calls"), s.get_int("dist_allreduce_calls"), s.get_int("device_bytes")) == calls
        assert sorted(os.listdir(tmp_path)) == files and s.get_int("trans_index_bytes") == 0
        x1, _ = s.solve(synth.b)
        assert_bits(x1, x0)
    finally:
        s.close()
        lib.nkp_comm_file_free(C.byref(ops))


# ---------------------------------------------------------------- timing entry points
def test_time_kernel_9_and_10(case):
    h = case.h
    for K in (1, 2, 4, 8):
        assert h.time_kernel(9, reps=2, arg=K) > 0.0
        assert h.time_kernel(10, reps=2, arg=K) > 0.0               # the composition it is compared against
    for which in (9, 10):
        with pytest.raises(solver.NkpError) as e:
            h.time_kernel(which, reps=2, arg=3)
        assert e.value.code == -1 and f"which = {which}" in str(e.value)
    assert_bits(product_trans(h, case, 3, 0.375, True)[:, :case.n], expected(case.T[:3], 0.375, case.Y0[:3]))      # the scratch was the timer's own
