"""nkp_values_product / nkp_solve_tangent_device on single-GPU solvers.

Product: on the ragged row blocks of tests/spmv_shapes.py (rows and blocks at the 2048-entry and 256-row caps, long rows, empty
rows, a block of empty rows) and on a one-row matrix, column c of y has the bits of alpha * nkp_spmv_device of a throwaway solver
that STORES the caller's values -- the parent's SpMV is the oracle, the numpy part is one product and at most one sum -- for every
nrhs, with and without accumulation, under the SpMV's tuning knobs, on clones, transposed handles and across a refactor; it lies
within the derived rounding bound of the exact product, writes nowhere else, and is the adjoint of nkp_value_gradient.
Tangent solve: bit for bit the composition it is documented to be, and its result passes the solver's stopping test evaluated in
numpy."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp

import spmv_shapes as sh
from nk_ocn_tracer_jacobian_precond_amd import solver

pytestmark = pytest.mark.gpu

F64P = C.POINTER(C.c_double)
SENTINEL = -7.25e77


# ---------------------------------------------------------------- helpers
def assert_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape
    bad = np.flatnonzero(got.view(np.uint64).ravel() != want.view(np.uint64).ravel())
    assert bad.size == 0, (bad.size, bad[:8], got.ravel()[bad[:8]], want.ravel()[bad[:8]])


class Device:
    """a float64 array on the device through the HIP runtime the library links (no second runtime in this process)"""

    def __init__(self, a):
        self.hip = C.CDLL("libamdhip64.so")
        a = np.ascontiguousarray(a, np.float64)
        self.shape, self.size, self.p = a.shape, a.size, C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(max(a.nbytes, 8))) == 0
        if a.nbytes:
            assert self.hip.hipMemcpy(self.p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
        self.ptr = self.p.value

    def get(self):
        out = np.empty(self.size)
        if out.nbytes:
            assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(out.nbytes), 2) == 0
        return out.reshape(self.shape)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.hip.hipFree(self.p)


def padded(v, ld, fill=np.nan):
    """(K, n) -> (K, ld) with a poison tail no kernel may read into the result"""
    out = np.full((v.shape[0], ld), fill)
    out[:, :v.shape[1]] = v
    return out


def spmv_oracle(rowptr, colind, val, X):
    """nkp_spmv_device, column by column, of a throwaway PRECOND_NONE solver that stores val: the parent's kernel, not the code under test"""
    n = rowptr.size - 1
    out = np.empty_like(X)
    with solver.NkpSolver(rowptr, colind, val, None, precond=solver.PRECOND_NONE, restart=4) as o:
        for c in range(X.shape[0]):
            with Device(X[c]) as dx, Device(np.full(n, np.nan)) as dy:
                o.spmv_device(dx.ptr, dy.ptr)
                out[c] = dy.get()
    return out


def restate_rows(rowptr, colind, val, x):
    """+0.0, then every stored entry of the row in stored order, each product and each sum rounded: rows within the 2048-entry block"""
    rowptr = np.asarray(rowptr, np.int64)
    ln = np.diff(rowptr)
    assert ln.max(initial=0) <= sh.LDS_NNZ
    acc = np.zeros(ln.size)
    col = np.asarray(colind, np.int64)
    for k in range(int(ln.max(initial=0))):
        rows = np.flatnonzero(ln > k)
        e = rowptr[rows] + k
        acc[rows] = acc[rows] + val[e] * x[col[e]]
    return acc


def expected(T, alpha, y0=None):
    """one product, or a product and a sum"""
    v = alpha * T
    return v if y0 is None else y0 + v


class Case:
    def __init__(self, name, rowptr, colind, val):
        self.name, self.rowptr, self.colind, self.val = name, rowptr, colind, val
        self.n, self.nnz = rowptr.size - 1, colind.size
        rng = np.random.default_rng(71)
        self.dval = rng.standard_normal(self.nnz)
        self.dval[::53] = 0.0
        self.X = rng.standard_normal((8, self.n))
        self.X[:, 5::89] = -0.0
        self.Y0 = rng.standard_normal((8, self.n))
        self.T = spmv_oracle(rowptr, colind, self.dval, self.X)
        self.h = solver.NkpSolver(rowptr, colind, val, None, precond=solver.PRECOND_NONE, restart=4)


def _shape_case(name):
    if name == "one_row":
        return Case(name, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.0]))
    s = getattr(sh, name)()
    return Case(name, s.rowptr, s.colind, s.val)


@pytest.fixture(scope="module", params=["ragged_empty", "ragged_dd", "one_row"])
def case(request):
    c = _shape_case(request.param)
    yield c
    c.h.close()


def product_device(h, c, nrhs, alpha, accumulate, pad=5, extra_cols=0, dval=None):
    """the device flavour with ldx, ldy > n; returns the whole y buffer (nrhs + extra_cols, ldy)"""
    ldx, ldy = c.n + pad, c.n + pad + 2
    y0 = np.full((nrhs + extra_cols, ldy), SENTINEL)
    y0[:nrhs, :c.n] = c.Y0[:nrhs] if accumulate else np.nan         # without accumulation y may hold anything, NaN included
    with Device(c.dval if dval is None else dval) as dv, Device(padded(c.X[:nrhs], ldx)) as dx, Device(y0) as dy:
        h.values_product_device(dv.ptr, dx.ptr, nrhs, ldx, dy.ptr, ldy, alpha=alpha, accumulate=accumulate)
        return dy.get()


# ---------------------------------------------------------------- 1. bits, 3. untouched rows and columns
@pytest.mark.parametrize("nrhs", [1, 2, 3, 4, 5, 6, 7, 8])
def test_bits_of_alpha_times_the_spmv_of_a_solver_that_stores_the_values(case, nrhs):
    c = case
    for alpha in (-1.0, 0.37):
        got = product_device(c.h, c, nrhs, alpha, False)
        assert_bits(got[:, :c.n], expected(c.T[:nrhs], alpha))
        assert np.all(got[:, c.n:] == SENTINEL)
        got = product_device(c.h, c, nrhs, alpha, True)
        assert_bits(got[:, :c.n], expected(c.T[:nrhs], alpha, c.Y0[:nrhs]))
        assert np.all(got[:, c.n:] == SENTINEL)


@pytest.mark.parametrize("nrhs", [1, 3, 5, 8])
def test_rows_behind_n_and_columns_behind_nrhs_keep_their_sentinel(case, nrhs):
    c = case
    for accumulate in (False, True):
        got = product_device(c.h, c, nrhs, 0.37, accumulate, pad=9, extra_cols=2)
        assert np.all(got[:, c.n:] == SENTINEL) and np.all(got[nrhs:] == SENTINEL)
        assert_bits(got[:nrhs, :c.n], expected(c.T[:nrhs], 0.37, c.Y0[:nrhs] if accumulate else None))


def test_host_flavour_and_python_wrapper(case):
    c = case
    for K in (1, 3):
        X = c.X[:K] if K > 1 else c.X[0]
        assert_bits(c.h.values_product(c.dval, X), expected(c.T[:K] if K > 1 else c.T[0], 1.0))
        Y0 = c.Y0[:K] if K > 1 else c.Y0[0]
        keep = Y0.copy()
        assert_bits(c.h.values_product(c.dval, X, alpha=-1.0, Y=Y0), expected(c.T[:K] if K > 1 else c.T[0], -1.0, Y0))
        assert_bits(Y0, keep)                                       # the caller's Y is not modified
    ld = c.n + 4
    y = np.full((2, ld), np.nan)
    x = padded(c.X[:2], ld)
    assert c.h._lib.nkp_values_product(c.h._h, 2, c.dval.ctypes.data_as(F64P), x.ctypes.data_as(F64P), ld, 0.37, 0, y.ctypes.data_as(F64P), ld) == 0, solver.last_error()
    assert_bits(y[:, :c.n], expected(c.T[:2], 0.37))
    assert np.all(np.isnan(y[:, c.n:]))


# ---------------------------------------------------------------- 2. accuracy, independently of any kernel
def test_product_lies_within_the_rounding_bound_of_the_exact_product(case):
    c = case
    got = product_device(c.h, c, 3, 1.0, False)[:, :c.n]
    for k in range(3):
        ex = sh.Exact(c.rowptr, c.colind, c.dval, c.X[k])
        err = np.abs(got[k] - ex.y)
        worst = int(np.argmax(err - ex.e))
        print(f"{c.name} column {k}: largest error / bound = {np.max(err[ex.e > 0] / ex.e[ex.e > 0]) if np.any(ex.e > 0) else 0.0:.3f} (row {worst})")
        assert np.all(err <= ex.e), (k, worst, err[worst], ex.e[worst])


# ---------------------------------------------------------------- 4. knobs
@pytest.mark.parametrize("tuning", [dict(spmv_compress=1), dict(batch_spmv_rows=0)], ids=["spmv_compress", "batch_products_in_lds"])
def test_tuning_knobs_of_the_spmv_do_not_change_the_bits(case, tuning):
    c = case
    with solver.NkpSolver(c.rowptr, c.colind, c.val, None, precond=solver.PRECOND_NONE, restart=4, tuning=tuning) as h:
        for nrhs in (1, 2, 4, 7):
            assert_bits(product_device(h, c, nrhs, 0.37, True)[:, :c.n], expected(c.T[:nrhs], 0.37, c.Y0[:nrhs]))


# ---------------------------------------------------------------- 5. handles
def test_clone_gives_the_same_bits(case):
    c = case
    k = c.h.clone()
    try:
        for nrhs in (1, 3):
            assert_bits(product_device(k, c, nrhs, -1.0, True)[:, :c.n], expected(c.T[:nrhs], -1.0, c.Y0[:nrhs]))
        assert k.get_int("values_product_calls") == 2
    finally:
        k.close()


def test_result_does_not_change_across_a_refactor():
    s = sh.ragged_dd()
    c = Case("ragged_dd", s.rowptr, s.colind, s.val)
    c.h.close()
    with solver.NkpSolver(s.rowptr, s.colind, s.val, np.arange(s.n + 1), precond=solver.PRECOND_COLUMN_JACOBI, restart=30) as h:
        before = product_device(h, c, 3, 0.37, True)
        h.refactor(sh.refactored_values(s))
        assert h.get_int("refactor_count") == 1
        after = product_device(h, c, 3, 0.37, True)
    assert_bits(before, after)
    assert_bits(after[:, :c.n], expected(c.T[:3], 0.37, c.Y0[:3]))


def test_transposed_handle_multiplies_with_the_pattern_of_the_transpose(monkeypatch):
    from test_gpu_transpose import _gen, _transpose
    monkeypatch.setenv("NKP_ML_DEVICE_MIN", "0")
    monkeypatch.setenv("NKP_ML_COARSEST_ROWS", "300")
    p = _gen()
    n = p.flat_len
    T, src = _transpose(p.rowptr, p.colind, p.nzval)                # scipy's transpose, and where each of its entries comes from
    rng = np.random.default_rng(72)
    dval, X, Y0 = rng.standard_normal(p.colind.size), rng.standard_normal((3, n)), rng.standard_normal((3, n))
    dvalT = dval[src]
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    with solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, 1, col_i=ci, col_j=cj) as s:
        t = s.transposed()
        got = t.values_product(dvalT, X, alpha=0.37, Y=Y0)
        want = np.stack([restate_rows(T.indptr, T.indices, dvalT, X[k]) for k in range(3)])
        assert_bits(got, expected(want, 0.37, Y0))
        ref = sp.csr_matrix((dval, p.colind, p.rowptr), shape=(n, n)).T @ X.T
        assert np.allclose(want, ref.T, rtol=1e-12, atol=1e-12)
        own = s.values_product(dval, X)
        assert_bits(own, np.stack([restate_rows(p.rowptr, p.colind, dval, X[k]) for k in range(3)]))


# ---------------------------------------------------------------- 6. the adjoint identity with nkp_value_gradient
def test_adjoint_identity_with_the_value_gradient(case):
    """sum_c <lam_c, P_c> with P = values_product (dval, x) against <g, dval> with g = value_gradient (lam, x, alpha = 1): the same
    sum of lam_c[i] dval_e x_c[j] over c and e.  Forwards a term meets at most len + 2 roundings (its product, the row's sums),
    backwards K + 1 (its product, the sum over c, alpha), doubled for second order: (len_max + K + 8) 2^-52 sum |lam| |dval| |x|."""
    c, K = case, 3
    lam = np.random.default_rng(73).standard_normal((K, c.n))
    x = c.X[:K]
    g = c.h.value_gradient(lam, x, alpha=1.0)
    P = c.h.values_product(c.dval, x)
    forwards = math.fsum((lam * P).ravel().tolist())
    backwards = math.fsum((g * c.dval).tolist())
    rowptr = c.rowptr.astype(np.int64)
    row_of = np.repeat(np.arange(c.n), np.diff(rowptr))
    col = c.colind.astype(np.int64)
    mag = math.fsum(sum(np.abs(lam[k][row_of]) * np.abs(c.dval) * np.abs(x[k][col]) for k in range(K)).tolist())
    # the products lam * P and g * dval formed above in numpy round once more each: within the + 8
    bound = (int(np.diff(rowptr).max()) + K + 8) * sh.U * mag
    print(f"{c.name}: forwards {forwards:.17g}, backwards {backwards:.17g}, difference {abs(forwards - backwards):.3e}, bound {bound:.3e}")
    assert abs(forwards - backwards) <= bound


# ---------------------------------------------------------------- 7. errors, 8. counters and work space
@pytest.fixture(scope="module")
def solvable():
    s = sh.ragged_dd()
    c = Case("ragged_dd", s.rowptr, s.colind, s.val)
    c.h.close()
    c.h = solver.NkpSolver(s.rowptr, s.colind, s.val, np.arange(s.n + 1), precond=solver.PRECOND_COLUMN_JACOBI, restart=30, rtol=1e-10)
    yield c
    c.h.close()


def test_bad_arguments_are_refused_and_leave_the_solver_as_it_was(solvable):
    c, h = solvable, solvable.h
    b = sh.vectors(sh.ragged_dd())[1]
    x0, _ = h.solve(b)
    product_device(h, c, 4, 1.0, False)                             # work space of a valid call exists: no bad call may change it
    bytes0, calls0, tang0 = h.get_int("device_bytes"), h.get_int("values_product_calls"), h.get_int("tangent_calls")
    n = c.n
    with Device(c.dval) as dv, Device(np.vstack([c.X, c.X[:1]])) as dx, Device(np.full((9, n), 2.5)) as dy:
        for nrhs, ldx, ldy, y, what in ((0, n, n, dy.ptr, "nrhs"), (9, n, n, dy.ptr, "nrhs"), (2, n - 1, n, dy.ptr, "ldx"), (2, n, n - 1, dy.ptr, "ldy"),
                                        (2, n, n, dx.ptr, "same buffer")):
            with pytest.raises(solver.NkpError) as e:
                h.values_product_device(dv.ptr, dx.ptr, nrhs, ldx, y, ldy)
            assert e.value.code == -1 and what in str(e.value), (nrhs, ldx, ldy, str(e.value))
        for args, what in (((None, None, n, None, dy.ptr, 2, n), "both NULL"), ((dv.ptr, dx.ptr, n, dy.ptr, dy.ptr, 0, n), "nrhs"),
                           ((dv.ptr, dx.ptr, n, dy.ptr, dy.ptr, 9, n), "nrhs"), ((dv.ptr, dx.ptr, n, dy.ptr, dy.ptr, 2, n - 1), "ld ="),
                           ((dv.ptr, dx.ptr, n - 1, dy.ptr, dy.ptr, 2, n), "ldx")):
            with pytest.raises(solver.NkpError) as e:
                h.solve_tangent_device(*args)
            assert e.value.code == -1 and what in str(e.value), (args, str(e.value))
        assert np.all(dy.get() == 2.5)
    assert (h.get_int("device_bytes"), h.get_int("values_product_calls"), h.get_int("tangent_calls")) == (bytes0, calls0, tang0)
    x1, _ = h.solve(b)
    assert_bits(x1, x0)


def test_counters_and_work_space():
    s = sh.ragged_empty()
    c = Case("ragged_empty", s.rowptr, s.colind, s.val)
    h, n, nnz = c.h, c.n, c.nnz
    try:
        assert h.get_int("values_product_calls") == 0 and h.get_int("values_product_us") == 0 and h.get_int("tangent_calls") == 0
        b0 = h.get_int("device_bytes")
        product_device(h, c, 1, 1.0, False)
        assert h.get_int("device_bytes") == b0                      # K = 1 on device buffers needs no work space
        product_device(h, c, 3, 1.0, False)
        b1 = h.get_int("device_bytes")
        assert b1 - b0 == 8 * 4 * n, (b0, b1)                       # the K = 4 interleaved copy of x
        h.values_product(c.dval, c.X[:3])
        b2 = h.get_int("device_bytes")
        assert b2 - b1 == 8 * (nnz + 2 * 3 * n), (b1, b2)           # the staging of the host flavour: val, x and y
        for K in (4, 2, 1, 3):
            h.values_product(c.dval[:], c.X[:K]) if K <= 3 else product_device(h, c, K, 1.0, True)
        assert h.get_int("device_bytes") == b2
        assert h.get_int("values_product_calls") == 7 and h.get_int("values_product_us") > 0 and h.get_int("tangent_calls") == 0
        assert h.get_int("value_gradient_calls") == 0
    finally:
        h.close()


def test_tangent_work_space_is_reserved_once(golden_by_name):
    g = golden_by_name("tri_12x10x6")
    ci, cj = solver.column_coords(g.ind_i, g.ind_j, g.col_start, g.cnt)
    n, ld = g.n, g.n + 2
    dB = np.random.default_rng(82).standard_normal((2, ld))
    with solver.NkpSolver(g.rowptr, g.colind, g.val, g.blk_start, g.cnt, col_i=ci, col_j=cj, rtol=1e-10, restart=150, max_iters=5000) as s:
        with Device(dB) as db, Device(np.zeros((2, ld))) as dx, Device(g.val) as dv:
            s.solve_batch_device(db.ptr, dx.ptr, 2, ld)             # the batched solve's own buffers exist from here on
            b0 = s.get_int("device_bytes")
            s.solve_tangent_device(None, None, 0, db.ptr, dx.ptr, 2, ld)
            b1 = s.get_int("device_bytes")
            assert b1 - b0 == 8 * 2 * ld, (b0, b1)                  # R
            s.solve_tangent_device(dv.ptr, db.ptr, ld, db.ptr, dx.ptr, 2, ld)
            b2 = s.get_int("device_bytes")
            assert b2 - b1 == 8 * 2 * n, (b1, b2)                   # the K = 2 interleaved copy of x
            s.solve_tangent_device(dv.ptr, db.ptr, ld, db.ptr, dx.ptr, 2, ld)
            s.solve_tangent_device(None, None, 0, db.ptr, dx.ptr, 1, ld)
            assert s.get_int("device_bytes") == b2
            assert s.get_int("tangent_calls") == 4 and s.get_int("values_product_calls") == 2


def test_time_kernel_6_runs_the_product_kernel_alone(case):
    h = case.h
    for K in (1, 2, 4, 8):
        assert h.time_kernel(6, reps=2, arg=K) > 0.0
        assert h.time_kernel(7, reps=2, arg=K) > 0.0                # the composition it is compared against
    with pytest.raises(solver.NkpError) as e:
        h.time_kernel(6, reps=2, arg=3)
    assert e.value.code == -1 and "which = 6" in str(e.value)


# ---------------------------------------------------------------- 9. the tangent solve on the golden fixtures
RTOL = 1e-10


@pytest.fixture(scope="module")
def tangent(golden):
    """one multilevel solver per fixture, X = A^-1 B for three seeded right-hand sides, a perturbation of the values and of B"""
    g = golden
    ci, cj = solver.column_coords(g.ind_i, g.ind_j, g.col_start, g.cnt)
    rng = np.random.default_rng(81)
    B = rng.standard_normal((3, g.n))
    dval = g.val * rng.standard_normal(g.val.size)
    dval[::7] = 0.0                                                 # zero diagonals among them: nothing a refactor would accept
    dB = rng.standard_normal((3, g.n))
    s = solver.NkpSolver(g.rowptr, g.colind, g.val, g.blk_start, g.cnt, col_i=ci, col_j=cj, rtol=RTOL, restart=150, max_iters=5000)
    assert s.get_int("levels") >= 1
    X, _ = s.solve_many(B)
    yield dict(g=g, s=s, X=X, dval=dval, dB=dB)
    s.close()


@pytest.mark.parametrize("K", [1, 2, 3])
def test_tangent_solve_is_the_documented_composition(tangent, K):
    g, s, X, dval, dB = (tangent[k] for k in ("g", "s", "X", "dval", "dB"))
    n, ld, ldx = g.n, g.n + 3, g.n + 1
    A = sp.csr_matrix((g.val, g.colind, g.rowptr), shape=(n, n))
    with Device(dval) as dv, Device(padded(X[:K], ldx)) as dx, Device(padded(dB[:K], ld, SENTINEL)) as db:
        # the composition by hand: a copy of dB, R -= dA X, the batched solve
        with Device(padded(dB[:K], ld, SENTINEL)) as dr, Device(np.full((K, ld), SENTINEL)) as dm:
            s.values_product_device(dv.ptr, dx.ptr, K, ldx, dr.ptr, ld, alpha=-1.0, accumulate=True)
            R = dr.get()
            info_m = s.solve_batch_device(dr.ptr, dm.ptr, K, ld)
            manual = dm.get()
        calls, tang = s.get_int("values_product_calls"), s.get_int("tangent_calls")
        bytes0 = s.get_int("device_bytes")
        with Device(np.full((K, ld), SENTINEL)) as dt:
            info_t = s.solve_tangent_device(dv.ptr, dx.ptr, ldx, db.ptr, dt.ptr, K, ld)
            got = dt.get()
        grown = s.get_int("device_bytes") - bytes0
        assert grown % (8 * ld) == 0 and 0 <= grown <= 8 * K * ld, grown      # R alone grows (the rest exists since the manual run)
        assert_bits(got, manual)
        assert info_t == info_m
        assert np.all(got[:, n:] == SENTINEL) and np.all(db.get()[:, :n] == dB[:K])
        assert s.get_int("values_product_calls") == calls + 1 and s.get_int("tangent_calls") == tang + 1
        # without dval: the plain batched solve of dB, and no product
        with Device(np.full((K, ld), SENTINEL)) as dp, Device(np.full((K, ld), SENTINEL)) as dt:
            s.solve_batch_device(db.ptr, dp.ptr, K, ld)
            s.solve_tangent_device(None, None, 0, db.ptr, dt.ptr, K, ld)
            assert_bits(dt.get(), dp.get())
        assert s.get_int("values_product_calls") == calls + 1 and s.get_int("tangent_calls") == tang + 2
        # without dB: R = 0 - dA X
        with Device(np.zeros((K, ld))) as dz, Device(np.full((K, ld), SENTINEL)) as dm, Device(np.full((K, ld), SENTINEL)) as dt:
            s.values_product_device(dv.ptr, dx.ptr, K, ldx, dz.ptr, ld, alpha=-1.0, accumulate=True)
            s.solve_batch_device(dz.ptr, dm.ptr, K, ld)
            s.solve_tangent_device(dv.ptr, dx.ptr, ldx, None, dt.ptr, K, ld)
            assert_bits(dt.get()[:, :n], dm.get()[:, :n])
    # the host wrapper stages the same call
    hx, _ = s.solve_tangent(X[:K] if K > 1 else X[0], dval=dval, dB=dB[:K] if K > 1 else dB[0])
    assert_bits(np.atleast_2d(hx), got[:, :n])
    # R is what the formula says, to rounding; and dX passes the solver's own stopping test, evaluated here:
    # ||R - A dX|| <= rtol ||R|| + ||e||, e = the rounding bound of evaluating R - A dX in f64 (spmv_shapes: (len + 2) 2^-52 (|A||dX| + |R|))
    dA = sp.csr_matrix((dval, g.colind, g.rowptr), shape=(n, n))
    absA, ln = abs(A), np.diff(g.rowptr.astype(np.int64))
    for k in range(K):
        Rk = R[k, :n]
        assert np.all(np.abs(Rk - (dB[k] - dA @ X[k])) <= (ln + 3) * sh.U * (abs(dA) @ np.abs(X[k]) + np.abs(dB[k])))
        res = np.linalg.norm(Rk - A @ got[k, :n])
        e = np.linalg.norm((ln + 2) * sh.U * (absA @ np.abs(got[k, :n]) + np.abs(Rk)))
        print(f"{g.name} K = {K} column {k}: ||R - A dX|| = {res:.3e}, rtol ||R|| = {RTOL * np.linalg.norm(Rk):.3e}, ||e|| = {e:.3e}, relres {info_t[k]['relres']:.3e}")
        assert res <= RTOL * np.linalg.norm(Rk) + e
