"""nkp_residual_batch / nkp_residual_batch_device on single-GPU solvers: residual, norms and componentwise backward error of K
given solutions in one pass over A.

On the ragged row blocks of tests/spmv_shapes.py (rows and blocks at the 2048-entry and 256-row caps, long rows first, last and in
succession, empty rows, a block of empty rows) and on a one-row matrix, for every nrhs:
  R      has, bit for bit, b - t with t restated in numpy in stored order (a row of more than 2048 entries in the SpMV's tree), which
         are also the bits of b - nkp_spmv_device (x);
  berr   has the bits of the host restatement: q per row from the restated r and den = d + |b| by berr_kernel's rule (den == 0
         included), the maximum NaN-sticky -- a maximum is order-free, so the bits are exact;
  rnorm, bnorm lie within a relative n 2^-52 of the correctly rounded values computed from the restated r (error-free squares,
         math.fsum): n squares rounded once each (2^-53 relative each), n - 1 additions of non-negative terms in ANY order (each
         partial sum is off by at most 2^-53 of itself, and no partial sum exceeds the total: (n - 1) 2^-53 of the total to first
         order), one square root (halves the relative error of its argument, adds 2^-53), the reference's own rounding 2^-53:
         (2 n + 1) 2^-54 + second order < n 2^-52 for n >= 2; the one-row case has one square and no addition: 2^-52 covers it;
         they are bit-identical between nrhs = 1 and the same vector at any column of nrhs = 2 .. 8, and between two calls.
Then the consistency with the solves (berr bit-identical to nkp_solve_device's on the returned x, before and after a refactor),
sentinels, R == B, one bad column, transposed handles, clones, the host flavour and the Python wrappers, refusals, counters, the
caller's stream behind pending work, and nkp_time_kernel 11 / 12."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import spmv_shapes as sh
from dist_values_product_trans_worker import tree_sum
from nk_ocn_tracer_jacobian_precond_amd import solver
from test_gpu_values_product import Device, assert_bits, padded

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F64P = C.POINTER(C.c_double)
RTOL = 1e-10


# ---------------------------------------------------------------- the restatement
def restate_td(rowptr, colind, val, x):
    """t and d of every row: +0.0, then every stored entry in stored order, each product and each sum rounded; a row of more than
    2048 entries in the tree of the SpMV kernels, t and d alike"""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(colind, np.int64)
    val = np.asarray(val, np.float64)
    ln = np.diff(rowptr)
    long_rows = np.flatnonzero(ln > sh.LDS_NNZ)
    short = np.where(ln > sh.LDS_NNZ, 0, ln)
    t, d = np.zeros(ln.size), np.zeros(ln.size)
    with np.errstate(invalid="ignore"):
        for k in range(int(short.max(initial=0))):
            rows = np.flatnonzero(short > k)
            e = rowptr[rows] + k
            p = val[e] * x[col[e]]
            t[rows] = t[rows] + p
            d[rows] = d[rows] + np.abs(p)
        for i in long_rows:
            p = val[rowptr[i]:rowptr[i + 1]] * x[col[rowptr[i]:rowptr[i + 1]]]
            t[i], d[i] = tree_sum(p), tree_sum(np.abs(p))
    return t, d


def quotients(r, den):
    """berr_kernel's rule: a / den keeps a NaN of either; den == 0 gives 0 for r == 0 and 1e300 otherwise"""
    a = np.abs(r)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((den > 0.0) | np.isnan(den), a / den, np.where(np.isnan(a), a, np.where(a > 0.0, 1.0e300, 0.0)))


def max_or_nan(q):
    return float("nan") if np.isnan(q).any() else float(np.max(q, initial=0.0))


def exact_norm(v):
    """sqrt of the exact sum of squares, correctly rounded up to the final square root"""
    p, e = sh._two_prod(v, v)
    return math.sqrt(math.fsum(p.tolist() + e.tolist()))


def restate(rowptr, colind, val, B, X):
    """(R, berr, rnorm, bnorm) for the rows of B and X"""
    R, berr, rn, bn = [], [], [], []
    for b, x in zip(B, X):
        t, d = restate_td(rowptr, colind, val, x)
        with np.errstate(invalid="ignore"):
            r = b - t
            q = quotients(r, d + np.abs(b))
        R.append(r)
        berr.append(max_or_nan(q))
        rn.append(float("nan") if np.isnan(r).any() else exact_norm(r))
        bn.append(float("nan") if np.isnan(b).any() else exact_norm(b))
    return np.stack(R), np.array(berr), np.array(rn), np.array(bn)


def assert_within(got, ref, n, what):
    bound = max(n, 2) * sh.U
    rel = np.abs(got - ref) / np.where(ref > 0.0, ref, 1.0)
    print(f"{what}: largest |got - exact| / exact = {rel.max():.3e}, bound n 2^-52 = {bound:.3e}")
    assert np.all(rel <= bound), (what, got, ref)


# ---------------------------------------------------------------- the cases
class Case:
    def __init__(self, name, rowptr, colind, val, empty_rows=()):
        self.name, self.rowptr, self.colind, self.val = name, rowptr, colind, val
        self.n, self.nnz = rowptr.size - 1, colind.size
        rng = np.random.default_rng(91)
        self.B = rng.standard_normal((8, self.n))
        self.X = rng.standard_normal((8, self.n))
        self.X[:, 5::89] = -0.0
        if len(empty_rows):                                          # b = 0 on every empty row of the even columns: den == 0, r == 0, q = 0;
            self.B[0::2, np.asarray(empty_rows)] = 0.0               # the odd columns keep b != 0 there: r = b, q = 1 exactly
        self.R, self.berr, self.rnorm, self.bnorm = restate(rowptr, colind, val, self.B, self.X)
        self.h = solver.NkpSolver(rowptr, colind, val, None, precond=solver.PRECOND_NONE, restart=4)


def _shape_case(name):
    if name == "one_row":
        return Case(name, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.0]))
    s = getattr(sh, name)()
    empty = np.flatnonzero(s.len == 0) if name == "ragged_empty" else []
    if name == "ragged_empty":
        assert empty.size > 300 and s.marks["empty_at_block_start"] in empty and s.marks["empty_block"] + 7 in empty
    return Case(name, s.rowptr, s.colind, s.val, empty)


@pytest.fixture(scope="module", params=["ragged_empty", "ragged_dd", "one_row"])
def case(request):
    c = _shape_case(request.param)
    yield c
    c.h.close()


class Result:
    pass


def run_device(h, B, X, n, pad=5, extra_cols=0, want_r=True, r_is_b=False):
    """the device flavour with every ld > n and all different; NaN sentinels behind n and behind nrhs"""
    nrhs = B.shape[0]
    ldb, ldx, ldr = n + pad, n + pad + 1, (n + pad if r_is_b else n + pad + 2)
    b0 = np.full((nrhs + extra_cols, ldb), np.nan)
    b0[:nrhs, :n] = B
    o = Result()
    with Device(b0) as db, Device(padded(X, ldx)) as dx, Device(np.full((nrhs + extra_cols, ldr), np.nan)) as dr:
        r_ptr = db.ptr if r_is_b else (dr.ptr if want_r else None)
        o.rnorm, o.bnorm, o.berr = h.residual_batch_device(db.ptr, ldb, dx.ptr, ldx, nrhs, r_ptr, ldr)
        o.Rbuf, o.Bbuf, o.Xbuf = (db.get() if r_is_b else dr.get()), db.get(), dx.get()
    o.R = o.Rbuf[:nrhs, :n]
    o.sentinels = bool(np.all(np.isnan(o.Rbuf[:, n:])) and np.all(np.isnan(o.Rbuf[nrhs:])))
    o.x_unchanged = bool(np.array_equal(o.Xbuf[:, :n].view(np.uint64), np.ascontiguousarray(X).view(np.uint64)) and np.all(np.isnan(o.Xbuf[:, n:])))
    return o


def same_numbers(a, b, cols=None):
    cols = slice(None) if cols is None else cols
    for name in ("rnorm", "bnorm", "berr"):
        assert_bits(getattr(a, name)[cols], getattr(b, name)[cols])


# ---------------------------------------------------------------- R, berr, the norms, the sentinels
@pytest.mark.parametrize("nrhs", [1, 2, 3, 4, 5, 6, 7, 8])
def test_residual_backward_error_and_norms(case, nrhs):
    c = case
    o = run_device(c.h, c.B[:nrhs], c.X[:nrhs], c.n, extra_cols=2)
    assert_bits(o.R, c.R[:nrhs])
    assert o.sentinels and o.x_unchanged
    assert_bits(o.Bbuf[:nrhs, :c.n], c.B[:nrhs])                    # B is not modified
    assert np.all(np.isnan(o.Bbuf[:, c.n:])) and np.all(np.isnan(o.Bbuf[nrhs:]))
    assert_bits(o.berr, c.berr[:nrhs])
    assert np.all(o.berr >= 0.0)
    assert_within(o.rnorm, c.rnorm[:nrhs], c.n, f"{c.name} nrhs {nrhs} rnorm")
    assert_within(o.bnorm, c.bnorm[:nrhs], c.n, f"{c.name} nrhs {nrhs} bnorm")
    # without R: the same numbers, nothing written
    p = run_device(c.h, c.B[:nrhs], c.X[:nrhs], c.n, want_r=False)
    same_numbers(p, o)
    assert np.all(np.isnan(p.Rbuf))


def test_residual_has_the_bits_of_b_minus_the_spmv(case):
    c = case
    o = run_device(c.h, c.B, c.X, c.n)
    for k in range(8):
        with Device(c.X[k]) as dx, Device(np.full(c.n, np.nan)) as dy:
            c.h.spmv_device(dx.ptr, dy.ptr)
            assert_bits(o.R[k], c.B[k] - dy.get())


def test_an_empty_row_with_b_zero_takes_the_den_zero_rule():
    c = _shape_case("ragged_empty")
    try:
        s = sh.ragged_empty()
        i = s.marks["empty_at_block_start"]
        t, d = restate_td(c.rowptr, c.colind, c.val, c.X[0])
        assert c.B[0, i] == 0.0 and d[i] == 0.0 and t[i] == 0.0 and c.B[1, i] != 0.0
        # alone in its system the row decides berr: a one-row-block view is the whole matrix with b = A x restated elsewhere
        b = t.copy()                                                 # r == 0 everywhere, den == 0 on the empty rows: berr 0, not NaN
        o = run_device(c.h, b[None], c.X[:1], c.n)
        assert o.berr[0] == 0.0 and o.rnorm[0] == 0.0 and not np.isnan(o.berr[0])
        assert np.all(o.R == 0.0)
        # b != 0 on an empty row: r = b, den = |b|, q = 1 exactly
        b[i + 1] = -3.5
        o = run_device(c.h, b[None], c.X[:1], c.n)
        assert o.berr[0] == 1.0 and o.R[0, i + 1] == -3.5 and o.rnorm[0] == 3.5
    finally:
        c.h.close()


def test_norms_do_not_depend_on_nrhs_on_the_position_or_on_the_call(case):
    c = case
    one = run_device(c.h, c.B[3:4], c.X[3:4], c.n)
    again = run_device(c.h, c.B[3:4], c.X[3:4], c.n)
    same_numbers(one, again)
    assert_bits(one.R, again.R)
    for nrhs in range(2, 9):
        for pos in range(nrhs):
            order = [k for k in range(8) if k != 3][:nrhs - 1]
            order.insert(pos, 3)
            o = run_device(c.h, c.B[order], c.X[order], c.n, pad=1)
            for name in ("rnorm", "bnorm", "berr"):
                assert_bits(getattr(o, name)[pos:pos + 1], getattr(one, name))
            assert_bits(o.R[pos], one.R[0])


def test_residual_written_over_b(case):
    c = case
    for nrhs in (1, 3, 8):
        sep = run_device(c.h, c.B[:nrhs], c.X[:nrhs], c.n, extra_cols=1)
        inp = run_device(c.h, c.B[:nrhs], c.X[:nrhs], c.n, extra_cols=1, r_is_b=True)
        assert_bits(inp.R, sep.R)
        assert inp.sentinels and inp.x_unchanged
        same_numbers(inp, sep)


def test_one_bad_column_does_not_disturb_the_others(case):
    c = case
    clean = run_device(c.h, c.B[:5], c.X[:5], c.n)
    j = int(c.colind[c.colind.size // 2])                            # a column some row gathers
    X = c.X[:5].copy()
    X[2, j] = np.nan
    o = run_device(c.h, c.B[:5], X, c.n)
    assert np.isnan(o.rnorm[2]) and np.isnan(o.berr[2]) and not np.isnan(o.bnorm[2])
    keep = [0, 1, 3, 4]
    same_numbers(o, clean, keep)
    assert_bits(o.R[keep], clean.R[keep])
    B = c.B[:5].copy()
    B[0, c.n // 2] = np.nan
    o = run_device(c.h, B, c.X[:5], c.n)
    assert np.isnan(o.rnorm[0]) and np.isnan(o.berr[0]) and np.isnan(o.bnorm[0])
    same_numbers(o, clean, [1, 2, 3, 4])
    assert_bits(o.R[1:], clean.R[1:])
    B[0, c.n // 2] = np.inf                                          # Inf in b: r = Inf, den = Inf, q = NaN; the norms Inf
    o = run_device(c.h, B, c.X[:5], c.n)
    assert np.isinf(o.rnorm[0]) and np.isinf(o.bnorm[0]) and np.isnan(o.berr[0])
    same_numbers(o, clean, [1, 2, 3, 4])


# ---------------------------------------------------------------- other handles and flavours
def test_clone_host_flavour_and_python_wrappers(case):
    c = case
    dev = run_device(c.h, c.B[:3], c.X[:3], c.n)
    k = c.h.clone()
    try:
        o = run_device(k, c.B[:3], c.X[:3], c.n)
        same_numbers(o, dev)
        assert_bits(o.R, dev.R)
        assert k.get_int("residual_batch_calls") == 1
    finally:
        k.close()
    res = c.h.residual_batch(c.B[:3], c.X[:3], want_residual=True)
    assert_bits(res.R, dev.R)
    for name in ("rnorm", "bnorm", "berr"):
        assert_bits(getattr(res, name), getattr(dev, name))
    with np.errstate(divide="ignore", invalid="ignore"):
        assert_bits(res.relres, dev.rnorm / dev.bnorm)
    res = c.h.residual_batch(c.B[1], c.X[1])
    assert res.R is None and res.rnorm.shape == (1,)
    assert_bits(res.berr, dev.berr[1:2])
    assert_bits(res.rnorm, dev.rnorm[1:2])
    # the C host flavour with every ld > n and R == B
    ld = c.n + 4
    b, x = padded(c.B[:2], ld), padded(c.X[:2], ld)
    out = np.full((3, 2), np.nan)
    rc = c.h._lib.nkp_residual_batch(c.h._h, 2, b.ctypes.data_as(F64P), ld, x.ctypes.data_as(F64P), ld, b.ctypes.data_as(F64P), ld,
                                     out[0].ctypes.data_as(F64P), out[1].ctypes.data_as(F64P), out[2].ctypes.data_as(F64P))
    assert rc == 0, solver.last_error()
    assert_bits(b[:, :c.n], dev.R[:2])
    assert np.all(np.isnan(b[:, c.n:]))
    assert_bits(out, np.stack([dev.rnorm[:2], dev.bnorm[:2], dev.berr[:2]]))
    # only one number asked for
    only = np.full(2, np.nan)
    rc = c.h._lib.nkp_residual_batch(c.h._h, 2, padded(c.B[:2], ld).ctypes.data_as(F64P), ld, x.ctypes.data_as(F64P), ld, None, 0, None, None, only.ctypes.data_as(F64P))
    assert rc == 0, solver.last_error()
    assert_bits(only, dev.berr[:2])


def test_transposed_handle_is_the_solver_of_the_host_transpose(monkeypatch):
    from test_gpu_transpose import _gen, _transpose
    monkeypatch.setenv("NKP_ML_DEVICE_MIN", "0")
    monkeypatch.setenv("NKP_ML_COARSEST_ROWS", "300")
    p = _gen()
    n = p.flat_len
    T, src = _transpose(p.rowptr, p.colind, p.nzval)
    rng = np.random.default_rng(92)
    B, X = rng.standard_normal((3, n)), rng.standard_normal((3, n))
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    with solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, 1, col_i=ci, col_j=cj) as s:
        t = s.transposed()
        got = run_device(t, B, X, n)
        own = run_device(s, B, X, n)
    with solver.NkpSolver(T.indptr.astype(np.int32), T.indices.astype(np.int32), np.asarray(p.nzval)[src], None, precond=solver.PRECOND_NONE, restart=4) as f:
        want = run_device(f, B, X, n)
    assert_bits(got.R, want.R)
    same_numbers(got, want)
    R, berr, rn, bn = restate(T.indptr, T.indices, np.asarray(p.nzval)[src], B, X)
    assert_bits(got.R, R)
    assert_bits(got.berr, berr)
    R, berr, rn, bn = restate(p.rowptr, p.colind, p.nzval, B, X)
    assert_bits(own.R, R)
    assert_bits(own.berr, berr)


# ---------------------------------------------------------------- consistency with the solves, across a refactor
def check_against_the_solve(make, n, b, new_val, what):
    """nkp_solve_device with berr, then nkp_residual_batch_device on the returned x: berr bit-identical, rnorm / bnorm <= rtol when the
    solve said NKP_OK; after nkp_refactor the same x gives the numbers of a fresh solver created from the new values"""
    with make(None) as s:
        with Device(b) as db, Device(np.zeros(n)) as dx:
            info = s.solve_device(db.ptr, dx.ptr, raise_on_fail=False)
            x = dx.get()
        o = run_device(s, b[None], x[None], n)
        print(f"{what}: solve status {info['status']}, iters {info['iters']}, relres {info['relres']:.3e}, berr {info['berr']:.3e}; "
              f"residual_batch rnorm / bnorm {o.rnorm[0] / o.bnorm[0]:.3e}, berr {o.berr[0]:.3e}")
        assert_bits(o.berr, np.array([info["berr"]]))
        assert info["status"] == solver.NKP_OK
        assert o.rnorm[0] / o.bnorm[0] <= RTOL
        s.refactor(new_val)
        assert s.get_int("refactor_count") == 1
        after = run_device(s, b[None], x[None], n)
    with make(new_val) as f:
        fresh = run_device(f, b[None], x[None], n)
    assert_bits(after.R, fresh.R)
    same_numbers(after, fresh)
    assert not np.array_equal(after.R, o.R)                          # the new values were read


def test_consistent_with_the_multilevel_solve_on_a_golden_fixture(golden):
    g = golden
    ci, cj = solver.column_coords(g.ind_i, g.ind_j, g.col_start, g.cnt)
    new_val = g.val * (1.0 + 0.01 * np.random.default_rng(93).standard_normal(g.val.size))

    def make(val):
        return solver.NkpSolver(g.rowptr, g.colind, g.val if val is None else val, g.blk_start, g.cnt, col_i=ci, col_j=cj, rtol=RTOL, restart=150, max_iters=5000)
    check_against_the_solve(make, g.n, g.rhs(g.groups()[0]), new_val, g.name)


def test_consistent_with_the_point_jacobi_solve_on_ragged_dd():
    s = sh.ragged_dd()

    def make(val):
        return solver.NkpSolver(s.rowptr, s.colind, s.val if val is None else val, np.arange(s.n + 1), precond=solver.PRECOND_COLUMN_JACOBI, restart=30, rtol=RTOL)
    check_against_the_solve(make, s.n, sh.vectors(s)[1], sh.refactored_values(s), "ragged_dd")


# ---------------------------------------------------------------- refusals, counters and work space
@pytest.fixture(scope="module")
def solvable():
    s = sh.ragged_dd()
    c = Case("ragged_dd", s.rowptr, s.colind, s.val)
    c.h.close()
    c.h = solver.NkpSolver(s.rowptr, s.colind, s.val, np.arange(s.n + 1), precond=solver.PRECOND_COLUMN_JACOBI, restart=30, rtol=1e-10)
    yield c
    c.h.close()


def test_bad_arguments_are_refused_and_leave_the_solver_as_it_was(solvable):
    c, h, n = solvable, solvable.h, solvable.n
    b = sh.vectors(sh.ragged_dd())[1]
    x0, _ = h.solve(b)
    run_device(h, c.B[:4], c.X[:4], n)                               # work space of a valid call exists: no bad call may change it
    bytes0, calls0 = h.get_int("device_bytes"), h.get_int("residual_batch_calls")
    with Device(np.vstack([c.B, c.B[:1]])) as db, Device(np.vstack([c.X, c.X[:1]])) as dx, Device(np.full((9, n), 2.5)) as dr:
        for nrhs, ldb, ldx, r, ldr, what in ((0, n, n, dr.ptr, n, "nrhs = 0"), (9, n, n, dr.ptr, n, "nrhs = 9"), (2, n - 1, n, dr.ptr, n, "ldb"),
                                             (2, n, n - 1, dr.ptr, n, "ldx"), (2, n, n, dr.ptr, n - 1, "ldr"), (2, n, n, dx.ptr, n, "same buffer")):
            with pytest.raises(solver.NkpError) as e:
                h.residual_batch_device(db.ptr, ldb, dx.ptr, ldx, nrhs, r, ldr)
            assert e.value.code == -1 and what in str(e.value), (nrhs, ldb, ldx, ldr, str(e.value))
        with pytest.raises(solver.NkpError) as e:
            h.residual_batch_device(db.ptr, n, dx.ptr, n, 9)
        assert "call again" in str(e.value)
        lib = h._lib
        for args, what in (((None, 2, db.p, n, dx.p, n, dr.p, n), "NULL solver"), ((h._h, 2, None, n, dx.p, n, dr.p, n), "NULL argument d_B"),
                           ((h._h, 2, db.p, n, None, n, dr.p, n), "NULL argument d_X")):
            assert lib.nkp_residual_batch_device(*args, None, None, None) == -1
            assert what in solver.last_error(), solver.last_error()
        assert lib.nkp_residual_batch_device(h._h, 2, db.p, n, dx.p, n, None, 0, None, None, None) == -1
        assert "nothing is asked" in solver.last_error()
        v = np.ones(2 * n)
        p = v.ctypes.data_as(F64P)
        assert lib.nkp_residual_batch(h._h, 2, p, n, p, n, p, n, None, None, None) == -1 and "same buffer" in solver.last_error()
        assert lib.nkp_residual_batch(h._h, 2, None, n, p, n, None, n, p, None, None) == -1 and "NULL argument B" in solver.last_error()
        assert lib.nkp_residual_batch(h._h, 2, p, n, None, n, None, n, p, None, None) == -1 and "NULL argument X" in solver.last_error()
        assert np.all(dr.get() == 2.5)
        assert_bits(db.get()[:8], c.B)
        assert_bits(dx.get()[:8], c.X)
    assert (h.get_int("device_bytes"), h.get_int("residual_batch_calls")) == (bytes0, calls0)
    x1, _ = h.solve(b)
    assert_bits(x1, x0)


def test_counters_and_work_space():
    s = sh.ragged_empty()
    c = Case("ragged_empty", s.rowptr, s.colind, s.val)
    h, n = c.h, c.n
    nrb = sh.row_blocks(s.rowptr).size - 1
    try:
        assert h.get_int("residual_batch_calls") == 0 and h.get_int("residual_batch_us") == 0
        b0 = h.get_int("device_bytes")
        run_device(h, c.B[:1], c.X[:1], n)
        b1 = h.get_int("device_bytes")
        assert b1 - b0 == 8 * 3 * (nrb + 1), (b0, b1)                # K = 1 reads x in place: the partials alone
        run_device(h, c.B[:1], c.X[:1], n)
        assert h.get_int("device_bytes") == b1                       # once, not per call
        run_device(h, c.B[:3], c.X[:3], n)
        b2 = h.get_int("device_bytes")
        assert b2 - b1 == 8 * 4 * n + 8 * 3 * 3 * (nrb + 1), (b1, b2)      # the K = 4 interleaved copy of x, the partials from K = 1 to K = 4
        h.residual_batch(c.B[:3], c.X[:3], want_residual=True)
        b3 = h.get_int("device_bytes")
        assert b3 - b2 == 8 * 3 * 3 * n, (b2, b3)                    # the staging of the host flavour: B, X and R
        for K in (4, 2, 1, 3):
            h.residual_batch(c.B[:K], c.X[:K], want_residual=K == 3) if K <= 3 else run_device(h, c.B[:K], c.X[:K], n)
        assert h.get_int("device_bytes") == b3
        assert h.get_int("residual_batch_calls") == 8 and h.get_int("residual_batch_us") > 0
        with pytest.raises(solver.NkpError):
            h.residual_batch_device(1, n, 1, n, 0)
        assert h.get_int("residual_batch_calls") == 8                # successes only
        assert h.get_int("values_product_calls") == 0
    finally:
        h.close()


def test_time_kernel_11_and_12(case):
    h = case.h
    for K in (1, 2, 4, 8):
        assert h.time_kernel(11, reps=2, arg=K) > 0.0
        assert h.time_kernel(12, reps=2, arg=K) > 0.0                # the composition it is compared against
    for which in (11, 12):
        with pytest.raises(solver.NkpError) as e:
            h.time_kernel(which, reps=2, arg=3)
        assert e.value.code == -1 and f"which = {which}" in str(e.value)


# ---------------------------------------------------------------- the caller's stream behind pending work
def test_a_late_x_on_the_callers_stream(tmp_path):
    """tests/residual_batch_stream_worker.py: the solver is on a caller's non-blocking stream; X is NaN until a copy enqueued on that
    stream behind a pending long kernel fills it; the call is made at once, without a synchronisation, and has the bits of the
    synchronised call"""
    out = str(tmp_path / "stream.json")
    r = subprocess.run([sys.executable, os.path.join(HERE, "residual_batch_stream_worker.py"), "--out", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.load(open(out))
    print(res)
    assert res["control_saw_nan"] and res["late_values_arrived"], res
    for c in res["calls"]:
        assert c["unfinished_at_entry"], f"the producer had finished when the library was entered: {c}"
        assert c["numbers_equal"] and c["residual_equal"] and c["finite"], c
    assert [c["nrhs"] for c in res["calls"]] == [1, 3, 8]
