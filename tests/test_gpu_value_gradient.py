"""nkp_value_gradient: g[e] = alpha * sum_c lambda_c[row of e] * x_c[colind[e]] on the CSR pattern.

Kernel: on the ragged row blocks of tests/spmv_shapes.py (rows and blocks at the 2048-entry and 256-row caps, long rows, empty
rows, a block of empty rows) host and device flavours give bit for bit the numpy restatement -- one product or one sum per numpy
operation, in ascending c -- for every K, with and without accumulation, and write nowhere else.
End to end: with the library's own X = A^-1 B and Lambda = A^-T W the gradient agrees with a central difference of scipy splu
solves, and the torch wrapper's backward pass gives the same bits as the calls it is made of."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import spmv_shapes as sh
from nk_ocn_tracer_jacobian_precond_amd import solver
from test_gpu_transpose import _gen, _transpose

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F64P = C.POINTER(C.c_double)


# ---------------------------------------------------------------- helpers
def restate(rowptr, colind, lam, x, alpha, g0=None):
    """the formula of include/nkp.h, one rounded operation per numpy operation"""
    rowptr = np.asarray(rowptr, np.int64)
    row_of = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    col = np.asarray(colind, np.int64)
    lam, x = np.atleast_2d(lam), np.atleast_2d(x)
    s = lam[0][row_of] * x[0][col]
    for c in range(1, lam.shape[0]):
        s = s + lam[c][row_of] * x[c][col]
    v = alpha * s
    return v if g0 is None else g0 + v


def bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, (bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


class Device:
    """a float64 array on the device through the HIP runtime the library links (no second runtime in this process)"""

    def __init__(self, a):
        self.hip = C.CDLL("libamdhip64.so")
        a = np.ascontiguousarray(a, np.float64)
        self.size, self.p = a.size, C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(max(a.nbytes, 8))) == 0
        if a.nbytes:
            assert self.hip.hipMemcpy(self.p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
        self.ptr = self.p.value

    def get(self):
        out = np.empty(self.size)
        if out.nbytes:
            assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(out.nbytes), 2) == 0
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.hip.hipFree(self.p)


def padded(v, ld):
    """(K, n) -> (K, ld) with a poison tail no kernel may read into the result"""
    out = np.full((v.shape[0], ld), np.nan)
    out[:, :v.shape[1]] = v
    return out


def call_host(h, lam, x, ld, alpha, accumulate, g):
    """nkp_value_gradient on (K, ld) host arrays; returns the code"""
    return h._lib.nkp_value_gradient(h._h, lam.shape[0], lam.ctypes.data_as(F64P), x.ctypes.data_as(F64P), ld, alpha, accumulate, g.ctypes.data_as(F64P))


def vectors(n, K, seed=3):
    """K pairs with zeros of either sign, a denormal and large magnitudes among ordinary values"""
    rng = np.random.default_rng(seed)
    lam, x = rng.standard_normal((K, n)), rng.standard_normal((K, n))
    lam[:, ::97] = 0.0
    x[:, 5::89] = -0.0
    lam[0, 11::101] *= 1e150
    x[-1, 13::103] = 5e-324
    return lam, x


@pytest.fixture(scope="module")
def ragged():
    s = sh.ragged_empty()
    assert s.long.sum() >= 6 and (s.len == 0).sum() > 300 and s.n > 256
    h = solver.NkpSolver(s.rowptr, s.colind, s.val, None, precond=solver.PRECOND_NONE, restart=4)
    yield s, h
    h.close()


# ---------------------------------------------------------------- kernel: bits
@pytest.mark.parametrize("pad", [0, 7])
@pytest.mark.parametrize("alpha", [-1.0, 0.37])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8])
def test_bits_of_the_numpy_restatement(ragged, K, alpha, pad):
    s, h = ragged
    nnz, ld = s.colind.size, s.n + pad
    lam, x = vectors(s.n, K)
    want = restate(s.rowptr, s.colind, lam, x, alpha)
    assert np.all(np.isfinite(want))
    L, X = padded(lam, ld), padded(x, ld)
    g = np.full(nnz, np.nan)
    assert call_host(h, L, X, ld, alpha, 0, g) == 0, solver.last_error()
    assert_bits(g, want)
    with Device(L) as dl, Device(X) as dx, Device(np.full(nnz, np.nan)) as dg:
        h.value_gradient_device(dl.ptr, dx.ptr, K, ld, dg.ptr, alpha=alpha)
        assert_bits(dg.get(), want)
    if pad == 0:
        assert_bits(h.value_gradient(lam if K > 1 else lam[0], x if K > 1 else x[0], alpha=alpha), want)


@pytest.mark.parametrize("K", [1, 3, 8])
def test_bits_with_64_bit_row_pointers(K):
    s = sh.ragged_empty()
    lam, x = vectors(s.n, K, seed=4)
    with solver.NkpSolver(s.rowptr.astype(np.int64), s.colind, s.val, None, precond=solver.PRECOND_NONE, restart=4) as h:
        assert_bits(h.value_gradient(lam, x, alpha=0.37), restate(s.rowptr, s.colind, lam, x, 0.37))


# ---------------------------------------------------------------- kernel: accumulation
@pytest.mark.parametrize("K", [1, 3, 4])
def test_accumulate_adds_to_the_old_bits(ragged, K):
    s, h = ragged
    nnz = s.colind.size
    lam, x = vectors(s.n, K, seed=5)
    g0 = np.random.default_rng(6).standard_normal(nnz)
    want = restate(s.rowptr, s.colind, lam, x, 0.37, g0)
    g = g0.copy()
    assert call_host(h, lam, x, s.n, 0.37, 1, g) == 0, solver.last_error()
    assert_bits(g, want)
    with Device(lam) as dl, Device(x) as dx, Device(g0) as dg:
        h.value_gradient_device(dl.ptr, dx.ptr, K, s.n, dg.ptr, alpha=0.37, accumulate=True)
        assert_bits(dg.get(), want)


def test_two_accumulated_calls_chain_per_call(ragged):
    """K = 4 then K = 4 with accumulate: (alpha * s_first) + alpha * s_second, the documented sum -- not the K = 8 single call"""
    s, h = ragged
    lam, x = vectors(s.n, 8, seed=7)
    first = restate(s.rowptr, s.colind, lam[:4], x[:4], -1.0)
    want = restate(s.rowptr, s.colind, lam[4:], x[4:], -1.0, first)
    with Device(lam) as dl, Device(x) as dx, Device(np.full(s.colind.size, np.nan)) as dg:
        h.value_gradient_device(dl.ptr, dx.ptr, 4, s.n, dg.ptr)
        h.value_gradient_device(dl.ptr + 8 * 4 * s.n, dx.ptr + 8 * 4 * s.n, 4, s.n, dg.ptr, accumulate=True)
        got = dg.get()
    assert_bits(got, want)
    single = restate(s.rowptr, s.colind, lam, x, -1.0)
    print(f"entries where the chained sum differs from the single K = 8 sum: {(got != single).sum()} of {got.size}")
    assert np.all(np.abs(got - single) <= 16 * sh.U * restate(s.rowptr, s.colind, np.abs(lam), np.abs(x), 1.0))      # the same sum, re-associated


# ---------------------------------------------------------------- kernel: no stray writes
@pytest.mark.parametrize("K", [1, 2, 8])
def test_guard_band_around_the_gradient_is_intact(ragged, K):
    s, h = ragged
    nnz, sentinel = s.colind.size, -7.25e77
    lam, x = vectors(s.n, K, seed=8)
    with Device(lam) as dl, Device(x) as dx, Device(np.full(nnz + 128, sentinel)) as dg:
        h.value_gradient_device(dl.ptr, dx.ptr, K, s.n, dg.ptr + 8 * 64, alpha=-1.0)
        got = dg.get()
    assert np.all(got[:64] == sentinel) and np.all(got[-64:] == sentinel)
    assert_bits(got[64:-64], restate(s.rowptr, s.colind, lam, x, -1.0))


@pytest.mark.parametrize("K", [1, 4])
def test_matrix_without_entries_writes_nothing(K):
    n = 300                                                        # two row blocks of empty rows
    lam, x = vectors(n, K, seed=9)
    with solver.NkpSolver(np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0), None, precond=solver.PRECOND_NONE, restart=4) as h:
        assert h.get_int("nnz") == 0
        g = np.full(4, 3.5)
        assert call_host(h, lam, x, n, -1.0, 0, g) == 0, solver.last_error()
        assert np.all(g == 3.5)
        with Device(lam) as dl, Device(x) as dx, Device(np.full(128, 3.5)) as dg:
            h.value_gradient_device(dl.ptr, dx.ptr, K, n, dg.ptr + 8 * 64)
            assert np.all(dg.get() == 3.5)
        assert h.value_gradient(lam, x).size == 0


# ---------------------------------------------------------------- arguments, introspection
def test_bad_arguments_are_refused_and_leave_the_solver_usable(ragged):
    s, h = ragged
    lam, x = vectors(s.n, 8, seed=10)
    L9, X9 = np.vstack([lam, lam[:1]]), np.vstack([x, x[:1]])
    g = np.full(s.colind.size, 2.5)
    calls = h.get_int("value_gradient_calls")
    for nrhs, ld, what in ((0, s.n, "nrhs"), (9, s.n, "nrhs"), (2, s.n - 1, "ld")):
        rc = h._lib.nkp_value_gradient(h._h, nrhs, L9.ctypes.data_as(F64P), X9.ctypes.data_as(F64P), ld, -1.0, 0, g.ctypes.data_as(F64P))
        assert rc == -1 and what in solver.last_error(), (nrhs, ld, rc, solver.last_error())
        with Device(L9) as dl, Device(X9) as dx, Device(g) as dg:
            with pytest.raises(solver.NkpError) as e:
                h.value_gradient_device(dl.ptr, dx.ptr, nrhs, ld, dg.ptr)
            assert e.value.code == -1 and what in str(e.value)
            assert np.all(dg.get() == 2.5)
    assert np.all(g == 2.5) and h.get_int("value_gradient_calls") == calls
    assert_bits(h.value_gradient(lam[:2], x[:2]), restate(s.rowptr, s.colind, lam[:2], x[:2], -1.0))
    assert h.get_int("value_gradient_calls") == calls + 1


def test_counters_and_work_space():
    s = sh.ragged_empty()
    lam, x = vectors(s.n, 4, seed=11)
    with solver.NkpSolver(s.rowptr, s.colind, s.val, None, precond=solver.PRECOND_NONE, restart=4) as h:
        assert h.get_int("value_gradient_calls") == 0 and h.get_int("value_gradient_us") == 0
        b0 = h.get_int("device_bytes")
        h.value_gradient(lam, x)
        b1 = h.get_int("device_bytes")
        # interleaved lambda and x (2 * 4 n), staged host vectors (2 * 4 n) and the staged gradient (nnz)
        assert b1 - b0 == 8 * (16 * s.n + s.colind.size), (b0, b1)
        assert h.get_int("value_gradient_calls") == 1 and h.get_int("value_gradient_us") > 0
        for K in (4, 3, 1, 2):
            h.value_gradient(lam[:K], x[:K])
        with Device(lam) as dl, Device(x) as dx, Device(np.zeros(s.colind.size)) as dg:
            h.value_gradient_device(dl.ptr, dx.ptr, 4, s.n, dg.ptr)
        assert h.get_int("device_bytes") == b1 and h.get_int("value_gradient_calls") == 6
        c = h.clone()                                               # only the pattern is read: a clone may be asked too
        assert_bits(c.value_gradient(lam, x), restate(s.rowptr, s.colind, lam, x, -1.0))
        assert c.get_int("value_gradient_calls") == 1 and h.get_int("value_gradient_calls") == 6
        c.close()


# ---------------------------------------------------------------- transposed handle
def test_transposed_handle_gives_the_gradient_of_the_transpose(monkeypatch):
    monkeypatch.setenv("NKP_ML_DEVICE_MIN", "0")
    monkeypatch.setenv("NKP_ML_COARSEST_ROWS", "300")
    p = _gen()
    T, src = _transpose(p.rowptr, p.colind, p.nzval)
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    lam, x = vectors(p.flat_len, 3, seed=12)
    with solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, 1, col_i=ci, col_j=cj) as s:
        assert s.get_int("levels") > 1
        t = s.transposed()
        gt = t.value_gradient(lam, x)
        assert_bits(gt, restate(T.indptr, T.indices, lam, x, -1.0))
        gs = s.value_gradient(x, lam)                               # lambda and x swapped on the source
        assert_bits(gs, restate(p.rowptr, p.colind, x, lam, -1.0))
        assert_bits(gt, gs[src])


# ---------------------------------------------------------------- end to end on the golden fixtures
@pytest.fixture(scope="module")
def adjoint(golden):
    """the library's X = A^-1 B and Lambda = A^-T W for two seeded right-hand sides and weight vectors, once per fixture"""
    g = golden
    ci, cj = solver.column_coords(g.ind_i, g.ind_j, g.col_start, g.cnt)
    rng = np.random.default_rng(31)
    B, W = rng.standard_normal((2, g.n)), rng.standard_normal((2, g.n))
    with solver.NkpSolver(g.rowptr, g.colind, g.val, g.blk_start, g.cnt, col_i=ci, col_j=cj, rtol=1e-12, restart=150, max_iters=5000) as s:
        X, _ = s.solve_many(B)
        Lam, _ = s.transposed().solve_many(W)
        grad = s.value_gradient(Lam, X)
    return dict(B=B, W=W, X=X, Lam=Lam, grad=grad)


def test_gradient_of_the_librarys_own_solves_has_the_bits_of_the_formula(golden, adjoint):
    assert_bits(adjoint["grad"], restate(golden.rowptr, golden.colind, adjoint["Lam"], adjoint["X"], -1.0))


@pytest.mark.parametrize("seed", [41, 42, 43])
def test_directional_derivative_against_central_differences(golden, adjoint, seed):
    """L(val) = sum_c w_c . x_c with x_c = A(val)^-1 b_c.  Reference: scipy splu solves of val +- h d, h = 1e-6 max |val|, and the
    central difference of L.  delta_ref is the discrepancy between that difference and scipy's OWN analytic
    - sum lambda_i x_j d_ij; the library's g . d must agree with the difference within 10 delta_ref (one decade for the
    iterative solves' 1e-12 residuals against the direct ones)."""
    g, n = golden, golden.n
    B, W = adjoint["B"], adjoint["W"]
    d = np.random.default_rng(seed).standard_normal(g.val.size)
    h = 1e-6 * np.abs(g.val).max()

    def objective(val):
        lu = spla.splu(sp.csr_matrix((val, g.colind, g.rowptr), shape=(n, n)).tocsc())
        return sum(float(W[c] @ lu.solve(B[c])) for c in range(2))

    central = (objective(g.val + h * d) - objective(g.val - h * d)) / (2.0 * h)
    A = sp.csr_matrix((g.val, g.colind, g.rowptr), shape=(n, n))
    lu, luT = spla.splu(A.tocsc()), spla.splu(A.T.tocsc())
    Xs = np.stack([lu.solve(B[c]) for c in range(2)])
    Ls = np.stack([luT.solve(W[c]) for c in range(2)])
    analytic = float(restate(g.rowptr, g.colind, Ls, Xs, -1.0) @ d)
    delta_ref = abs(central - analytic)
    mine = float(adjoint["grad"] @ d)
    delta = abs(central - mine)
    print(f"{g.name} seed {seed}: central difference {central:.17g}, scipy analytic {analytic:.17g} (delta_ref {delta_ref:.3e}), "
          f"library {mine:.17g} (delta {delta:.3e}, {delta / delta_ref if delta_ref else float('inf'):.3f} delta_ref)")
    assert delta <= 10.0 * delta_ref
    # On these fixtures (cond_1 ~ 1e7) the step the comparison above prescribes is far outside the linear regime, so delta_ref is
    # of the size of the derivative itself.  The sharper statement: the library's g . d against scipy's analytic value.  The
    # solves agree with a direct solve to 1e-7 in the 2-norm at rtol = 1e-12 (the bound of test_solve_matches_superlu_fixture), so
    #   |sum_e d_e (lam_i x_j - lam'_i x'_j)| <= 1e-7 sum_c (|lam_c| . |D| |x_c| scaled by norms), Cauchy-Schwarz per pair
    D = sp.csr_matrix((np.abs(d), g.colind, g.rowptr), shape=(n, n))
    bound = 1e-7 * sum(np.linalg.norm(Ls[c]) * np.linalg.norm(D @ np.abs(Xs[c])) + np.linalg.norm(Xs[c]) * np.linalg.norm(D.T @ np.abs(Ls[c])) for c in range(2))
    print(f"    library against scipy analytic: {abs(mine - analytic):.3e} (bound {bound:.3e}, relative {abs(mine - analytic) / abs(analytic):.3e})")
    assert abs(mine - analytic) <= bound


# ---------------------------------------------------------------- torch
def test_torch_backward_has_the_bits_of_the_calls_it_is_made_of(tmp_path):
    """NkpTorchSolver in a process of its own (torch brings its own HIP runtime along): see tests/torch_value_gradient_worker.py"""
    out = str(tmp_path / "torch.json")
    env = dict(os.environ, NKP_ML_DEVICE_MIN="0", NKP_ML_COARSEST_ROWS="300")
    r = subprocess.run([sys.executable, os.path.join(HERE, "torch_value_gradient_worker.py"), "--out", out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.load(open(out))
    for step in ("first", "second"):
        c = res[step]
        assert c["grad_B_is_transposed_solve"] and c["grad_val_is_value_gradient"] and c["grad_val_is_formula"], c
        assert c["residual"] <= 1e-9 and c["grad_val_shape"] == [res["nnz"]], c
    assert res["second"]["x_changed"] and res["second"]["grad_val_changed"], res["second"]
    assert res["no_grad_for_values"] and res["not_converged_raises"], res
