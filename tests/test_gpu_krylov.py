"""The Krylov drivers (csrc/krylov.hip: fg_begin, fg_restart, fg_post_step, fg_end_cycle, fgmres, bicgstab) and their vector
kernels (csrc/blas1.hip:47-486) step by step against the drivers restated in tests/krylov_reference.py, on the shapes of
tests/krylov_cases.py.

The restatement runs on the host with the solver's own spmv and precond_apply as operators (both pinned elsewhere), so the
only thing that differs between the two sides is the driver and its vector kernels.  A solve cut at max_iters = k returns x_k,
which GMRES fixes uniquely: the comparison is at the tolerance of the run's class in krylov_cases.TOL (100 times what two
correct implementations differ by, measured on the CPU in tests/test_krylov_reference.py), orders of magnitude below what a
dropped tail element, a skipped basis vector or a mis-taken f32 copy changes (shown there too).

Which test reaches which kernel of blas1.hip, and the smallest n of the suite at which the kernel's grid has reached its cap and
its grid-stride loop takes a second pass (red_grid: 1024 blocks of 256 threads for the kernels of two elements per thread,
2048 for the streams of one element per thread; both wrap from n = 524 289 on, zero_kernel from n = 1 048 577 on):
  multi_dot_kernel <double> / <float>, multi_dot_finish_kernel     test_multi_dot, test_truncated (f64 / f32 basis); wrapped at
                                                                    n524291; 64 chunks in grid.y: test_multi_dot_at_the_restart_clamp
  update_w_kernel <double> / <float>, sum_partials_kernel          test_truncated (also as launch_axpy_multi: x += Z y); wrapped at
                                                                    n524291; k = 510 of hs[NKP_MAX_K = 512]: test_restart_clamp_cycle
  scale_to_kernel (f64, and its f32 twin yf)                       test_truncated; wrapped at n524291
  finish_column_kernel (plain norm, h += h2)                       test_truncated (reorth 0 / 1)
  finish_column_pythagoras_kernel                                  test_gpu_krylov_dist.py (one reduction per step)
  dot_kernel                                                       test_truncated (||b||, true residuals), test_bicgstab; wrapped at
                                                                    n524291
  axpby_kernel                                                     test_bicgstab (every call form of the driver), test_truncated with
                                                                    precond_steps = 2 (the defect correction between two cycles);
                                                                    wrapped at n524291-jacobi-k2-bicgstab and n524291-...-steps2
  vmul_kernel                                                      test_truncated with equil (on w, on v_j, on the restart residual);
                                                                    wrapped at n524291_rows-...-equil
  zero_kernel                                                      test_truncated (b = 0 in test_zero_rhs; bicgstab's p, v: two
                                                                    passes of 2048 blocks only from n = 1 048 577 on, which
                                                                    tests/test_gpu_grid_caps.py reaches on its level 0; at n524291
                                                                    the grid is at its cap and every thread has its pair)
  berr_kernel, max_partials_kernel                                 every solve () (info["berr"]), checked in test_full_solves
  count_entries_kernel, and NaN / Inf through the above            test_gpu_vector_range.py
  multi_dot_group, multi_dot_finish_group, update_w_group, sum_partials_group, scale_to_group, finish_column_group
                                                                    test_batched_bits (against the single solves); wrapped at n524291
  gather_kernel, cycle_entry_kernel, restrict_sum_kernel, restrict_sum_fill_kernel, prolong_add_kernel (the cycle's glue)
                                                                    tests/test_gpu_grid_caps.py (its table), wrapped at n = 2 105 351

Measured on an MI355X, ||dx|| / ||x|| and its share of the tolerance of the class, for the runs on wrapped grids and at the clamp:
  n524291-jacobi-k2-bicgstab                          0          (tolerance 1.5e-13)
  n524291-jacobi-k2-*-steps2 (four option pairs)      at most 6.8e-17 with an f32 basis (2e-8 of the tolerance), 7.3e-19 with an
                                                      f64 basis (1.5e-6 of it)
  n524291_rows-jacobi-k2-*-equil (two option pairs)   at most 4.0e-18 = 4e-6 of 1.0e-12
  diag1025-none-k510-reorth1-f32_0-m510               1.66e-12 = 0.33 % of 5.0e-10; relres 5.321964e-03 on both sides (diff 4.1e-14)
  multi_dot at k = 505 and 511, restart 510 and 100000 (clamped): worst error 0.000 of its bound with an f64 basis, 0.065 with an
  f32 basis; w.w 0.004 of its bound
"""
import ctypes
import functools

import numpy as np
import pytest

import krylov_cases as kc
import krylov_reference as kr
import oracle_binding as ora
from nk_ocn_tracer_jacobian_precond_amd import solver

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def make_solver(run, **more):
    c = kc.case(run.case)
    kw = run.options()
    kw.update(more)
    if run.precond == kc.MULTILEVEL:
        kw.update(col_i=c.col_i, col_j=c.col_j, tuning=dict(kc.ML_TUNING))
    return solver.NkpSolver(c.rowptr, c.colind, c.val, None if run.precond == kc.NONE else c.blk, **kw)


def rel(x, y):
    d = np.linalg.norm(y)
    return float(np.linalg.norm(x - y) / d) if d > 0 else float(np.linalg.norm(x - y))


class Device:
    """a float64 array on the device through the HIP runtime the library links (as tests/test_gpu_spmv_shapes.py does: an
    `import torch` here would bring a second runtime into the process)"""

    def __init__(self, a):
        self.hip = ctypes.CDLL("libamdhip64.so")
        a = np.ascontiguousarray(a, np.float64)
        self.size, self.p = a.size, ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(self.p), ctypes.c_size_t(a.nbytes)) == 0
        assert self.hip.hipMemcpy(self.p, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.nbytes), 1) == 0           # host to device
        self.ptr = self.p.value

    def get(self):
        out = np.empty(self.size)
        assert self.hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), self.p, ctypes.c_size_t(out.nbytes), 2) == 0       # device to host
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.hip.hipFree(self.p)


def check(run, x0=None):
    """One solve on the device against the restatement on the same operators; returns (reference, info, x) for further checks."""
    c = kc.case(run.case)
    tol = kc.TOL[run.cls][1]
    with make_solver(run) as s:
        ref = kc.reference(run, s.spmv, s.precond_apply, x0=x0)
        if x0 is None:
            x, info = s.solve(c.b, raise_on_fail=False)
        else:
            with Device(c.b) as d_b, Device(x0) as d_x:
                info = s.solve_device(d_b.ptr, d_x.ptr, use_guess=True, raise_on_fail=False)
                x = d_x.get()
    dx, bound = rel(x, ref.x), c.relres_bound(ref.x, ref.relres, tol)
    print(f"{run.id}: iters {info['iters']} / {ref.iters}, status {info['status']} / {ref.status}, dx {dx:.2e} (tol {tol:.1e}), "
          f"relres {info['relres']:.6e} / {ref.relres:.6e} (diff {abs(info['relres'] - ref.relres):.2e}, bound {bound:.2e})")
    assert not ref.stagnated
    assert info["iters"] == ref.iters, (run, info, ref.iters)
    assert info["status"] == ref.status, (run, info, ref.status)
    assert dx <= tol, (run, dx, tol)
    assert abs(info["relres"] - ref.relres) <= bound, (run, info["relres"], ref.relres, bound)
    return ref, info, x


# ---------------------------------------------------------------- truncated solves
@pytest.mark.parametrize("run", kc.truncated_runs(), ids=lambda r: r.id)
def test_truncated(run):
    ref, info, _ = check(run)
    assert info["iters"] == run.k


def test_start_from_a_guess():
    run = kc.Run("n2001", kc.JACOBI, 5, reorth=0, f32=1)
    ref, info, _ = check(run, x0=kc.guess(kc.case(run.case)))
    assert info["iters"] == 5


def test_zero_rhs():
    """fg_begin and bicgstab with b = 0: x = 0 after no iteration, whatever the start vector was"""
    c = kc.case("n513")
    for krylov in ("fgmres", "bicgstab"):
        with make_solver(kc.Run("n513", kc.JACOBI, 5, krylov=krylov, restart=4)) as s:
            x, info = s.solve(np.zeros(c.n))
        assert info["iters"] == 0 and info["status"] == 0 and info["relres"] == 0.0 and not x.any()


# ---------------------------------------------------------------- full solves
def margins(run, ref):
    """no host decision of the restated solve within 1000 tolerances of its threshold: the device takes the same ones"""
    tol = kc.TOL[run.cls][1]
    worst = min(ref.log, key=lambda d: d.dist)
    print(f"{run.id}: closest decision {worst.kind} at {worst.its}: {worst.dist:.2e} = {worst.dist / tol:.1e} tolerances")
    assert worst.dist >= 1000.0 * tol, (run, worst)


@pytest.mark.parametrize("run", kc.full_runs(), ids=lambda r: r.id)
def test_full_solves(run):
    c = kc.case(run.case)
    ref, info, x = check(run)
    assert ref.status == kr.OK and info["relres"] <= run.rtol
    margins(run, ref)
    # berr_kernel / max_partials_kernel: max_i |r_i| / (|A||x| + |b|)_i; either side evaluates r_i within (len_i + 2) 2^-52 of
    # the denominator, whatever the order of the sum
    be = ora.berr(c.rowptr, c.colind, c.val, x, c.b)
    assert abs(info["berr"] - be) <= 2.0 * (np.diff(c.rowptr).max() + 2) * 2.0 ** -52 + 1e-14 * be, (run, info["berr"], be)
    if run is kc.INNER_SCALE_RUN or run.id == kc.INNER_SCALE_RUN.id:
        assert ref.inner_scale < 1.0
    if c.exact is not None:
        # lucky breakdown: the Krylov space closes at step 3 and x is the exact solution to rounding
        assert ref.iters == 3
        assert rel(x, c.exact) <= 64 * 2.0 ** -52


# ---------------------------------------------------------------- BiCGStab
@pytest.mark.parametrize("run", kc.bicgstab_runs(), ids=lambda r: r.id)
def test_bicgstab(run):
    ref, info, _ = check(run)
    if run.k is None:
        assert ref.status == kr.OK
        margins(run, ref)
    else:
        assert info["iters"] == run.k


def test_bicgstab_needs_restart_2():
    c = kc.case("n513")
    with solver.NkpSolver(c.rowptr, c.colind, c.val, c.blk, precond=kc.JACOBI, krylov=solver.KRYLOV_BICGSTAB, restart=1) as s:
        with pytest.raises(solver.NkpError) as e:
            s.solve(c.b)
    assert e.value.code < 0 and "restart >= 2" in str(e.value)


# ---------------------------------------------------------------- nkp_multi_dot directly
@functools.lru_cache(maxsize=None)
def _dot_operands(n, kmax):
    rng = np.random.default_rng(100 + n % 97)
    return rng.standard_normal((kmax, n)), rng.standard_normal(n)


def _ld_dot(x, y):
    return np.dot(np.asarray(x, np.longdouble), np.asarray(y, np.longdouble))


@pytest.mark.parametrize("n", [1, 2, 3, 511, 513, 2001, 524291])
def test_multi_dot(n):
    restart = 20
    V, w = _dot_operands(n, restart + 1)
    c = kc.case(f"n{n}")
    gamma = (n + 2) * U / (1.0 - (n + 2) * U)
    wn = float(np.sqrt(_ld_dot(w, w)))
    for f32 in (0, 1):
        Vr = V.astype(np.float32) if f32 else V        # what the kernel reads
        exact = np.array([float(_ld_dot(V[j], w)) for j in range(restart + 1)])
        exact_r = np.array([float(_ld_dot(Vr[j], w)) for j in range(restart + 1)])
        vn = np.array([float(np.sqrt(_ld_dot(V[j], V[j]))) for j in range(restart + 1)])
        with solver.NkpSolver(c.rowptr, c.colind, c.val, None, precond=kc.NONE, restart=restart, basis_f32=f32) as s:
            for k in (0, 1, 7, 8, 9, 16, 17, restart + 1):
                out = s.multi_dot(V[:k], w)
                again = s.multi_dot(V[:k], w)
                assert out.shape == (k + 1,)
                assert np.array_equal(out.view(np.uint64), again.view(np.uint64)), (n, f32, k)
                err = np.abs(out[:k] - exact[:k])
                bound = (gamma + (2.0 ** -24 if f32 else 0.0)) * vn[:k] * wn
                worst = float((err / bound).max()) if k else 0.0
                print(f"multi_dot n {n} f32 {f32} k {k}: worst error / bound {worst:.3f}, w.w error {abs(out[k] - wn * wn) / (gamma * wn * wn):.3f} of its bound")
                assert np.all(err <= bound), (n, f32, k, err, bound)
                # against the operands as the kernel reads them the rounding of V is no part of the bound
                assert np.all(np.abs(out[:k] - exact_r[:k]) <= gamma * vn[:k] * (1.0 + 2.0 ** -24) * wn), (n, f32, k)
                assert abs(out[k] - wn * wn) <= gamma * wn * wn, (n, f32, k)          # slot k is w.w


@pytest.mark.parametrize("restart", [kc.RESTART_CLAMP, 100000], ids=lambda m: f"restart{m}")
def test_multi_dot_at_the_restart_clamp(restart):
    """nkp_create clamps restart to NKP_MAX_K - 2 = 510 and does not refuse a longer one.  k = 511 = m + 1 is 64 chunks of
    NKP_DOT_CHUNK in grid.y, the last one with 7 vectors, and fills `partial` and h_dev () as create.hip sizes them; k = 505 ends
    on a chunk of one vector.  k = 512 is beyond the basis of either solver."""
    n, m = 513, kc.RESTART_CLAMP
    V, w = _dot_operands(n, m + 2)
    c = kc.case(f"n{n}")
    gamma = (n + 2) * U / (1.0 - (n + 2) * U)
    wn = float(np.sqrt(_ld_dot(w, w)))
    exact = np.array([float(_ld_dot(V[j], w)) for j in range(m + 1)])
    vn = np.array([float(np.sqrt(_ld_dot(V[j], V[j]))) for j in range(m + 1)])
    for f32 in (0, 1):
        Vr = V.astype(np.float32) if f32 else V        # what the kernel reads
        exact_r = np.array([float(_ld_dot(Vr[j], w)) for j in range(m + 1)])
        with solver.NkpSolver(c.rowptr, c.colind, c.val, None, precond=kc.NONE, restart=restart, basis_f32=f32) as s:
            for k in (505, m + 1):
                out = s.multi_dot(V[:k], w)
                again = s.multi_dot(V[:k], w)
                assert out.shape == (k + 1,)
                assert np.array_equal(out.view(np.uint64), again.view(np.uint64)), (restart, f32, k)
                err = np.abs(out[:k] - exact[:k])
                bound = (gamma + (2.0 ** -24 if f32 else 0.0)) * vn[:k] * wn
                print(f"multi_dot restart {restart} f32 {f32} k {k}: worst error / bound {float((err / bound).max()):.3f}, "
                      f"w.w error {abs(out[k] - wn * wn) / (gamma * wn * wn):.3f} of its bound")
                assert np.all(err <= bound), (restart, f32, k, err, bound)
                assert np.all(np.abs(out[:k] - exact_r[:k]) <= gamma * vn[:k] * (1.0 + 2.0 ** -24) * wn), (restart, f32, k)
                assert abs(out[k] - wn * wn) <= gamma * wn * wn, (restart, f32, k)          # slot k is w.w
            with pytest.raises(solver.NkpError) as e:
                s.multi_dot(V[:m + 2], w)
            assert e.value.code == -1 and "restart+1" in str(e.value), (restart, f32, e.value)          # NKP_EINVAL


# ---------------------------------------------------------------- one restart cycle of the longest length
@pytest.mark.parametrize("run", kc.clamp_runs(), ids=lambda r: r.id)
def test_restart_clamp_cycle(run):
    """update_w_kernel with k = 1 .. 510 and launch_axpy_multi with k = 510 (kc.clamp_runs: the case still uses its last basis
    vector); a solver asked for a longer restart is the same solver"""
    c = kc.case(run.case)
    ref, info, x = check(run)
    assert info["iters"] == run.k == kc.RESTART_CLAMP and info["status"] == kr.NOT_CONVERGED
    with make_solver(run, restart=100000) as s:
        x2, info2 = s.solve(c.b, raise_on_fail=False)
    assert kc.same_bits(x, x2) and info2["iters"] == info["iters"] and info2["relres"] == info["relres"], (info, info2)


# ---------------------------------------------------------------- batched
@pytest.mark.parametrize("name,reorth", [("n513", 0), ("n513", 1), ("n2001", 0), ("n2001", 1), ("n524291", 0)])
def test_batched_bits(name, reorth):
    """solve_many with K = 2 and 3 right-hand sides has the bits of the single solves (the *_group kernels against their single
    twins, which test_truncated pins against the restatement), cut at k = 9."""
    c = kc.case(name)
    rng = np.random.default_rng(17)
    B = np.stack([c.b, rng.standard_normal(c.n), 1e-3 * rng.standard_normal(c.n)])
    run = kc.Run(name, kc.JACOBI, 9, reorth=reorth, f32=0)
    with make_solver(run) as s:
        single = [s.solve(B[q], raise_on_fail=False) for q in range(3)]
        for K in (2, 3):
            steps = s.get_int("batch_steps")
            X, infos = s.solve_many(B[:K], raise_on_fail=False)
            assert s.get_int("batch_steps") > steps            # the batched path ran
            for q in range(K):
                x1, i1 = single[q]
                assert infos[q]["iters"] == i1["iters"] == 9 and infos[q]["relres"] == i1["relres"], (name, K, q, infos[q], i1)
                assert np.array_equal(X[q].view(np.uint64), x1.view(np.uint64)), (name, K, q, np.abs(X[q] - x1).max())
