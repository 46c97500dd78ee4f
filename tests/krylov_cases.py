"""Shapes, matrices and tolerances of the Krylov-driver tests -- TEST INFRASTRUCTURE.

Tolerances.  What two correct implementations differ by was measured on the CPU (tests/test_krylov_reference.py: the restated
drivers with longdouble accumulation, with plain f64 accumulation in reversed order and, where it restates the mode,
ora.fgmres; operators ora.spmv and ora.colblock_apply), as the largest ||dx|| / ||x|| over the runs of a class; the GPU
comparison allows 100 times that (FMA contraction, the reduction tree):

  class      basis, Gram-Schmidt passes      measured   at                                        in TOL    tolerance
  f64_cgs1   f64, one                        1.77e-14   n524291-jacobi-k9-reorth0-f32_0-m20       2.0e-14   2.0e-12
  f64_cgs2   f64, two                        4.86e-15   n524291-none-k2-reorth1-f32_0-m20         5.0e-15   5.0e-13
  f32_cgs1   f32, one                        4.75e-11   n513-none-k17-reorth0-f32_1-m20           5.0e-11   5.0e-09
  f32_cgs2   f32, two                        3.24e-11   n513-none-k17-reorth1-f32_1-m20           3.5e-11   3.5e-09
  equil      row equilibration (any basis)   9.57e-15   n524291_rows-jacobi-k2-reorth0-f32_0-m20  1.0e-14   1.0e-12
  bicgstab   BiCGStab                        1.32e-15   n2001-jacobi-k1-bicgstab                  1.5e-15   1.5e-13
  clamp510   f64, two, one cycle of 510      4.97e-12   diag1025-none-k510-reorth1-f32_0-m510     5.0e-12   5.0e-10

(An f32 basis is orthonormal to 6e-8 only; by k = 17 without a preconditioner that has grown into 5e-11 of x.  Below k = 10 the
f32 classes measure 5e-15.  The equil class measured 3.96e-15 at n2001_rows-jacobi-k9-reorth0-f32_1-m20 before the runs on
n524291_rows joined it.)  Measured on an MI355X, the largest ||dx|| / ||x|| of a run is 1.5 % of its tolerance.

Matrices.  column_grid (n, seed): ragged water columns (1 .. 12 rows) on a lattice, rows numbered column by column; a row
couples to its vertical neighbours and to the same level of the four neighbouring columns with positive, unsymmetric entries
and a_ii = -((1 + shift) sum_j |a_ij| + (0.05 .. 0.15)): the sign convention of a tracer tendency Jacobian (what the
hierarchy's low-order twin expects), -A a strictly diagonally dominant M-matrix, so every preconditioner of the library works on it and restart 30 needs a few tens of iterations to 1e-10.  The last column is cut so that n is met exactly.
column_lattice (ni, nj, seed): the same matrix on ni x nj columns of one depth (2), the last one a row shorter.

Sizes, from the kernels of csrc/blas1.hip (B1_THREADS = 256, two elements per thread):
  n = 1, 2, 3          one element; the scalar tail of an odd n (i + 1 < n fails); a pair and a tail
  n = 511, 513         one block of 512 elements short of one, and just over (a second block with one element)
  n = 2001             ld = (n + 63) & ~63 = 2048 padding, four blocks, odd tail
  n = 524 291          red_grid caps at NKP_RED_BLOCKS = 1024 blocks of 512 elements = 524 288: the first odd n whose
                       grid-stride loop takes a second pass; the streams of one element per thread (axpby, vmul, gather) run
                       on twice as many blocks and wrap at the same n
  k = 1, 3, 4, 5, 8, 9, 16, 17   update_w unrolls by 4 (remainders 1, 3, 0, 1); NKP_DOT_CHUNK = 8 gives one chunk, two, three
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

NONE, JACOBI, MULTILEVEL = 0, 1, 3            # solver.PRECOND_*
OPTION_PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1)]          # (reorth, basis_f32)


class Case:
    def __init__(self, name, A, blk, b, col_i=None, col_j=None, exact=None):
        A = sp.csr_matrix(A)
        A.sort_indices()
        self.name, self.A = name, A
        self.n = A.shape[0]
        self.rowptr, self.colind, self.val = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)
        self.blk = np.asarray(blk, np.int32)
        self.b = b
        self.col_i, self.col_j = col_i, col_j
        self.exact = exact

    def norm2_bound(self):
        """||A||_2 <= sqrt (||A||_1 ||A||_inf)"""
        a = abs(self.A)
        return float(np.sqrt(a.sum(0).max() * a.sum(1).max()))

    def residual_eval_error(self, x):
        """2-norm of the rounding bound of one evaluation of b - A x: (len_i + 2) 2^-52 (|A||x| + |b|)_i per row, as
        spmv_shapes.Exact.e"""
        d = abs(self.A) @ np.abs(x) + np.abs(self.b)
        return float(np.linalg.norm((np.diff(self.A.indptr) + 2) * 2.0 ** -52 * d))

    def relres_bound(self, x_ref, relres_ref, tol):
        """|relres - relres_ref| of two solves whose x differ by at most tol ||x_ref||: (||A|| ||dx|| + the rounding of the two
        evaluations of b - A x) / ||b|| + the rounding of the two norms (gamma_n in any summation order)."""
        bn = np.linalg.norm(self.b)
        return ((self.norm2_bound() * tol * np.linalg.norm(x_ref) + 2.0 * self.residual_eval_error(x_ref)) / bn
                + 2.0 * (self.n + 2) * 2.0 ** -53 * relres_ref)


def _columns_matrix(depths, ni, rng, shift):
    """(A, blk_start, col_i, col_j) of water columns of the given depths, ni to a lattice row (module docstring)."""
    ncol = depths.size
    n = int(depths.sum())
    blk = np.concatenate([[0], np.cumsum(depths)]).astype(np.int64)
    col_of = np.repeat(np.arange(ncol), depths)
    rows = np.arange(n)
    lev = rows - blk[col_of]
    R, C, V = [], [], []

    def add(mask, cols, lo, hi):
        R.append(rows[mask])
        C.append(cols[mask])
        V.append(rng.uniform(lo, hi, size=int(mask.sum())))

    add(lev > 0, rows - 1, 0.5, 1.5)
    add(lev < depths[col_of] - 1, rows + 1, 0.5, 1.5)
    for dc in (-1, 1, -ni, ni):
        c2 = col_of + dc
        ok = (c2 >= 0) & (c2 < ncol)
        if abs(dc) == 1:
            ok &= (np.clip(c2, 0, ncol - 1) // ni) == (col_of // ni)
        c2c = np.clip(c2, 0, ncol - 1)
        ok &= lev < depths[c2c]
        add(ok, blk[c2c] + lev, 0.1, 0.6)
    R, C, V = np.concatenate(R), np.concatenate(C), np.concatenate(V)
    off = np.bincount(R, weights=np.abs(V), minlength=n)
    diag = -((1.0 + shift) * off + rng.uniform(0.05, 0.15, size=n))
    A = sp.csr_matrix((np.concatenate([V, diag]), (np.concatenate([R, rows]), np.concatenate([C, rows]))), shape=(n, n))
    cols = np.arange(ncol)
    return A, blk.astype(np.int32), (cols % ni).astype(np.int32), (cols // ni).astype(np.int32)


def column_grid(n, seed, shift=0.35, kmax=12):
    """(A, blk_start, col_i, col_j) of the module docstring."""
    rng = np.random.default_rng(seed)
    depths = rng.integers(1, kmax + 1, size=n)
    ends = np.cumsum(depths)
    ncol = int(np.searchsorted(ends, n)) + 1
    depths = depths[:ncol].copy()
    depths[-1] -= ends[ncol - 1] - n
    return _columns_matrix(depths, max(1, int(np.sqrt(ncol))), rng, shift)


def column_lattice(ni, nj, seed, shift=0.35, depth=2):
    """column_grid's matrix on ni x nj water columns of one depth, the last column cut to depth - 1: n = ni nj depth - 1, odd
    for an even depth (the scalar tail of the kernels that take two elements per thread).  The smallest shape whose hierarchy
    has two levels beyond the grid caps of csrc/blas1.hip (tests/test_gpu_grid_caps.py)."""
    depths = np.full(ni * nj, depth, np.int64)
    depths[-1] -= 1
    return _columns_matrix(depths, ni, np.random.default_rng(seed), shift)


# ---------------------------------------------------------------- the matrices
SHIFT = 0.15          # restart 30 to 1e-10: 54 iterations without preconditioner, 25 with column Jacobi (n = 513 and 2001)


def _rhs(n, seed):
    b = np.random.default_rng(seed).standard_normal(n)
    b[b == 0.0] = 1.0
    return b


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "lucky513":
        # A diagonal with exactly three distinct values, b with a component in every eigenspace: the Krylov space closes at step 3
        n = 513
        d = np.array([1.0, 2.5, 4.0])[np.arange(n) % 3]
        b = _rhs(n, 31)
        return Case(name, sp.diags(d).tocsr(), np.arange(n + 1), b, exact=b / d)
    if name in ("n2001_rows", "n524291_rows"):
        # the rows of n2001 (n524291) scaled by 10^(-2 .. 2): what row equilibration is for
        base = case(name[:-len("_rows")])
        D = 10.0 ** np.random.default_rng(41).uniform(-2.0, 2.0, size=base.n)
        return Case(name, sp.diags(D) @ base.A, base.blk, D * base.b, base.col_i, base.col_j)
    if name == "n2001_fast":
        # more dominant: column Jacobi converges in 17 iterations, so that eight steps gain five digits and the recurrence of an
        # f32 basis with one Gram-Schmidt pass runs 1e-4 ahead of the true residual (INNER_SCALE_RUN)
        A, blk, ci, cj = column_grid(2001, seed=7, shift=0.6)
        return Case(name, A, blk, _rhs(2001, 1), ci, cj)
    if name == "diag1025":
        # a diagonal of 1025 values spread geometrically over six decades, b with a component in every one: GMRES (510) is still
        # converging at step 510 (relres 5e-3), so the last basis vectors carry weight in x (clamp_runs)
        n = 1025
        return Case(name, sp.diags(np.geomspace(1.0, 1.0e6, n)).tocsr(), np.arange(n + 1), _rhs(n, 31))
    if name == "lattice1026":
        # 1026 x 1026 columns of depth 2, the last one of depth 1: n = 2 105 351 (odd).  With col_i / col_j the hierarchy merges
        # 2 x 2 columns per level: 526 338 rows on level 1, both beyond the grid caps (tests/test_gpu_grid_caps.py)
        A, blk, ci, cj = column_lattice(1026, 1026, seed=7, shift=SHIFT)
        return Case(name, A, blk, _rhs(A.shape[0], 1), ci, cj)
    n = int(name[1:])
    A, blk, ci, cj = column_grid(n, seed=7, shift=SHIFT)
    return Case(name, A, blk, _rhs(n, 1), ci, cj)


def guess(c):
    """The start vector of the use_guess case: not zero, not near the solution."""
    return np.random.default_rng(5).standard_normal(c.n)


# ---------------------------------------------------------------- vectors no solve accepts (include/nkp.h at nkp_solve)
# name -> what it does to a right-hand side.  The positions sit in different 512-element blocks of the reductions where n allows.
BAD_RHS = ["nan", "inf", "inf_pair", "up520", "down600"]


def bad_rhs(b, kind):
    """b with one NaN, one +Inf, a +Inf and a -Inf, or scaled by 2^520 (||b||^2 overflows) or 2^-600 (every square underflows)"""
    b = np.array(b, np.float64)
    n = b.size
    if kind == "nan":
        b[n // 3] = np.nan
    elif kind == "inf":
        b[n // 3] = np.inf
    elif kind == "inf_pair":
        b[n // 3], b[n - 1] = np.inf, -np.inf
    elif kind == "up520":
        b = np.ldexp(b, 520)
    elif kind == "down600":
        b = np.ldexp(b, -600)
    else:
        raise ValueError(kind)
    return b


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


# several levels on 2001 rows, and one smoothing sweep per half cycle: FGMRES then takes 9 iterations to 1e-10 (5 with two
# chained cycles, BiCGStab 5), so that a cut at k = 5 is still a cut
ML_TUNING = dict(ml_coarsest_rows=60)
ML_SMOOTH = 1


class Run:
    """One solve: case, preconditioner, options and where it is cut (k = None: to convergence)."""

    def __init__(self, case, precond, k, reorth=0, f32=0, equil=0, steps=1, restart=20, krylov="fgmres", rtol=1e-10, cls=None):
        self.case, self.precond, self.k, self.reorth, self.f32 = case, precond, k, reorth, f32
        self.equil, self.steps, self.restart, self.krylov, self.rtol = equil, steps, restart, krylov, rtol
        self.own_cls = cls

    @property
    def max_iters(self):
        return 500 if self.k is None else self.k

    @property
    def cls(self):
        if self.own_cls:
            return self.own_cls
        if self.krylov == "bicgstab":
            return "bicgstab"
        if self.equil:
            return "equil"
        return ("f32" if self.f32 else "f64") + ("_cgs2" if self.reorth else "_cgs1")

    @property
    def id(self):
        p = {NONE: "none", JACOBI: "jacobi", MULTILEVEL: "ml"}[self.precond]
        s = f"{self.case}-{p}-" + ("full" if self.k is None else f"k{self.k}")
        if self.krylov == "bicgstab":
            return s + "-bicgstab" + (f"-steps{self.steps}" if self.steps > 1 else "")
        s += f"-reorth{self.reorth}-f32_{self.f32}-m{self.restart}"
        return s + ("-equil" if self.equil else "") + (f"-steps{self.steps}" if self.steps > 1 else "")

    def __repr__(self):
        return self.id

    def options(self):
        """nkp_options of the solver of this run"""
        o = dict(precond=self.precond, restart=self.restart, max_iters=self.max_iters, rtol=self.rtol, atol=0.0,
                 krylov=1 if self.krylov == "bicgstab" else 0, precond_steps=self.steps)
        if self.precond == MULTILEVEL:
            o["ml_smooth"] = ML_SMOOTH
        if self.krylov == "fgmres":
            o.update(reorth=self.reorth, basis_f32=self.f32, equil=1 if self.equil else -1)
        return o


def truncated_runs():
    """Every (case, options, k) of the truncated solves (module docstring; every row value with every (reorth, basis_f32))."""
    runs = []

    def pairs(case, precond, ks, which=OPTION_PAIRS, **kw):
        runs.extend(Run(case, precond, k, reorth=ro, f32=f32, **kw) for k in ks for ro, f32 in which)

    # n = 1: the space closes at k = 1; n = 2, 3: k below n.  Column Jacobi on one water column is the exact inverse: one step
    pairs("n1", NONE, [1])
    pairs("n2", NONE, [1])
    pairs("n3", NONE, [1, 2])
    pairs("n3", JACOBI, [1], [(0, 0), (1, 1)])
    pairs("n513", JACOBI, [1, 3, 4, 5, 8, 9, 16, 17])
    pairs("n513", NONE, [4, 9, 17])
    pairs("n511", JACOBI, [5, 16])
    pairs("n2001", JACOBI, [1, 3, 8, 17])
    pairs("n2001", MULTILEVEL, [3, 4, 5])
    pairs("n2001_rows", JACOBI, [4, 9], equil=1)
    pairs("n2001_rows", MULTILEVEL, [5], [(0, 0), (1, 1)], equil=1)
    pairs("n2001", JACOBI, [4, 9], steps=2)
    pairs("n2001", MULTILEVEL, [3], [(0, 1), (1, 0)], steps=2)
    pairs("n2001", JACOBI, [9, 17], restart=4)              # cut inside the third and the fifth restart cycle
    pairs("n524291", JACOBI, [9])
    pairs("n524291", NONE, [2], [(0, 1), (1, 0)])
    # the streams of one element per thread (axpby_kernel, vmul_kernel) on a grid of 2 * NKP_RED_BLOCKS blocks wrap from
    # n = 524 289 on: the defect-correction axpby of chained cycles, and row equilibration on w, on v_j and on the restart residual
    pairs("n524291", JACOBI, [2], steps=2)
    pairs("n524291_rows", JACOBI, [2], [(0, 0), (1, 1)], equil=1)
    return runs


# reorth = 0, basis_f32 = 1, restart 8.  After 16 iterations the recurrence says 9.845606e-11 ||b|| and the true residual is
# 9.846765e-11 ||b||; rtol sits between the two, so the second cycle ends on the estimate, the restart finds the true residual
# above the target, sets inner_scale = 0.5 est / beta < 1 and the solve ends one step later (test_krylov_reference.py checks it).
INNER_SCALE_RUN = Run("n2001_fast", JACOBI, None, 0, 1, restart=8, rtol=9.8462e-11)


def full_runs():
    """Solves to 1e-10."""
    return [Run("n513", NONE, None, 0, 0, restart=30),
            Run("n2001", JACOBI, None, 1, 0, restart=30),
            Run("n2001", JACOBI, None, 1, 1, restart=4),
            Run("n2001", MULTILEVEL, None, 0, 1, restart=30),
            Run("n2001_rows", JACOBI, None, 0, 0, equil=1, restart=30),
            Run("n2001", JACOBI, None, 1, 0, steps=2, restart=30),
            INNER_SCALE_RUN,
            Run("lucky513", NONE, None, 1, 0, restart=30)]


def bicgstab_runs():
    runs = [Run("n2001", JACOBI, k, krylov="bicgstab", restart=2) for k in (1, 2, 3, 5, None)]
    runs += [Run("n2001", MULTILEVEL, k, krylov="bicgstab", restart=2) for k in (1, 2, 3, None)]
    runs.append(Run("n513", JACOBI, 3, krylov="bicgstab", restart=2, steps=2))
    runs.append(Run("n524291", JACOBI, 2, krylov="bicgstab", restart=2))          # axpby_kernel in every call form, launch_fill of p and v, wrapped
    return runs


RESTART_CLAMP = 510          # NKP_MAX_K - 2 (csrc/create.hip, check_arguments)


def clamp_runs():
    """One restart cycle of the longest length nkp_create allows, run to its end: update_w_kernel and launch_axpy_multi with
    k = 510 (hs[NKP_MAX_K]), 64 multi-dot chunks.  rtol is out of reach but inside the range of a solve (rtol = 0 is refused:
    a target below 2^-480).  Candidates measured on the CPU (largest ||dx|| / ||x|| between the two arithmetics of
    tests/test_krylov_reference.py; what leaving basis vector 509 out of the update of w changes in x):
      n513, n2001 (column_grid, no preconditioner)      2.3e-16, 2.2e-16    0       at rounding level by step 100
      diagonal 1 .. 513 linear, n = 513                 6.3e-16             0       at rounding level before step 300
      diagonal 1 .. 1e6 geometric, n = 513              3.7e-12             0       at rounding level before step 500
      diagonal 1 .. 1e9 geometric, n = 513              9.2e-10             0       at rounding level before step 500
      diagonal 1 .. 1e6 geometric, n = 2001             3.3e-12             3.0e-3  relres 0.11 at step 510
      diagonal 1 .. 1e6 geometric, n = 1025             3.3e-12             3.7e-4  relres 5.3e-3 at step 510: taken (diag1025)
    Every one is determined to better than 1e-8; only the last two still use their last basis vectors."""
    return [Run("diag1025", NONE, RESTART_CLAMP, reorth=1, f32=0, restart=RESTART_CLAMP, rtol=1e-100, cls="clamp510")]


def reference(run, A, M, arith=None, pythagoras=False, x0=None):
    """The restated driver of tests/krylov_reference.py on the operators A and M with the options of `run`."""
    import krylov_reference as kr
    c = case(run.case)
    if run.krylov == "bicgstab":
        return kr.bicgstab(A, M, c.b, x0, max_iters=run.max_iters, rtol=run.rtol, precond_steps=run.steps, arith=arith)
    rs, ri = kr.row_equilibration(c.rowptr, c.val) if run.equil else (None, None)
    return kr.fgmres(A, M, c.b, x0, restart=run.restart, max_iters=run.max_iters, rtol=run.rtol, reorth=run.reorth, basis_f32=run.f32,
                     rscale=rs, rinv=ri, precond_steps=run.steps, pythagoras=pythagoras, arith=arith)


# class -> (largest relative difference in x of two correct implementations, measured on the CPU by
# tests/test_krylov_reference.py; the tolerance of the GPU comparison = 100 x that)
TOL = {
    "f64_cgs1": (2.0e-14, 2.0e-12),
    "f64_cgs2": (5.0e-15, 5.0e-13),
    "f32_cgs1": (5.0e-11, 5.0e-09),
    "f32_cgs2": (3.5e-11, 3.5e-09),
    "equil": (1.0e-14, 1.0e-12),
    "bicgstab": (1.5e-15, 1.5e-13),
    "clamp510": (5.0e-12, 5.0e-10),
}


def dist_one_rank_runs():
    """One rank forced distributed, column Jacobi: cut at k = 4 and 9, one full solve, the lucky breakdown.

    The full solve restarts every 8 steps.  With one reduction per step the norm of the new direction is sqrt (w.w - sum h^2),
    which is the norm only as far as the basis is orthonormal; one Gram-Schmidt pass loses orthogonality with the square of
    the residual reduction inside a cycle, and from a reduction of about 1e-8 on (restart 30 reaches it at step 19) the two
    summation orders of tests/test_krylov_reference.py take different paths (26 and 30 iterations): no implementation is
    determined to rounding there.  Cycles of 8 steps gain 3 digits each and stay determined."""
    return ([Run("n2001", JACOBI, k, reorth=0, f32=f32) for k in (4, 9) for f32 in (0, 1)] + [Run("n2001", JACOBI, 9, reorth=1, f32=0)]
            + [Run("n2001", JACOBI, None, 0, 0, restart=8), Run("lucky513", NONE, None, 0, 0, restart=30)])


def dist_two_rank_runs():
    return [Run("n2001", JACOBI, 9, reorth=ro, f32=f32) for ro, f32 in ((0, 0), (1, 1))]
