"""The cycle's glue kernels and the Krylov step's entry on grids that have reached their cap: values, not iteration counts.

red_grid (csrc/blas1.hip) caps every vector kernel's grid at NKP_RED_BLOCKS = 1024 blocks (2048 for the streams launched on
red_grid * 2) of 256 threads, so a stream of one element per thread takes a second pass of its grid-stride loop from
n = 524 289 on, zero_kernel (two elements per thread on 2048 blocks) from n = 1 048 577 on.  The case is the smallest hierarchy
the planner builds whose levels 0 AND 1 are beyond those sizes: kc.case ("lattice1026"), 1026 x 1026 water columns of depth 2
with the last one cut to depth 1, n = 2 105 351 (odd: the scalar tail of the two-per-thread kernels), merged 2 x 2 columns per
level with col_i / col_j: 2 105 351, 526 338, 132 098, 33 282, 8 450, 2 178 rows.  (Without col_i / col_j the graph fallback
merges four rows per step as well: 725 x 725 columns give 1 051 249, 264 134, ... rows, level 1 under the cap.)  The coarsest
size and the hand-over to the device-built levels stay at their defaults: what production runs.

Which test wraps which kernel, and the smallest n that wraps it:
  gather_kernel (launch_gather, launch_scatter)         n > 524 288     (a) level 0, step_glue 12 and 0; (c) step_glue 0
  cycle_entry_kernel (step_glue bit 8)                  n > 524 288     (c) step_glue 12 against step_glue 0 and against kr.fgmres
  restrict_sum_fill_kernel (step_glue bit 4)            nc > 524 288    (a) level 0 -> 1 at step_glue 12
  restrict_sum_kernel                                   nc > 524 288    (a) level 0 -> 1 at step_glue 0
  prolong_add_kernel                                    nf > 524 288    (a) level 1 -> 0 and level 2 -> 1
  zero_kernel (launch_fill, fill_x)                     n > 1 048 576   (a) level 0; level 1 at step_glue 0 is under it
  gather_kernel, restrict_sum, prolong_add, fill at K = 2 (one text for both widths)      (d) against the single solves
  axpby_kernel, vmul_kernel                             n > 524 288     tests/test_gpu_krylov.py at n524291 (its table)

  (a) precond_apply on one fixed vector against the cycle restated in tests/ml_cycle_reference.py on the device's own levels,
      evaluated with the grouped half sweeps (a Python loop over a million columns takes minutes), f64 storage at
      step_glue = 12 and 0, the two bit for bit.  Tolerance: the f64 rule of tests/test_gpu_cycle_options.py,
      max (1e-12, 4096 d) ||z_ref|| with d (LU blocks against explicit inverses) measured on this hierarchy.  With f32 storage
      the two step_glue settings are compared bit for bit only: the yardstick e of the f32 rule needs the LU factors of every
      block rounded to f32, which only the per-column evaluation does, minutes at this size.
  (b) on the CPU: the same cycle restated with one operation truncated at its cap, as a kernel without its stride loop would
      compute it, moves z by at least 1e6 bounds of (a).  At a scaled-down cap on the five-level hierarchy of
      tests/test_ml_cycle_reference.py (2813, 889, 275, 100, 13 rows; caps 512 and 1024: levels 0 and 1 beyond, the rest
      under, as here).  Measured, ||z - z_ref|| / ||z_ref|| and its ratio to the bound of 1.0e-12:
        gather     9.8e-01   9.8e+11
        scatter    9.8e-01   9.8e+11
        restrict   1.6e-01   1.6e+11
        prolong    1.7e-01   1.7e+11
        fill       1.9e-02   1.9e+10      (x of the previous cycle left in the elements the fill skips)
  (c) solve cut at max_iters = 2 (multilevel, f64 basis, restart 20): step_glue = 12 and 0 bit for bit in x, iters and relres;
      the default against kr.fgmres on the solver's own spmv and precond_apply at class f64_cgs1 of krylov_cases.TOL
  (d) solve_many of two right-hand sides cut at k = 2 has the bits of the two single solves

Measured on an MI355X (d = 1.22e-16 on this hierarchy; three levels built on the device), ||z - z_ref|| / ||z_ref|| and its
ratio to the bound, then ||x - x_ref|| / ||x_ref|| of (c) and its ratio to the tolerance of the class:
  lattice1026 / step_glue 12         f64  1.2e-16  bound 1.0e-12  ratio 0.00012
  lattice1026 / step_glue 0          f64  1.2e-16  bound 1.0e-12  ratio 0.00012
  lattice1026-ml-k2-reorth0-f32_0-m20: dx 2.36e-16  tol 2.0e-12  ratio 0.00012; relres 3.236118e-06 / 3.236118e-06 (diff 1.71e-19,
  bound 9.55e-12)
The module takes 5 s there, 2.7 s of it the two f64 solvers, the read-back of the levels and the two reference cycles.
"""
import numpy as np
import pytest

import krylov_cases as kc
import krylov_reference as kr
import ml_cycle_reference as mcr
import ml_reference as mlr
from nk_ocn_tracer_jacobian_precond_amd import solver, synth

gpu = pytest.mark.gpu

CASE = "lattice1026"
CAP = 2 * 1024 * 256                 # one element per thread on red_grid * 2 blocks of B1_THREADS
CAP_FILL = 2 * CAP                   # zero_kernel: two elements per thread
ROWS = [2105351, 526338, 132098, 33282, 8450, 2178]


def check_rows(rows):
    """what the tests below rest on: levels 0 and 1 beyond the caps, an odd n, and a level under both caps left to show that the
    unwrapped launches of the same kernels still work"""
    assert rows[0] > CAP_FILL, rows
    assert rows[1] > CAP, rows
    assert rows[0] % 2 == 1, rows
    assert len(rows) >= 3 and rows[2] <= CAP, rows


def test_the_planner_builds_two_levels_beyond_the_caps():
    """A condition of the whole file (host planner, no GPU): without it the GPU tests wrap nothing."""
    c = kc.case(CASE)
    assert c.n == 1026 * 1026 * 2 - 1 and np.diff(c.blk).max() == 2 and np.diff(c.blk).min() == 1
    rows, _, _ = solver.ml_plan_host(c.rowptr, c.colind, c.val, c.blk, c.col_i, c.col_j)
    rows = [int(v) for v in rows]
    print("rows per level", rows)
    check_rows(rows)
    assert rows == ROWS


# ================================================================ (b) what the tolerance sees
class Truncated(mcr.Glue):
    """One operation as a kernel that lost its grid-stride loop computes it: elements from `cap` on are not touched.  What they
    hold instead is what the buffer held: zeros for a right-hand side, a sum or z, the x of the previous cycle for the fill."""

    def __init__(self, which, cap, cap_fill, stale_x0):
        self.which, self.cap, self.cap_fill, self.stale_x0 = which, cap, cap_fill, stale_x0
        self.hit = 0

    def gather(self, r, perm0):
        out = super().gather(r, perm0)
        if self.which == "gather":
            self.hit += out[self.cap:].size
            out[self.cap:] = 0.0
        return out

    def scatter(self, x, perm0):
        if self.which != "scatter":
            return super().scatter(x, perm0)
        self.hit += x[self.cap:].size
        z = np.zeros_like(x)
        z[perm0[:self.cap]] = x[:self.cap]
        return z

    def restrict(self, l, P, res):
        rc = super().restrict(l, P, res)
        if self.which == "restrict":
            self.hit += rc[self.cap:].size
            rc[self.cap:] = 0.0
        return rc

    def prolong(self, l, P, xc, omega, x):
        if self.which != "prolong":
            return super().prolong(l, P, xc, omega, x)
        self.hit += x[self.cap:].size
        x[:self.cap] += omega * (P @ xc)[:self.cap]

    def fill(self, l, n):
        x = super().fill(l, n)
        if self.which == "fill" and l == 0:
            self.hit += x[self.cap_fill:].size
            x[self.cap_fill:] = self.stale_x0[self.cap_fill:]
        return x


def test_an_operation_truncated_at_its_cap_is_seen():
    """(b) of the module docstring, which records the measured ratios."""
    cap, cap_fill = 512, 1024
    p = synth.generate(24, 20, 10, adv="upwind3", hmix="isop", seed=2)
    colid = np.cumsum(p.ind_k == 0) - 1
    levels = mcr.levels_from_mlr(mlr.build(p.scipy_csr(), p.ind_i.astype(np.int64), p.ind_j.astype(np.int64), p.ind_k.astype(np.int64), colid,
                                           coarsest_rows=60))
    rows = [lv.n for lv in levels]
    assert rows == [2813, 889, 275, 100, 13]
    assert rows[0] > cap_fill and cap < rows[1] <= cap_fill and rows[2] <= cap          # the shape of check_rows at the small caps
    rng = np.random.default_rng(17)
    levels[0].perm0 = rng.permutation(rows[0])
    r, r_before = rng.standard_normal(rows[0]), rng.standard_normal(rows[0])
    ref = mcr.Reference(levels, r, 0, {"default": {}}, grouped=True)
    bound = ref.bound("default")
    assert bound == max(1e-12, 4096 * ref.yard["default"])
    stale_x0 = mcr.cycle(levels, r_before, grouped=True)[levels[0].perm0]              # level 0's x after the cycle before
    assert np.array_equal(mcr.cycle(levels, r, grouped=True, glue=mcr.Glue()), ref.z["default"])
    for which in ("gather", "scatter", "restrict", "prolong", "fill"):
        glue = Truncated(which, cap, cap_fill, stale_x0)
        moved = mcr.relative_difference(mcr.cycle(levels, r, grouped=True, glue=glue), ref.z["default"])
        print("%-10s %.1e   %.1e bounds (bound %.1e)" % (which, moved, moved / bound, bound))
        assert glue.hit > 0, which
        assert moved >= 1e6 * bound, (which, moved, bound)


# ================================================================ the solvers, once per module
class Solvers:
    """kc.case (CASE) under the multilevel preconditioner, one solver per (ml_f32, step_glue), made on first use"""

    def __init__(self):
        self.c = c = kc.case(CASE)
        self.run = kc.Run(CASE, kc.MULTILEVEL, 2, reorth=0, f32=0, restart=20)
        self.options = {k: v for k, v in self.run.options().items() if k != "ml_smooth"}      # the default cycle: three sweeps
        rng = np.random.default_rng(29)
        self.r = rng.standard_normal(c.n)
        self.b2 = rng.standard_normal(c.n)
        self.made = {}

    def get(self, f32, glue):
        if (f32, glue) not in self.made:
            c = self.c
            s = solver.NkpSolver(c.rowptr, c.colind, c.val, c.blk, col_i=c.col_i, col_j=c.col_j, tuning=dict(ml_f32=f32, step_glue=glue), **self.options)
            self.made[f32, glue] = s
            rows = [s.ml_level_array(l, "rowptr").size - 1 for l in range(s.get_int("levels"))]
            print("ml_f32", f32, "step_glue", glue, "rows per level", rows, "levels built on the device", s.get_int("ml_levels_on_device"))
            check_rows(rows)
            assert rows == ROWS
            assert s.get_int("ml_levels_on_device") >= 2            # the big levels are device-built, as in production
        return self.made[f32, glue]

    def close(self):
        for s in self.made.values():
            s.close()
        self.made = {}


@pytest.fixture(scope="module")
def solvers():
    out = Solvers()
    yield out
    out.close()


@pytest.fixture(scope="module")
def reference(solvers):
    """the restated cycle on the device's levels (f64 storage), grouped half sweeps: z_ref and d, once"""
    levels = mcr.levels_from_solver(solvers.get(0, 12))
    assert [lv.n for lv in levels] == ROWS and levels[-1].coarse_inv is not None
    return mcr.Reference(levels, solvers.r, 0, {"default": {}}, grouped=True)


# ================================================================ (a) the cycle
@gpu
def test_precond_apply_matches_the_restated_cycle(solvers, reference):
    z = {glue: solvers.get(0, glue).precond_apply(solvers.r) for glue in (12, 0)}
    again = solvers.get(0, 12).precond_apply(solvers.r)              # on the level vectors the first cycle left
    assert np.isfinite(z[12]).all()
    print("d = %.2e" % reference.yard["default"])
    for glue in (12, 0):
        reference.check("%s / step_glue %d" % (CASE, glue), "default", z[glue])
    # restrict_sum_fill_kernel against restrict_sum_kernel + zero_kernel, cycle for cycle the same doubles (include/nkp.h)
    assert np.array_equal(z[12], z[0]), np.abs(z[12] - z[0]).max()
    assert np.array_equal(z[12], again), np.abs(z[12] - again).max()


@gpu
def test_f32_storage_keeps_its_bits_across_step_glue(solvers):
    z = {glue: solvers.get(1, glue).precond_apply(solvers.r) for glue in (12, 0)}
    assert np.isfinite(z[12]).all() and np.abs(z[12]).max() > 0.0
    assert np.array_equal(z[12], z[0]), np.abs(z[12] - z[0]).max()


# ================================================================ (c) Krylov steps through the wrapped entry
def rel(x, y):
    return float(np.linalg.norm(x - y) / np.linalg.norm(y))


@gpu
def test_two_krylov_steps_through_the_wrapped_entry(solvers):
    c, run = solvers.c, solvers.run
    out = {glue: solvers.get(0, glue).solve(c.b, raise_on_fail=False) for glue in (12, 0)}
    (x, info), (x0, info0) = out[12], out[0]
    assert info["iters"] == info0["iters"] == 2 and info["status"] == info0["status"], (info, info0)
    assert kc.same_bits(x, x0), np.abs(x - x0).max()
    assert kc.same_bits(np.array([info["relres"]]), np.array([info0["relres"]])), (info, info0)
    s = solvers.get(0, 12)
    ref = kc.reference(run, s.spmv, s.precond_apply)
    tol = kc.TOL[run.cls][1]
    assert run.cls == "f64_cgs1"
    dx, bound = rel(x, ref.x), c.relres_bound(ref.x, ref.relres, tol)
    print("MEASURED %s: dx %.2e  tol %.1e  ratio %.2g; relres %.6e / %.6e (diff %.2e, bound %.2e)"
          % (run.id, dx, tol, dx / tol, info["relres"], ref.relres, abs(info["relres"] - ref.relres), bound))
    assert not ref.stagnated and ref.iters == 2 and info["status"] == ref.status, (info, ref.iters, ref.status)
    assert dx <= tol, (dx, tol)
    assert abs(info["relres"] - ref.relres) <= bound, (info["relres"], ref.relres, bound)


# ================================================================ (d) two right-hand sides
@gpu
def test_batched_solve_has_the_bits_of_the_single_solves(solvers):
    c = solvers.c
    s = solvers.get(0, 12)
    B = np.stack([c.b, solvers.b2])
    single = [s.solve(B[q], raise_on_fail=False) for q in range(2)]
    steps = s.get_int("batch_steps")
    X, infos = s.solve_many(B, raise_on_fail=False)
    assert s.get_int("batch_steps") > steps                           # the batched path ran
    for q in range(2):
        x1, i1 = single[q]
        assert infos[q]["iters"] == i1["iters"] == 2 and infos[q]["relres"] == i1["relres"], (q, infos[q], i1)
        assert kc.same_bits(X[q], x1), (q, np.abs(X[q] - x1).max())
