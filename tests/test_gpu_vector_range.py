"""NaN, Inf and vectors whose squared norm leaves the f64 range, through every solve driver (include/nkp.h at nkp_solve, "Vectors
the solve refuses"; csrc/krylov.hip: classify_rhs, fg_begin, bicgstab, fg_restart; csrc/krylov_host.cpp: rhs_verdict;
csrc/blas1.hip: count_entries_kernel, berr_kernel, max_partials_kernel).  No tolerances: statuses, NaN patterns, bit equality.

  (a) test_multi_dot_keeps_nan, test_berr_keeps_nan     a NaN is not lost in any stage of a reduction
  (b) test_refused_and_clean_afterwards                 NaN / +Inf / (+Inf, -Inf) / b 2^520 / b 2^-600 through solve, solve_device, the
                                                        transposed solver and solve_tangent, for every driver configuration: NKP_BREAKDOWN,
                                                        iters 0, relres NaN, berr NaN, x all NaN, NkpError under raise_on_fail
  (c) test_covariance                                   b 2^+-300: the bits of 2^+-300 x, the same iters, relres and berr
  (d) test_batched_columns                              bad, zero and ordinary columns in one solve_many, widths 2, 4 and 8
  (e) (b) again, and test_column_jacobi_confines_nan    after all of (b) and a NaN through spmv and precond_apply, clean calls have
                                                        the bits of a fresh solver; M^-1 of column Jacobi is block diagonal for NaN too

What these tests returned on an MI355X with the library as it was before the right-hand side was classified and berr kept NaN
(56 of the 78 cases failed):
  (a) test_berr_keeps_nan[nan]: x0[0] = NaN gave NKP_BREAKDOWN, relres NaN and berr 1.0 -- the NaN row's quotient became 0 and
      every `q > m ? q : m` dropped it.  [inf]: NKP_NOT_CONVERGED (1) with relres inf and a finite berr.
      test_non_finite_guess_through_the_iteration: NKP_BREAKDOWN with relres NaN, but berr 1.0.
      test_multi_dot_keeps_nan passed: sums keep a NaN by themselves.
  (b) all 42 cases failed at the first call, solve of b with a NaN: status 0 (NKP_OK), iters 0, relres 0.0, berr 1.0, x = 0.
      (Read from the code and reproduced with the restated drivers, tests/test_krylov_reference.py: the same for b 2^520 and
      b 2^-600; with +Inf NKP_OK and relres NaN.)
  (c) test_covariance passed, all ten runs: no absolute constant takes part in an ordinary solve.
  (d) all 10 cases failed: the call with a NaN column returned NKP_OK.
  (e) test_column_jacobi_confines_nan passed under all eight layouts.
"""
import functools

import numpy as np
import pytest

import colsolve_cases as cc
import krylov_cases as kc
import krylov_reference as kr
from nk_ocn_tracer_jacobian_precond_amd import solver
from test_gpu_krylov import Device, make_solver

pytestmark = pytest.mark.gpu

same_bits = kc.same_bits
REFUSED_TEXT = {"nan": "holds a non-finite entry", "inf": "holds a non-finite entry", "inf_pair": "holds a non-finite entry",
                "up520": "is outside the range", "down600": "is outside the range"}


def assert_refused(info, x, where):
    assert info["status"] == kr.BREAKDOWN and info["iters"] == 0, (where, info)
    assert info["relres"] != info["relres"] and info["berr"] != info["berr"], (where, info)
    assert np.isnan(x).all(), (where, int(np.isnan(x).sum()), x.size)


# ---------------------------------------------------------------- (a) reductions
@functools.lru_cache(maxsize=None)
def _dot_operands(n, k):
    rng = np.random.default_rng(300 + n)
    return rng.standard_normal((k, n)), rng.standard_normal(n)


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("n", [513, 2001])
def test_multi_dot_keeps_nan(n, f32):
    """multi_dot_kernel / multi_dot_finish_kernel, k = 9 (two chunks of NKP_DOT_CHUNK): positions 0 and 1 are one thread's pair,
    511 the last element of block 0, 512 the first of block 1, n - 1 the scalar tail of an odd n"""
    k = 9
    V, w = _dot_operands(n, k)
    c = kc.case(f"n{n}")
    with solver.NkpSolver(c.rowptr, c.colind, c.val, None, precond=kc.NONE, restart=20, basis_f32=f32) as s:
        clean = s.multi_dot(V, w)
        assert np.isfinite(clean).all()
        for pos in (0, 1, 511, 512, n - 1):
            wn = w.copy()
            wn[pos] = np.nan
            out = s.multi_dot(V, wn)
            assert np.isnan(out).all(), (n, f32, pos, out)              # every dot, and w.w
            for j in (0, 7, 8):                                          # first and last row of chunk 0, the row of chunk 1
                Vn = V.copy()
                Vn[j, pos] = np.nan
                out = s.multi_dot(Vn, w)
                assert np.isnan(out[j]), (n, f32, pos, j, out)
                keep = np.arange(k + 1) != j
                assert same_bits(out[keep], clean[keep]), (n, f32, pos, j, out, clean)
        # +Inf and -Inf where every row of V is positive: Inf - Inf in each dot, Inf + Inf in w.w
        wi, Vp = w.copy(), V.copy()
        wi[3], wi[n - 1] = np.inf, -np.inf
        Vp[:, [3, n - 1]] = np.abs(Vp[:, [3, n - 1]]) + 0.5
        out = s.multi_dot(Vp, wi)
        assert np.isnan(out[:k]).all() and out[k] == np.inf, (n, f32, out)
        assert same_bits(s.multi_dot(V, w), clean)


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_berr_keeps_nan(bad):
    """berr_kernel / max_partials_kernel on lucky513 (A diagonal, no preconditioner), max_iters = 0 from a guess: r = b - A x0 and
    |A||x0| + |b| are NaN (Inf: -Inf and Inf) in row j alone.  j = 0, 63: the ends of the first wave; 64: the first lane of the
    second; 255: the last thread of block 0; 256, 511: the ends of block 1; 512: the second trip of the grid-stride loop.
    A non-finite guess is NKP_BREAKDOWN with relres NaN (nkp.h)."""
    c = kc.case("lucky513")
    A = c.A
    run = kc.Run("lucky513", kc.NONE, 0, restart=4)
    with make_solver(run) as s, Device(c.b) as d_b:
        with Device(c.exact + 0.25) as d_x:
            info = s.solve_device(d_b.ptr, d_x.ptr, use_guess=True, raise_on_fail=False)
        want = kr.berr(c.b - A @ (c.exact + 0.25), abs(A) @ np.abs(c.exact + 0.25) + np.abs(c.b))
        print(f"clean guess: berr {info['berr']!r}, numpy {want!r}")
        assert info["status"] == kr.NOT_CONVERGED and np.isfinite(info["berr"]) and info["berr"] > 0.0 and np.isfinite(want)
        for j in (0, 63, 64, 255, 256, 511, 512):
            x0 = c.exact + 0.25
            x0[j] = bad
            with np.errstate(invalid="ignore"):
                want = kr.berr(c.b - A @ x0, abs(A) @ np.abs(x0) + np.abs(c.b))
            assert want != want                                      # the rule of the contract, in numpy
            with Device(x0) as d_x:
                info = s.solve_device(d_b.ptr, d_x.ptr, use_guess=True, raise_on_fail=False)
                with pytest.raises(solver.NkpError) as e:
                    s.solve_device(d_b.ptr, d_x.ptr, use_guess=True)
            print(f"x0[{j}] = {bad}: {info}")
            assert e.value.code == kr.BREAKDOWN
            assert info["berr"] != info["berr"], (j, info)
            assert info["status"] == kr.BREAKDOWN and info["iters"] == 0 and info["relres"] != info["relres"], (j, info)


@pytest.mark.parametrize("krylov", ["fgmres", "bicgstab"])
def test_non_finite_guess_through_the_iteration(krylov):
    """the same with iterations allowed and column Jacobi: nothing iterates on a residual that is not a number"""
    c = kc.case("n513")
    run = kc.Run("n513", kc.JACOBI, 5, krylov=krylov, restart=4)
    with make_solver(run) as s, Device(c.b) as d_b:
        for bad in (np.nan, np.inf):
            x0 = kc.guess(c)
            x0[c.n // 2] = bad
            with Device(x0) as d_x:
                info = s.solve_device(d_b.ptr, d_x.ptr, use_guess=True, raise_on_fail=False)
            assert info["status"] == kr.BREAKDOWN and info["iters"] == 0 and info["relres"] != info["relres"] and info["berr"] != info["berr"], (bad, info)
        x, info = s.solve(c.b, raise_on_fail=False)
        with make_solver(run) as fresh:
            x1, info1 = fresh.solve(c.b, raise_on_fail=False)
        assert same_bits(x, x1) and info == info1


# ---------------------------------------------------------------- (b) refusal through every driver, (e) clean afterwards
CONFIGS = ([(f"reorth{ro}-f32_{f32}", dict(reorth=ro, f32=f32)) for ro, f32 in kc.OPTION_PAIRS]
           + [("equil", dict(equil=1)), ("steps2", dict(steps=2)), ("bicgstab", dict(krylov="bicgstab", restart=2))])
PRECONDS = [(kc.NONE, "n513"), (kc.JACOBI, "n2001"), (kc.MULTILEVEL, "n2001")]


def _tuned_solver(run, spmv_diag, **more):
    tuning = dict(kc.ML_TUNING) if run.precond == kc.MULTILEVEL else {}
    if spmv_diag is not None:
        tuning["spmv_diag"] = spmv_diag
    c = kc.case(run.case)
    kw = run.options()
    kw.update(more)
    if run.precond == kc.MULTILEVEL:
        kw.update(col_i=c.col_i, col_j=c.col_j)
    return solver.NkpSolver(c.rowptr, c.colind, c.val, None if run.precond == kc.NONE else c.blk, tuning=tuning, **kw)


def _entry_points(s, n):
    """name -> callable (b, raise_on_fail) -> (x, info) for the four ways into a solve"""
    def host(b, rf):
        return s.solve(b, raise_on_fail=rf)

    def device(b, rf):
        with Device(b) as d_b, Device(np.zeros(n)) as d_x:
            info = s.solve_device(d_b.ptr, d_x.ptr, raise_on_fail=rf)
            return d_x.get(), info

    def transposed(b, rf):
        return s.transposed().solve(b, raise_on_fail=rf)

    def tangent(b, rf):
        dx, infos = s.solve_tangent(np.zeros(n), dB=b, raise_on_fail=rf)
        return dx, infos[0]

    return dict(solve=host, solve_device=device, transposed=transposed, solve_tangent=tangent)


def _clean_calls(s, c):
    """what a solver gives on clean data: A v, M v, a solve, a transposed solve, a tangent"""
    v = kc.guess(c)
    out = [s.spmv(v), s.precond_apply(v)]
    for name, call in _entry_points(s, c.n).items():
        x, info = call(c.b, False)
        out += [x, np.array([info["status"], info["iters"], info["relres"], info["berr"]])]
    return out


@pytest.mark.parametrize("spmv_diag", [None, 0], ids=["default", "csr"])
@pytest.mark.parametrize("config", CONFIGS, ids=[name for name, _ in CONFIGS])
@pytest.mark.parametrize("precond,case", PRECONDS, ids=["none", "jacobi", "ml"])
def test_refused_and_clean_afterwards(precond, case, config, spmv_diag):
    c = kc.case(case)
    run = kc.Run(case, precond, None, **dict(dict(restart=8), **config[1]))
    with _tuned_solver(run, spmv_diag) as fresh:
        want = _clean_calls(fresh, c)
    assert want[3][0] == kr.OK and want[3][1] > 0                       # [status, iters, ..] of the clean host solve: it iterates
    with _tuned_solver(run, spmv_diag) as s:
        # default tuning keeps A on per-column diagonals wherever the solver knows the water columns (padded +0.0 slots: nkp.h)
        assert s.get_int("spmv_diag") == (1 if spmv_diag is None and precond != kc.NONE else 0)
        entries = _entry_points(s, c.n)
        for what in kc.BAD_RHS:
            b = kc.bad_rhs(c.b, what)
            for name, call in entries.items():
                x, info = call(b, False)
                assert_refused(info, x, (what, name))
                with pytest.raises(solver.NkpError) as e:
                    call(b, True)
                assert e.value.code == kr.BREAKDOWN and REFUSED_TEXT[what] in str(e.value), (what, name, str(e.value))
        # a NaN through the operator and the preconditioner alone: work vectors, halo slots and level vectors have held it
        v = kc.guess(c)
        v[c.n // 3] = np.nan
        assert np.isnan(s.spmv(v)).any() and np.isnan(s.precond_apply(v)).any()
        got = _clean_calls(s, c)
    for q, (a, b) in enumerate(zip(got, want)):
        assert same_bits(a, b), (q, a, b)


# ---------------------------------------------------------------- (c) covariance
@pytest.mark.parametrize("run", kc.full_runs() + [r for r in kc.bicgstab_runs() if r.k is None], ids=lambda r: r.id)
def test_covariance(run):
    """b 2^e, e = +-300, is inside the range, and a power of two on b is the same power of two on every vector of the solve: the
    bits of 2^e x, the same iteration count, the same bits of relres and berr.  No absolute constant takes part in an ordinary solve
    (the 1.0e300 of berr_kernel stands for a residual over a zero denominator and the 2^-480 floor of the target is 180 binary
    orders away)."""
    c = kc.case(run.case)
    with make_solver(run) as s:
        x, info = s.solve(c.b, raise_on_fail=False)
        assert info["status"] == kr.OK
        for e in (300, -300):
            xe, ie = s.solve(np.ldexp(c.b, e), raise_on_fail=False)
            print(f"{run.id} 2^{e}: {ie} / {info}")
            assert (ie["status"], ie["iters"]) == (info["status"], info["iters"]), (run, e, ie, info)
            assert same_bits(xe, np.ldexp(x, e)), (run, e, float(np.abs(np.ldexp(xe, -e) - x).max()))
            assert same_bits(np.array([ie["relres"], ie["berr"]]), np.array([info["relres"], info["berr"]])), (run, e, ie, info)


# ---------------------------------------------------------------- (d) batches
def _columns(c, ordinary, width):
    """the calls of one width: lists of (tag, column); an int tag is the index of an ordinary column"""
    nan, zero, down = kc.bad_rhs(c.b, "nan"), np.zeros(c.n), kc.bad_rhs(c.b, "down600")
    if width == 2:
        return [[("nan", nan), (0, ordinary[0])], [(1, ordinary[1]), ("zero", zero)], [("down600", down), (2, ordinary[2])]]
    if width == 4:
        return [[(0, ordinary[0]), ("nan", nan), ("zero", zero), ("down600", down)]]
    return [[(0, ordinary[0]), ("nan", nan), (1, ordinary[1]), ("zero", zero), ("down600", down), (2, ordinary[2])]]


BATCH_MODES = {"plain": (dict(), dict()), "equil-steps2": (dict(equil=1, steps=2), dict()), "spmv_rows0": (dict(), dict(batch_spmv_rows=0)),
               "clone": (dict(), dict()), "basis_f32": (dict(f32=1), dict())}


@pytest.mark.parametrize("mode", sorted(BATCH_MODES))
@pytest.mark.parametrize("precond", [kc.JACOBI, kc.MULTILEVEL], ids=["jacobi", "ml"])
def test_batched_columns(precond, mode):
    """solve_many of 2, 4 and 6 (rhs_batch = 8) right-hand sides of which one holds a NaN, one is zero and one is b 2^-600: the
    ordinary columns have the bits of their single solves, b = 0 gives x = 0 with relres 0, the bad ones are refused, and the call
    returns NKP_BREAKDOWN.  A clone and an f32 basis take their columns one at a time, with the same answers."""
    c = kc.case("n2001")
    opts, tuning = BATCH_MODES[mode]
    run = kc.Run("n2001", precond, None, **dict(dict(restart=8), **opts))
    batched = mode not in ("clone", "basis_f32")
    rng = np.random.default_rng(23)
    ordinary = [c.b, rng.standard_normal(c.n), 1e-3 * rng.standard_normal(c.n)]
    for width in (2, 4, 8):
        tune = dict(tuning, **(dict(kc.ML_TUNING) if precond == kc.MULTILEVEL else {}))
        if width == 8:
            tune["rhs_batch"] = 8
        kw = run.options()
        if precond == kc.MULTILEVEL:
            kw.update(col_i=c.col_i, col_j=c.col_j)
        with solver.NkpSolver(c.rowptr, c.colind, c.val, c.blk, tuning=tune, **kw) as parent:
            s = parent.clone() if mode == "clone" else parent
            try:
                single = [s.solve(b, raise_on_fail=False) for b in ordinary]
                assert all(i["status"] == kr.OK and i["iters"] > 0 for _, i in single)
                for cols in _columns(c, ordinary, width):
                    steps = parent.get_int("batch_steps")
                    B = np.stack([b for _, b in cols])
                    X, infos = s.solve_many(B, raise_on_fail=False)
                    assert (parent.get_int("batch_steps") > steps) == batched, (width, mode)
                    refused = any(tag in kc.BAD_RHS for tag, _ in cols)
                    if refused:
                        with pytest.raises(solver.NkpError) as e:
                            s.solve_many(B)
                        assert e.value.code == kr.BREAKDOWN
                    for q, (tag, _) in enumerate(cols):
                        i = infos[q]
                        assert i["status"] == (kr.BREAKDOWN if refused else kr.OK)      # the call's status: the worst column's
                        if tag == "zero":
                            assert not X[q].any() and i["iters"] == 0 and i["relres"] == 0.0 and i["berr"] == 0.0, (width, q, i)
                        elif isinstance(tag, str):
                            assert_refused(i, X[q], (width, tag))
                        else:
                            x1, i1 = single[tag]
                            assert same_bits(X[q], x1), (width, mode, q, float(np.abs(X[q] - x1).max()))
                            assert i["iters"] == i1["iters"] and same_bits(np.array([i["relres"], i["berr"]]), np.array([i1["relres"], i1["berr"]])), (width, q, i, i1)
                # and afterwards the members' work vectors give clean columns their bits again
                X, infos = s.solve_many(np.stack(ordinary[:2]), raise_on_fail=False)
                assert all(same_bits(X[q], single[q][0]) and infos[q]["iters"] == single[q][1]["iters"] for q in range(2))
            finally:
                if s is not parent:
                    s.close()


# ---------------------------------------------------------------- (e) column Jacobi confines a NaN to its water column
@pytest.mark.parametrize("layout", cc.JACOBI_LAYOUTS)
def test_column_jacobi_confines_nan(layout):
    """M^-1 of column Jacobi is block diagonal: a NaN in one water column of r makes NaN inside that column's block of M^-1 r and
    nowhere else, whatever layout packs several columns into one wave, group or LDS tile; every other block keeps its bits"""
    grid, band, km = cc.GRID_BIG, 4, 60
    p = cc.problem(grid, km, band)
    blk = cc.column_blocks(p)
    r = np.random.default_rng(9).standard_normal(p.flat_len)
    nblk = blk.size - 1
    with solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, precond=solver.PRECOND_COLUMN_JACOBI, tuning=cc.FAMILIES[layout], restart=4) as s:
        clean = s.precond_apply(r)
        assert np.isfinite(clean).all()
        for col in (0, 1, nblk // 2, 31, 32, nblk - 1):                # first, a neighbour in its group, the ends of a group of 32, last
            a, b = int(blk[col]), int(blk[col + 1])
            for row in sorted({a, (a + b) // 2, b - 1}):
                rn = r.copy()
                rn[row] = np.nan
                z = s.precond_apply(rn)
                bad = np.flatnonzero(np.isnan(z))
                assert bad.size and a <= bad.min() and bad.max() < b and np.isnan(z[row]), (layout, col, row, a, b, bad[:8])
                outside = np.r_[0:a, b:p.flat_len]
                assert same_bits(z[outside], clean[outside]), (layout, col, row)
        assert same_bits(s.precond_apply(r), clean)
