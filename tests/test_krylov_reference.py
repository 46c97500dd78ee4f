"""The restated Krylov drivers of tests/krylov_reference.py pinned on the CPU, with the oracle's operators (ora.spmv,
ora.colblock_apply, the oracle's multilevel cycle): against ora.fgmres, against the dense minimal-residual solution, on the
lucky breakdown, against three deliberately wrong variants, and the margins of every host decision of the full solves.

The noise that the tolerance table of tests/krylov_cases.py is built from is measured here: the largest relative difference in x
between (a) the restatement with longdouble accumulation, (b) the same with plain f64 accumulation in reversed order and (c),
where ora.fgmres restates the mode, ora.fgmres."""
import functools

import numpy as np
import pytest

import krylov_cases as kc
import krylov_reference as kr
import oracle_binding as ora

def oracle_operators(c, precond):
    A = lambda x: ora.spmv(c.rowptr, c.colind, c.val, x)
    if precond == kc.NONE:
        return A, (lambda r: r.copy())
    if precond == kc.JACOBI:
        bw, _, _ = ora.colblock_measure(c.rowptr, c.colind, c.val, c.blk)
        P = 1 if bw <= 1 else 2 if bw <= 2 else 4
        fac, _ = ora.colblock_factor(c.rowptr, c.colind, c.val, c.blk, P)
        return A, (lambda r: ora.colblock_apply(c.n, c.blk, P, fac, r))
    raise ValueError("the oracle has no twin of the library's hierarchy: multilevel runs are compared on the GPU only")


def rel(x, y):
    d = np.linalg.norm(y)
    return float(np.linalg.norm(x - y) / d) if d > 0 else float(np.linalg.norm(x - y))


@functools.lru_cache(maxsize=None)
def solved(run, arith=None):
    c = kc.case(run.case)
    A, M = oracle_operators(c, run.precond)
    return kc.reference(run, A, M, arith=arith)


def oracle_restates(run):
    return run.krylov == "fgmres" and run.reorth == 1 and run.f32 == 0 and not run.equil and run.steps == 1 and run.precond != kc.MULTILEVEL


def ora_fgmres(run):
    c = kc.case(run.case)
    return ora.fgmres(c.rowptr, c.colind, c.val, c.blk, c.b, precond=1 if run.precond == kc.JACOBI else 0, restart=run.restart,
                      max_iters=run.max_iters, rtol=run.rtol)


REVERSED = kr.ReversedF64()


def noise(run):
    a, b = solved(run), solved(run, REVERSED)
    d = rel(b.x, a.x)
    if oracle_restates(run):
        xo, _ = ora_fgmres(run)
        d = max(d, rel(xo, a.x), rel(xo, b.x))
    return d


ALL_RUNS = kc.truncated_runs() + kc.full_runs() + kc.bicgstab_runs() + kc.clamp_runs()
CPU_RUNS = [r for r in ALL_RUNS if r.precond != kc.MULTILEVEL]          # the oracle has no twin of the library's hierarchy
CLASSES = sorted(kc.TOL)
TABLE_K = [1, 3, 4, 5, 8, 9, 16, 17]


# ---------------------------------------------------------------- the tolerance table
@pytest.mark.parametrize("cls", CLASSES)
def test_measured_noise_is_what_the_table_says(cls):
    runs = [r for r in CPU_RUNS if r.cls == cls]
    assert runs
    worst, where = max((noise(r), r.id) for r in runs)
    measured, tol = kc.TOL[cls]
    print(f"{cls}: largest relative difference in x {worst:.2e} ({where}); table: measured {measured:.1e}, tolerance {tol:.1e}")
    assert tol == pytest.approx(100.0 * measured, rel=1e-12)
    assert worst <= tol / 100.0
    assert worst >= measured / 4.0                 # the table holds what was measured, not a loose guess
    if cls.startswith("f64"):
        assert tol <= 1e-11


def test_every_row_value_meets_every_option_pair():
    runs = kc.truncated_runs()
    rows = {("n", r.case.split("_")[0]) for r in runs} | {("k", r.k) for r in runs} | {("precond", r.precond) for r in runs}
    rows |= {("equil", r.equil) for r in runs} | {("steps", r.steps) for r in runs} | {("restart4", r.restart == 4) for r in runs}
    assert {f"n{n}" for n in (1, 2, 3, 511, 513, 2001, 524291)} <= {v for kind, v in rows if kind == "n"}
    assert set(TABLE_K) <= {v for kind, v in rows if kind == "k"}
    key = dict(n=lambda r: r.case.split("_")[0], k=lambda r: r.k, precond=lambda r: r.precond, equil=lambda r: r.equil,
               steps=lambda r: r.steps, restart4=lambda r: r.restart == 4)
    for kind, v in rows:
        if kind == "k" and v not in TABLE_K:
            continue
        got = {(r.reorth, r.f32) for r in runs if key[kind](r) == v}
        assert got == set(kc.OPTION_PAIRS), (kind, v, got)
    for r in runs:
        if r.case == "n524291":
            assert r.k <= 9 and r.precond in (kc.NONE, kc.JACOBI)


# ---------------------------------------------------------------- against the oracle's port
@pytest.mark.parametrize("restart", [20, 4])
@pytest.mark.parametrize("precond", [kc.NONE, kc.JACOBI])
def test_truncated_against_the_oracle(precond, restart):
    for k in TABLE_K:
        run = kc.Run("n2001", precond, k, reorth=1, f32=0, restart=restart)
        a = solved(run)
        xo, io = ora_fgmres(run)
        assert a.iters == io["iters"] == k and a.status == io["status"]
        assert rel(a.x, xo) <= kc.TOL["f64_cgs2"][1] / 100.0, (run, rel(a.x, xo))
        assert abs(a.relres - io["relres"]) <= kc.case(run.case).relres_bound(a.x, a.relres, kc.TOL["f64_cgs2"][1] / 100.0)


@pytest.mark.parametrize("run", [r for r in kc.full_runs() if oracle_restates(r)], ids=lambda r: r.id)
def test_full_solves_take_the_oracles_iterations(run):
    a = solved(run)
    xo, io = ora_fgmres(run)
    assert a.iters == io["iters"] and a.status == io["status"] == kr.OK
    assert rel(a.x, xo) <= kc.TOL[run.cls][1] / 100.0


# ---------------------------------------------------------------- x_k is the minimal-residual solution
def _orthonormalise(cols):
    """modified Gram-Schmidt, twice, in longdouble: Q, R with cols = Q R"""
    k = len(cols)
    Q, R = [], np.zeros((k, k), np.longdouble)
    for j, c in enumerate(cols):
        q = np.asarray(c, np.longdouble).copy()
        for _ in range(2):
            for i in range(j):
                t = np.dot(Q[i], q)
                R[i, j] += t
                q -= t * Q[i]
        R[j, j] = np.sqrt(np.dot(q, q))
        Q.append(q / R[j, j])
    return Q, R


def minimal_residual(run):
    """x = M R^-1 K y with y the minimiser of ||R b - (R A M R^-1) K y|| over an orthonormal basis K of the Krylov space of
    R A M R^-1 and R b, by dense least squares in longdouble (R = 1 without equilibration)."""
    c = kc.case(run.case)
    A, M1 = oracle_operators(c, run.precond)
    M = kr.chained_precond(A, M1, run.steps)
    rs, ri = kr.row_equilibration(c.rowptr, c.val) if run.equil else (np.ones(c.n), np.ones(c.n))
    B = lambda v: rs * A(M(ri * v))
    rb = rs * c.b
    K, W = [], []
    q = np.asarray(rb, np.longdouble)
    for j in range(run.k):
        for _ in range(2):
            for p in K:
                q = q - np.dot(np.asarray(p, np.longdouble), q) * np.asarray(p, np.longdouble)
        q = (q / np.sqrt(np.dot(q, q))).astype(np.float64)            # the basis vector the operator is applied to
        K.append(q)
        W.append(B(q))
        q = np.asarray(W[-1], np.longdouble)
    Q, R = _orthonormalise(W)
    g = np.array([np.dot(Q[i], np.asarray(rb, np.longdouble)) for i in range(run.k)], np.longdouble)
    y = np.zeros(run.k, np.longdouble)
    for i in range(run.k - 1, -1, -1):
        y[i] = (g[i] - np.dot(R[i, i + 1:], y[i + 1:])) / R[i, i]
    v = sum(y[i] * np.asarray(K[i], np.longdouble) for i in range(run.k))
    return M(ri * np.asarray(v, np.float64))


MINRES_RUNS = [r for r in kc.truncated_runs() if r.precond != kc.MULTILEVEL and r.f32 == 0 and r.k <= 9 and r.restart >= r.k
               and kc.case(r.case).n <= 2001 and r.k <= kc.case(r.case).n]


@pytest.mark.parametrize("run", MINRES_RUNS, ids=lambda r: r.id)
def test_truncated_solve_is_the_minimal_residual_solution(run):
    a = solved(run)
    x = minimal_residual(run)
    d = rel(a.x, x)
    print(f"{run.id}: {d:.2e}")
    assert a.iters == run.k
    assert d <= kc.TOL[run.cls][1]


# ---------------------------------------------------------------- lucky breakdown
@pytest.mark.parametrize("reorth", [0, 1])
def test_lucky_breakdown_plain(reorth):
    c = kc.case("lucky513")
    A, M = oracle_operators(c, kc.NONE)
    a = kr.fgmres(A, M, c.b, restart=30, max_iters=500, rtol=1e-10, reorth=reorth)
    est = [d for d in a.log if d.kind == "estimate"]
    assert a.iters == 3 and a.status == kr.OK and len(est) == 3
    assert est[-1].taken and est[-1].lhs <= 1e-13 * np.linalg.norm(c.b)       # ends on h_{j+1,j} ~ 0: the estimate drops to rounding
    assert [d.taken for d in est[:-1]] == [False, False]
    assert rel(a.x, c.exact) <= 64 * 2.0 ** -52


def test_lucky_breakdown_pythagoras():
    c = kc.case("lucky513")
    A, M = oracle_operators(c, kc.NONE)
    a = kr.fgmres(A, M, c.b, restart=30, max_iters=500, rtol=1e-10, reorth=0, pythagoras=True)
    weak = [d for d in a.log if d.kind == "weak"]
    assert a.iters == 3 and a.status == kr.OK
    assert [d.taken for d in weak] == [False, False, True]                    # the weak mark ends the cycle at step 3
    assert rel(a.x, c.exact) <= 64 * 2.0 ** -52


def test_pythagoras_is_the_plain_norm_where_it_has_digits():
    run = kc.Run("n2001", kc.JACOBI, 9)
    c = kc.case(run.case)
    A, M = oracle_operators(c, run.precond)
    a, p = solved(run), kc.reference(run, A, M, pythagoras=True)
    assert p.iters == 9 and not any(d.taken for d in p.log if d.kind == "weak")
    assert rel(p.x, a.x) <= 1e-9          # sqrt (w.w - sum h^2) loses log10 (w.w / result) digits of 16, here at most 7


# ---------------------------------------------------------------- the comparison can fail
class DropsLastElement(kr.Arith):
    def dot(self, x, y):
        return super().dot(x[:-1], y[:-1])


class SkipsVector8(kr.Arith):
    def update(self, w, V, h, sign=-1.0):
        if sign > 0.0 or len(V) <= 8:
            return super().update(w, V, h, sign)
        keep = [j for j in range(len(V)) if j != 8]
        return super().update(w, [V[j] for j in keep], [h[j] for j in keep], sign)


class F32CopyOfUnscaledW(kr.Arith):
    def scale_to(self, w, a, f32):
        y = a * w
        with np.errstate(over="ignore"):           # the iteration diverges
            return y, (w.astype(np.float32) if f32 else None)


# A dropped tail element changes a dot product by one part in n: at n = 3 that is a third of it, and the runs on n = 3 see it
# by far more than 1000 tolerances; at n = 513 FGMRES hides most of it (x_17 moves by 4e-10 with an f64 basis, hundreds of
# tolerances, but only ten with an f32 basis), which is why the table of sizes starts at n = 1, 2, 3 and why test_multi_dot
# checks the dots themselves at every n.  A skipped basis vector and a mis-taken f32 copy need k > 8 and are shown at k = 17.
SENSITIVITY_RUNS = ([(kc.Run("n3", kc.NONE, 2, reorth=ro, f32=f32), DropsLastElement) for ro, f32 in kc.OPTION_PAIRS]
                    + [(kc.Run(name, kc.JACOBI, 17, reorth=ro, f32=f32), wrong) for name in ("n513", "n2001") for ro, f32 in kc.OPTION_PAIRS
                       for wrong in [SkipsVector8] + ([F32CopyOfUnscaledW] if f32 else [])])


@pytest.mark.parametrize("run,wrong", SENSITIVITY_RUNS, ids=lambda v: v.id if isinstance(v, kc.Run) else v.__name__)
def test_wrong_restatements_are_seen(run, wrong):
    assert run.id in {r.id for r in kc.truncated_runs()}          # a run of the GPU comparison
    a = solved(run)
    tol = kc.TOL[run.cls][1]
    c = kc.case(run.case)
    A, M = oracle_operators(c, run.precond)
    d = rel(kc.reference(run, A, M, arith=wrong()).x, a.x)
    print(f"{run.id} {wrong.__name__}: {d:.2e} = {d / tol:.1e} tolerances")
    assert d > 1000.0 * tol, (run, wrong.__name__, d, tol)


class SkipsVector509(kr.Arith):
    def update(self, w, V, h, sign=-1.0):
        if len(V) <= 509:
            return super().update(w, V, h, sign)
        keep = [j for j in range(len(V)) if j != 509]
        return super().update(w, [V[j] for j in keep], [h[j] for j in keep], sign)


def test_the_restart_clamp_case_is_determined_and_uses_its_last_vector():
    """kc.clamp_runs: x_510 is determined to better than 1e-8 between the arithmetics, the cycle runs to its end without
    converging, and basis vector 509 (the last one update_w_kernel reads at k = 510) left out of the update of w and of
    x += Z y moves x by 3.7e-4: more than a thousand tolerances of the class"""
    (run,) = kc.clamp_runs()
    c = kc.case(run.case)
    assert run.k == run.restart == kc.RESTART_CLAMP and np.unique(c.val).size == c.n >= kc.RESTART_CLAMP + 1
    a = solved(run)
    assert a.iters == run.k and a.status == kr.NOT_CONVERGED and a.relres > 1e-3
    assert [d.taken for d in a.log if d.kind == "estimate"] == [False] * run.k
    assert noise(run) <= 1e-8
    A, M = oracle_operators(c, run.precond)
    d = rel(kc.reference(run, A, M, arith=SkipsVector509()).x, a.x)
    print(f"{run.id} without basis vector 509: {d:.2e} = {d / kc.TOL[run.cls][1]:.1e} tolerances")
    assert d > 1000.0 * kc.TOL[run.cls][1]


# ---------------------------------------------------------------- no decision within rounding of its threshold
@pytest.mark.parametrize("run", [r for r in kc.full_runs() + kc.bicgstab_runs() if r.k is None and r.precond != kc.MULTILEVEL], ids=lambda r: r.id)
def test_decision_margins(run):
    a = solved(run)
    tol = kc.TOL[run.cls][1]
    assert a.status == kr.OK and not a.stagnated and a.log
    worst = min(a.log, key=lambda d: d.dist)
    print(f"{run.id}: {a.iters} iterations, closest decision {worst.kind} at {worst.its}: {worst.dist:.2e} = {worst.dist / tol:.1e} tolerances")
    assert worst.dist >= 1000.0 * tol, (run, worst)


def test_the_inner_scale_case_walks_that_path():
    a = solved(kc.INNER_SCALE_RUN)
    assert a.status == kr.OK and a.inner_scale < 1.0
    ended = [d for d in a.log if d.kind == "estimate" and d.taken]
    assert len(ended) == 2 and ended[0].its == 16          # the second cycle ends on the estimate, the true residual disagrees


def test_zero_rhs_and_guess():
    c = kc.case("n513")
    A, M = oracle_operators(c, kc.JACOBI)
    for r in (kr.fgmres(A, M, np.zeros(c.n), kc.guess(c), restart=4, max_iters=5), kr.bicgstab(A, M, np.zeros(c.n), kc.guess(c), max_iters=5)):
        assert r.iters == 0 and r.status == kr.OK and not r.x.any()
    run = kc.Run("n513", kc.JACOBI, 5)
    g = kc.reference(run, A, M, x0=kc.guess(c))
    assert g.iters == 5 and rel(g.x, solved(run).x) > 1e-3        # another Krylov space


@pytest.mark.parametrize("run", [r for r in kc.dist_one_rank_runs() if not r.reorth], ids=lambda r: r.id)
def test_pythagoras_epilogue_stays_within_the_class_noise(run):
    """what tests/test_gpu_krylov_dist.py compares under one reduction per step: the two summation orders agree as closely with
    the norm taken as sqrt (w.w - sum h^2) as the table says for the class, and take the same decisions"""
    c = kc.case(run.case)
    A, M = oracle_operators(c, run.precond)
    a, b = kc.reference(run, A, M, pythagoras=True), kc.reference(run, A, M, pythagoras=True, arith=REVERSED)
    d = rel(b.x, a.x)
    print(f"{run.id}: {d:.2e}, closest decision {min(x.dist for x in a.log):.2e}")
    assert (a.iters, a.status) == (b.iters, b.status)
    if c.exact is None:          # (the sign of the rounding left of w.w - sum h^2 at the breakdown is anybody's: weak or exactly zero)
        assert [x.taken for x in a.log] == [x.taken for x in b.log]
    assert d <= kc.TOL[run.cls][1] / 100.0
    if run.k is None:
        assert a.status == kr.OK and min(x.dist for x in a.log) >= 1000.0 * kc.TOL[run.cls][1]


# ---------------------------------------------------------------- vectors outside the range of a solve (include/nkp.h at nkp_solve)
RANGE_RUNS = [kc.Run("n2001", kc.JACOBI, None, ro, f32, restart=8) for ro, f32 in kc.OPTION_PAIRS] + [kc.Run("n2001", kc.JACOBI, None, krylov="bicgstab", restart=2)]


def _solve_scaled(run, b):
    c = kc.case(run.case)
    A, M = oracle_operators(c, run.precond)
    with np.errstate(all="ignore"):
        if run.krylov == "bicgstab":
            return kr.bicgstab(A, M, b, max_iters=run.max_iters, rtol=run.rtol)
        return kr.fgmres(A, M, b, restart=run.restart, max_iters=run.max_iters, rtol=run.rtol, reorth=run.reorth, basis_f32=run.f32)


@pytest.mark.parametrize("run", RANGE_RUNS, ids=lambda r: r.id)
def test_a_power_of_two_on_b_is_a_power_of_two_on_x(run):
    """b 2^e with e = +-300 is inside the range: every product and sum of the solve scales exactly, so x has the bits of
    2^e x, with the same iteration count and the same bits of relres.  No absolute constant enters a decision."""
    c = kc.case(run.case)
    plain = solved(run)
    assert plain.status == kr.OK and plain.iters > 8
    for e in (300, -300):
        r = _solve_scaled(run, np.ldexp(c.b, e))
        assert (r.status, r.iters) == (plain.status, plain.iters), (run, e, r.iters, plain.iters)
        assert kc.same_bits(r.x, np.ldexp(plain.x, e)), (run, e)
        assert kc.same_bits(np.array([r.relres]), np.array([plain.relres])), (run, e, r.relres, plain.relres)


@pytest.mark.parametrize("what", kc.BAD_RHS + ["down520", "up600"])
@pytest.mark.parametrize("run", RANGE_RUNS, ids=lambda r: r.id)
def test_a_right_hand_side_outside_the_range_is_refused(run, what):
    """NaN, Inf, ||b||^2 beyond f64, a target below 2^-480: NKP_BREAKDOWN before any iteration, relres NaN, x all NaN -- where the
    drivers used to return x = 0 with NKP_OK (NaN, 2^520, 2^-600), relres NaN with NKP_OK (Inf), or NKP_OK two iterations
    early on a subnormal ||r||^2 (2^-520)"""
    c = kc.case(run.case)
    b = np.ldexp(c.b, {"down520": -520, "up600": 600}[what]) if what in ("down520", "up600") else kc.bad_rhs(c.b, what)
    r = _solve_scaled(run, b)
    assert r.status == kr.BREAKDOWN and r.iters == 0 and r.relres != r.relres
    assert r.x.shape == (c.n,) and np.isnan(r.x).all()


@pytest.mark.parametrize("krylov", ["fgmres", "bicgstab"])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_non_finite_guess_is_a_breakdown(krylov, bad):
    c = kc.case("n513")
    A, M = oracle_operators(c, kc.JACOBI)
    x0 = kc.guess(c)
    x0[c.n // 2] = bad
    with np.errstate(all="ignore"):
        for max_iters in (0, 5):
            r = kr.fgmres(A, M, c.b, x0, restart=4, max_iters=max_iters) if krylov == "fgmres" else kr.bicgstab(A, M, c.b, x0, max_iters=max_iters)
            assert r.status == kr.BREAKDOWN and r.iters == 0 and r.relres != r.relres, (krylov, bad, max_iters, r.status, r.relres)


def test_berr_rule():
    """kr.berr, the rule test_gpu_vector_range.py holds berr_kernel to: the quotient rule of the library, NaN sticky"""
    assert kr.berr([1.0, -3.0, 0.0], [2.0, 4.0, 0.0]) == 0.75
    assert kr.berr([1.0, 1e-300], [2.0, 0.0]) == 1.0e300            # a residual where the denominator is zero
    assert kr.berr([0.0, 0.0], [0.0, 0.0]) == 0.0
    assert kr.berr([np.inf, 1.0], [1.0, 1.0]) == np.inf
    for r, d in (([np.nan, 1.0], [1.0, 1.0]), ([1.0, 1.0], [1.0, np.nan]), ([1.0, np.inf], [1.0, np.inf]), ([np.nan, 1.0], [0.0, 1.0])):
        assert kr.berr(r, d) != kr.berr(r, d), (r, d)
