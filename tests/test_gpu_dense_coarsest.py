"""The coarsest level's dense inverse beyond the blocked elimination: the pivoted routine (dense_inverse_device of csrc/dense.hip:
gj_pivot_kernel, gj_swap_scale_kernel, gj_column_kernel, gj_update_kernel), the state it leaves an f32 hierarchy in (an f64
inverse without an f32 copy), and the dense products at the sizes where their loops turn.  The matrices are tests/dense_cases.py;
what they must be for these tests to mean anything is asserted without a GPU in tests/test_dense_cases.py and, for every test
that relies on a planted pivot, once more here from the last level as the device stores it (_assert_pivoted).

  C1  the pivoted routine on one-level hierarchies: the bits of the host routine dense_inverse (csrc/ml_plan.cpp), and the solve
      against elimination in longdouble
  C2  dense_matvec_f32_kernel / dense_matvec_kernel against a longdouble product with the device's own inverse, row by row within
      n 2^-52 (|M| |b|), and their K-wide versions against single solves, at row tails, quad tails and lane-loop steps
  C3  ml_tail_kernel against the launched kernels at a last level of 223 quads (four quads per lane in the tail's loop)
  C4  an f32 hierarchy whose inverse came from the pivoted routine: ml_tail_kernel's f64 branch, dense_matvec_kernel and
      dense_matvec_batch_kernel inside f32 storage
  C5  nkp_refactor across that storage change, with batch members, with a live clone, with singular values; nkp_transpose"""
import numpy as np
import pytest

import dense_cases as dc
import ml_cycle_reference as mcr
from nk_ocn_tracer_jacobian_precond_amd import solver, synth

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
NKP_EINVAL, NKP_ESINGULAR = -1, -4
TAIL_LINE = "multilevel: levels %d..%d run as one single-workgroup launch"          # ml_setup at verbose >= 1, when tail_from is set


def _create(A, blk, ci, cj, tuning, **options):
    options = dict(dict(precond=solver.PRECOND_MULTILEVEL, restart=10), **options)
    return solver.NkpSolver(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data, blk, col_i=ci, col_j=cj, tuning=tuning, **options)


def _one_level(A, tuning, **options):
    s = _create(A, *dc.one_level_columns(A.shape[0]), tuning, **options)
    assert s.get_int("levels") == 1
    return s


def _two_level(t, tuning, **options):
    s = _create(t.A, t.blk, t.col_i, t.col_j, dict(tuning, ml_coarsest_rows=dc.COARSEST_ROWS_TWO_LEVEL), **options)
    assert [s.ml_level_array(l, "rowptr").size - 1 for l in range(s.get_int("levels"))] == [768, 192]
    return s


def _stored_last_level(s):
    last = s.get_int("levels") - 1
    rowptr, colind, val = (s.ml_level_array(last, what) for what in ("rowptr", "colind", "val"))
    assert val.size == colind.size == rowptr[-1]
    return dc.dense_of(rowptr, colind, val)


def _assert_pivoted(s):
    """The last level as stored has a pivot the blocked elimination refuses, and the pivoted routine made the inverse."""
    D = _stored_last_level(s)
    assert dc.unpivoted_min_pivot(D) <= 1e-14 * np.abs(np.diag(D)).max()
    assert s.get_int("ml_inverse_pivoted") == 1
    return D


def _inverse(s):
    n = s.ml_level_array(s.get_int("levels") - 1, "rowptr").size - 1
    return s.ml_level_array(s.get_int("levels") - 1, "coarse_inv").reshape(n, n)


def _rhs(n, count, seed=11):
    B = np.random.default_rng(seed).standard_normal((count, n))
    if count > 2:
        B[2] *= 1e-3                                            # systems of a group leave it at different steps
    return B


def _assert_column_bits(tag, X, infos, single):
    for c, (x1, i1) in enumerate(single[:len(infos)]):
        assert infos[c]["iters"] == i1["iters"] and infos[c]["relres"] == i1["relres"] and infos[c]["berr"] == i1["berr"], (tag, c, infos[c], i1)
        assert np.array_equal(X[c], x1), (tag, c, np.abs(X[c] - x1).max())


def _batched_against_single(tag, s, B, nrhs_list, width):
    """solve_many of the first nrhs rows of B for every nrhs against the single solves; the batched driver must have run at the
    width the group asks for.  Returns the single solves."""
    single = [s.solve(b, raise_on_fail=False) for b in B]
    assert all(i["iters"] > 0 for _, i in single), (tag, [i for _, i in single])
    for nrhs in nrhs_list:
        before = s.get_int("batch_steps")
        X, infos = s.solve_many(B[:nrhs], raise_on_fail=False)
        assert s.get_int("batch_steps") > before, (tag, nrhs, "the call fell back to one solve at a time")
        last = [g for g in range(0, nrhs, width) if nrhs - g > 1][-1]              # first column of the last group of two or more
        k = min(nrhs - last, width)
        assert s.get_int("batch_width") == (2 if k <= 2 else 4 if k <= 4 else 8), (tag, nrhs, s.get_int("batch_width"))
        _assert_column_bits((tag, nrhs), X, infos, single)
    return single


# ================================================================ C1  the pivoted routine
@pytest.mark.parametrize("n,q,far_tie", [(n, q, False) for n, q in dc.PIVOTED_CASES] + [dc.FAR_TIE_CASE + (True,)],
                         ids=["%d-%d" % c for c in dc.PIVOTED_CASES] + ["%d-%d-far_tie" % dc.FAR_TIE_CASE])
def test_pivoted_inverse_has_the_bits_of_the_host_routine(n, q, far_tie):
    """planted(n, q): the blocked elimination meets an exactly zero pivot at q + 1 and hands the level to the pivoted routine.
    Its inverse has the bits of dense_inverse on the host, as the header of the routine says (same operations in the same order,
    one multiply and one subtract per element; the first maximum wins the pivot search); the solve agrees with elimination in
    longdouble to 1e-10 (cond <= 538, test_dense_cases).  n = 300 takes two strides of gj_pivot_kernel's 256 threads and two
    column blocks of gj_swap_scale_kernel and gj_update_kernel; with q = 255 the tie is met at step 255 and the rows of step 256 are
    exchanged over both column blocks.  Those ties are between rows q and q + 1, two threads of the search, and pin its tree
    reduction; far_tie adds row q + 256 to the tie, which the thread of row q scans after it and must not prefer."""
    A = dc.planted(n, q, far_tie=far_tie)
    b = np.random.default_rng(n + q).standard_normal(n)
    with _one_level(A, dict(ml_f32=0)) as s:
        D = _assert_pivoted(s)
        assert np.array_equal(D, A.toarray())                       # the twin is A and the device's order the given one
        inv = _inverse(s)
        z = s.precond_apply(b)
    with _one_level(A, dict(ml_f32=0, ml_host_inverse=1)) as s:
        assert s.get_int("ml_inverse_pivoted") == 0                 # the host routine counts as 0
        inv_host = _inverse(s)
    assert np.isfinite(inv).all()
    assert np.array_equal(inv, inv_host), np.abs(inv - inv_host).max()
    x = dc.solve_longdouble(D, b).astype(np.float64)
    assert np.linalg.norm(z - x) <= 1e-10 * np.linalg.norm(x), np.linalg.norm(z - x) / np.linalg.norm(x)
    # what the pivot search met on the way, from the restated elimination on the stored matrix
    ties, exchanges, is_singular = dc.partial_pivoting_events(D)
    assert not is_singular
    assert q in ties and q + 1 in exchanges, (ties, exchanges)      # the pair's |-1| = |1|, then the zero pivot
    assert list(ties.rows[q]) == [q, q + 1] + ([q + dc.FAR] if far_tie else []), ties.rows[q]


# ================================================================ C2  the dense products
@pytest.mark.parametrize("f32", [1, 0], ids=["f32", "f64"])
def test_dense_products_at_their_edges(f32):
    """benign(n) as a one-level hierarchy: precond_apply is the dense product, a solve's cycle is it too.
    Single vector: row by row |z - M b| <= n 2^-52 (|M| |b|), the textbook bound of a sum of n products in any order, with M the
    inverse as the device holds it (f32 storage: rounded to f32 and widened, what dense_export_kernel stores) and M b in
    longdouble.  With nq = ceil (n / 4) quads per row: n = 1 .. 9 leave row tails of the 4- and 2-row waves and quad tails of 1,
    2 and 3 columns; n = 255, 256, 257 are nq = 64, 64, 65, the 64 lanes once and the first quad of a second round (the second
    of the four quads a lane of dense_matvec_f32_kernel has in flight, the second step of the K-wide kernels' loop); n = 1023 is
    nq = 256, exactly one step of 64 lanes x 4 quads, and n = 1025, 1030 (nq = 257, 258) begin a second step.
    Batched: 2, 3, 4, 5 and (rhs_batch = 8) 9 right-hand sides have the bits of their single solves, widths 2, 4 and 8 (2-row
    waves) all run.  max_iters = 3: equal bits after three steps say what equal bits after a full solve say."""
    for n in dc.PRODUCT_SIZES:
        A = dc.benign(n)
        b = np.random.default_rng(1000 + n).standard_normal(n)
        with _one_level(A, dict(ml_f32=f32), max_iters=3) as s:
            assert s.get_int("ml_inverse_pivoted") == 0
            M = _inverse(s)
            if f32:
                M = M.astype(np.float32).astype(np.float64)
            z = s.precond_apply(b)
            ref = (M.astype(np.longdouble) @ b.astype(np.longdouble)).astype(np.float64)
            bound = n * EPS * (np.abs(M) @ np.abs(b))
            excess = np.abs(z - ref) - bound
            print("MEASURED n = %4d %s  max |z - M b| / bound = %.3g" % (n, "f32" if f32 else "f64", (np.abs(z - ref) / bound).max()))
            assert (excess <= 0).all(), (n, f32, int(np.argmax(excess)), excess.max())
            if n > 1:
                assert np.linalg.norm(z) > 0
            B = _rhs(n, 9)
            _batched_against_single((n, f32), s, B[:5], (2, 3, 4, 5), 4)              # widths 2, 4, 4, 4 (asserted there)
        with _one_level(A, dict(ml_f32=f32, rhs_batch=8), max_iters=3) as s:
            _batched_against_single((n, f32, "rhs_batch 8"), s, B, (9,), 8)
            assert s.get_int("batch_width") == 8


# ================================================================ C3  the tail kernel at several quads per lane
@pytest.fixture(scope="module")
def cycle_problem():
    p = synth.generate(imt=24, jmt=20, km=10, adv="upwind3", hmix="isop", seed=2)          # the problem of test_gpu_cycle_options
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    r = np.random.default_rng(17).standard_normal(p.flat_len)

    def make(tuning, **options):
        return solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, precond=solver.PRECOND_MULTILEVEL, col_i=ci, col_j=cj, restart=4, tuning=tuning, **options)
    return make, r


@pytest.fixture(scope="module")
def tail_references(cycle_problem):
    make, r = cycle_problem
    cache = {}

    def get(f32):
        if f32 not in cache:
            with make(dict(ml_coarsest_rows=1000, ml_f32=f32)) as s:
                levels = mcr.levels_from_solver(s)
            if f32:
                levels = mcr.with_exact_blocks(levels, get(0).levels)
            cache[f32] = mcr.Reference(levels, r, f32, {"default": {}})
        return cache[f32]
    return get


@pytest.mark.parametrize("f32", [1, 0], ids=["f32", "f64"])
def test_tail_kernel_at_four_quads_per_lane(f32, cycle_problem, tail_references, capfd):
    """ml_coarsest_rows = 1000 ends the 24 x 20 x 10 hierarchy at 889 rows: 223 quads, so a lane of ml_tail_kernel's f32 loop
    adds up to four quads and one of its f64 loop fourteen columns, where the cycle tests' last levels (at most 35 quads) never
    let a lane add a second.  The tail repeats the launched kernels' summation order, so the cycle keeps its bits; both meet the
    restated cycle within the bounds of test_gpu_cycle_options.
    That the tail serves the cycle is read from the setup's line at verbose = 1 (tail_from is set); ml_cycle then launches it
    unless a W-level is asked for (none here) or there are more levels than TAIL_MAX_LEVELS (two here).  No counter says that the
    launch happened: as in test_gpu_cycle_options, a tail that silently declined would show the same bits."""
    make, r = cycle_problem
    ref = tail_references(f32)
    assert ref.rows == [2813, 889]
    z = {}
    for tail_rows in (16000, 0):
        capfd.readouterr()
        with make(dict(ml_coarsest_rows=1000, ml_f32=f32, ml_tail_rows=tail_rows), verbose=1) as s:
            assert (TAIL_LINE % (0, 1) in capfd.readouterr().out) == (tail_rows > 0)
            assert [s.ml_level_array(l, "rowptr").size - 1 for l in range(s.get_int("levels"))] == [2813, 889]
            assert s.get_int("ml_inverse_pivoted") == 0
            z[tail_rows] = s.precond_apply(r)
    assert np.isfinite(z[0]).all()
    assert np.array_equal(z[16000], z[0]), np.abs(z[16000] - z[0]).max()
    for tail_rows in (16000, 0):
        ref.check("last level of 889 rows / tail_rows %d" % tail_rows, "default", z[tail_rows])


# ================================================================ C4  an f32 hierarchy with an f64 inverse
@pytest.fixture(scope="module")
def two_level_cases():
    return {kind: dc.two_level(kind=kind, **dc.TWO_LEVEL) for kind in ("planted", "mild", "singular", "regular")}


def test_f32_hierarchy_with_an_inverse_from_the_pivoted_routine(two_level_cases, capfd):
    """two_level: the coarse operator carries the planted pair, so the pivoted routine makes the inverse and returns it in f64
    alone; the f32 hierarchy then has no f32 copy of it.  The cycle multiplies with dense_matvec_kernel, the batched cycle with
    dense_matvec_batch_kernel and ml_tail_kernel takes its f64 branch: the tail keeps the bits of the launched kernels, batched
    solves those of single ones, and the cycle meets the restated one within the f32-storage bound of test_gpu_cycle_options.
    That bound's yardstick rounds the last level's inverse to f32, which the device does not do here: the bound is loose for
    this case."""
    t = two_level_cases["planted"]
    r = np.random.default_rng(23).standard_normal(t.A.shape[0])
    B = _rhs(t.A.shape[0], 4)
    with _two_level(t, dict(ml_f32=0)) as s:
        _assert_pivoted(s)
        levels_f64 = mcr.levels_from_solver(s)
    z, singles = {}, {}
    for tail_rows in (16000, 0):
        capfd.readouterr()
        with _two_level(t, dict(ml_f32=1, ml_tail_rows=tail_rows), max_iters=6, verbose=1) as s:
            out = capfd.readouterr().out
            assert (TAIL_LINE % (0, 1) in out) == (tail_rows > 0)                                  # as in the test above
            assert "a pivot too small for it, pivoted routine instead" in out
            D = _assert_pivoted(s)
            assert np.array_equal(D[np.ix_(np.argsort(t.order), np.argsort(t.order))], t.Ac)      # the coarse operator, cell by cell
            assert s.ml_level_array(0, "valf").size and not s.ml_level_array(0, "val").size      # f32 storage above the last level
            if tail_rows:
                levels = mcr.with_exact_blocks(mcr.levels_from_solver(s), levels_f64)
            z[tail_rows] = s.precond_apply(r)
            singles[tail_rows] = _batched_against_single(("two_level", tail_rows), s, B, (2, 4), 4)
    assert np.isfinite(z[0]).all()
    assert np.array_equal(z[16000], z[0]), np.abs(z[16000] - z[0]).max()
    for (xa, ia), (xb, ib) in zip(singles[16000], singles[0]):
        assert np.array_equal(xa, xb) and ia == ib
    ref = mcr.Reference(levels, r, 1, {"default": {}})               # z_ref multiplies with the f64 inverse as it is
    for tail_rows in (16000, 0):
        ref.check("two_level, f64 inverse / tail_rows %d" % tail_rows, "default", z[tail_rows])


# ================================================================ C5  refactor across the storage change
def _answers(s, n):
    """precond_apply, one solve and one batched solve of fixed right-hand sides."""
    B = _rhs(n, 3, seed=29)
    z = s.precond_apply(B[0])
    x, info = s.solve(B[1], raise_on_fail=False)
    X, infos = s.solve_many(B, raise_on_fail=False)
    return dict(z=z, x=x, info=info, X=X, infos=infos, inv=_inverse(s))


def _assert_same_answers(tag, a, b):
    for key in ("z", "x", "X", "inv"):
        assert np.array_equal(a[key], b[key]), (tag, key, np.abs(a[key] - b[key]).max())
    assert a["info"] == b["info"] and a["infos"] == b["infos"], (tag, a["info"], b["info"])


def _maker(case, two_level_cases):
    """A -> an f32-storage solver of A, for the one-level matrices and for the fine matrices of two_level."""
    if case == "one_level":
        return lambda A: _one_level(A, dict(ml_f32=1), max_iters=6)
    t = two_level_cases["mild"]                                      # every kind has the same columns
    return lambda A: _create(A, t.blk, t.col_i, t.col_j, dict(ml_f32=1, ml_coarsest_rows=dc.COARSEST_ROWS_TWO_LEVEL), max_iters=6)


def _refactor_cases(two_level_cases):
    """(mild values, planted values on the same pattern, maker, refactor_rebuilt)"""
    n, q = dc.REFACTOR_ONE_LEVEL
    return {"one_level": (dc.mild(n, q), dc.planted(n, q), _maker("one_level", two_level_cases), 1),
            "two_level": (two_level_cases["mild"].A, two_level_cases["planted"].A, _maker("two_level", two_level_cases), 0)}


@pytest.mark.parametrize("case", ["one_level", "two_level"])
def test_refactor_round_trip_across_the_storage_change(case, two_level_cases):
    """mild -> planted -> mild values on one pattern, f32 storage, with batch members alive.  The planted values send the last
    level to the pivoted routine, whose inverse has no f32 copy; the mild values bring the copy back.  two_level takes the
    value-refresh path (refactor_rebuilt == 0): rf_commit replaces the inverse buffers and the batch members are dropped.  A
    one-level hierarchy has no coarse cells to keep and is rebuilt (refactor_rebuilt == 1), which carries its own value of
    ml_inverse_pivoted.  Either way the solver then answers with the bits of a solver created from those values, and holds the
    device memory of a solver that was refactored mild -> mild twice."""
    M, P, make, rebuilt = _refactor_cases(two_level_cases)[case]
    assert np.array_equal(M.indices, P.indices) and np.array_equal(M.indptr, P.indptr)
    n = M.shape[0]
    with make(M) as s, make(P) as fresh_planted, make(M) as fresh_mild, make(M) as twin:
        assert s.get_int("ml_inverse_pivoted") == 0 and fresh_mild.get_int("ml_inverse_pivoted") == 0
        _assert_pivoted(fresh_planted)
        want_planted, want_mild = _answers(fresh_planted, n), _answers(fresh_mild, n)
        assert not np.array_equal(want_planted["z"], want_mild["z"])
        for h in (s, twin):
            h.solve_many(_rhs(n, 3), raise_on_fail=False)            # batch members exist before the refactor
            assert h.get_int("batch_member_bytes") > 0
        s.refactor(P.data)
        assert s.get_int("refactor_rebuilt") == rebuilt and s.get_int("refactor_count") == 1
        _assert_pivoted(s)
        _assert_same_answers((case, "planted"), _answers(s, n), want_planted)
        s.refactor(M.data)
        assert s.get_int("refactor_rebuilt") == rebuilt and s.get_int("refactor_count") == 2
        assert s.get_int("ml_inverse_pivoted") == 0
        _assert_same_answers((case, "mild again"), _answers(s, n), want_mild)
        for _ in range(2):
            twin.refactor(M.data)
            assert twin.get_int("refactor_rebuilt") == rebuilt and twin.get_int("ml_inverse_pivoted") == 0
            _assert_same_answers((case, "twin"), _answers(twin, n), want_mild)
        assert s.get_int("device_bytes") == twin.get_int("device_bytes"), (s.get_int("device_bytes"), twin.get_int("device_bytes"))
        assert s.get_int("batch_member_bytes") == twin.get_int("batch_member_bytes")


@pytest.mark.parametrize("case", ["one_level", "two_level"])
def test_refactor_across_the_storage_change_is_refused_with_a_live_clone(case, two_level_cases):
    """A clone points at the inverse buffers of the solver it came from: new buffers (two_level) or a new hierarchy (one level)
    would leave it behind, so the call is refused before anything is written."""
    M, P, make, rebuilt = _refactor_cases(two_level_cases)[case]
    n = M.shape[0]
    b = _rhs(n, 1, seed=31)[0]
    with make(M) as s:
        c = s.clone()
        try:
            before = [(h.precond_apply(b), h.solve(b, raise_on_fail=False)) for h in (s, c)]
            with pytest.raises(solver.NkpError) as e:
                s.refactor(P.data)
            assert e.value.code == NKP_EINVAL and "1 live clone" in str(e.value), str(e.value)
            # which check refused: the storage of the prepared inverse (value-refresh path), or the rebuild a clone would not see
            assert ("needs other storage" if case == "two_level" else "has to be rebuilt") in str(e.value), str(e.value)
            assert s.get_int("refactor_count") == 0 and s.get_int("ml_inverse_pivoted") == 0
            for h, (z0, (x0, i0)) in zip((s, c), before):
                x1, i1 = h.solve(b, raise_on_fail=False)
                assert np.array_equal(h.precond_apply(b), z0) and np.array_equal(x1, x0) and i1 == i0
        finally:
            c.close()
        s.refactor(P.data)
        assert s.get_int("refactor_rebuilt") == rebuilt
        _assert_pivoted(s)
        with make(P) as fresh:
            assert np.array_equal(s.precond_apply(b), fresh.precond_apply(b))


@pytest.mark.parametrize("case", ["one_level", "two_level"])
def test_singular_values_are_refused(case, two_level_cases):
    """An exactly singular last level: both eliminations find it (the blocked one a zero pivot, the pivoted one a column of
    zeros) and report it; nkp_create fails with NKP_ESINGULAR, nkp_refactor with the same code and the solver unchanged."""
    if case == "one_level":
        n, q = dc.SINGULAR_ONE_LEVEL
        S, R = dc.singular(n, q), dc.singular(n, q, coupling=1.0)
    else:
        S, R = two_level_cases["singular"].A, two_level_cases["regular"].A
    make = _maker(case, two_level_cases)
    assert np.array_equal(S.indices, R.indices) and np.array_equal(S.indptr, R.indptr)
    with pytest.raises(solver.NkpError) as e:
        make(S)
    assert e.value.code == NKP_ESINGULAR and "singular" in str(e.value), str(e.value)
    b = _rhs(S.shape[0], 1, seed=37)[0]
    with make(R) as s:
        assert s.get_int("ml_inverse_pivoted") == 0 and s.get_int("levels") == (1 if case == "one_level" else 2)
        z0, (x0, i0) = s.precond_apply(b), s.solve(b, raise_on_fail=False)
        with pytest.raises(solver.NkpError) as e:
            s.refactor(S.data)
        assert e.value.code == NKP_ESINGULAR and "singular" in str(e.value), str(e.value)
        assert s.get_int("refactor_count") == 0
        x1, i1 = s.solve(b, raise_on_fail=False)
        assert np.array_equal(s.precond_apply(b), z0) and np.array_equal(x1, x0) and i1 == i0
        s.refactor(R.data)                                           # and it still takes values it can invert
        assert np.array_equal(s.precond_apply(b), z0)


def test_transposed_solver_of_a_planted_matrix():
    """nkp_transpose builds its hierarchy from A^T, whose pair is the same 2 x 2 block: the pivoted routine once more.  The
    matrix is planted(n, q) with the entries above the diagonal halved, since planted(n, q) itself is symmetric."""
    n, q, upper = dc.TRANSPOSE_ONE_LEVEL
    A = dc.planted(n, q, upper=upper)                               # not symmetric
    b = np.random.default_rng(41).standard_normal(n)
    with _one_level(A, dict(ml_f32=0)) as s:
        _assert_pivoted(s)
        t = s.transposed()
        assert t.get_int("is_transpose") == 1 and t.get_int("levels") == 1
        D = _assert_pivoted(t)
        assert np.array_equal(D, A.toarray().T)
        z = t.precond_apply(b)
        x = dc.solve_longdouble(A.toarray().T, b).astype(np.float64)
        assert np.linalg.norm(z - x) <= 1e-10 * np.linalg.norm(x), np.linalg.norm(z - x) / np.linalg.norm(x)
        zs = s.precond_apply(b)
        assert np.linalg.norm(z - zs) >= 1e-3 * np.linalg.norm(zs)  # another solve than the owner's
