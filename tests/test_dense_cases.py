"""What tests/test_gpu_dense_coarsest.py relies on in the matrices of tests/dense_cases.py, checked without a GPU: the sign
pattern (so that the low-order twin is the matrix itself), which elimination each case takes in the order the device uses, that
every case is well conditioned, and that the two-level case coarsens to the operator it was expanded from."""
import numpy as np
import pytest

import dense_cases as dc
import ml_reference as mlr

MAX_COND = 1e3


def _check_signs_and_twin(A):
    D = A.toarray()
    d = np.diag(D)
    assert (d < 0).all() and (D - np.diag(d) >= 0).all()
    assert (A.data != 0).all()                                       # zeros are not stored
    n = A.shape[0]
    assert (mlr.low_order(A, np.arange(n)) != A).nnz == 0            # single-row columns: every off-diagonal entry is between columns


def _maxdiag(D):
    return np.abs(np.diag(D)).max()


@pytest.mark.parametrize("n", sorted(set(dc.PRODUCT_SIZES) | {63, 64, 65, 200}))
def test_benign_keeps_the_blocked_routine(n):
    A = dc.benign(n)
    _check_signs_and_twin(A)
    D = A.toarray()
    assert dc.unpivoted_min_pivot(D) >= 1e-3 * _maxdiag(D)
    assert np.linalg.cond(D) <= MAX_COND


def test_benign_is_the_generator_the_blocked_test_had():
    """The (A, b) of test_blocked_dense_inverse_sizes, drawn here as that test drew them before the generator moved."""
    import scipy.sparse as sp
    for n in (1, 65, 200):
        rng = np.random.default_rng(n)
        A = sp.random(n, n, density=min(1.0, 6.0 / n), random_state=int(n), format="csr")
        A = -abs(A) - abs(A.T)
        A = (A - sp.diags(np.asarray(A.sum(axis=1)).ravel() - 1.0 - rng.random(n))).tocsr()
        A = (-A).tocsr()
        A.sort_indices()
        b = rng.standard_normal(n)
        A2, b2 = dc.benign_with_rhs(n)
        assert np.array_equal(A.indptr, A2.indptr) and np.array_equal(A.indices, A2.indices) and np.array_equal(A.data, A2.data)
        assert np.array_equal(b, b2)


@pytest.mark.parametrize("n,q", sorted(set(dc.PIVOTED_CASES) | {dc.REFACTOR_ONE_LEVEL}))
def test_planted_and_mild(n, q):
    P, M = dc.planted(n, q), dc.mild(n, q)
    for A in (P, M):
        _check_signs_and_twin(A)
        assert np.linalg.cond(A.toarray()) <= MAX_COND
    assert np.array_equal(P.indptr, M.indptr) and np.array_equal(P.indices, M.indices)          # one pattern
    blk, ci, cj = dc.one_level_columns(n)
    assert np.array_equal(dc.colour_major(ci, cj), np.arange(n))     # the device eliminates in the given order
    D = P.toarray()
    assert dc.unpivoted_min_pivot(D) == 0.0
    assert dc.unpivoted_min_pivot(D[:q + 2, :q + 2]) == 0.0 and dc.unpivoted_min_pivot(D[:q + 1, :q + 1]) > 0.0      # ... at q + 1
    assert dc.unpivoted_min_pivot(M.toarray()) >= 1e-3 * _maxdiag(M.toarray())
    ties, exchanges, is_singular = dc.partial_pivoting_events(D)
    assert q in ties and q not in exchanges and q + 1 in exchanges and not is_singular
    # the transposed pair is singular as well (nkp_transpose builds its hierarchy from A^T)
    assert dc.unpivoted_min_pivot(D.T) == 0.0


def test_far_tie_is_scanned_by_one_thread():
    """Step q of the pivot search meets its maximum in rows q, q + 1 and q + 256; thread 0 of gj_pivot_kernel scans the first and
    the last of them, in that order, and must keep the first."""
    n, q = dc.FAR_TIE_CASE
    A = dc.planted(n, q, far_tie=True)
    _check_signs_and_twin(A)
    D = A.toarray()
    assert np.linalg.cond(D) <= MAX_COND
    assert dc.unpivoted_min_pivot(D) == 0.0 and dc.unpivoted_min_pivot(D[:q + 2, :q + 2]) == 0.0
    ties, exchanges, is_singular = dc.partial_pivoting_events(D)
    assert list(ties.rows[q]) == [q, q + 1, q + dc.FAR] and q not in exchanges and q + 1 in exchanges and not is_singular


def test_unpivoted_min_pivot_restates_plain_elimination():
    """The panelled elimination of unpivoted_min_pivot against the textbook loop, on a matrix of more than one panel."""
    a = dc.mild(200, 130).toarray()
    ref = a.copy()
    smallest = np.inf
    for k in range(200):
        smallest = min(smallest, abs(ref[k, k]))
        ref[k + 1:, k + 1:] -= np.outer(ref[k + 1:, k] / ref[k, k], ref[k, k + 1:])
    assert abs(dc.unpivoted_min_pivot(a) - smallest) <= 1e-12 * smallest


def test_planted_for_the_transposed_solver_is_not_symmetric():
    n, q, upper = dc.TRANSPOSE_ONE_LEVEL
    A = dc.planted(n, q, upper=upper)
    _check_signs_and_twin(A)
    D = A.toarray()
    assert not np.array_equal(D, D.T) and np.abs(D - D.T).max() >= 0.25
    assert np.linalg.cond(D) <= MAX_COND
    for M in (D, D.T):
        assert dc.unpivoted_min_pivot(M) == 0.0 and dc.unpivoted_min_pivot(M[:q + 1, :q + 1]) > 0.0
        ties, exchanges, is_singular = dc.partial_pivoting_events(M)
        assert q in ties and q + 1 in exchanges and not is_singular


def test_singular_is_found_by_both_eliminations():
    n, q = dc.SINGULAR_ONE_LEVEL
    S, R = dc.singular(n, q), dc.singular(n, q, coupling=1.0)
    for A in (S, R):
        _check_signs_and_twin(A)
    assert np.array_equal(S.indptr, R.indptr) and np.array_equal(S.indices, R.indices)
    assert dc.unpivoted_min_pivot(S.toarray()) == 0.0
    assert dc.partial_pivoting_events(S.toarray())[2]                # an exact zero column, not a small pivot
    assert np.linalg.matrix_rank(S.toarray()) == n - 1
    D = R.toarray()
    assert dc.unpivoted_min_pivot(D) >= 1e-3 * _maxdiag(D) and np.linalg.cond(D) <= MAX_COND
    assert not dc.partial_pivoting_events(D)[2]


@pytest.fixture(scope="module")
def two_level_plans():
    out = {}
    for kind in ("planted", "mild", "regular"):
        t = dc.two_level(kind=kind, **dc.TWO_LEVEL)
        n = t.A.shape[0]
        levels = mlr.build(t.A, t.col_i.astype(np.int64), t.col_j.astype(np.int64), np.zeros(n, np.int64), np.arange(n),
                           coarsest_rows=dc.COARSEST_ROWS_TWO_LEVEL)
        out[kind] = (t, levels)
    return out


@pytest.mark.parametrize("kind", ["planted", "mild", "regular"])
def test_two_level_coarsens_to_its_coarse_operator(kind, two_level_plans):
    t, levels = two_level_plans[kind]
    _check_signs_and_twin(t.A)
    assert [lv.n for lv in levels] == [768, 192]
    assert (levels[0].A != t.A).nnz == 0                             # the twin
    assert np.array_equal(levels[0].cmap, t.cell_of)                 # the 2 x 2 groups are the coarse cells, numbered as here
    assert np.array_equal(levels[1].A.toarray(), t.Ac)               # dyadic values: the Galerkin product is exact
    assert np.array_equal(levels[1].ci, t.cell_i) and np.array_equal(levels[1].cj, t.cell_j)
    assert np.linalg.cond(t.Ac) <= MAX_COND and np.linalg.cond(t.A.toarray()) <= MAX_COND
    # the last level in the device's order
    order = dc.colour_major(levels[1].ci, levels[1].cj)
    assert np.array_equal(order, t.order)
    D = t.Ac[np.ix_(order, order)]
    q = t.q
    if kind == "planted":
        assert dc.unpivoted_min_pivot(D) == 0.0 and dc.unpivoted_min_pivot(D[:q + 1, :q + 1]) > 0.0
        assert dc.unpivoted_min_pivot(D[:q + 2, :q + 2]) == 0.0
        assert 64 <= q < 126                                         # inside the second 64-block of the blocked elimination
    else:
        assert dc.unpivoted_min_pivot(D) >= 1e-3 * _maxdiag(D)


def test_two_level_patterns_and_singular_values(two_level_plans):
    P, M, R = (two_level_plans[k][0] for k in ("planted", "mild", "regular"))
    assert np.array_equal(P.A.indptr, M.A.indptr) and np.array_equal(P.A.indices, M.A.indices)
    S = dc.two_level(kind="singular", **dc.TWO_LEVEL)
    _check_signs_and_twin(S.A)
    assert np.array_equal(S.A.indptr, R.A.indptr) and np.array_equal(S.A.indices, R.A.indices)
    D = S.Ac[np.ix_(S.order, S.order)]
    assert dc.unpivoted_min_pivot(D) == 0.0 and dc.partial_pivoting_events(D)[2]
    # the same cells and the coarse operator of the singular values: the Galerkin product on the cells of the regular ones
    Pm = two_level_plans["regular"][1][0].P
    assert np.array_equal((Pm.T @ S.A @ Pm).toarray(), S.Ac)
