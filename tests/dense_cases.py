"""Matrices for the coarsest level's dense inverse (csrc/dense.hip, ml_coarse_inverse of csrc/multilevel.hip) -- TEST
INFRASTRUCTURE for tests/test_dense_cases.py (no GPU) and tests/test_gpu_dense_coarsest.py.

Every matrix here has a negative diagonal and non-negative off-diagonal entries, so the low-order twin of the multilevel setup
is the matrix itself (ml_reference.low_order) and a test knows the operator the last level inverts.  Zeros are never stored.

  benign(n)            the generator of test_gpu_parity.test_blocked_dense_inverse_sizes: random, row dominant, 1 + U(0, 1) of
                       slack per row.  Elimination without row exchanges keeps it: the blocked routine (bgj_*) inverts it.
  planted(n, q)        benign(n) with a pair of rows q, q + 1 that nothing ordered before it couples to, whose 2 x 2 block is
                       [[-1, 1], [1, -1]]: elimination without row exchanges meets an exactly zero pivot at q + 1, the blocked
                       routine raises its flag and the pivoted routine (gj_*) computes the inverse.  The couplings q <-> q + 2
                       (0.5) and q + 1 <-> q + 3 (0.25) keep the matrix regular and well conditioned.  benign(n) is symmetric
                       and so is planted(n, q); planted(n, q, upper = 0.5) halves the entries above the diagonal first, and
                       planted(n, q, far_tie = True) adds a third row to the tie of step q, 256 rows below the pair.
  mild(n, q)           the pattern of planted(n, q) with the pair's diagonals at -3: the blocked routine keeps it.  Refactor
                       cases move between mild and planted values on one pattern.
  singular(n, q)       mild(n, q) whose rows q + 2, q + 3 hold nothing but the block [[-8, c], [c, -8]] on the diagonal: c = 8
                       makes the two rows the negatives of each other, an exactly singular matrix with the sign pattern kept
                       (8 exceeds every other entry, so partial pivoting takes row q + 2 as it stands, row q + 3 becomes
                       exactly zero and stays so to the last step, where the pivot search finds nothing but it); coupling = 1
                       is a regular matrix on the same pattern, for the refactor that must be refused.
  two_level(gx, gy, q) a coarse operator Ac on gx * gy cells (5-point, diagonal -3, neighbours 0.5) carrying the same pair,
                       expanded to a fine matrix on 2 gx x 2 gy single-row water columns whose 2 x 2 groups are the cells:
                       A[4 C + m][4 D + m] = Ac[C][D] / 4 for the four members m of a cell, a ring of 0.25 between the members
                       of a cell, member diagonals (Ac[C][C] - 2) / 4.  All values are dyadic, so P^T A P == Ac exactly in any
                       summation order.

The device eliminates the last level in its COLOUR-MAJOR order: the columns of colour (i + j) % 2 == 0 in their given order,
then those of colour 1 (colour_major).  The one-level cases come with columns at (2 c, 0) -- one colour, so the device's order
is the given one (one_level_columns) -- and two_level plants its pair at positions q .. q + 3 of the colour-major order of the
cells.  Those are cells of colour 0, which the 5-point operator couples to cells of colour 1 only, that is, to nothing ordered
before them; the planted couplings join cells that are no grid neighbours, which the twin (signs only) does not mind.

unpivoted_min_pivot and partial_pivoting_events restate the two eliminations in numpy, so that a test can assert from the
matrix as the device stores it that its case does what it is there for."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

COARSEST_ROWS_TWO_LEVEL = 192
FAR = 256                     # threads of gj_pivot_kernel: rows k and k + FAR of a column are scanned by the same thread


def benign_with_rhs(n):
    """(A, b) exactly as test_blocked_dense_inverse_sizes drew them."""
    rng = np.random.default_rng(n)
    A = sp.random(n, n, density=min(1.0, 6.0 / n), random_state=int(n), format="csr")
    A = -abs(A) - abs(A.T)
    A = (A - sp.diags(np.asarray(A.sum(axis=1)).ravel() - 1.0 - rng.random(n))).tocsr()
    A = (-A).tocsr()                                  # the sign of an ocean Jacobian: negative diagonal (the twin keeps such a matrix as it is)
    A.sort_indices()
    b = rng.standard_normal(n)
    return A, b


def benign(n):
    return benign_with_rhs(n)[0]


def _csr(D):
    A = sp.csr_matrix(D)
    A.eliminate_zeros()
    A.sort_indices()
    return A


def _plant(D, q, diag):
    """The pair at positions q, q + 1 of the dense D (in place): see planted."""
    n = D.shape[0]
    assert n >= q + 4
    D[q:q + 2, :q] = 0.0
    D[:q, q:q + 2] = 0.0
    D[q, q] = D[q + 1, q + 1] = diag
    D[q, q + 1] = D[q + 1, q] = 1.0
    D[q, q + 2] = D[q + 2, q] = 0.5
    D[q + 1, q + 3] = D[q + 3, q + 1] = 0.25
    return D


def _isolate_block(D, q, coupling):
    """Rows q + 2, q + 3 hold nothing but [[-8, coupling], [coupling, -8]] (in place): see singular."""
    D[q + 2:q + 4, :] = 0.0
    D[q + 2, q + 2] = D[q + 3, q + 3] = -8.0
    D[q + 2, q + 3] = D[q + 3, q + 2] = coupling
    return D


def planted(n, q, upper=1.0, far_tie=False):
    """upper != 1 scales benign(n)'s entries above the diagonal before the pair is planted: benign(n) is symmetric, and a test
    of A^T needs a matrix that is not.  far_tie couples q <-> q + FAR (1.0): the pivot search of step q then meets |-1| = |1| in
    rows q and q + FAR as well, which one thread of gj_pivot_kernel scans one after the other."""
    B = benign(n).toarray()
    D = _plant(np.tril(B) + upper * np.triu(B, 1), q, -1.0)
    if far_tie:
        assert n > q + FAR
        D[q, q + FAR] = D[q + FAR, q] = 1.0
    return _csr(D)


def mild(n, q):
    return _csr(_plant(benign(n).toarray(), q, -3.0))


def singular(n, q=0, coupling=8.0):
    return _csr(_isolate_block(_plant(benign(n).toarray(), q, -3.0), q, coupling))


def one_level_columns(n):
    """blk_start, col_i, col_j of n single-row water columns of one colour: the device keeps the given order."""
    return np.arange(n + 1, dtype=np.int32), 2 * np.arange(n, dtype=np.int32), np.zeros(n, np.int32)


def colour_major(col_i, col_j):
    """Position -> column of the device's order of a level: colour 0 in the given order, then colour 1."""
    colour = (np.asarray(col_i) + np.asarray(col_j)) % 2
    return np.concatenate([np.flatnonzero(colour == 0), np.flatnonzero(colour == 1)])


class TwoLevel:
    """A: the fine matrix (csr); blk, col_i, col_j: its 2 gx x 2 gy single-row columns; Ac: the coarse operator in the natural
    order of the cells (C = J * gx + I, dense); cell_i, cell_j: the cells' grid positions; order: the device's order of the
    cells; cell_of: cell of every fine row."""


def two_level(gx=16, gy=12, q=70, kind="planted"):
    """kind: "planted" | "mild" (one pattern), "singular" | "regular" (another one: singular(.., coupling = 8 | 1) on the cells)."""
    assert kind in ("planted", "mild", "singular", "regular")
    nc = gx * gy
    I, J = np.arange(nc) % gx, np.arange(nc) // gx
    Ac = np.zeros((nc, nc))
    Ac[np.arange(nc), np.arange(nc)] = -3.0
    for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        ok = (I + di >= 0) & (I + di < gx) & (J + dj >= 0) & (J + dj < gy)
        Ac[np.arange(nc)[ok], ((J + dj) * gx + I + di)[ok]] = 0.5
    order = colour_major(I, J)
    assert q + 4 <= np.count_nonzero((I + J) % 2 == 0)          # the pair and its two partners are cells of colour 0
    Ap = Ac[np.ix_(order, order)]
    _plant(Ap, q, -1.0 if kind == "planted" else -3.0)
    if kind in ("singular", "regular"):
        _isolate_block(Ap, q, 8.0 if kind == "singular" else 1.0)
    back = np.empty(nc, np.int64)
    back[order] = np.arange(nc)
    Ac = Ap[np.ix_(back, back)]
    # members of a cell in ring order: (0, 0), (1, 0), (1, 1), (0, 1)
    mi, mj = np.array([0, 1, 1, 0]), np.array([0, 0, 1, 1])
    ring = np.zeros((4, 4))
    for m in range(4):
        ring[m, (m + 1) % 4] = ring[m, (m - 1) % 4] = 0.25
    A = sp.kron(sp.csr_matrix(Ac - np.diag(np.diag(Ac))), sp.identity(4)) / 4.0
    A = A + sp.kron(sp.identity(nc), sp.csr_matrix(ring)) + sp.kron(sp.diags((np.diag(Ac) - 2.0) / 4.0), sp.identity(4))
    t = TwoLevel()
    t.A = _csr(A)
    t.Ac, t.cell_i, t.cell_j, t.order = Ac, I, J, order
    t.cell_of = np.repeat(np.arange(nc), 4)
    t.col_i = (2 * I[t.cell_of] + np.tile(mi, nc)).astype(np.int32)
    t.col_j = (2 * J[t.cell_of] + np.tile(mj, nc)).astype(np.int32)
    t.blk = np.arange(4 * nc + 1, dtype=np.int32)
    t.q = q
    return t


def unpivoted_min_pivot(dense):
    """The smallest |pivot| of elimination without row exchanges, in the given order (0.0 as soon as one is exactly zero)."""
    a = np.array(dense, np.float64)
    n = a.shape[0]
    smallest = np.inf
    nb = 64                                             # right-looking in panels of 64 columns: the rest is one matrix product each
    for k0 in range(0, n, nb):
        k1 = min(k0 + nb, n)
        for k in range(k0, k1):
            p = a[k, k]
            smallest = min(smallest, abs(p))
            if p == 0.0:
                return 0.0
            a[k + 1:, k] /= p
            a[k + 1:, k + 1:k1] -= np.outer(a[k + 1:, k], a[k, k + 1:k1])
        if k1 < n:
            a[k0:k1, k1:] = sla.solve_triangular(a[k0:k1, k0:k1], a[k0:k1, k1:], lower=True, unit_diagonal=True, check_finite=False)
            a[k1:, k1:] -= a[k1:, k0:k1] @ a[k0:k1, k1:]
    return float(smallest)


class _Ties(list):
    """The steps with a tie; rows[k]: the rows (of the matrix as permuted by then) that met the maximum of step k."""

    def __init__(self):
        super().__init__()
        self.rows = {}


def partial_pivoting_events(dense):
    """Elimination with partial pivoting, first maximum wins (dense_inverse of csrc/ml_plan.cpp and gj_pivot_kernel choose that
    row): the steps whose largest |entry| is met by more than one row (ties), the steps that exchange rows, and whether a step
    found nothing but exact zeros (what both routines report as singular)."""
    a = np.array(dense, np.float64)
    n = a.shape[0]
    ties, exchanges = _Ties(), []
    tied_rows = ties.rows
    for k in range(n):
        col = np.abs(a[k:, k])
        p = k + int(np.argmax(col))                     # the first maximum
        if np.count_nonzero(col == col[p - k]) > 1:
            ties.append(k)
            tied_rows[k] = k + np.flatnonzero(col == col[p - k])
        if p != k:
            exchanges.append(k)
            a[[k, p]] = a[[p, k]]
        if a[k, k] == 0.0:
            return ties, exchanges, True
        f = a[k + 1:, k] / a[k, k]
        a[k + 1:, k + 1:] -= np.outer(f, a[k, k + 1:])
        a[k + 1:, k] = 0.0
    return ties, exchanges, False


def solve_longdouble(dense, b):
    """x with dense @ x = b by elimination with partial pivoting in numpy's longdouble (numpy.linalg has no such solve)."""
    a = np.array(dense, np.longdouble)
    x = np.array(b, np.longdouble)
    n = a.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(a[k:, k])))
        if p != k:
            a[[k, p]] = a[[p, k]]
            x[[k, p]] = x[[p, k]]
        f = a[k + 1:, k] / a[k, k]
        a[k + 1:, k:] -= np.outer(f, a[k, k:])
        x[k + 1:] -= f * x[k]
    for k in range(n - 1, -1, -1):
        x[k] = (x[k] - a[k, k + 1:] @ x[k + 1:]) / a[k, k]
    return x


def dense_of(rowptr, colind, val):
    n = len(rowptr) - 1
    return sp.csr_matrix((val, colind, rowptr), shape=(n, n)).toarray()


# the cases of tests/test_gpu_dense_coarsest.py, as data (tests/test_dense_cases.py asserts what they rely on)
PIVOTED_CASES = [(4, 0), (65, 60), (200, 0), (200, 130), (200, 194), (300, 255)]          # planted(n, q), one level
FAR_TIE_CASE = (300, 0)                                                                  # planted(n, q, far_tie = True), one level
PRODUCT_SIZES = [1, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1025, 1030]                  # benign(n), one level
REFACTOR_ONE_LEVEL = (200, 130)                                                          # mild / planted (n, q)
SINGULAR_ONE_LEVEL = (200, 130)
TRANSPOSE_ONE_LEVEL = (200, 130, 0.5)                                                    # planted (n, q, upper)
TWO_LEVEL = dict(gx=16, gy=12, q=70)
