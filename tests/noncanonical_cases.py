"""One matrix stored in eight ways: unsorted rows, repeated columns and stored zeros for every reader of A -- TEST INFRASTRUCTURE.

include/nkp.h (nkp_create): A is the sum of its stored entries; NKP_PRECOND_NONE and NKP_PRECOND_COLUMN_JACOBI take rows in any
order, repeated columns and stored zeros.  tests/test_noncanonical_cases.py checks the claims below without a GPU,
tests/test_gpu_noncanonical.py runs the variants through the kernels.

Base matrix.  Ten water columns on a ring, LENGTHS = 1, 2, 5, 33, 63, 64, 65, 127, 128, 10 rows (n = 498): both sides of the
64-row wave boundary, the 128-row limit, one- and two-row columns, neighbours of very different length.  Row k of column c holds
the in-column offsets -2 .. 2 and rows k - 1, k, k + 1 of columns c - 1 and c + 1 (mod 10) where they exist, nothing clamped.
Off-diagonals: magnitude U(0.1, 1), random sign; a_ii = 1 + sum_j |a_ij|, so every row is strictly dominant and kappa_2 is small
(computed in the CPU test).  The pattern and the stored order of every variant depend on ORDER_SEED alone, the values on the seed
given: values(name, seed) gives other values on the same stored pattern (nkp_refactor).

Variants, all the same matrix as a sum of stored entries (halving is exact, and 0 + a/2 + a/2 == a exactly):
  canonical        rows strictly ascending
  reversed         every row in descending column order
  shuffled         a seeded permutation per row
  split_adjacent   every third stored entry (canonical position % 3 == 0) stored twice as a/2, a/2, side by side: rows
                   non-descending, not strictly ascending
  split_apart      shuffled, the same entries split, first halves at the front of the row and second halves at its back in
                   the opposite order
  zeros_near       canonical plus a stored 0.0 at rows k - 2 and k + 2 of the neighbour columns
  zeros_wide       canonical plus a stored 0.0 at the in-column offsets +-3 and +-5 in columns of 6 rows or more: the measured
                   half bandwidth is 5, the band factors keep 4 and report dropped entries, all of them zero
  singular_pair    split_apart with the two halves of one split diagonal stored as +1, -1 (row SINGULAR_ROW): NOT the same sum

References: spmv_shapes.Exact on the stored entries (bound (len_i + 2) 2^-52 d_i with the STORED length, valid for any order of
summation and for repeated entries), a dense longdouble elimination of the summed matrix for solutions, and per-block dense
longdouble solves for the preconditioner."""
from __future__ import annotations

import functools

import numpy as np

LENGTHS = (1, 2, 5, 33, 63, 64, 65, 127, 128, 10)
BLK = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int32)
N = int(BLK[-1])
NCOL = len(LENGTHS)
ORDER_SEED = 4242
VALUE_SEED = 7
OTHER_SEED = 19
VARIANTS = ("canonical", "reversed", "shuffled", "split_adjacent", "split_apart", "zeros_near", "zeros_wide", "singular_pair")
SAME_SUM = VARIANTS[:-1]
ASCENDING = ("canonical", "zeros_near", "zeros_wide")                # strictly ascending rows: the per-column diagonals take them
SAME_BAND_BITS = ("reversed", "shuffled", "split_adjacent", "split_apart", "zeros_near")
DIAG_CAP = 32


# ---------------------------------------------------------------- the canonical pattern
@functools.lru_cache(maxsize=None)
def pattern():
    """(row, col) of the canonical entries, rows strictly ascending"""
    rows, cols = [], []
    for c in range(NCOL):
        for k in range(LENGTHS[c]):
            r = int(BLK[c]) + k
            mine = [r + d for d in range(-2, 3) if 0 <= k + d < LENGTHS[c]]
            for nb in ((c - 1) % NCOL, (c + 1) % NCOL):
                mine += [int(BLK[nb]) + kk for kk in (k - 1, k, k + 1) if 0 <= kk < LENGTHS[nb]]
            mine = sorted(mine)
            assert len(set(mine)) == len(mine)
            rows += [r] * len(mine)
            cols += mine
    return np.array(rows, np.int64), np.array(cols, np.int64)


@functools.lru_cache(maxsize=None)
def canonical_values(seed):
    row, col = pattern()
    rng = np.random.default_rng(seed)
    val = rng.uniform(0.1, 1.0, row.size) * rng.choice(np.array([-1.0, 1.0]), row.size)
    diag = row == col
    val[diag] = 0.0
    val[diag] = 1.0 + np.bincount(row, weights=np.abs(val), minlength=N)
    return val


def column_of(r):
    return int(np.searchsorted(BLK, r, side="right") - 1)


def zero_columns(name, r):
    """columns of the stored zeros of row r"""
    c = column_of(r)
    k = r - int(BLK[c])
    if name == "zeros_near":
        return [int(BLK[nb]) + kk for nb in ((c - 1) % NCOL, (c + 1) % NCOL) for kk in (k - 2, k + 2) if 0 <= kk < LENGTHS[nb]]
    if name == "zeros_wide" and LENGTHS[c] >= 6:
        return [r + d for d in (-5, -3, 3, 5) if 0 <= k + d < LENGTHS[c]]
    return []


# ---------------------------------------------------------------- stored order
class Layout:
    """The stored entries of one variant: src = canonical entry (-1: a stored zero), scale = 1 or 1/2."""

    def __init__(self, name, rowptr, colind, src, scale, fixed):
        self.name, self.rowptr, self.colind, self.src, self.scale, self.fixed = name, rowptr, colind, src, scale, fixed
        self.n, self.nnz = N, colind.size
        self.row = np.repeat(np.arange(N, dtype=np.int64), np.diff(rowptr.astype(np.int64)))


def _singular_row():
    """the first row in the lower half of the 63-row column whose diagonal is one of the split entries"""
    row, col = pattern()
    at = np.flatnonzero((row == col) & (np.arange(row.size) % 3 == 0) & (row >= int(BLK[4]) + 31))
    return int(row[at[0]])


SINGULAR_ROW = _singular_row()


@functools.lru_cache(maxsize=None)
def layout(name):
    row, col = pattern()
    rng = np.random.default_rng(ORDER_SEED)                           # the same permutations for shuffled, split_apart and singular_pair
    split = np.arange(row.size) % 3 == 0
    starts = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=N))])
    rowptr, colind, src, scale, fixed = [0], [], [], [], {}
    for r in range(N):
        ids = list(range(int(starts[r]), int(starts[r + 1])))
        perm = [ids[q] for q in rng.permutation(len(ids))]
        if name in ("canonical", "zeros_near", "zeros_wide"):
            ent = [(int(col[e]), e, 1.0) for e in ids] + [(z, -1, 0.0) for z in zero_columns(name, r)]
            ent.sort()
        elif name == "reversed":
            ent = [(int(col[e]), e, 1.0) for e in reversed(ids)]
        elif name == "shuffled":
            ent = [(int(col[e]), e, 1.0) for e in perm]
        elif name == "split_adjacent":
            ent = []
            for e in ids:
                ent += [(int(col[e]), e, 0.5)] * 2 if split[e] else [(int(col[e]), e, 1.0)]
        elif name in ("split_apart", "singular_pair"):
            halves = [(int(col[e]), e, 0.5) for e in perm if split[e]]
            ent = halves + [(int(col[e]), e, 1.0) for e in perm if not split[e]] + halves[::-1]
            if name == "singular_pair" and r == SINGULAR_ROW:
                at = [q for q, t in enumerate(ent) if t[0] == r]
                assert len(at) == 2, "the diagonal of SINGULAR_ROW must be a split entry"
                fixed[len(colind) + at[0]], fixed[len(colind) + at[1]] = 1.0, -1.0
        else:
            raise KeyError(name)
        colind += [t[0] for t in ent]
        src += [t[1] for t in ent]
        scale += [t[2] for t in ent]
        rowptr.append(len(colind))
    return Layout(name, np.array(rowptr, np.int32), np.array(colind, np.int32), np.array(src, np.int64), np.array(scale), fixed)


def values(name, seed=VALUE_SEED):
    """the stored values of a variant for the canonical values of `seed`"""
    L = layout(name)
    base = canonical_values(seed)
    val = np.where(L.src >= 0, base[np.maximum(L.src, 0)] * L.scale, 0.0)
    for at, v in L.fixed.items():
        val[at] = v
    return val


class Variant:
    def __init__(self, name, seed=VALUE_SEED):
        L = layout(name)
        self.name, self.layout, self.rowptr, self.colind, self.n, self.nnz = name, L, L.rowptr, L.colind, N, L.nnz
        self.val = values(name, seed)
        self.blk = BLK
        self.len = np.diff(L.rowptr.astype(np.int64))


@functools.lru_cache(maxsize=None)
def variant(name, seed=VALUE_SEED):
    return Variant(name, seed)


def dense(rowptr, colind, val, dtype=np.float64):
    """the sum of the stored entries, added in stored order"""
    n = rowptr.size - 1
    A = np.zeros((n, n), dtype)
    row = np.repeat(np.arange(n), np.diff(np.asarray(rowptr, np.int64)))
    np.add.at(A, (row, np.asarray(colind, np.int64)), np.asarray(val, dtype))
    return A


def transposed_csr(v):
    """A^T with the stored entries of v, every row in the order of the rows they come from (repeated entries stay repeated)"""
    row, col = v.layout.row, v.colind.astype(np.int64)
    order = np.lexsort((np.arange(col.size), row, col))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=v.n))]).astype(np.int32)
    return rowptr, row[order].astype(np.int32), v.val[order]


# ---------------------------------------------------------------- restatements
def band_measure(v):
    """colblock_measure_kernel: (largest in-block |col - row|, rows whose summed diagonal is zero)"""
    row, col = v.layout.row, v.colind.astype(np.int64)
    cr, cc = np.searchsorted(BLK, row, side="right"), np.searchsorted(BLK, col, side="right")
    inside = cr == cc
    diag = np.zeros(v.n)
    np.add.at(diag, row[row == col], v.val[row == col])
    return int(np.abs(col - row)[inside].max()), int(np.sum(diag == 0.0))


def band_extraction(v, P):
    """colblock_factor_kernel's extraction: in-block entries with |col - row| <= P added in stored order to +0.0; returns
    (band[2 P + 1, n], dropped)"""
    row, col = v.layout.row, v.colind.astype(np.int64)
    inside = np.searchsorted(BLK, row, side="right") == np.searchsorted(BLK, col, side="right")
    d = col - row
    keep = inside & (np.abs(d) <= P)
    band = np.zeros((2 * P + 1, v.n))
    np.add.at(band, (d[keep] + P, row[keep]), v.val[keep])
    return band, int(np.any(inside & (np.abs(d) > P)))


def diag_layout_accepts(v, cap=DIAG_CAP):
    """The rules by which diag_build (csrc/diagop.hip) puts A on per-column diagonals, as tests/test_gpu_spmv_diag.py checks them
    on the device's arrays: strictly ascending rows, key = column - position of the row in its water column, at most `cap`
    distinct keys per column, columns of at most 256 rows, and values with padding at most 1.5 nnz.  Returns (accepted, most
    keys, padding / nnz)."""
    row, col = v.layout.row, v.colind.astype(np.int64)
    same_row = np.diff(row) == 0
    ascending = bool(np.all(np.diff(col)[same_row] > 0))
    c = np.searchsorted(BLK, row, side="right") - 1
    key = col - (row - BLK[c])
    nk = np.array([np.unique(key[c == q]).size for q in range(NCOL)])
    nval = int(np.sum(nk * np.array(LENGTHS)))
    ok = ascending and nk.max() <= cap and max(LENGTHS) <= 256 and 2 * nval <= 3 * v.nnz
    return ok, int(nk.max()), nval / v.nnz


# ---------------------------------------------------------------- references
LD = np.longdouble


def ld_solve(A, B):
    """A X = B by Gaussian elimination with partial pivoting, every operation in longdouble; B: (n,) or (n, k)"""
    A = np.array(A, LD)
    X = np.array(B, LD).reshape(A.shape[0], -1)
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            X[[k, p]] = X[[p, k]]
        m = A[k + 1:, k] / A[k, k]
        A[k + 1:, k + 1:] -= np.outer(m, A[k, k + 1:])
        X[k + 1:] -= np.outer(m, X[k])
    for k in range(n - 1, -1, -1):
        X[k] = (X[k] - A[k, k + 1:] @ X[k + 1:]) / A[k, k]
    return X.reshape(np.shape(B))


@functools.lru_cache(maxsize=None)
def dense_sum(seed=VALUE_SEED, transpose=False):
    v = variant("canonical", seed)
    A = dense(v.rowptr, v.colind, v.val, LD)
    return A.T.copy() if transpose else A


@functools.lru_cache(maxsize=None)
def kappa2(seed=VALUE_SEED):
    s = np.linalg.svd(np.array(dense_sum(seed), np.float64), compute_uv=False)
    return float(s[0] / s[-1])


def vectors(seed=1):
    """x of the products and b of the solves, b without a zero"""
    rng = np.random.default_rng(seed)
    x, b = rng.standard_normal(N), rng.standard_normal(N)
    b[b == 0.0] = 1.0
    return x, b


@functools.lru_cache(maxsize=None)
def solution(seed=VALUE_SEED, transpose=False, rhs_seed=1):
    """x_ref = A^-1 b (A^-T b) in longdouble for b = vectors(rhs_seed)[1]"""
    return ld_solve(dense_sum(seed, transpose), vectors(rhs_seed)[1])


def relative_residual(x, seed=VALUE_SEED, transpose=False, rhs_seed=1):
    """rho = ||b - A x|| / ||b|| in longdouble from the dense sum"""
    b = np.asarray(vectors(rhs_seed)[1], LD)
    r = b - dense_sum(seed, transpose) @ np.asarray(x, LD)
    return float(np.sqrt(r @ r) / np.sqrt(b @ b))


@functools.lru_cache(maxsize=None)
def block_reference(seed=VALUE_SEED, rhs_seed=17):
    """(r, z_ref, d): z_ref = the per-block longdouble solves of r; d = the yardstick of the f64 bound max (1e-12, 4096 d) of
    tests/test_gpu_cycle_options.py, from the reference alone: f64 LU solves of the blocks against their explicit inverses"""
    r = np.random.default_rng(rhs_seed).standard_normal(N)
    A = dense_sum(seed)
    z, z_lu, z_inv = np.empty(N, LD), np.empty(N), np.empty(N)
    for a, b in zip(BLK[:-1], BLK[1:]):
        B = A[a:b, a:b]
        z[a:b] = ld_solve(B, r[a:b])
        B64 = np.array(B, np.float64)
        z_lu[a:b] = np.linalg.solve(B64, r[a:b])
        z_inv[a:b] = np.linalg.inv(B64) @ r[a:b]
    d = float(np.linalg.norm(z_inv - z_lu) / np.linalg.norm(z_lu))
    return r, z, d
