"""Adversarial CSR shapes for the SpMV family (csrc/spmv.hip, the csr_spmv_batch* kernels of csrc/batch.hip) -- TEST INFRASTRUCTURE.

Two seeded matrices with the same row-length plan (n about 12 000):

  ragged_empty   truly empty rows, no diagonal forced: PRECOND_NONE only, never solved
  ragged_dd      every row holds its diagonal, a_ii = 1 + 2 sum_{j != i} |a_ij| with mixed signs: solvable with point Jacobi

Stretches of rows with 0..8 random columns (the 2-byte coder gives up on their blocks) alternate with stretches of a fixed banded
stencil (coded), and scripted rows sit on top: long rows first, last and in succession, rows and blocks exactly at the 2048-entry
and 256-row caps, a whole block of empty rows, blocks with exactly 256 and 257 distinct column offsets.  events() names where
each of them is; tests/test_spmv_shapes.py asserts with the restatements below that the partitioner and the coder see them.

Restated from the library, in Python: build_rowblocks_host (row_blocks), the decision of build_spmv_codes_host (coded_blocks)
and the workgroup arithmetic of launch_range / csr_spmv_pipe_kernel (pipe_runs).

exact() is the reference: every product split into two doubles without error (Veltkamp / Dekker), every row summed with
math.fsum, so y = A x, r = b - A x and d = |A||x| + |b| are the correctly rounded exact values.  bound() is the rounding bound
e_i = (len_i + 2) 2^-52 d_i: len_i rounded products and len_i additions in ANY order stay within (len_i + 1) 2^-53 d_i to first
order, the rest covers the second-order terms and the reference's own final rounding.  Derived, not measured."""
from __future__ import annotations

import functools
import math

import numpy as np

LDS_NNZ = 2048          # NKP_SPMV_LDS_NNZ
MAX_ROWS = 256          # NKP_SPMV_MAX_ROWS
N = 12000
U = 2.0 ** -52

BAND = np.array([-3000, -1200, -1199, -601, -600, -599, -41, -40, -39, -2, -1, 0, 1, 2, 39, 40, 41, 599, 600, 601, 1199, 1200], np.int64)


# ---------------------------------------------------------------- restatements of the library's host code
def row_blocks(rowptr):
    """build_rowblocks_host: at most 256 rows and 2048 entries per block; a row that exceeds the budget stays alone."""
    rowptr = np.asarray(rowptr, np.int64)
    n = rowptr.size - 1
    rb = [0]
    r = 0
    while r < n:
        end = r + 1
        base = rowptr[r]
        while end < n and end - r < MAX_ROWS and rowptr[end + 1] - base <= LDS_NNZ:
            end += 1
        rb.append(end)
        r = end
    return np.array(rb, np.int64)


def block_offsets(rowptr, colind, rb):
    """Number of distinct (column - row) offsets of every row block."""
    rowptr = np.asarray(rowptr, np.int64)
    row_of = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    delta = np.asarray(colind, np.int64) - row_of
    return np.array([np.unique(delta[rowptr[rb[k]]:rowptr[rb[k + 1]]]).size for k in range(rb.size - 1)], np.int64)


def coded_blocks(rowptr, colind, rb):
    """build_spmv_codes_host's decision: coded iff <= 256 rows, <= 2048 entries and 1 .. 256 distinct offsets."""
    rowptr = np.asarray(rowptr, np.int64)
    cnt = rowptr[rb[1:]] - rowptr[rb[:-1]]
    nd = block_offsets(rowptr, colind, rb)
    return (np.diff(rb) <= 256) & (cnt <= LDS_NNZ) & (nd >= 1) & (nd <= 256)


def pipe_runs(nrowblk, run, wgs_per_cu=256):
    """The runs of row blocks [lb, lb_end) the workgroups of csr_spmv_pipe_kernel walk when launch_range covers nrowblk blocks
    with spmv_run = run (variant 4, at least spmv_pipe_min blocks)."""
    wgs = nrowblk // max(run, 1)
    wgs = min(wgs, 256 * wgs_per_cu) & ~7
    wgs = max(wgs, 8)
    wg_per_xcd = wgs >> 3
    per_xcd = (nrowblk + 7) // 8
    runs = []
    for xcd in range(8):
        xb0 = min(xcd * per_xcd, nrowblk)
        xb1 = min(xb0 + per_xcd, nrowblk)
        chunk = (xb1 - xb0 + wg_per_xcd - 1) // wg_per_xcd
        for idx in range(wg_per_xcd):
            lb = xb0 + idx * chunk
            lb_end = min(lb + chunk, xb1)
            if lb < lb_end:
                runs.append((lb, lb_end))
    return runs


# ---------------------------------------------------------------- the two matrices
class Shape:
    def __init__(self, name, rowptr, colind, val, marks):
        self.name, self.rowptr, self.colind, self.val, self.marks = name, rowptr, colind, val, marks
        self.n = rowptr.size - 1
        self.len = np.diff(rowptr.astype(np.int64))
        self.long = self.len > LDS_NNZ


def _pick(rng, r, length, dd):
    """`length` distinct sorted columns of row r, the diagonal among them when dd."""
    if dd:
        others = rng.choice(N - 1, size=length - 1, replace=False)
        others[others >= r] += 1
        return np.sort(np.append(others, r))
    return np.sort(rng.choice(N, size=length, replace=False))


def _build(dd):
    rng = np.random.default_rng(20 + dd)
    rows, marks = [], {}
    low = 1 if dd else 0                      # an "empty" row of ragged_dd is its diagonal alone

    def add(cols):
        rows.append(np.asarray(cols, np.int64))

    def scripted(length):
        add(_pick(rng, len(rows), max(length, low), dd))

    def mark(key):
        marks[key] = len(rows)

    def stretch_random(count):
        for _ in range(count):
            scripted(int(rng.integers(0, 9)))

    def stretch_band(count):
        for _ in range(count):
            c = len(rows) + BAND
            add(c[(c >= 0) & (c < N)])

    def stretches(upto):
        # the two kinds alternate in pieces of one to three row blocks
        k = 0
        while len(rows) < upto:
            left = upto - len(rows)
            if k % 2 == 0:
                stretch_random(min(left, int(rng.integers(200, 420))))
            else:
                stretch_band(min(left, int(rng.integers(90, 260))))
            k += 1

    def dictionary_block(distinct):
        # rows of the diagonal and three further offsets, every further offset used once: `distinct` offsets in the block
        pool = [(k // 2 + 1) * 11 * (1 if k % 2 else -1) for k in range(distinct - 1)]
        for q in range(0, len(pool), 3):
            r = len(rows)
            add(np.sort(r + np.array([0] + pool[q:q + 3], np.int64)))

    mark("long_first")
    scripted(3000)
    mark("empty_at_block_start")
    scripted(0)
    scripted(0)
    stretches(2900)
    mark("long_pair")
    scripted(5000)
    scripted(2049)
    for _ in range(3):
        scripted(3)
    mark("row_2048")
    scripted(2048)
    mark("row_2047_then_2")
    scripted(2047)
    mark("block_2048")
    scripted(2)
    scripted(1023)
    scripted(1023)
    mark("empty_at_block_end")
    scripted(0)
    scripted(0)
    scripted(5)
    stretches(6000)
    mark("long_before_dictionaries")
    scripted(2100)
    mark("dict_256")
    dictionary_block(256)
    scripted(2048)
    mark("dict_257")
    dictionary_block(257)
    mark("long_before_empty_block")
    scripted(2500)
    mark("empty_block")
    for _ in range(300):
        scripted(0)
    scripted(4)
    stretches(N - 2)
    mark("long_last")
    scripted(0)
    scripted(N // 2)
    assert len(rows) == N

    rowptr = np.concatenate([[0], np.cumsum([c.size for c in rows])]).astype(np.int32)
    colind = np.concatenate(rows).astype(np.int32)
    val = rng.standard_normal(colind.size)
    if dd:
        row_of = np.repeat(np.arange(N), np.diff(rowptr))
        diag = colind == row_of
        off = np.bincount(row_of[~diag], weights=np.abs(val[~diag]), minlength=N)
        sign = np.where(rng.random(N) < 0.5, -1.0, 1.0)
        val[diag] = (sign * (1.0 + 2.0 * off))[row_of[diag]]
    return Shape("ragged_dd" if dd else "ragged_empty", rowptr, colind, val, marks)


@functools.lru_cache(maxsize=None)
def ragged_empty():
    return _build(0)


@functools.lru_cache(maxsize=None)
def ragged_dd():
    return _build(1)


def refactored_values(shape, seed=5):
    """New values on the pattern of ragged_dd, the diagonal still dominant in the same way."""
    rng = np.random.default_rng(seed)
    val = rng.standard_normal(shape.colind.size)
    row_of = np.repeat(np.arange(shape.n), shape.len)
    diag = shape.colind == row_of
    off = np.bincount(row_of[~diag], weights=np.abs(val[~diag]), minlength=shape.n)
    sign = np.where(rng.random(shape.n) < 0.5, -1.0, 1.0)
    val[diag] = (sign * (1.0 + 2.0 * off))[row_of[diag]]
    return val


# ---------------------------------------------------------------- exact reference
def _two_prod(a, b):
    """a * b = p + e exactly (Veltkamp split, Dekker's product); the inputs here are far from over- and underflow."""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah = ca - (ca - a)
    bh = cb - (cb - b)
    al, bl = a - ah, b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


class Exact:
    """y = A x, r = b - A x, d = |A||x| + |b| correctly rounded, and the bound e of every row (module docstring)."""

    def __init__(self, rowptr, colind, val, x, b=None):
        rowptr = np.asarray(rowptr, np.int64)
        n = rowptr.size - 1
        x = np.asarray(x, np.float64)
        bb = np.zeros(n) if b is None else np.asarray(b, np.float64)
        p, e = _two_prod(np.asarray(val, np.float64), x[np.asarray(colind, np.int64)])
        s = np.where(p < 0.0, -1.0, 1.0)
        ap, ae = s * p, s * e                 # |p + e| = sign (p) (p + e): |e| <= ulp (p) / 2
        self.y, self.r, self.d = np.empty(n), np.empty(n), np.empty(n)
        ends = rowptr.tolist()
        for i in range(n):
            a, z = ends[i], ends[i + 1]
            terms = p[a:z].tolist() + e[a:z].tolist()
            self.y[i] = math.fsum(terms)
            terms.append(-bb[i])
            self.r[i] = -math.fsum(terms)             # rounding to nearest is symmetric: -(A x - b) rounded is b - A x rounded
            self.d[i] = math.fsum(ap[a:z].tolist() + ae[a:z].tolist() + [abs(bb[i])])
        self.e = (np.diff(rowptr) + 2) * U * self.d


def exact(shape, x, b=None, val=None):
    return Exact(shape.rowptr, shape.colind, shape.val if val is None else val, x, b)


def vectors(shape, seed=1):
    """x0 and a right-hand side without a zero entry, the same for every test that asks."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape.n)
    b = rng.standard_normal(shape.n)
    b[b == 0.0] = 1.0
    return x, b


def solve_rhs(shape, count=5):
    """Right-hand sides of the solves on ragged_dd: systems of a group leave it at different steps."""
    B = np.random.default_rng(11).standard_normal((count, shape.n))
    B[2] *= 1e-3
    return B
