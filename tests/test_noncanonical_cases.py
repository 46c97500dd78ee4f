"""The claims of tests/noncanonical_cases.py about its own data, without a GPU: what tests/test_gpu_noncanonical.py relies on."""
import numpy as np
import pytest

import noncanonical_cases as nc
import spmv_shapes as sh


def rows_of(v):
    return [v.colind[a:b].astype(np.int64) for a, b in zip(v.rowptr[:-1], v.rowptr[1:])]


def test_base_matrix():
    v = nc.variant("canonical")
    assert nc.LENGTHS == (1, 2, 5, 33, 63, 64, 65, 127, 128, 10) and v.n == 498 and nc.BLK[-1] == 498
    row, col = nc.pattern()
    assert all(np.all(np.diff(r) > 0) for r in rows_of(v))                                    # strictly ascending
    A = nc.dense(v.rowptr, v.colind, v.val)
    for c in range(nc.NCOL):
        for k in range(nc.LENGTHS[c]):
            r = int(nc.BLK[c]) + k
            want = {r + d for d in range(-2, 3) if 0 <= k + d < nc.LENGTHS[c]}
            for nb in ((c - 1) % nc.NCOL, (c + 1) % nc.NCOL):
                want |= {int(nc.BLK[nb]) + kk for kk in (k - 1, k, k + 1) if 0 <= kk < nc.LENGTHS[nb]}   # no clamping
            assert set(col[row == r].tolist()) == want, r
    off = A - np.diag(np.diag(A))
    mag = np.abs(off[off != 0.0])
    assert mag.min() >= 0.1 and mag.max() <= 1.0 and np.any(off > 0) and np.any(off < 0)
    # a_ii = 1 + sum |a_ij|, up to the order of a sum of at most 11 terms
    assert np.all(np.abs(np.diag(A) - (1.0 + np.abs(off).sum(axis=1))) <= 12 * 2.0 ** -52 * np.diag(A))
    assert nc.band_measure(v) == (2, 0)


def test_row_orders():
    canon = rows_of(nc.variant("canonical"))
    rev, shuf = rows_of(nc.variant("reversed")), rows_of(nc.variant("shuffled"))
    adj, apart = nc.variant("split_adjacent"), nc.variant("split_apart")
    assert all(np.array_equal(r[::-1], c) for r, c in zip(rev, canon))
    assert all(np.array_equal(np.sort(r), c) for r, c in zip(shuf, canon))
    unsorted = sum(1 for r in shuf if np.any(np.diff(r) < 0))
    assert unsorted >= 0.9 * sum(1 for c in canon if c.size >= 4)
    # split_adjacent: non-descending everywhere, a repeated column in almost every row, the halves side by side
    assert all(np.all(np.diff(r) >= 0) for r in rows_of(adj))
    assert sum(1 for r in rows_of(adj) if np.any(np.diff(r) == 0)) >= 0.9 * nc.N
    assert adj.nnz == apart.nnz == nc.variant("canonical").nnz + (nc.variant("canonical").nnz + 2) // 3
    # split_apart: the two halves of a split entry sit symmetrically about the middle of the row, the rest is shuffled
    for v in (adj, apart):
        L = v.layout
        half = L.scale == 0.5
        assert np.all(v.val[half] == 0.5 * nc.canonical_values(nc.VALUE_SEED)[L.src[half]])
        assert np.all(np.bincount(L.src[half]) [np.unique(L.src[half])] == 2)
    L = apart.layout
    for r in range(nc.N):
        a, b = int(apart.rowptr[r]), int(apart.rowptr[r + 1])
        m = int(np.sum(L.scale[a:b] == 0.5)) // 2
        assert np.all(L.scale[a:a + m] == 0.5) and np.all(L.scale[b - m:b] == 0.5) and np.all(L.scale[a + m:b - m] == 1.0)
        assert np.array_equal(L.src[a:a + m], L.src[b - m:b][::-1])
    assert sum(1 for r in rows_of(apart) if np.any(np.diff(r) < 0)) >= 0.9 * nc.N
    # the split entries include diagonals and in-band off-diagonals
    row, col = nc.pattern()
    split = np.arange(row.size) % 3 == 0
    same_col = np.searchsorted(nc.BLK, row, side="right") == np.searchsorted(nc.BLK, col, side="right")
    assert np.sum(split & (row == col)) >= 100 and np.sum(split & same_col & (row != col)) >= 100 and np.sum(split & ~same_col) >= 100


def test_stored_zeros():
    canon = nc.variant("canonical")
    for name in ("zeros_near", "zeros_wide"):
        v = nc.variant(name)
        assert all(np.all(np.diff(r) > 0) for r in rows_of(v))
        zero = v.layout.src < 0
        assert zero.sum() == v.nnz - canon.nnz > 0 and np.all(v.val[zero] == 0.0) and not np.any(np.signbit(v.val[zero]))
        assert np.all(v.val[~zero] != 0.0)
    near, wide = nc.variant("zeros_near"), nc.variant("zeros_wide")
    for v, inside in ((near, False), (wide, True)):
        zero = v.layout.src < 0
        row, col = v.layout.row[zero], v.colind[zero].astype(np.int64)
        cr, cc = np.searchsorted(nc.BLK, row, side="right") - 1, np.searchsorted(nc.BLK, col, side="right") - 1
        assert np.all((cr == cc) == inside)
        if inside:
            assert set(np.abs(col - row).tolist()) == {3, 5} and np.all(np.array(nc.LENGTHS)[cr] >= 6)
        else:
            assert np.all(((cc - cr) % nc.NCOL == 1) | ((cr - cc) % nc.NCOL == 1))
            assert set(np.abs((col - nc.BLK[cc]) - (row - nc.BLK[cr])).tolist()) == {2}
    assert nc.band_measure(near) == (2, 0)
    assert nc.band_measure(wide) == (5, 0)                   # stored as P = 4 with the dropped flag
    band, dropped = nc.band_extraction(wide, 4)
    assert dropped == 1
    row, col = wide.layout.row, wide.colind.astype(np.int64)
    gone = (np.searchsorted(nc.BLK, row, side="right") == np.searchsorted(nc.BLK, col, side="right")) & (np.abs(col - row) > 4)
    assert gone.any() and np.all(wide.val[gone] == 0.0)      # everything dropped is zero
    b2, _ = nc.band_extraction(nc.variant("canonical"), 2)
    assert np.array_equal(band[2:7].view(np.uint64), b2.view(np.uint64)) and not band[:2].any() and not band[7:].any()


def test_variants_are_one_matrix_bit_for_bit():
    for seed in (nc.VALUE_SEED, nc.OTHER_SEED):
        want = nc.dense(nc.variant("canonical", seed).rowptr, nc.variant("canonical", seed).colind, nc.variant("canonical", seed).val)
        for name in nc.SAME_SUM:
            v = nc.variant(name, seed)
            assert np.array_equal(nc.dense(v.rowptr, v.colind, v.val).view(np.uint64), want.view(np.uint64)), (name, seed)
            assert np.array_equal(v.rowptr, nc.variant(name).rowptr) and np.array_equal(v.colind, nc.variant(name).colind)   # same stored pattern
    assert not np.array_equal(nc.variant("canonical", nc.OTHER_SEED).val, nc.variant("canonical").val)


def test_band_extraction_has_the_bits_of_canonical():
    want, dropped = nc.band_extraction(nc.variant("canonical"), 2)
    assert dropped == 0
    for name in nc.SAME_BAND_BITS:
        got, dropped = nc.band_extraction(nc.variant(name), 2)
        assert dropped == 0 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), name
        assert nc.band_measure(nc.variant(name)) == (2, 0)


def test_singular_pair():
    s, a = nc.variant("singular_pair"), nc.variant("split_apart")
    assert np.array_equal(s.rowptr, a.rowptr) and np.array_equal(s.colind, a.colind)
    differ = np.flatnonzero(s.val != a.val)
    assert differ.size == 2 and np.all(s.colind[differ] == nc.SINGULAR_ROW) and np.all(s.layout.row[differ] == nc.SINGULAR_ROW)
    assert s.val[differ].tolist() == [1.0, -1.0] and differ[1] - differ[0] > 1            # apart, +1 first
    assert nc.BLK[4] <= nc.SINGULAR_ROW < nc.BLK[5]
    assert nc.band_measure(s) == (2, 1)
    assert nc.dense(s.rowptr, s.colind, s.val)[nc.SINGULAR_ROW, nc.SINGULAR_ROW] == 0.0


def test_condition_number():
    k = nc.kappa2()
    print(f"kappa_2 = {k:.3f}, with the other values {nc.kappa2(nc.OTHER_SEED):.3f}")
    assert k <= 100.0 and nc.kappa2(nc.OTHER_SEED) <= 100.0


def test_which_variants_the_diagonal_layout_accepts():
    for name in nc.VARIANTS:
        ok, most, pad = nc.diag_layout_accepts(nc.variant(name), nc.DIAG_CAP)
        print(f"{name}: accepted {ok}, most keys {most}, padding / nnz {pad:.3f}")
        assert ok == (name in nc.ASCENDING), name
        assert most <= nc.DIAG_CAP                                # the rows refuse the other variants, not the cap
    assert not nc.diag_layout_accepts(nc.variant("canonical"), 8)[0]


def test_references():
    """the longdouble elimination solves to longdouble accuracy, Exact takes repeated entries, the transpose keeps them"""
    x = nc.solution()
    assert x.dtype == np.longdouble and nc.relative_residual(x) <= 64 * float(np.finfo(np.longdouble).eps) * nc.kappa2()
    xt = nc.solution(transpose=True)
    assert nc.relative_residual(xt, transpose=True) <= 64 * float(np.finfo(np.longdouble).eps) * nc.kappa2()
    xv, b = nc.vectors()
    canon, apart = nc.variant("canonical"), nc.variant("split_apart")
    ec, ea = sh.exact(canon, xv, b), sh.exact(apart, xv, b)
    assert np.array_equal(ec.y, ea.y) and np.array_equal(ec.r, ea.r) and np.array_equal(ec.d, ea.d)   # the same exact sums, correctly rounded
    assert np.all(ea.e >= ec.e) and np.any(ea.e > ec.e)                                                # the stored length is in the bound
    rp, ci, v = nc.transposed_csr(apart)
    assert np.array_equal(nc.dense(rp, ci, v), nc.dense(apart.rowptr, apart.colind, apart.val).T) and ci.size == apart.nnz
    r, z, d = nc.block_reference()
    A = nc.dense_sum()
    for a, e in zip(nc.BLK[:-1], nc.BLK[1:]):
        res = A[a:e, a:e] @ z[a:e] - r[a:e]
        assert float(np.abs(res).max()) <= 1e-17 * max(1.0, float(np.abs(r[a:e]).max())) * 64
    assert 0.0 < d < 1e-13
