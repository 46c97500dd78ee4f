"""Checks of a hierarchy against the identities that define it, shared by tests/test_ml_plan.py, tests/test_gpu_cycle_options.py
and tests/test_gpu_setup_options.py.  TEST INFRASTRUCTURE."""
import numpy as np
import scipy.sparse as sp

import ml_reference as mlr

EPS = 2.0 ** -52


def same_partition(a, b):
    """two labelings of the same items describe the same partition"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if a.size != b.size:
        return False
    pairs = np.unique(a * (int(b.max()) + 1) + b)
    return pairs.size == np.unique(a).size == np.unique(b).size


def check_structure(levels, s):
    """Every level against the one above it (f64 storage: the device keeps the f64 values)."""
    for l, lv in enumerate(levels):
        n = lv.n
        if lv.col_of is not None:
            blk = lv.blk_start
            assert blk[0] == 0 and blk[-1] == n and (np.diff(blk) > 0).all(), l
            cb = s.ml_level_array(l, "color_blk")
            assert cb.size == 3 and cb[0] == 0 and 0 <= cb[1] <= cb[2] == blk.size - 1, (l, cb)
        if l == len(levels) - 1:
            break
        nc = levels[l + 1].n
        cmap, rptr, ridx = (s.ml_level_array(l, what).astype(np.int64) for what in ("cmap", "rptr", "ridx"))
        assert cmap.size == n and cmap.min() == 0 and cmap.max() == nc - 1, l
        assert rptr.size == nc + 1 and rptr[0] == 0 and rptr[-1] == n and (np.diff(rptr) > 0).all(), l
        assert np.array_equal(np.sort(ridx), np.arange(n)), l                              # each fine row once
        assert np.array_equal(cmap[ridx], np.repeat(np.arange(nc), np.diff(rptr))), l      # ... under its own coarse row
        # Galerkin: a stored entry is a sum of m fine entries in some order, so it is within m * 2^-52 * sum |terms| of any
        # other evaluation of that sum (the textbook bound; this product is one more such evaluation)
        P = lv.P
        ones = lv.L.copy()
        ones.data[:] = 1.0
        D = abs(levels[l + 1].L - P.T @ lv.L @ P)
        bound = (P.T @ ones @ P).multiply(P.T @ abs(lv.L) @ P) * EPS
        excess = (D - bound).tocoo()
        assert not (excess.data > 0).any(), (l, excess.data.max())


def check_twin(level0, prob):
    """Level 0, rows back in their original order, is the low-order twin of A."""
    p = prob.p
    colid = np.cumsum(p.ind_k == 0) - 1
    want = mlr.low_order(p.scipy_csr(), colid)
    C = level0.L.tocoo()
    got = sp.csr_matrix((C.data, (level0.perm0[C.row], level0.perm0[C.col])), shape=C.shape)
    excess = (abs(got - want) - 4 * EPS * abs(want)).tocoo()
    assert not (excess.data > 0).any(), excess.data.max()
