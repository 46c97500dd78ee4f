"""What nkp_create refuses and what it takes (the contract at nkp_create in include/nkp.h), line by line, without a GPU.

create_impl validates on the host before it touches the device (check_arguments, check_rows, check_blocks of csrc/create.hip),
so a refusal shows its code and message on any host.  Accepted input then reaches the device: on a host without a GPU that is
NKP_EDEVICE "no HIP device", on a GPU host success -- accepted() covers both and frees what was created.  Every call goes through
ctypes, with one tiny matrix (n <= 8, the two block-length lines 128 and 129 rows of a diagonal matrix) per line.

A is the sum of its stored entries.  NKP_PRECOND_NONE and NKP_PRECOND_COLUMN_JACOBI take rows in any order, repeated columns and
stored zeros; NKP_PRECOND_MULTILEVEL takes strictly ascending rows only.  The diagonal the two preconditioners need is judged on
the sum of the row's diagonal entries: check_rows sums them, so +1, -1 is refused before the device.

On the parent commit check_rows never compared a row's non-zero diagonal entry with its predecessor: the two diagonal lines
under MULTILEVEL (`diagonal_out_of_order`, row 3 stored as [5, 3], and `repeated_diagonal`, [3, 3]) were accepted there, with
nkp_create and with nkp_create64, and the +1, -1 diagonal passed every check (either entry is non-zero).  Failed on the parent
commit, measured on a GPU host (all five returned 0 and a solver); every other line passes on both:
  test_multilevel_refuses_rows_that_are_not_strictly_ascending [diagonal_out_of_order], [repeated_diagonal]
  test_create64_shares_the_order_test [diagonal_out_of_order]
  test_a_repeated_diagonal_is_an_order_error_under_multilevel_whatever_its_sum
  test_a_zero_diagonal_is_singular_under_column_jacobi [plus_minus_one]
Under MULTILEVEL a diagonal stored as +1, -1 repeats a column, so the order test refuses it (NKP_EINVAL) before the diagonal
test can (NKP_ESINGULAR): both are a refusal before the device.
"""
import ctypes as C

import numpy as np
import pytest

from nk_ocn_tracer_jacobian_precond_amd import solver

NONE, JACOBI, MULTILEVEL = solver.PRECOND_NONE, solver.PRECOND_COLUMN_JACOBI, solver.PRECOND_MULTILEVEL
EINVAL, EDEVICE, ESINGULAR = -1, -3, -4
N = 6


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def create(precond, rowptr, colind, val, blk=None, n=None, nnz=None, nblk=None, wide=False, out=True, options=None):
    """nkp_create (wide: nkp_create64) through ctypes; returns (code, message).  What was created is destroyed."""
    lib = solver.load_library()
    opt = solver.default_options(precond=precond, **(options or {}))
    rowptr = None if rowptr is None else np.ascontiguousarray(rowptr, np.int64 if wide else np.int32)
    colind = None if colind is None else np.ascontiguousarray(colind, np.int32)
    val = None if val is None else np.ascontiguousarray(val, np.float64)
    blk = None if blk is None else np.ascontiguousarray(blk, np.int32)
    n = rowptr.size - 1 if n is None else n
    nblk = (0 if blk is None else blk.size - 1) if nblk is None else nblk
    h = C.c_void_p()
    href = C.byref(h) if out else None
    if wide:
        rc = lib.nkp_create64(href, C.byref(opt), n, ptr(rowptr, C.c_int64), ptr(colind, C.c_int32), ptr(val, C.c_double), ptr(blk, C.c_int32), nblk, 1)
    else:
        nnz = (0 if colind is None else colind.size) if nnz is None else nnz
        rc = lib.nkp_create(href, C.byref(opt), n, nnz, ptr(rowptr, C.c_int32), ptr(colind, C.c_int32), ptr(val, C.c_double), ptr(blk, C.c_int32), nblk, 1)
    message = solver.last_error() if rc else ""
    if rc == 0:
        assert h.value
        lib.nkp_destroy(h)
    else:
        assert not h.value
    return rc, message


def accepted(result):
    """the validation let the matrix through: created on a GPU host, "no HIP device" on a host without one"""
    rc, message = result
    if solver.device_count() > 0:
        return rc == 0
    return rc == EDEVICE and "no HIP device" in message


def refused(result, code, fragment):
    rc, message = result
    return rc == code and fragment in message


def csr(rows):
    """rows: one list of (column, value) per row, stored in the order given"""
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    colind = np.array([c for r in rows for c, _ in r], np.int32)
    val = np.array([v for r in rows for _, v in r], np.float64)
    return rowptr, colind, val


def base_rows():
    """6 rows, tridiagonal and diagonally dominant, strictly ascending"""
    return [[(c, 4.0 if c == r else -1.0) for c in (r - 1, r, r + 1) if 0 <= c < N] for r in range(N)]


def with_row3(entries):
    rows = base_rows()
    rows[3] = entries
    return csr(rows)


def diagonal_matrix(n):
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.full(n, 2.0)


def test_the_base_matrix_is_accepted_by_the_flat_preconditioners():
    for precond in (NONE, JACOBI):
        assert accepted(create(precond, *csr(base_rows()))), precond


# ---------------------------------------------------------------- arguments
def test_out_is_null():
    assert refused(create(NONE, *csr(base_rows()), out=False), EINVAL, "out is NULL")


def test_struct_size_mismatch():
    size = C.sizeof(solver.NkpOptions)
    assert refused(create(NONE, *csr(base_rows()), options=dict(struct_size=size - 4)), EINVAL, "struct_size mismatch")


def test_unknown_preconditioner():
    assert refused(create(2, *csr(base_rows())), EINVAL, "unknown preconditioner 2")


def test_negative_n():
    rp, ci, v = csr(base_rows())
    assert refused(create(NONE, rp, ci, v, n=-1), EINVAL, "bad matrix arguments")


@pytest.mark.parametrize("missing", ["colind", "val"])
def test_entries_without_their_arrays(missing):
    rp, ci, v = csr(base_rows())
    nnz = ci.size
    if missing == "colind":
        ci = None
    else:
        v = None
    assert refused(create(NONE, rp, ci, v, nnz=nnz), EINVAL, "bad matrix arguments")


# ---------------------------------------------------------------- row pointers
def test_rowptr_does_not_start_at_zero():
    rp, ci, v = csr(base_rows())
    rp = rp.copy()
    rp[0] = 1
    assert refused(create(NONE, rp, ci, v), EINVAL, "rowptr[0]=1")


def test_rowptr_does_not_end_at_nnz():
    rp, ci, v = csr(base_rows())
    rp = rp.copy()
    rp[-1] -= 1
    assert refused(create(NONE, rp, ci, v), EINVAL, "rowptr[n]=%d inconsistent with nnz=%d" % (rp[-1], ci.size))


def test_rowptr_decreases_and_the_lowest_row_is_named():
    rp = np.array([0, 1, 3, 2, 4, 3, 6], np.int32)             # rows 2 and 4 decrease
    ci = np.array([0, 1, 2, 3, 4, 5], np.int32)
    result = create(NONE, rp, ci, np.ones(6))
    assert refused(result, EINVAL, "rowptr decreases at row 2"), result


# ---------------------------------------------------------------- columns
@pytest.mark.parametrize("precond", [NONE, JACOBI, MULTILEVEL])
@pytest.mark.parametrize("col", [-1, N])
def test_column_out_of_range(precond, col):
    result = create(precond, *with_row3([(2, -1.0), (3, 4.0), (col, -1.0)]))
    assert refused(result, EINVAL, "column index %d out of range in row 3" % col), result


# ---------------------------------------------------------------- the diagonal
DIAGONALS = {
    "missing": [(2, -1.0), (4, -1.0)],
    "stored_zero": [(2, -1.0), (3, 0.0), (4, -1.0)],
    "plus_minus_one": [(3, 1.0), (2, -1.0), (4, -1.0), (3, -1.0)],             # two entries that sum to zero, apart
}


@pytest.mark.parametrize("name", list(DIAGONALS))
def test_a_zero_diagonal_is_singular_under_column_jacobi(name):
    result = create(JACOBI, *with_row3(DIAGONALS[name]))
    assert refused(result, ESINGULAR, "row 3 has no (or a zero) diagonal entry"), result


@pytest.mark.parametrize("name", ["missing", "stored_zero"])
def test_a_zero_diagonal_is_singular_under_multilevel(name):
    result = create(MULTILEVEL, *with_row3(DIAGONALS[name]))
    assert refused(result, ESINGULAR, "row 3 has no (or a zero) diagonal entry"), result


def test_a_repeated_diagonal_is_an_order_error_under_multilevel_whatever_its_sum():
    """+1, -1 needs a repeated column, which MULTILEVEL refuses as such: the order test comes first"""
    result = create(MULTILEVEL, *with_row3([(2, -1.0), (3, 1.0), (3, -1.0), (4, -1.0)]))
    assert refused(result, EINVAL, "row 3 is not sorted by column"), result


@pytest.mark.parametrize("name", list(DIAGONALS))
def test_no_preconditioner_needs_no_diagonal(name):
    assert accepted(create(NONE, *with_row3(DIAGONALS[name])))


def test_a_diagonal_in_two_parts_that_do_not_cancel_is_one():
    assert accepted(create(JACOBI, *with_row3([(3, 1.0), (2, -1.0), (4, -1.0), (3, 3.0)])))


def test_no_preconditioner_takes_empty_rows():
    rows = base_rows()
    rows[0], rows[3], rows[5] = [], [], []
    assert accepted(create(NONE, *csr(rows)))


# ---------------------------------------------------------------- row order
ORDER = {
    "off_diagonal_pair_out_of_order": [(4, -1.0), (2, -1.0), (3, 4.0)],
    "diagonal_out_of_order": [(5, -1.0), (3, 4.0)],                           # accepted by the parent commit
    "repeated_off_diagonal": [(2, -0.5), (2, -0.5), (3, 4.0)],
    "repeated_diagonal": [(3, 2.0), (3, 2.0)],                                # accepted by the parent commit
}


@pytest.mark.parametrize("name", list(ORDER))
def test_multilevel_refuses_rows_that_are_not_strictly_ascending(name):
    result = create(MULTILEVEL, *with_row3(ORDER[name]))
    assert refused(result, EINVAL, "row 3 is not sorted by column"), result


@pytest.mark.parametrize("precond", [NONE, JACOBI])
@pytest.mark.parametrize("name", list(ORDER))
def test_the_flat_preconditioners_take_any_row_order(name, precond):
    assert accepted(create(precond, *with_row3(ORDER[name])))


@pytest.mark.parametrize("name", ["off_diagonal_pair_out_of_order", "diagonal_out_of_order"])
def test_create64_shares_the_order_test(name):
    result = create(MULTILEVEL, *with_row3(ORDER[name]), wide=True)
    assert refused(result, EINVAL, "row 3 is not sorted by column"), result
    assert accepted(create(NONE, *with_row3(ORDER[name]), wide=True))


# ---------------------------------------------------------------- blocks
def test_blocks_do_not_start_at_zero():
    assert refused(create(JACOBI, *csr(base_rows()), blk=[1, 3, N]), EINVAL, "blk_start must run from 0 to n")


def test_blocks_do_not_end_at_n():
    assert refused(create(JACOBI, *csr(base_rows()), blk=[0, 3, N - 1]), EINVAL, "blk_start must run from 0 to n")


def test_an_empty_block():
    assert refused(create(JACOBI, *csr(base_rows()), blk=[0, 3, 3, N]), EINVAL, "empty or descending block 1")


def test_a_descending_block():
    assert refused(create(JACOBI, *csr(base_rows()), blk=[0, 4, 2, N]), EINVAL, "empty or descending block 1")


def test_a_block_of_129_rows_names_the_limit():
    result = create(JACOBI, *diagonal_matrix(131), blk=[0, 2, 131])
    assert refused(result, EINVAL, "block 1 has 129 rows") and "at most 128 levels" in result[1], result


def test_a_block_of_128_rows_is_accepted():
    assert accepted(create(JACOBI, *diagonal_matrix(130), blk=[0, 2, 130]))


def test_no_blocks_is_accepted():
    assert accepted(create(JACOBI, *csr(base_rows()), blk=None))
    assert accepted(create(JACOBI, *diagonal_matrix(130), blk=None))       # default blocks of one wave: 64 + 64 + 2 rows
