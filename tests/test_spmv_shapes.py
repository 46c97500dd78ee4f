"""The matrices of tests/spmv_shapes.py really contain what tests/test_gpu_spmv_shapes.py relies on: every row-block, dictionary
and run-shape event is asserted here with the Python restatements of the partitioner, the coder and the launch arithmetic, and
the restatement of the partitioner is itself held against the library's where a solver is built (the GPU module compares
get_int("rowblocks")).  No GPU."""
import numpy as np
import pytest

import oracle_binding as ora
import spmv_shapes as sh

SHAPES = {"ragged_empty": sh.ragged_empty, "ragged_dd": sh.ragged_dd}


@pytest.fixture(scope="module", params=list(SHAPES))
def shape(request):
    s = SHAPES[request.param]()
    rb = sh.row_blocks(s.rowptr)
    return s, rb, np.searchsorted(rb, np.arange(s.n), side="right") - 1        # block of every row


def test_row_blocks_restatement_on_small_cases():
    rp = np.array([0, 2048, 2048, 2049, 4098, 4098])
    assert sh.row_blocks(rp).tolist() == [0, 2, 3, 4, 5]                       # 2048 + 0 | 1 | long, alone | empty
    assert sh.row_blocks(np.zeros(601, np.int64)).tolist() == [0, 256, 512, 600]
    assert sh.row_blocks(np.array([0])).tolist() == [0]


def test_matrix_is_well_formed(shape):
    s, rb, _ = shape
    assert 11000 <= s.n <= 13000 and s.rowptr[0] == 0 and s.rowptr[-1] == s.colind.size == s.val.size
    row_of = np.repeat(np.arange(s.n), s.len)
    assert s.colind.min() >= 0 and s.colind.max() < s.n
    same_row = row_of[1:] == row_of[:-1]
    assert np.all(np.diff(s.colind.astype(np.int64))[same_row] > 0)            # sorted, no duplicates
    diag = s.colind == row_of
    if s.name == "ragged_dd":
        assert diag.sum() == s.n and s.len.min() >= 1
        off = np.bincount(row_of[~diag], weights=np.abs(s.val[~diag]), minlength=s.n)
        assert np.array_equal(np.abs(s.val[diag]), 1.0 + 2.0 * off)
        assert (s.val[diag] > 0).any() and (s.val[diag] < 0).any()
    else:
        assert (s.len == 0).sum() > 300


def test_row_block_events(shape):
    s, rb, blk_of = shape
    m, L = s.marks, s.len
    cnt = s.rowptr[rb[1:]].astype(np.int64) - s.rowptr[rb[:-1]]
    rows = np.diff(rb)
    assert rows.max() <= sh.MAX_ROWS and np.all((cnt <= sh.LDS_NNZ) | (rows == 1))
    low = 1 if s.name == "ragged_dd" else 0                                    # what an "empty" row holds
    alone = lambda r: rb[blk_of[r]] == r and rb[blk_of[r] + 1] == r + 1
    # a long row as the first row of the matrix
    assert L[0] >= 2049 and alone(0)
    # a long row as the last row, preceded by an empty row
    assert L[s.n - 1] >= 2049 and alone(s.n - 1) and L[s.n - 2] == low
    # 5000 entries, then 2049, followed by short rows
    r = m["long_pair"]
    assert L[r] == 5000 and L[r + 1] == 2049 and alone(r) and alone(r + 1) and np.all(L[r + 2:r + 5] == 3)
    # exactly 2048 entries: alone in its block, not long
    r = m["row_2048"]
    assert L[r] == 2048 and alone(r) and not s.long[r]
    # 2047 + 2 must split
    r = m["row_2047_then_2"]
    assert L[r] == 2047 and L[r + 1] == 2 and alone(r) and rb[blk_of[r + 1]] == r + 1
    # exactly 2048 entries in several rows
    k = blk_of[m["block_2048"]]
    assert cnt[k] == 2048 and rows[k] >= 3
    # a block that ends on the 256-row cap
    capped = (rows == sh.MAX_ROWS) & (cnt < sh.LDS_NNZ)
    assert capped.any()
    if low == 0:
        # >= 300 truly empty rows: one whole block without an entry
        r = m["empty_block"]
        assert np.all(L[r:r + 300] == 0)
        assert ((cnt == 0) & (rows == sh.MAX_ROWS)).any() and rb[blk_of[r]] == r
        # empty rows at the start and at the end of blocks
        first, last = rb[:-1], rb[1:] - 1
        assert ((L[first] == 0) & (cnt > 0)).any() and ((L[last] == 0) & (cnt > 0)).any()
        assert rb[blk_of[m["empty_at_block_start"]]] == m["empty_at_block_start"]
        r = m["empty_at_block_end"]
        assert L[r] == 0 and L[r + 1] == 0 and rb[blk_of[r] + 1] == r + 2 and blk_of[r] == blk_of[m["block_2048"]]
    else:
        assert L.min() == 1


def test_dictionary_events(shape):
    s, rb, blk_of = shape
    nd = sh.block_offsets(s.rowptr, s.colind, rb)
    coded = sh.coded_blocks(s.rowptr, s.colind, rb)
    k256, k257 = blk_of[s.marks["dict_256"]], blk_of[s.marks["dict_257"]]
    assert nd[k256] == 256 and coded[k256]
    assert nd[k257] == 257 and not coded[k257]
    # long rows are never coded; the banded stretches are, the random ones are not
    assert not coded[blk_of[np.flatnonzero(s.long)]].any()
    assert 0.2 < coded.mean() < 0.8, coded.mean()
    # coded, uncoded and coded blocks follow each other (the double-buffered dictionary changes hands and is skipped)
    c = coded.astype(int)
    assert np.any((c[:-2] == 1) & (c[1:-1] == 0) & (c[2:] == 1)) and np.any((c[:-2] == 0) & (c[1:-1] == 1) & (c[2:] == 0))


def test_run_shape_events(shape):
    """Which runs of row blocks the workgroups of the pipelined kernel walk (variant 4, spmv_pipe_min = 1).

    spmv_run = 4: runs of several blocks with a long-row block first, in the middle and last, and coded / uncoded / coded
    blocks inside one run.

    spmv_run = 1: launch_range starts (blocks & ~7) workgroups, nrowblk / 8 rounded DOWN per XCD, for nrowblk / 8 rounded UP
    blocks per XCD, so a workgroup walks two blocks at the most whatever the matrix (one when the block count is a multiple of
    8).  Runs of three and a long row in the middle of a run cannot occur there; what can is asserted: runs of two exist, one
    starts with a long-row block (the reload after it) and one ends with it (the long row reached through a prefetch)."""
    s, rb, blk_of = shape
    nb = rb.size - 1
    longb = np.zeros(nb, bool)
    longb[blk_of[np.flatnonzero(s.long)]] = True
    coded = sh.coded_blocks(s.rowptr, s.colind, rb)
    for run in (1, 4):
        runs = sh.pipe_runs(nb, run)
        assert sorted(b for a, z in runs for b in range(a, z)) == list(range(nb))          # every block once
        several = [(a, z) for a, z in runs if z - a >= 2]
        assert several
        assert any(longb[a] for a, z in several), run
        assert any(longb[z - 1] for a, z in several), run
        if run == 1:
            assert nb % 8 != 0 and max(z - a for a, z in runs) == 2
            continue
        assert any(z - a >= 3 for a, z in runs)
        assert any(longb[a + 1:z - 1].any() for a, z in runs if z - a >= 3), run
        assert any("101" in "".join("01"[int(t)] for t in coded[a:z]) for a, z in runs), run
        assert any(longb[b] and longb[b + 1] for a, z in runs for b in range(a, z - 1)), run      # long after long inside a run


def test_exact_reference_and_bound():
    """The reference against integer arithmetic on a row where f64 summation in stored order loses everything, and the oracle's
    stored-order sums within the bound on the real matrix."""
    rp = np.array([0, 3, 3, 5])
    ci = np.array([0, 1, 2, 0, 2])
    v = np.array([2.0 ** 60, 1.0, -2.0 ** 60, 1.0 + 2.0 ** -30, 1.0])
    x = np.array([1.0, 1.0, 1.0])
    b = np.array([0.5, -2.0, 1.0])
    E = sh.Exact(rp, ci, v, x, b)
    assert E.y.tolist() == [1.0, 0.0, 2.0 + 2.0 ** -30] and E.r.tolist() == [-0.5, -2.0, -1.0 - 2.0 ** -30]
    assert E.d.tolist() == [2.0 ** 61, 2.0, 3.0 + 2.0 ** -30]                                  # 2^61 + 1.5 rounded once
    x2 = np.array([1.0 + 2.0 ** -30, 0.0, 0.0])
    assert sh.Exact(rp, ci, v, x2).y[2] == 1.0 + 2.0 ** -29                                      # (1 + 2^-30)^2 rounded once
    s = sh.ragged_empty()
    xv, _ = sh.vectors(s)
    E = sh.exact(s, xv)
    y = ora.spmv(s.rowptr, s.colind, s.val, xv)
    assert np.all(np.abs(y - E.y) <= E.e) and np.all(y[s.len == 0] == 0.0)
    assert np.abs(y - E.y).max() > 0.0                                                           # and it is not the same computation


def test_conditions_of_the_solves():
    """What the GPU tests take for granted about ragged_dd: point Jacobi FGMRES (the CPU oracle) reaches 1e-10 in at most 60
    iterations for every right-hand side used there, and no denominator of the backward error is zero."""
    s = sh.ragged_dd()
    B = sh.solve_rhs(s, 8)
    for c in range(B.shape[0]):
        x, info = ora.fgmres(s.rowptr, s.colind, s.val, None, B[c], precond=1, restart=60, max_iters=60, rtol=1e-10)
        assert info["status"] == 0 and 0 < info["iters"] <= 60 and info["relres"] <= 1e-10, (c, info)
    for shape in (s, sh.ragged_empty()):
        x0, b = sh.vectors(shape)
        assert np.all(b != 0.0) and np.all(sh.exact(shape, x0, b).d > 0.0)


def test_create_accepts_both_matrices(shape):
    """nkp_create validates the matrix on the host before it looks for a device: ragged_empty passes without a preconditioner
    (rows without any entry), ragged_dd with point Jacobi; without a GPU the call then stops at the device, not at the matrix."""
    from nk_ocn_tracer_jacobian_precond_amd import solver
    s = shape[0]
    try:
        if s.name == "ragged_empty":
            solver.NkpSolver(s.rowptr, s.colind, s.val, None, precond=solver.PRECOND_NONE, restart=4).close()
        else:
            solver.NkpSolver(s.rowptr, s.colind, s.val, np.arange(s.n + 1), precond=solver.PRECOND_COLUMN_JACOBI, restart=4).close()
    except solver.NkpError as e:
        assert e.code == -3 and "no HIP device" in str(e), e
