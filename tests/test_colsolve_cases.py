"""The claims of tests/colsolve_cases.py, checked without a GPU: what widen() builds (against the oracle's band measure, band LU
and band solve), the properties of the shapes that the GPU cases are chosen for, and that the case lists of
tests/test_gpu_colsolve_families.py reach every instantiation a column-solve launcher can select."""
import numpy as np
import pytest

import colsolve_cases as cc
import ml_cycle_reference as mcr
import oracle_binding as ora

DISTS = [((3,), 3, 4, 0), ((3, 4), 4, 4, 0), ((4,), 4, 4, 0), ((6,), 6, 4, 1), ((3, 4, 6), 6, 4, 1)]


def relative(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("grid,km", [(cc.GRID_BIG, 10), (cc.GRID_BIG, 60), (cc.GRID_BIG, 128), (cc.GRID_SMALL, 81)],
                         ids=["12x10_km10", "12x10_km60", "12x10_km128", "8x8_km81"])
@pytest.mark.parametrize("dists,band,P,dropped", DISTS, ids=[str(d[0]) for d in DISTS])
def test_widen_gives_the_claimed_band_and_a_solvable_block(grid, km, dists, band, P, dropped):
    base = cc.problem(grid, km, 2, dists=())
    p = cc.widen(base, dists, 5)
    rp, ci, v = p.rowptr, p.colind, p.nzval
    blk = cc.column_blocks(p)
    n = p.flat_len
    # sorted, duplicate-free rows with a diagonal
    for r in range(n):
        row = ci[rp[r]:rp[r + 1]]
        assert (np.diff(row) > 0).all() and r in row
    assert rp[-1] - base.rowptr[-1] > 0 and (p.scipy_csr().diagonal() != 0).all()
    bw, nodiag, max_len = ora.colblock_measure(rp, ci, v, blk)
    assert (bw, nodiag) == (band, 0) and max_len == np.diff(blk).max()
    assert cc.stored_band(bw) == P
    fac, drop = ora.colblock_factor(rp, ci, v, blk, P)
    assert drop == dropped
    # Row dominance inside the column blocks.  The blocks of synth.generate are NOT row dominant (vertical advection against a
    # small diagonal: |a_rr| is below the sum of the other in-column magnitudes in half of the rows, under every adv / hmix), so
    # strict dominance cannot be asked of the widened matrix; what widen() guarantees, and what is asserted, is that no row's
    # margin |a_rr| - sum |in-column others| falls, and that every added entry is at most 2 % of its row's diagonal.  That the
    # unpivoted band LU is nevertheless accurate on these blocks is the 1e-13 agreement with the pivoted dense solve below.
    for (a, B), (_, B0) in zip(cc.column_dense_blocks(p), cc.column_dense_blocks(base)):
        d, d0 = np.abs(np.diag(B)), np.abs(np.diag(B0))
        margin, margin0 = 2 * d - np.abs(B).sum(1), 2 * d0 - np.abs(B0).sum(1)
        assert (margin >= margin0 - 8 * 2.0 ** -52 * np.abs(B).sum(1)).all(), a
        added = np.abs(B - B0)
        np.fill_diagonal(added, 0.0)
        assert (added <= 0.02 * d0[:, None]).all() and (np.sign(np.diag(B)) == np.sign(np.diag(B0))).all(), a
    r = np.random.default_rng(3).standard_normal(n)
    z = ora.colblock_apply(n, blk, P, fac, r)
    capped = cc.dense_block_solve(p, r, cap=cc.MAX_BAND)
    assert relative(z, capped) <= 1e-13
    exact = cc.dense_block_solve(p, r)
    if dropped:
        assert relative(capped, exact) > 1e-3               # a kernel that keeps or drops the wrong diagonal is far outside any tolerance
    else:
        assert np.array_equal(capped, exact)


def test_band_table_of_the_cases():
    for band, (adv, hmix, dists) in cc.BANDS.items():
        p = cc.problem(cc.GRID_SMALL, 60, band)
        bw, _, _ = ora.colblock_measure(p.rowptr, p.colind, p.nzval, cc.column_blocks(p))
        assert bw == band, (band, bw)
    for band, dists in cc.BAND_ALTERNATIVES.items():
        p = cc.problem(cc.GRID_SMALL, 60, band, dists=dists)
        assert ora.colblock_measure(p.rowptr, p.colind, p.nzval, cc.column_blocks(p))[0] == band


def test_shapes():
    for km in cc.KMS:
        p = cc.problem(cc.GRID_BIG, km, 1)
        lens = cc.fine_level_colour_lens(p)
        assert sorted(l.size for l in lens) == [33, 34]                       # a full group of 32 and a last group of one or two
        longest = max(int(l.max()) for l in lens)
        assert longest == km                                                  # a column of exactly km rows
        if km >= 81:
            assert 3897 <= p.flat_len <= 6136, (km, p.flat_len)
        if km == 10:
            assert longest < 16                                               # every column shorter than one 16-step chunk
        if km == 96:
            every = np.concatenate(lens)
            for a, b in ((64, 65), (80, 81)):                                  # both sides of the thresholds in one launch
                assert (every <= a).any() and (every >= b).any()
        q = cc.problem(cc.GRID_SMALL, km, 1)
        assert [l.size for l in cc.fine_level_colour_lens(q)] == [14, 14]      # a single partial group per colour
        assert q.flat_len > 5 * cc.BASE["ml_coarsest_rows"]                    # level 0 is never the last level


def test_selection_rule_on_hand_worked_levels():
    e = cc.expected_kernel
    for family, f32, P, dropped, max_len, multilevel, field, want in cc.HAND_WORKED:
        got = e(family, f32, P, dropped, max_len, cc.HAND_WORKED_NCOLS, multilevel=multilevel)
        value = got["batch"](field[1]) if isinstance(field, tuple) else got[field]
        assert value == want and type(value) is type(want), (family, f32, P, dropped, max_len, field, value, want)
    assert len(cc.HAND_WORKED) == 34
    lens = [np.full(33, 128), np.full(34, 128)]
    got = e("lanes8", 0, 2, 0, 128, 67, lens)
    assert got["lds_doubles"] == 1024 + 32 + 2 + 5 * 128 * 8 and got["lds_over_48k"] and got["ngrp"] == 10
    assert cc.batch_groups(5) == [4] and cc.batch_groups(3) == [4] and cc.batch_groups(6, 8) == [8] and cc.batch_groups(2) == [2]


def test_the_case_lists_reach_every_instantiation():
    """A condition on the case lists: every instantiation a launcher can select is selected on level 0 of at least one case,
    one lanes case needs the opt-in for more than 48 KB of dynamic LDS and one gs_fused case falls back.  Nothing is waived."""
    hit, extra = cc.covered_instantiations()
    assert len(cc.INSTANTIATIONS) == 3 * 2 * 13 + 3 * 2 * 3 + 3 * 2 * 2 + 2
    missing = sorted(cc.INSTANTIATIONS - set(hit), key=str)
    assert not missing, missing
    assert not set(hit) - cc.INSTANTIATIONS, sorted(set(hit) - cc.INSTANTIATIONS, key=str)
    assert extra["lanes_lds_over_48k"] and extra["gs_fused_fallback"]
    # the GPU module's cases the issue names
    cyc = set(cc.CASES_CYCLE)
    assert {(cc.GRID_BIG, b, km, f) for b in (2, 4, 6) for km in (60, 80, 128) for f in (0, 1)} <= cyc
    assert {(cc.GRID_BIG, b, km, f) for b in (1, 3) for km in (10, 96) for f in (0, 1)} <= cyc
    assert {(cc.GRID_SMALL, 4, km, f) for km in (60, 128) for f in (0, 1)} <= cyc
    assert {(cc.GRID_BIG, b, km, f) for b in (2, 4, 6) for km in (60, 80, 128) for f in (0, 1)} <= set(cc.CASES_BATCH)
    assert {km for _, _, km in cc.CASES_JACOBI} >= {10, 60, 64, 65, 80, 81, 128} and {b for _, b, _ in cc.CASES_JACOBI} == {1, 2, 3, 4, 6}


def test_capped_blocks_of_the_restated_cycle():
    """CycleLevel(band_cap = 4): the half sweep solves the band-capped block, the residual keeps every entry."""
    p = cc.problem(cc.GRID_SMALL, 60, 6)
    A = p.scipy_csr()
    cs = np.asarray(p.col_start())
    col_of = np.repeat(np.arange(cs.size - 1), np.diff(cs))
    half = cs[cs.size // 2]
    rows = [np.arange(0, half), np.arange(half, p.flat_len)]
    capped = mcr.CycleLevel(A, col_of=col_of, rows=rows, band_cap=4)
    whole = mcr.CycleLevel(A, col_of=col_of, rows=rows)
    assert capped.band == whole.band == 6
    assert abs(capped.L - A).max() == 0
    D = (whole.Bd - capped.Bd).tocoo()
    assert D.nnz and set(np.abs(D.row - D.col)[D.data != 0]) == {6}
    r = np.random.default_rng(1).standard_normal(p.flat_len)
    x = np.zeros(p.flat_len)
    mcr._half(capped, x, r, 0, "lu", "f64")
    want = cc.dense_block_solve(p, r, cap=4)
    assert relative(x[rows[0]], want[rows[0]]) <= 1e-13 and not x[rows[1]].any()
