"""colblock_apply_ldspack_kernel (32 water columns per wave, the column resident in LDS, factors packed four steps to a 16-byte
load) stages the right-hand side of all 32 columns in one burst of unconditional loads and requests the accumulate target of
all 32 from inside the backward sweep.  What that relies on: a lane behind the end of its column reads a valid address and
its value is dropped, the slots of absent columns of a colour's last group stay zero, the LDS image is zero behind every
column's end, and target + solution keeps its operand order.

The packed kernel runs inside the multilevel cycle only (f32 factor storage; the column-Jacobi preconditioner stores f64
factors and takes colblock_apply_ldsres_kernel under the same switches), on every level but the last, which is solved densely.
So the hierarchy is made to coarsen below these small shapes (NKP_ML_COARSEST_ROWS), and what is compared is the cycle with
every level's column solves on the packed kernel against the cycle with them on the 8-columns-per-wave kernel: same
substitutions in the same order => the same bits.  The cycle's first half sweep starts from x = 0 and does not accumulate,
all later ones do, so both write-back paths run in every case."""
import numpy as np
import pytest

from nk_ocn_tracer_jacobian_precond_amd import solver, synth

# (imt, jmt, seed): land rows at j = 0 and jmt - 1, so 12 x 10 has at most 96 water columns and 8 x 8 at most 48.  The fine level
# is coloured like a checkerboard, (i + j) & 1, and a colour's columns go to groups of 32, the longest first (columns, fine level):
#   12 x 10, seed 33: 33 + 33: each colour one full group and a last group of ONE column; lengths 17..51 of 60 levels, the widest spread
#   12 x 10, seed 36: 33 + 34: last groups of one and of two columns; the deepest columns (all km levels: 70 and 80 take the fifth chunk)
#   8 x 8, seed 7: 14 + 14: a single group per colour, 18 of its 32 slots absent; lengths 25..53 of 60
#   8 x 8, seed 1: 15 + 18: a single group per colour; 67 of 70 and 76 of 80 levels
# The coarser levels (aggregated columns, two-coloured again) run the same kernel with fewer columns still.
GRIDS = [(12, 10, 33), (12, 10, 36), (8, 8, 7), (8, 8, 1)]
# chunks of 16 steps a group runs: km = 10 -> 1 (columns shorter than a chunk), 20 -> 2, 40 -> 3, 60 -> 4, 70 -> 4 or 5, 80 -> 5
# (more than 64 levels: the five-chunk instantiation, rows 64-79 staged and written back through the second half)
KMS = [10, 20, 40, 60, 70, 80]
BANDS = [("centred", "const", 1), ("upwind3", "isop", 2)]

PACKED = dict(NKP_COLSTREAM="1", NKP_COL_LDSRES="2", NKP_COL_PACKED="1")
LANES = dict(NKP_COLSTREAM="0", NKP_COL_LDSRES="0", NKP_COL_PACKED="0")


# the smallest shape has 207 rows: no level 0 is the last (dense) level, and coarsening goes on below it
SMALL_LEVELS = dict(NKP_ML_COARSEST_ROWS="40")


def fine_level_colours(p):
    """columns per colour of the fine level (ml_plan.cpp: (i + j) & 1 of the column's horizontal cell)"""
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    odd = int(((np.asarray(ci) + np.asarray(cj)) & 1).sum())
    return len(ci) - odd, odd


def test_shapes_cover_the_chunk_counts_and_the_partial_groups():
    """The properties of the synthetic shapes that the cases below are chosen for (no GPU work)."""
    ncol, chunks = {}, {}
    for imt, jmt, seed in GRIDS:
        for km in KMS:
            p = synth.generate(imt=imt, jmt=jmt, km=km, adv="centred", hmix="const", seed=seed)
            lens = np.diff(np.asarray(p.col_start()))
            ncol[(imt, jmt, seed)] = fine_level_colours(p)
            chunks.setdefault(km, set()).add((int(lens.max()) + 15) // 16)
            assert p.flat_len > 5 * int(SMALL_LEVELS["NKP_ML_COARSEST_ROWS"])    # level 0 is not the last level
            if km == 10:
                assert lens.max() < 16                                        # columns shorter than one chunk
            if km == 60 and seed in (33, 7):
                assert lens.max() > 2 * lens.min()                            # land-heavy: lengths in one group differ widely
            if seed == 36:
                assert lens.max() == km                                       # rows 64-79 of the five-chunk kernel all in use at km = 80
    assert [sorted(chunks[km]) for km in KMS] == [[1], [2], [3], [4], [4, 5], [5]]
    assert ncol[(12, 10, 33)] == (33, 33) and 33 in ncol[(12, 10, 36)]         # a full group and a last group of one column
    assert all(1 < n < 32 for g in ((8, 8, 7), (8, 8, 1)) for n in ncol[g])   # a single, partial group per colour


@pytest.mark.gpu
@pytest.mark.parametrize("km", KMS)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d_seed%d" % g)
def test_packed_column_solve_is_bit_identical(grid, km, monkeypatch):
    """precond_apply of the multilevel cycle with every level's column solves on the packed kernel against the same cycle with
    them on the 8-columns-per-wave kernel, f32 factor storage: np.array_equal, band half-width 1 and 2.  The column-Jacobi
    preconditioner is compared under the same switches as the issue asks; its f64 factors take colblock_apply_ldsres_kernel
    there, not the packed kernel."""
    imt, jmt, seed = grid
    monkeypatch.setenv("NKP_COLSTREAM_MIN", "1")
    monkeypatch.setenv("NKP_COLWAVE_MAX", "0")              # no wave-per-column kernel on the small levels: every level takes the kernel under test
    monkeypatch.setenv("NKP_ML_F32", "1")
    for name, value in SMALL_LEVELS.items():
        monkeypatch.setenv(name, value)
    for adv, hmix, band in BANDS:
        p = synth.generate(imt=imt, jmt=jmt, km=km, adv=adv, hmix=hmix, seed=seed)
        blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
        ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
        r = np.random.default_rng(41).standard_normal(p.flat_len)
        for precond, kw in ((solver.PRECOND_COLUMN_JACOBI, {}), (solver.PRECOND_MULTILEVEL, dict(col_i=ci, col_j=cj))):
            z = {}
            for variant, env in (("lanes", LANES), ("packed", PACKED)):
                for name, value in env.items():
                    monkeypatch.setenv(name, value)
                with solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, precond=precond, restart=4, **kw) as s:
                    if precond == solver.PRECOND_COLUMN_JACOBI:
                        assert s.get_int("band") == band                      # (the cycle keeps its bands per level, not here)
                    else:
                        assert s.get_int("levels") >= 2, s.get_int("levels")  # level 0 runs sweeps, i.e. the column kernel
                    z[variant] = s.precond_apply(r)
            assert np.isfinite(z["packed"]).all() and np.linalg.norm(z["packed"]) > 0
            assert np.array_equal(z["lanes"], z["packed"]), (grid, km, adv, precond, np.abs(z["lanes"] - z["packed"]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("f32", ["0", "1"], ids=["f64", "f32"])
@pytest.mark.parametrize("km", [70, 80])
@pytest.mark.parametrize("grid", [g for g in GRIDS if g[:2] == (8, 8)], ids=lambda g: "%dx%d_seed%d" % g)
def test_capped_lanes_kernel_is_bit_identical(grid, km, f32, monkeypatch):
    """The 8-columns-per-wave kernel on columns of 65-80 levels: its instantiation capped at three waves per SIMD,
    colblock_apply_lanes_kernel<P, 80, FT, 3> (NKP_COL_W3=1, the default), against the uncapped <P, 128, FT, 1> that
    NKP_COL_W3=0 selects.  Same text, other register allocation => precond_apply of the multilevel cycle is np.array_equal,
    band half-width 1 and 2, f64 and f32 factor storage.  (Columns of at most 64 levels take <P, 64, FT, 1> under either
    setting: seed 7 at km = 70.)"""
    imt, jmt, seed = grid
    monkeypatch.setenv("NKP_COLSTREAM_MIN", "1")
    monkeypatch.setenv("NKP_COLWAVE_MAX", "0")              # no wave-per-column kernel on the small levels
    monkeypatch.setenv("NKP_ML_F32", f32)
    for name, value in {**SMALL_LEVELS, **LANES}.items():
        monkeypatch.setenv(name, value)
    for adv, hmix, band in BANDS:
        p = synth.generate(imt=imt, jmt=jmt, km=km, adv=adv, hmix=hmix, seed=seed)
        blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
        ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
        r = np.random.default_rng(41).standard_normal(p.flat_len)
        z = {}
        for w3 in ("1", "0"):
            monkeypatch.setenv("NKP_COL_W3", w3)
            with solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, precond=solver.PRECOND_MULTILEVEL, restart=4, col_i=ci, col_j=cj) as s:
                assert s.get_int("levels") >= 2, s.get_int("levels")      # level 0 runs sweeps, i.e. the column kernel
                z[w3] = s.precond_apply(r)
        assert np.isfinite(z["1"]).all() and np.linalg.norm(z["1"]) > 0
        assert np.array_equal(z["1"], z["0"]), (grid, km, adv, f32, np.abs(z["1"] - z["0"]).max())
