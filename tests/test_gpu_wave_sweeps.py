"""The wave-per-column band solves (colblock_apply_kernel, gs_wave_kernel) run both substitution sweeps as straight-line code:
one text, wave_band_sweeps (csrc/nkp_dev.h), written out step by step, every step guarded by the column's length.  What that
relies on: no step runs beyond the column's end, the steps that cross from the first register of a lane to the second (row 64
of a column of 65-128 rows) pick the right one, a column shorter than the band still takes every product it is due, and per row
the products are subtracted in the order of the lane-per-column kernels (farthest diagonal first, then the scaling by 1 / u_kk).
gs_wave_kernel also stages its column through LDS without a workgroup barrier and lets a wave without a column return at once.

As in test_gpu_colsolve_packed.py the hierarchy is made to coarsen below these small shapes (NKP_ML_COARSEST_ROWS) and what is
compared is precond_apply of the multilevel cycle on a fixed random vector under three settings:
  reference          NKP_COLWAVE_MAX=0: every level on the lane-per-column kernels
  wave, two kernels  NKP_COLWAVE_MAX=1000000 NKP_ML_WAVE_FUSED=0: residual SpMV + colblock_apply_kernel on every level
  wave, fused        NKP_COLWAVE_MAX=1000000 NKP_ML_WAVE_FUSED=1: gs_wave_kernel on every level
Same substitutions in the same order => the same bits, with f32 and with f64 storage of the factors (NKP_ML_F32).

Band half-width 4: synth cannot produce it.  A column's own stencil reaches k +- 2 at most (upwind3), and coupled tracers are
stored tracer-major (solver.column_blocks: one block per column AND tracer), so their cross terms sit tracer_state_len rows
away, outside every block; the band half-width is 1 or 2 for everything synth.generate makes (0 or 1 below three levels).
The P = 4 instantiations are the same text with two more off-chain updates per step and are compiled, not run, here."""
import numpy as np
import pytest

from nk_ocn_tracer_jacobian_precond_amd import solver, synth

# (imt, jmt, seed) of test_gpu_colsolve_packed.py: 8 x 8, seed 7 has 14 + 14 columns per colour of the fine level, 12 x 10,
# seed 36 has 33 + 34 (and columns of all km levels): neither is a multiple of the 4 waves of a workgroup, so the last
# workgroup of every launch has waves without a column
GRIDS = [(8, 8, 7), (12, 10, 36)]
# 3: every column has 3 rows = P + 1 with upwind3 (synth's shallowest column; rows 1 and 2 take products the band reaches
# only in part); 5: 3-5 rows; 60: the benchmark's depth; 64 / 65: the last column of one row per lane and the first of two
# (seed 36); 80: 42-80 rows, both sides of the boundary in one launch
KMS = [3, 5, 60, 64, 65, 80]
# shorter still (seed 36 only: 67 columns): 2 rows = one forward step, 1 row = none (band half-width 1 resp. 0 there)
SHORT_KMS = [1, 2]
BANDS = [("centred", "const", 1), ("upwind3", "isop", 2)]

SMALL_LEVELS = dict(NKP_ML_COARSEST_ROWS="40")
SETTINGS = [("reference", dict(NKP_COLWAVE_MAX="0", NKP_ML_WAVE_FUSED="0")),
            ("wave", dict(NKP_COLWAVE_MAX="1000000", NKP_ML_WAVE_FUSED="0")),
            ("fused", dict(NKP_COLWAVE_MAX="1000000", NKP_ML_WAVE_FUSED="1"))]


def fine_level_colours(p):
    """columns per colour of the fine level (ml_plan.cpp: (i + j) & 1 of the column's horizontal cell)"""
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    odd = int(((np.asarray(ci) + np.asarray(cj)) & 1).sum())
    return len(ci) - odd, odd


def test_shapes_cover_the_short_columns_and_the_register_boundary():
    """The properties of the synthetic shapes that the cases below are chosen for (no GPU work).

    Two of the properties first asked for do not hold for any seed and are stated here as they are: synth.make_bathymetry
    gives every water column at least 3 levels, so at km = 3 every column has exactly 3 rows (none has 1 or 2; SHORT_KMS adds
    those); and 8 x 8 at km = 3 and 5 has 84 and 115 rows, fewer than 5 x NKP_ML_COARSEST_ROWS.  Level 0 is the last (dense)
    level only when it has at most NKP_ML_COARSEST_ROWS rows (multilevel.hip), which no shape here has, and the GPU cases
    assert that there are two levels."""
    coarsest = int(SMALL_LEVELS["NKP_ML_COARSEST_ROWS"])
    lens = {}
    for imt, jmt, seed in GRIDS:
        for km in KMS + (SHORT_KMS if seed == 36 else []):
            p = synth.generate(imt=imt, jmt=jmt, km=km, adv="centred", hmix="const", seed=seed)
            lens[(seed, km)] = np.diff(np.asarray(p.col_start()))
            assert all(n % 4 != 0 for n in fine_level_colours(p))                  # waves without a column
            assert p.flat_len > coarsest                                            # level 0 is not the last level
            if not (km in SHORT_KMS or ((imt, jmt) == (8, 8) and km in (3, 5))):
                assert p.flat_len > 5 * coarsest
    assert fine_level_colours(synth.generate(imt=8, jmt=8, km=60, seed=7)) == (14, 14)
    assert sorted(fine_level_colours(synth.generate(imt=12, jmt=10, km=60, seed=36))) == [33, 34]
    for seed in (7, 36):
        assert set(lens[(seed, 3)]) == {3}                                          # = P + 1 with upwind3
        assert lens[(seed, 5)].min() == 3 and lens[(seed, 5)].max() == 5
    assert set(lens[(36, 1)]) == {1} and set(lens[(36, 2)]) == {2}
    assert (lens[(36, 64)] == 64).any() and lens[(36, 64)].max() == 64             # the longest column of one row per lane
    assert (lens[(36, 65)] == 65).any() and lens[(36, 65)].max() == 65             # the shortest of two rows per lane
    for seed in (7, 36):                                                            # both sides of the boundary in one launch
        assert lens[(seed, 80)].min() < 64 and (lens[(seed, 80)] == 64).any() and (lens[(seed, 80)] == 65).any()
    assert lens[(36, 80)].max() == 80


def cycle_under_settings(grid, km, f32, monkeypatch):
    imt, jmt, seed = grid
    monkeypatch.setenv("NKP_COLSTREAM_MIN", "1")
    monkeypatch.setenv("NKP_ML_F32", f32)
    for name, value in SMALL_LEVELS.items():
        monkeypatch.setenv(name, value)
    for adv, hmix, band in BANDS:
        p = synth.generate(imt=imt, jmt=jmt, km=km, adv=adv, hmix=hmix, seed=seed)
        blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
        ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
        r = np.random.default_rng(41).standard_normal(p.flat_len)
        z = {}
        for variant, env in SETTINGS:
            for name, value in env.items():
                monkeypatch.setenv(name, value)
            with solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, precond=solver.PRECOND_MULTILEVEL, restart=4, col_i=ci, col_j=cj) as s:
                assert s.get_int("levels") >= 2, s.get_int("levels")          # level 0 runs sweeps, i.e. the column kernels
                z[variant] = s.precond_apply(r)
        assert np.isfinite(z["reference"]).all() and np.linalg.norm(z["reference"]) > 0
        for variant in ("wave", "fused"):
            assert np.array_equal(z["reference"], z[variant]), (grid, km, adv, f32, variant, np.abs(z["reference"] - z[variant]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("f32", ["1", "0"], ids=["f32", "f64"])
@pytest.mark.parametrize("km", KMS)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d_seed%d" % g)
def test_wave_sweeps_are_bit_identical(grid, km, f32, monkeypatch):
    """precond_apply with every level on colblock_apply_kernel, and with every level on gs_wave_kernel, against the same cycle
    on the lane-per-column kernels: np.array_equal, band half-width 1 and 2, f32 and f64 factor storage."""
    cycle_under_settings(grid, km, f32, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("f32", ["1", "0"], ids=["f32", "f64"])
@pytest.mark.parametrize("km", SHORT_KMS)
def test_wave_sweeps_on_columns_of_one_and_two_rows(km, f32, monkeypatch):
    """The same on columns of 2 rows (one forward step, two backward) and of 1 row (no forward step at all)."""
    cycle_under_settings((12, 10, 36), km, f32, monkeypatch)
