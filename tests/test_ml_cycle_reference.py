"""tests/ml_cycle_reference.py checked on the CPU, on the levels of ml_reference.build (no GPU, no library): it restates the
cycle that tests/test_gpu_cycle_options.py holds the HIP cycle against, so it has to (1) agree with the older restatement at the
defaults, (2) react to every option that test sets -- otherwise the GPU test could pass with a knob ignored on both sides -- and
(3) react to an off-by-one in any of them by far more than the tolerances of the GPU test (1e-12 with f64 storage, at most 2e-5
with f32 storage); and (4) its grouped evaluation of the half sweeps, which tests/test_gpu_grid_caps.py runs at two million rows,
has to be the per-column one.

Rounding sizes of the reference itself on these levels, recorded, not asserted (the GPU test recomputes both on the device's levels and
sizes its tolerances from them): blocks="lu" against blocks="inverse" at most 2.9e-16 relative over the option cases;
factors="f32" against exact blocks on f32-rounded operators 8.0e-10 to 1.5e-8 when the factors are those of the rounded blocks,
3.2e-9 to 9.2e-8 when they are those of the unrounded blocks, as the setup makes them (mcr.with_exact_blocks)."""
import numpy as np
import pytest

import ml_cycle_reference as mcr
import ml_reference as mlr
from nk_ocn_tracer_jacobian_precond_amd import synth


@pytest.fixture(scope="module")
def problem():
    p = synth.generate(24, 20, 10, adv="upwind3", hmix="isop", seed=2)
    colid = np.cumsum(p.ind_k == 0) - 1
    args = (p.scipy_csr(), p.ind_i.astype(np.int64), p.ind_j.astype(np.int64), p.ind_k.astype(np.int64), colid)
    return args, np.random.default_rng(17).standard_normal(p.flat_len)


@pytest.fixture(scope="module")
def hierarchies(problem):
    args, _ = problem
    deep = mlr.build(*args, coarsest_rows=60)
    shallow = mlr.build(*args, coarsest_rows=300)
    assert [lv.n for lv in deep] == [2813, 889, 275, 100, 13]
    assert [lv.n for lv in shallow] == [2813, 889, 275]
    return dict(deep_mlr=deep, deep=mcr.levels_from_mlr(deep), iterated=mcr.levels_from_mlr(shallow, dense_last=False),
                shallow_dense=mcr.levels_from_mlr(shallow), two=mcr.levels_from_mlr(mlr.build(*args, coarsest_rows=60, max_levels=2)))


@pytest.fixture(scope="module")
def z_default(problem, hierarchies):
    return mcr.cycle(hierarchies["deep"], problem[1])


def test_defaults_equal_the_older_restatement(problem, hierarchies, z_default):
    z_old = mlr.cycle(hierarchies["deep_mlr"], 0, problem[1])
    assert mcr.relative_difference(z_default, z_old) <= 1e-12
    assert all(lv.band <= 2 for lv in hierarchies["deep"][:-1])          # what the GPU shapes rely on


@pytest.mark.parametrize("name,hierarchy,knobs", [c for c in mcr.OPTION_CASES if c[1] != "iterated" and c[0] != "default"], ids=lambda v: v if isinstance(v, str) else "")
def test_every_option_case_moves_the_answer(name, hierarchy, knobs, problem, hierarchies, z_default):
    """By at least 1e-3 of the default cycle: nine orders above the f64 tolerance of the GPU test, two above the f32 one."""
    assert len(hierarchies[hierarchy]) == (2 if hierarchy == "two" else 5)
    z = mcr.cycle(hierarchies[hierarchy], problem[1], **mcr.cycle_kwargs(**knobs))
    d = mcr.relative_difference(z, z_default)
    print(name, "relative change", d)
    assert d >= 1e-3, (name, d)


def test_sweep_count_of_an_iterated_last_level_shows(problem, hierarchies):
    """On 13 rows 30 sweeps are the dense solve (to 1e-11): no sweep count can show there.  On 275 rows it does."""
    r = problem[1]
    dense13 = mcr.cycle(hierarchies["deep"], r)
    it13 = mcr.cycle(mcr.levels_from_mlr(hierarchies["deep_mlr"], dense_last=False), r)
    assert mcr.relative_difference(it13, dense13) <= 1e-9
    dense = mcr.cycle(hierarchies["shallow_dense"], r)
    z = {s: mcr.cycle(hierarchies["iterated"], r, coarsest_sweeps=s) for s in (4, 5, 6, 30, 0)}
    assert np.array_equal(z[0], z[30])                                   # <= 0 means 30
    for s in (4, 5, 6, 30):
        print(s, "sweeps against the dense solve", mcr.relative_difference(z[s], dense))
    assert mcr.relative_difference(z[5], dense) >= 1e-3
    assert mcr.relative_difference(z[5], z[30]) >= 1e-3                  # the two sweep counts of the GPU test
    for a, b in ((4, 5), (5, 6), (4, 6)):
        assert mcr.relative_difference(z[a], z[b]) >= 1e-5, (a, b)


def _by_one(knobs):
    """The cases' knobs with one of them off by one: what a slip in one copy of the cycle would compute."""
    k = dict(mcr.DEFAULT_KNOBS, **knobs)
    out = []
    for name in ("ml_smooth", "ml_smooth_coarse", "ml_coarse_from", "ml_gamma_from", "ml_gamma_to", "ml_coarsest_sweeps"):
        for step in (-1, 1):
            v = k[name] + step
            if name in ("ml_smooth", "ml_coarse_from") and v < 1:
                continue
            if name == "ml_smooth_coarse" and (k[name] == 0 or v < 1):
                continue                                                 # 0 = "like the fine levels" is not a count
            if name in ("ml_gamma_from", "ml_gamma_to") and (k["ml_gamma_to"] <= k["ml_gamma_from"] or v < 0):
                continue                                                 # no W-level in this case
            out.append((name, v))
    return out


def test_a_slip_in_any_knob_is_orders_above_the_tolerances(problem, hierarchies):
    """For every knob, at least one option case in which that knob off by one (either way), the coarse correction unweighted, or
    one correction where two are due, changes the cycle by >= 1e-4."""
    r = problem[1]
    best = {}
    for case, hierarchy, knobs in mcr.OPTION_CASES:
        levels = hierarchies[hierarchy]
        z = mcr.cycle(levels, r, **mcr.cycle_kwargs(**knobs))
        slips = [(("%s%+d" % (n, v - dict(mcr.DEFAULT_KNOBS, **knobs)[n])), {n: v}) for n, v in _by_one(knobs)]
        slips.append(("omega dropped", dict(ml_omega=1.0)))
        slips.append(("one correction", dict(ml_gamma_from=0, ml_gamma_to=0)))
        for slip, change in slips:
            d = mcr.relative_difference(mcr.cycle(levels, r, **mcr.cycle_kwargs(**dict(knobs, **change))), z)
            if d > best.get(slip, (0.0, ""))[0]:
                best[slip] = (d, case)
    for slip, (d, case) in sorted(best.items()):
        print("%-24s %.2e in case %s" % (slip, d, case))
    expected = {"%s%+d" % (n, s) for n in ("ml_smooth", "ml_smooth_coarse", "ml_coarse_from", "ml_gamma_from", "ml_gamma_to", "ml_coarsest_sweeps")
                for s in (-1, 1)} | {"omega dropped", "one correction"}
    expected.discard("ml_smooth_coarse-1")                               # every case that sets it sets 1; 0 is not a count
    assert set(best) == expected, expected ^ set(best)
    for slip, (d, case) in best.items():
        assert d >= 1e-4, (slip, d, case)


def test_rounding_sizes_of_the_reference(problem, hierarchies):
    """Printed for the record: the two yardsticks the GPU test sizes its tolerances from, here on the CPU-built levels."""
    r = problem[1]
    rounded = {}
    for h in ("deep", "iterated", "two"):
        rounded[h] = [mcr.CycleLevel(lv.L.astype(np.float32).astype(np.float64), lv.col_of, lv.rows, lv.P, lv.coarse_inv) for lv in hierarchies[h]]
    d_all, e, e2 = [], [], []
    for name, hierarchy, knobs in mcr.OPTION_CASES:
        kw = mcr.cycle_kwargs(**knobs)
        d = mcr.relative_difference(mcr.cycle(hierarchies[hierarchy], r, blocks="inverse", **kw), mcr.cycle(hierarchies[hierarchy], r, **kw))
        z = mcr.cycle(rounded[hierarchy], r, **kw)
        e.append(mcr.relative_difference(mcr.cycle(rounded[hierarchy], r, factors="f32", **kw), z))
        d_all.append(d)
    for h in rounded:                                                    # factors of the unrounded blocks, as the setup makes them
        mcr.with_exact_blocks(rounded[h], hierarchies[h])
    for (name, hierarchy, knobs), d, e1 in zip(mcr.OPTION_CASES, d_all, e):
        kw = mcr.cycle_kwargs(**knobs)
        e2.append(mcr.relative_difference(mcr.cycle(rounded[hierarchy], r, factors="f32", **kw), mcr.cycle(rounded[hierarchy], r, **kw)))
        print("%-20s lu/inverse %.1e   f32 factors %.1e   f32 factors of the unrounded blocks %.1e" % (name, d, e1, e2[-1]))
    print("lu/inverse at most %.1e; f32 factors %.1e to %.1e, of the unrounded blocks %.1e to %.1e" % (max(d_all), min(e), max(e), min(e2), max(e2)))
    assert np.isfinite(d_all).all() and np.isfinite(e).all() and np.isfinite(e2).all()


@pytest.mark.parametrize("name,hierarchy,knobs", mcr.OPTION_CASES, ids=lambda v: v if isinstance(v, str) else "")
def test_grouped_half_sweeps_are_the_per_column_ones(name, hierarchy, knobs, problem, hierarchies):
    """The evaluation that stacks a colour's blocks by size (tests/test_gpu_grid_caps.py runs it at two million rows) against
    the per-column loop, LU blocks and explicit inverses each: within d, the difference between the per-column reference with LU
    blocks and with explicit inverses, which is what the f64 tolerance of the GPU tests is a multiple of.  Measured: 0 in every
    case, LU blocks and explicit inverses (the same LAPACK factorisation of the same block; d is 1.6e-16 to 2.9e-16)."""
    r = problem[1]
    kw = mcr.cycle_kwargs(**knobs)
    levels = hierarchies[hierarchy]
    sizes = {int(s) for lv in levels if lv.col_of is not None for s in np.bincount(lv.col_of)}
    assert len(sizes) >= 3                                               # several stacks per colour
    z = {(b, g): mcr.cycle(levels, r, blocks=b, grouped=g, **kw) for b in ("lu", "inverse") for g in (False, True)}
    d = mcr.relative_difference(z["inverse", False], z["lu", False])
    got = {b: mcr.relative_difference(z[b, True], z[b, False]) for b in ("lu", "inverse")}
    print("%-20s d %.2e   grouped against per-column: lu %.2e, inverse %.2e" % (name, d, got["lu"], got["inverse"]))
    assert d > 0.0
    assert got["lu"] <= d and got["inverse"] <= d, (name, d, got)
    with pytest.raises(AssertionError):
        mcr.cycle(levels, r, factors="f32", grouped=True, **kw)
