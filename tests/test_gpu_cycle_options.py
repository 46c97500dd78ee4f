"""Every cycle option and every hierarchy option against the cycle restated in tests/ml_cycle_reference.py.

The restatement takes the LEVELS from the device (nkp_ml_level_array: operator, column blocks, colours, cmap, the last level's
inverse) and restates only the cycle, so it runs on whatever hierarchy the planner built; each level is then checked against
the one above it through the identity that made it, L_{l+1} = P^T L_l P.  What is compared is precond_apply on one fixed vector.

  (a) the cycle options (mcr.OPTION_CASES) x f32 / f64 storage, each under the kernel families that must give the same bits:
      gs_wave_kernel (default), residual range + lane kernels (col_wave_max = 0), gs_fused_kernel (col_wave_max = 0, ml_fused = 1)
      and ml_tail_kernel (ml_tail_rows = 16000, which by design applies only with a dense last level and no W-level)
  (b) the hierarchy options, at the default cycle and at the combined case of (a), plus the structure of every level
  (c) ml_cycle at K >= 2: solve_many against solve, column by column, for the cases that change its control flow, and at the
      default and the combined case under each kernel family of (a) -- at K >= 2 every operation has one kernel, whatever
      family serves the single cycle, so the single solves it is compared with take other kernels in every family

Tolerances of (a) and (b), from the reference alone, computed here on the levels of the case at hand:
  f64 storage   ||z - z_ref|| <= max (1e-12, 4096 * d) ||z_ref||, d = reference with LU blocks against explicit inverses (the
                device sums in another order and factors the bands without pivoting: 12 of the 52 bits)
  f32 storage   ||z - z_ref|| <= min (2e-5, 16 * e) ||z_ref||, z_ref on the f32 operators with exact blocks, e = the largest
                change that f32 storage of the block factors and of the last level's inverse makes over the cases of that hierarchy.
                The factors are those of the f64 operator's blocks, rounded (the setup factors before it rounds the operator), so
                the emulation takes the f64 operators from a solver with f64 storage (mcr.with_exact_blocks).  A first emulation
                that factored the blocks of the ROUNDED operator gave an e 8 to 20 times smaller, and the graph fallback at the
                combined case then stood at 1.4 times its bound (9.6e-8 against 7.1e-8): the block solve and the residual it is
                applied to disagree by the rounding of the block's own entries, which is most of what f32 storage costs here.

Measured on an MI355X, ||z - z_ref|| / ||z_ref|| and its ratio to the bound:
  default                            f64  1.6e-16  bound 1.0e-12  ratio 0.00016
  default                            f32  3.6e-09  bound 1.5e-06  ratio 0.0024
  nu1                                f64  4.5e-16  bound 1.7e-12  ratio 0.00027
  nu1                                f32  8.0e-08  bound 1.5e-06  ratio 0.055
  nu2                                f64  2.1e-16  bound 1.0e-12  ratio 0.0002
  nu2                                f32  1.6e-08  bound 1.5e-06  ratio 0.011
  nu2_coarse1_from1                  f64  3.3e-16  bound 1.3e-12  ratio 0.00026
  nu2_coarse1_from1                  f32  2.5e-08  bound 1.5e-06  ratio 0.017
  coarse1_from2                      f64  1.6e-16  bound 1.0e-12  ratio 0.00016
  coarse1_from2                      f32  3.8e-09  bound 1.5e-06  ratio 0.0026
  gamma_0_1                          f64  1.5e-16  bound 1.0e-12  ratio 0.00015
  gamma_0_1                          f32  3.9e-09  bound 1.5e-06  ratio 0.0027
  gamma_1_3                          f64  1.8e-16  bound 1.0e-12  ratio 0.00018
  gamma_1_3                          f32  3.4e-09  bound 1.5e-06  ratio 0.0023
  gamma_0_9                          f64  1.5e-16  bound 1.0e-12  ratio 0.00015
  gamma_0_9                          f32  3.2e-09  bound 1.5e-06  ratio 0.0022
  omega_1.0                          f64  1.8e-16  bound 1.0e-12  ratio 0.00018
  omega_1.0                          f32  3.3e-09  bound 1.5e-06  ratio 0.0022
  omega_1.35                         f64  1.9e-16  bound 1.0e-12  ratio 0.00019
  omega_1.35                         f32  5.0e-09  bound 1.5e-06  ratio 0.0034
  sweeps5                            f64  2.5e-16  bound 1.0e-12  ratio 0.00025
  sweeps5                            f32  3.4e-09  bound 5.3e-08  ratio 0.064
  sweeps30                           f64  2.2e-16  bound 1.0e-12  ratio 0.00022
  sweeps30                           f32  3.4e-09  bound 5.3e-08  ratio 0.065
  levels2                            f64  1.5e-16  bound 1.0e-12  ratio 0.00015
  levels2                            f32  4.3e-09  bound 6.0e-08  ratio 0.072
  combined                           f64  1.8e-16  bound 1.0e-12  ratio 0.00018
  combined                           f32  3.5e-08  bound 1.5e-06  ratio 0.024
  device_built / default             f64  1.6e-16  bound 1.0e-12  ratio 0.00016
  device_built / combined            f64  1.8e-16  bound 1.0e-12  ratio 0.00018
  device_built / default             f32  3.6e-09  bound 4.7e-07  ratio 0.0076
  device_built / combined            f32  3.5e-08  bound 4.7e-07  ratio 0.073
  split0 / default                   f64  1.7e-16  bound 1.0e-12  ratio 0.00017
  split0 / combined                  f64  2.8e-16  bound 1.0e-12  ratio 0.00028
  split0 / default                   f32  3.5e-09  bound 3.1e-07  ratio 0.012
  split0 / combined                  f32  2.1e-08  bound 3.1e-07  ratio 0.068
  big_from1 / default                f64  1.5e-16  bound 1.0e-12  ratio 0.00015
  big_from1 / combined               f64  4.2e-16  bound 1.5e-12  ratio 0.00028
  big_from1 / default                f32  4.0e-09  bound 4.5e-07  ratio 0.0089
  big_from1 / combined               f32  2.8e-08  bound 4.5e-07  ratio 0.062
  huge_from1 / default               f64  2.3e-16  bound 1.0e-12  ratio 0.00023
  huge_from1 / combined              f64  2.4e-16  bound 1.1e-12  ratio 0.00021
  huge_from1 / default               f32  3.6e-09  bound 3.9e-07  ratio 0.0094
  huge_from1 / combined              f32  2.4e-08  bound 3.9e-07  ratio 0.061
  pocket0 / default                  f64  1.5e-16  bound 1.0e-12  ratio 0.00015
  pocket0 / combined                 f64  1.8e-16  bound 1.1e-12  ratio 0.00017
  pocket0 / default                  f32  3.6e-09  bound 5.3e-07  ratio 0.0067
  pocket0 / combined                 f32  3.9e-08  bound 5.3e-07  ratio 0.073
  theta0.25 / default                f64  1.9e-16  bound 1.0e-12  ratio 0.00019
  theta0.25 / combined               f64  1.5e-16  bound 1.0e-12  ratio 0.00015
  theta0.25 / default                f32  3.0e-09  bound 2.5e-07  ratio 0.012
  theta0.25 / combined               f32  1.5e-08  bound 2.5e-07  ratio 0.058
  tau0.2 / default                   f64  1.6e-16  bound 1.0e-12  ratio 0.00016
  tau0.2 / combined                  f64  2.4e-16  bound 1.6e-12  ratio 0.00015
  tau0.2 / default                   f32  3.6e-09  bound 4.5e-07  ratio 0.008
  tau0.2 / combined                  f32  3.3e-08  bound 4.5e-07  ratio 0.074
  graph_fallback / default           f64  1.7e-16  bound 1.0e-12  ratio 0.00017
  graph_fallback / combined          f64  4.5e-16  bound 2.3e-12  ratio 0.00019
  graph_fallback / default           f32  5.4e-09  bound 1.5e-06  ratio 0.0035
  graph_fallback / combined          f32  9.6e-08  bound 1.5e-06  ratio 0.062
  tracers2 / default                 f64  1.0e-15  bound 3.9e-12  ratio 0.00027
  tracers2 / combined                f64  1.3e-15  bound 4.4e-12  ratio 0.00029
  tracers2 / default                 f32  2.0e-08  bound 5.8e-07  ratio 0.035
  tracers2 / combined                f32  3.9e-08  bound 5.8e-07  ratio 0.067
  long_columns / default             f64  2.6e-15  bound 6.7e-12  ratio 0.00039
  long_columns / combined            f64  4.5e-15  bound 6.2e-12  ratio 0.00073
  long_columns / default             f32  7.8e-08  bound 5.2e-06  ratio 0.015
  long_columns / combined            f32  2.6e-07  bound 5.2e-06  ratio 0.049
"""
import numpy as np
import pytest

import ml_cycle_reference as mcr
from ml_structure_checks import check_structure, check_twin
from nk_ocn_tracer_jacobian_precond_amd import solver, synth

pytestmark = pytest.mark.gpu

OPTION_FIELDS = ("ml_smooth", "ml_levels")                 # knobs of nkp_options; every other one is in nkp_tuning

# (nkp_options, nkp_tuning) that make the hierarchies of the option cases, and their levels
CYCLE_HIERARCHIES = {
    "deep": (dict(), dict(ml_coarsest_rows=60), 5),
    "iterated": (dict(), dict(ml_coarsest_rows=300, ml_dense_max=100), 3),
    "two": (dict(ml_levels=2), dict(ml_coarsest_rows=60), 2),
}
FAMILIES = [("wave", dict()),
            ("lanes", dict(col_wave_max=0)),
            ("fused", dict(col_wave_max=0, ml_fused=1)),
            ("tail", dict(ml_tail_rows=16000))]

# (problem, nkp_tuning, rows per level of the stand-alone host planner, must differ from the default hierarchy)
HIERARCHY_CASES = {
    "device_built": ("one", dict(ml_device_min=0), [2813, 889, 275, 100, 13], False),
    "split0": ("one", dict(ml_split=0), [2813, 893, 266, 85, 10], True),
    "big_from1": ("one", dict(ml_big_from=1), [2813, 889, 104, 16], True),
    "huge_from1": ("one", dict(ml_huge_from=1), [2813, 889, 56], True),
    "pocket0": ("one", dict(ml_pocket=0), [2813, 894, 277, 102, 14], True),
    "theta0.25": ("one", dict(ml_theta=0.25), [2813, 1061, 363, 141, 23], True),
    "tau0.2": ("one", dict(ml_tau=0.2), [2813, 889, 275, 101, 13], True),
    "graph_fallback": ("graph", dict(), [2813, 767, 233, 82, 35], True),
    "tracers2": ("tracers2", dict(), [4970, 1702, 542, 230, 32], False),
    "long_columns": ("long", dict(ml_coarsest_rows=200), [17146, 5680, 1785, 684, 137], False),
}
DEFAULT_ROWS = [2813, 889, 275, 100, 13]

BATCH_CASES = ["nu2_coarse1_from1", "gamma_1_3", "gamma_0_9", "omega_1.0", "sweeps5", "combined"]
CASES = {name: (hierarchy, knobs) for name, hierarchy, knobs in mcr.OPTION_CASES}


class Problem:
    def __init__(self, name):
        cnt, kw = 1, dict(imt=24, jmt=20, km=10, adv="upwind3", hmix="isop", seed=2)
        if name == "tracers2":
            cnt, kw = 2, dict(kw, coupled_tracer_cnt=2, seed=3)
        elif name == "long":
            kw = dict(imt=24, jmt=20, km=70, adv="centred", hmix="const", seed=5)
        self.p = p = synth.generate(**kw)
        self.cnt = cnt
        self.blk = solver.column_blocks(p.col_start(), p.tracer_state_len, cnt)
        self.coords = {}
        if name != "graph":
            ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), cnt)
            self.coords = dict(col_i=ci, col_j=cj)
        self.r = np.random.default_rng(17).standard_normal(p.flat_len)

    def solver(self, options, tuning, **more):
        p = self.p
        return solver.NkpSolver(p.rowptr, p.colind, p.nzval, self.blk, coupled_tracer_cnt=self.cnt, precond=solver.PRECOND_MULTILEVEL,
                                tuning=tuning, **dict(dict(restart=4, **self.coords), **options, **more))


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Problem(name)
        return cache[name]
    return get


def split_knobs(knobs):
    return ({k: v for k, v in knobs.items() if k in OPTION_FIELDS}, {k: v for k, v in knobs.items() if k not in OPTION_FIELDS})


Reference = mcr.Reference          # z_ref per case and the yardsticks d / e of the tolerances above


@pytest.fixture(scope="module")
def cycle_references(problems):
    cache = {}

    def get(hierarchy, f32):
        if (hierarchy, f32) not in cache:
            options, tuning, nlev = CYCLE_HIERARCHIES[hierarchy]
            prob = problems("one")
            with prob.solver(options, dict(tuning, ml_f32=f32)) as s:
                assert s.get_int("levels") == nlev, (hierarchy, s.get_int("levels"))
                inv = s.ml_level_array(nlev - 1, "coarse_inv")
                assert (inv.size == 0) == (hierarchy == "iterated"), (hierarchy, inv.size)
                levels = mcr.levels_from_solver(s)
            if f32:
                levels = mcr.with_exact_blocks(levels, get(hierarchy, 0).levels)
            cases = {name: knobs for name, (h, knobs) in CASES.items() if h == hierarchy}
            cache[(hierarchy, f32)] = Reference(levels, prob.r, f32, cases)
        return cache[(hierarchy, f32)]
    return get


# ================================================================ (a) cycle options
@pytest.mark.parametrize("f32", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("case", list(CASES))
def test_cycle_options_match_the_restated_cycle(case, f32, problems, cycle_references):
    hierarchy, knobs = CASES[case]
    options, tuning, nlev = CYCLE_HIERARCHIES[hierarchy]
    ref = cycle_references(hierarchy, f32)
    prob = problems("one")
    case_options, case_tuning = split_knobs(knobs)
    z = {}
    for family, family_tuning in FAMILIES:
        with prob.solver(dict(options, **case_options), dict(tuning, ml_f32=f32, **case_tuning, **family_tuning)) as s:
            assert s.get_int("levels") == nlev
            assert [s.ml_level_array(l, "rowptr").size - 1 for l in range(nlev)] == ref.rows
            z[family] = s.precond_apply(prob.r)
    assert np.isfinite(z["wave"]).all()
    # the same cycle whatever kernels serve it; where the tail does not apply (a relaxed last level, a W-level) it falls
    # back by design, which shows as the same bits too
    for family, _ in FAMILIES[1:]:
        assert np.array_equal(z["wave"], z[family]), (case, f32, family, np.abs(z["wave"] - z[family]).max())
    ref.check(case, case, z["wave"])


# ================================================================ (b) hierarchy options
@pytest.fixture(scope="module")
def default_rows(cycle_references):
    return cycle_references("deep", 0).rows


@pytest.mark.parametrize("f32", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(HIERARCHY_CASES))
def test_hierarchy_options_match_the_restated_cycle(name, f32, problems, default_rows):
    problem, knobs, planner_rows, differs = HIERARCHY_CASES[name]
    prob = problems(problem)
    assert default_rows == DEFAULT_ROWS
    tuning = dict(dict(ml_coarsest_rows=60), ml_f32=f32, **knobs)
    cases = {"default": {}, "combined": mcr.COMBINED}
    with prob.solver({}, tuning) as s:
        nlev = s.get_int("levels")
        assert nlev >= 3, nlev
        if name == "device_built":
            assert s.get_int("ml_levels_on_device") >= 2
        levels = mcr.levels_from_solver(s)
        rows = [lv.n for lv in levels]
        print(name, "rows per level", rows)
        assert rows == planner_rows, rows
        if differs:
            assert rows != default_rows                                  # a knob that is ignored builds the default hierarchy
        if not f32:
            check_structure(levels, s)
            if prob.cnt == 1:
                check_twin(levels[0], prob)
        z = {"default": s.precond_apply(prob.r)}
    if f32:
        with prob.solver({}, dict(tuning, ml_f32=0)) as s:
            levels = mcr.with_exact_blocks(levels, mcr.levels_from_solver(s))
    case_options, case_tuning = split_knobs(mcr.COMBINED)
    with prob.solver(case_options, dict(tuning, **case_tuning)) as s:
        assert [s.ml_level_array(l, "rowptr").size - 1 for l in range(s.get_int("levels"))] == rows
        z["combined"] = s.precond_apply(prob.r)
    ref = Reference(levels, prob.r, f32, cases)
    for case in cases:
        ref.check("%s / %s" % (name, case), case, z[case])


# ================================================================ (c) the cycle on K interleaved right-hand sides
def batch_against_single(prob, options, tuning, nrhs_list, nmax):
    B = np.random.default_rng(11).standard_normal((nmax, prob.p.flat_len))
    B[2] *= 1e-3                                            # systems of a group converge at different steps
    with prob.solver(options, tuning, rtol=1e-10, restart=200, max_iters=4000) as s:
        single = [s.solve(B[c], raise_on_fail=False) for c in range(nmax)]
        assert all(i["status"] in (solver.NKP_OK, solver.NKP_OK_BERR) for _, i in single), [i for _, i in single]
        for nrhs in nrhs_list:
            X, infos = s.solve_many(B[:nrhs], raise_on_fail=False)
            for c in range(nrhs):
                x1, i1 = single[c]
                assert infos[c]["iters"] == i1["iters"] and infos[c]["relres"] == i1["relres"], (nrhs, c, infos[c], i1)
                assert np.array_equal(X[c], x1), (nrhs, c, np.abs(X[c] - x1).max())
        assert s.get_int("batch_width") >= 2                 # the batched path ran


# (case, kernel family of (a), widths): the cases that change the control flow under the default family, then the default and the
# combined case under every family -- at K >= 2 each operation has one kernel whatever family serves the single cycle, so the
# single solves of a column take other kernels there and must give the same bits
BATCH_PARAMS = [pytest.param(case, "wave", (2, 3, 4, 5), id=case) for case in BATCH_CASES]
BATCH_PARAMS += [pytest.param(case, family, (2, 3, 5), id="%s-%s" % (case, family))
                 for case in ("default", "combined") for family, _ in FAMILIES if (case, family) != ("combined", "wave")]


@pytest.mark.parametrize("f32", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("case, family, nrhs_list", BATCH_PARAMS)
def test_batched_cycle_options_have_the_bits_of_single_solves(case, family, nrhs_list, f32, problems):
    hierarchy, knobs = CASES[case]
    options, tuning, _ = CYCLE_HIERARCHIES[hierarchy]
    case_options, case_tuning = split_knobs(knobs)
    batch_against_single(problems("one"), dict(options, **case_options), dict(tuning, ml_f32=f32, **case_tuning, **dict(FAMILIES)[family]), nrhs_list, 5)


def test_eight_wide_batched_cycle_has_the_bits_of_single_solves(problems):
    hierarchy, knobs = CASES["combined"]
    options, tuning, _ = CYCLE_HIERARCHIES[hierarchy]
    case_options, case_tuning = split_knobs(knobs)
    batch_against_single(problems("one"), dict(options, **case_options), dict(tuning, rhs_batch=8, **case_tuning), (8,), 8)
