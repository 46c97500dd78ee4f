"""The inputs of the hierarchy-setup tests: one named case per option of the setup and per hand-over point between the setup
kernels (csrc/mlsetup.hip) and the host planner (csrc/ml_plan.cpp).  TEST INFRASTRUCTURE, shared by tests/test_ml_plan.py (host
planner against the restatement tests/ml_reference.py, no GPU) and tests/test_gpu_setup_options.py (kernels against both).

Every case is the smallest grid at which its branch is reached.  `rows` are the rows per level at the case's ml_coarsest_rows
(COARSEST where the case names none), as the restatement builds them; `rows200` are the rows per level at ml_coarsest_rows = 200
where the case was first checked at that setting -- the same hierarchy cut off earlier, so a prefix of `rows`."""
from collections import namedtuple

import numpy as np

from nk_ocn_tracer_jacobian_precond_amd import solver, synth

COARSEST = 60                                   # so that even the small grids get several levels
Case = namedtuple("Case", "group synth tuning rows rows200 cnt cell_major coord_scale")


def _case(group, synth_args, tuning, rows, rows200=None, cnt=1, cell_major=False, coord_scale=1):
    return Case(group, synth_args, tuning, rows, rows200, cnt, cell_major, coord_scale)


def _grid(imt, jmt, km, seed, adv="upwind3", hmix="isop", **more):
    return dict(imt=imt, jmt=jmt, km=km, adv=adv, hmix=hmix, seed=seed, **more)


BASE = _grid(24, 20, 10, 2)
DEFAULT_ROWS = [2813, 889, 275, 100, 13]
_TIES = dict(noise=0.0, hmix="const")

CASES = {
    "default": _case("default", BASE, {}, DEFAULT_ROWS, [2813, 889, 275, 100]),
    # ---- knobs: one option of the aggregation each
    "pocket0": _case("knobs", BASE, dict(ml_pocket=0), [2813, 894, 277, 102, 14], [2813, 894, 277, 102]),
    "pocket9": _case("knobs", BASE, dict(ml_pocket=9), [2813, 886, 272, 95, 17], [2813, 886, 272, 95]),
    "tau0": _case("knobs", BASE, dict(ml_tau=0.0), [2813, 889, 275, 99, 13], [2813, 889, 275, 99]),
    "tau0.2": _case("knobs", BASE, dict(ml_tau=0.2), [2813, 889, 275, 101, 13], [2813, 889, 275, 101]),
    "tau5": _case("knobs", BASE, dict(ml_tau=5.0), [2813, 889, 275, 101, 15], [2813, 889, 275, 101]),
    "big_from0": _case("knobs", BASE, dict(ml_big_from=0), [2813, 276, 52], [2813, 276, 52]),
    "big_from1": _case("knobs", BASE, dict(ml_big_from=1), [2813, 889, 104, 16], [2813, 889, 104]),
    "huge_from1": _case("knobs", BASE, dict(ml_huge_from=1), [2813, 889, 56]),
    "huge_from0": _case("knobs", BASE, dict(ml_huge_from=0), [2813, 105, 14]),
    # ---- other bathymetries and circulations at the default knobs
    **{"seed%d" % s: _case("seeds", dict(BASE, seed=s), {}, rows)
       for s, rows in ((0, [2406, 772, 247, 108, 19]), (1, [2413, 806, 252, 101, 13]), (3, [2485, 851, 271, 115, 16]), (4, [2643, 871, 260, 94, 14]),
                       (5, [2661, 879, 271, 98, 20]))},
    # ---- no eddy noise and constant mixing: many couplings of exactly equal strength, so the anchor of a stub is decided by
    # the tie rule (the last entry that attains the maximum)
    "ties_none": _case("ties", dict(BASE, adv="none", **_TIES), dict(ml_tau=0.2), [2813, 889, 275, 100, 15]),
    "ties_donor": _case("ties", dict(BASE, adv="donor", **_TIES), dict(ml_tau=0.5), [2813, 889, 275, 101, 15]),
    "ties_centred": _case("ties", dict(BASE, adv="centred", seed=3, **_TIES), dict(ml_tau=1.0), [2485, 851, 270, 115, 14]),
    # (in this one an absorbed stub's strongest coupling is attained twice, by entries that end in different coarse cells)
    "ties_none_seed3": _case("ties", dict(BASE, adv="none", seed=3, **_TIES), dict(ml_tau=0.5), [2485, 851, 271, 115, 14]),
    # ---- columns of 64 and more cells: several rounds of pointer jumping when the sets are threaded through depth
    # (12 x 10 x 70 at seed 5 has 3679 rows but no column longer than 63 cells, so the small grid has 75 levels)
    "deep_12x10x75": _case("depth", _grid(12, 10, 75, 5, "centred", "const"), {}, [3938, 1569, 631, 401, 120]),
    "deep_24x20x70": _case("depth", _grid(24, 20, 70, 5, "centred", "const"), dict(ml_tau=0.3, ml_pocket=9), [17146, 5661, 1760, 624, 111, 92], [17146, 5661, 1760, 624, 111]),
    # ---- odd extents: groups cut off at the grid's edge
    "odd_31x27x9": _case("odd", _grid(31, 27, 9, 6), dict(ml_tau=0.3, ml_pocket=2, ml_coarsest_rows=60), [4350, 1274, 418, 145, 14]),
    "odd_17x13x7": _case("odd", _grid(17, 13, 7, 1), dict(ml_coarsest_rows=60), [744, 261, 95, 44]),
    # ---- the largest case: more than one workgroup's worth of sets everywhere
    "larger_40x46x20": _case("larger", _grid(40, 46, 20, 7), dict(ml_pocket=9, ml_tau=0.2), [20246, 5933, 1869, 594, 124, 26], [20246, 5933, 1869, 594, 124]),
    # ---- coupled tracers, rows tracer-major (tracer of a column by position) and cell-major (col_t names it)
    "tracers2": _case("tracers", dict(BASE, seed=3, coupled_tracer_cnt=2), {}, [4970, 1702, 542, 230, 32], cnt=2),
    "tracers3": _case("tracers", dict(BASE, coupled_tracer_cnt=3), {}, [8439, 2667, 825, 300, 39], cnt=3),
    "tracers2_cell_major": _case("tracers", dict(BASE, seed=3, coupled_tracer_cnt=2), {}, [4970, 1702, 542, 230, 32], cnt=2, cell_major=True),
    "tracers3_cell_major": _case("tracers", dict(BASE, coupled_tracer_cnt=3), {}, [8439, 2667, 825, 300, 39], cnt=3, cell_major=True),
    # ---- grid coordinates multiplied by 4: every group holds one column, so only pockets and stubs can coarsen anything
    "stall": _case("stall", _grid(12, 10, 6, 2), dict(ml_pocket=0), [383], coord_scale=4),
    "near_stall": _case("stall", _grid(12, 10, 6, 2), {}, [383, 381], coord_scale=4),
}

KNOB_ENV = {"ml_pocket": "NKP_ML_POCKET", "ml_tau": "NKP_ML_TAU", "ml_theta": "NKP_ML_THETA", "ml_big_from": "NKP_ML_BIG_FROM",
            "ml_huge_from": "NKP_ML_HUGE_FROM"}


def names(*groups, single_tracer=False):
    return [n for n, c in CASES.items() if (not groups or c.group in groups) and not (single_tracer and c.cnt > 1)]


def coarsest_rows(case):
    return CASES[case].tuning.get("ml_coarsest_rows", COARSEST)


def plan_knobs(case):
    """the aggregation knobs of the case without ml_coarsest_rows, which the planner and the restatement take as an argument"""
    return {k: v for k, v in CASES[case].tuning.items() if k != "ml_coarsest_rows"}


def setenv(case, monkeypatch):
    """the case's knobs for nkp_ml_plan_host, which reads only the environment"""
    for env in KNOB_ENV.values():
        monkeypatch.delenv(env, raising=False)
    for k, v in plan_knobs(case).items():
        monkeypatch.setenv(KNOB_ENV[k], repr(v))


def restatement_knobs(case):
    """keyword arguments of ml_reference.build for the case"""
    t = CASES[case].tuning
    return dict(coarsest_rows=coarsest_rows(case), pocket=t.get("ml_pocket", 4), theta=t.get("ml_theta", 0.0), tau=t.get("ml_tau", 0.01),
                big_from=t.get("ml_big_from", 3), huge_from=t.get("ml_huge_from", -1))


_problems = {}


def problem(case, **synth_overrides):
    """(p, blk, col_i, col_j, col_t) of a case; col_t is None unless the rows are cell-major, and p then holds the renumbered
    matrix in p.rowptr / p.colind / p.nzval (nothing else of p is renumbered)."""
    c = CASES[case]
    key = (case, tuple(sorted(synth_overrides.items())))
    if key in _problems:
        return _problems[key]
    p = synth.generate(**dict(c.synth, **synth_overrides))
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, c.cnt)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), c.cnt)
    ci, cj = np.asarray(ci, np.int32) * c.coord_scale, np.asarray(cj, np.int32) * c.coord_scale
    col_t = None
    if c.cell_major:
        perm, inv, blk, col_t, col_src = solver.cell_major_order(blk, c.cnt)
        p.rowptr, p.colind, p.nzval = solver.permuted_rows(p.rowptr, p.colind, p.nzval, perm, inv, 0, p.flat_len)
        ci, cj = ci[col_src], cj[col_src]
    _problems[key] = (p, blk, ci, cj, col_t)
    return _problems[key]


def row_arrays(blk, ci, cj, cnt=1, col_t=None):
    """per row: i, j, depth, column and tracer, from the per-column arrays (every column starts at the surface)"""
    blk = np.asarray(blk, np.int64)
    nblk = blk.size - 1
    colid = np.repeat(np.arange(nblk), np.diff(blk))
    ck = np.arange(blk[-1]) - blk[colid]
    t = np.asarray(col_t, np.int64) if col_t is not None else np.arange(nblk) // (nblk // cnt)
    return np.asarray(ci, np.int64)[colid], np.asarray(cj, np.int64)[colid], ck, colid, t[colid]
