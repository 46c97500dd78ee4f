"""One-launch half sweeps of the packed lane-per-column levels on per-column diagonals (gs_lanes_diag_kernel,
csrc/col_gs_lanes.hip, tuning ml_lane_fused): the bits of everything that runs through them against the same solver on the
two-kernel path (ml_lane_fused = 0: diag_residual_kernel + colblock_apply_ldspack_kernel) and without diagonals (ml_diag = 0:
CSR residual rows + the packed kernel).

On these small grids the default tuning solves every level one column per wave, so every solver here gets
col_wave_max = 0 and col_ldsres_min = 1: the packed lane-per-column family on every level that is smoothed.  A small
ml_coarsest_rows gives several levels.  Every case runs with the levels built on the host (ml_device_min = -1) and by the setup
kernels (ml_device_min = 0), and asserts from nkp_ml_level_array (.., "lane_diag"), "dg_val" and "col_kernel" that each of the
three solvers is on the path it is named for.

Shapes: those of tests/test_gpu_wave_diag.py (upwind3 + isop unless said otherwise; 12x10x6 with hmix="const")
  12x10x6             short columns; colours of fewer than 32 columns: one partial group, absent columns
  24x20x12            several groups per colour, the last one partial
  40x36x24 seed 4     coarse levels with one-row columns and columns that start below the surface; groups of fewer than 4 chunks
  tracers2            two coupled tracers: keys to the other tracer's column
  10x8x64 seed 6      the deepest column has exactly 64 rows: 4 full chunks, groups of one key; cut at max_iters = 150
  10x8x70 seed 5      longest column 67 rows: no level qualifies (lane_diag = 0 everywhere), equal results; cut at 150
  noadv               12x10x6 without advection: half bandwidth 1
test_paths_cover checks over all of them that the kernel ran with half bandwidth 1 and 2, on a colour of one group and of
several, with a partial last group, and on groups of fewer than 4 and of 4 chunks of 16 steps.

Every comparison is np.array_equal: the residual rows are the text of diag_residual_kernel (dg_row_sum), the substitution
steps the text of the packed kernel (ldsp_step_fwd / ldsp_step_bwd) on the same LDS image, and x + solution has its operands
in the packed kernel's order.  The batched solve stays on CSR and two kernels and must give every column its single solve.
"""
import numpy as np
import pytest

from nk_ocn_tracer_jacobian_precond_amd import solver, synth

pytestmark = pytest.mark.gpu

SHAPES = {
    "12x10x6": (dict(imt=12, jmt=10, km=6, seed=2, hmix="const"), 1, 200, {}),
    "24x20x12": (dict(imt=24, jmt=20, km=12, seed=2), 1, 200, {}),
    "40x36x24": (dict(imt=40, jmt=36, km=24, seed=4), 1, 300, {}),
    "tracers2": (dict(imt=24, jmt=20, km=12, seed=3, coupled_tracer_cnt=2), 2, 200, {}),
    "10x8x64": (dict(imt=10, jmt=8, km=64, seed=6), 1, 200, dict(max_iters=150)),
    "10x8x70": (dict(imt=10, jmt=8, km=70, seed=5), 1, 200, dict(max_iters=150)),
    "noadv": (dict(imt=12, jmt=10, km=6, seed=2, hmix="const", adv="none"), 1, 200, {}),
}
LONG = ("10x8x70",)                      # columns over 64 rows: stays on two kernels
BUILDERS = {"host": -1, "device": 0}
PACKED = dict(col_wave_max=0, col_ldsres_min=1)
FUSED = dict(PACKED, ml_lane_fused=10 ** 6)
TWO_KERNEL = dict(PACKED, ml_lane_fused=0)
NO_DIAG = dict(FUSED, ml_diag=0)
WAVE_COLUMNS, LDSRES, GW, BAND, MAX_LEN = 0, 3, 4, 5, 7      # positions in "col_kernel"
CH, NCH = 16, 4


class Problem:
    def __init__(self, name):
        kw, self.cnt, self.coarsest, self.options = SHAPES[name]
        kw = dict(dict(adv="upwind3", hmix="isop"), **kw)
        self.p = p = synth.generate(**kw)
        self.other = synth.generate(**dict(kw, day_cnt=180.0))          # other values on the same pattern
        assert np.array_equal(p.rowptr, self.other.rowptr) and np.array_equal(p.colind, self.other.colind)
        assert not np.array_equal(p.nzval, self.other.nzval)
        self.blk = solver.column_blocks(p.col_start(), p.tracer_state_len, self.cnt)
        ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), self.cnt)
        self.coords = dict(col_i=ci, col_j=cj)
        self.n = p.flat_len

    def solver(self, builder, tuning, **more):
        p = self.p
        tuning = dict(dict(ml_coarsest_rows=self.coarsest, ml_device_min=BUILDERS[builder]), **tuning)
        return solver.NkpSolver(p.rowptr, p.colind, p.nzval, self.blk, coupled_tracer_cnt=self.cnt, precond=solver.PRECOND_MULTILEVEL,
                                tuning=tuning, **dict(dict(rtol=1e-10, restart=60, **self.coords), **self.options, **more))

    def rhs(self, k=0):
        return np.random.default_rng(47 + k).standard_normal(self.n)


_problems = {}
_seen = []            # (half bandwidth, groups of the colour, columns of its last group, chunks of a group) wherever the kernel ran


def problem(name):
    if name not in _problems:
        _problems[name] = Problem(name)
    return _problems[name]


@pytest.fixture(params=[(s, b) for s in SHAPES for b in BUILDERS], ids=lambda sb: f"{sb[0]}-{sb[1]}")
def case(request):
    name, builder = request.param
    return name, problem(name), builder


def smoothed_levels(s):
    return range(s.get_int("levels") - 1)


def assert_packed(s):
    for l in smoothed_levels(s):
        ck = s.ml_level_array(l, "col_kernel")
        assert ck[WAVE_COLUMNS] == 0 and ck[LDSRES] == 2 and ck[GW] == 32, (l, ck)


def record_groups(s, l):
    """the tile map against its definition (column c of every group slot, in group order, is the plan's), and what the
    kernel met on this level"""
    ck, blk, cb = s.ml_level_array(l, "col_kernel"), s.ml_level_array(l, "blk_start"), s.ml_level_array(l, "color_blk")
    lens = np.diff(blk)
    assert (lens > 0).all() and lens.max() <= 64                   # tiles are columns
    gt = s.ml_level_array(l, "grp_tile").reshape(-1, 32)
    assert gt.shape[0] == ck[9]
    g = 0
    for c in range(2):
        cols = np.arange(cb[c], cb[c + 1])
        ngrp = (cols.size + 31) // 32
        mine = gt[g:g + ngrp]
        members = mine[mine >= 0]
        assert sorted(members) == list(cols)                       # every column of the colour once, none of the other's
        for row in mine:
            nb = int((row >= 0).sum())
            assert nb >= 1 and (row[:nb] >= 0).all() and (row[nb:] == -1).all()
            _seen.append((int(ck[BAND]), ngrp, nb, int((lens[row[:nb]].max() + CH - 1) // CH)))
        g += ngrp
    assert g == gt.shape[0]


def assert_fused(s, record=False):
    """the new path: every smoothed level packed, on diagonals, lane_diag = 1 (level 0 at least)"""
    assert_packed(s)
    levels = [l for l in smoothed_levels(s) if s.ml_level_array(l, "lane_diag")[0] == 1]
    assert levels and 0 in levels, "level 0 does not run gs_lanes_diag_kernel: nothing would be tested"
    for l in levels:
        assert s.ml_level_array(l, "dg_val").size and s.ml_level_array(l, "col_kernel")[MAX_LEN] <= 64
        if record:
            record_groups(s, l)
    print(f"levels {s.get_int('levels')}, on gs_lanes_diag_kernel {levels}, (P, columns by colour) "
          f"{[(int(s.ml_level_array(l, 'col_kernel')[BAND]), *np.diff(s.ml_level_array(l, 'color_blk')).tolist()) for l in levels]}")
    return levels


def assert_not_fused(s, diagonals):
    """no level on the new kernel; diagonals True: the residual rows of level 0 at least read them, False: every level on CSR,
    None: either"""
    assert_packed(s)
    for l in smoothed_levels(s):
        assert s.ml_level_array(l, "lane_diag")[0] == 0
        if diagonals is False:
            assert s.ml_level_array(l, "dg_val").size == 0
    if diagonals:
        assert s.ml_level_array(0, "dg_val").size


def assert_same_cycle(a, b, P):
    for r in (P.rhs(), P.rhs(1)):
        za, zb = a.precond_apply(r), b.precond_apply(r)
        assert np.all(np.isfinite(za)) and np.any(za != 0.0)
        assert np.array_equal(za, zb)


def assert_same_solve(a, b, P):
    xa, ia = a.solve(P.rhs(2), raise_on_fail=False)
    xb, ib = b.solve(P.rhs(2), raise_on_fail=False)
    assert np.array_equal(xa, xb) and all(ia[k] == ib[k] for k in ("status", "iters", "relres")) and ia["iters"] > 0


def three(P, builder, **more):
    return P.solver(builder, FUSED, **more), P.solver(builder, TWO_KERNEL, **more), P.solver(builder, NO_DIAG, **more)


def assert_paths(name, a, b, c, record=False):
    if name in LONG:
        # a column of 67 rows on every level: five chunks, two tiles -- the two-kernel path, silently
        assert a.ml_level_array(0, "col_kernel")[MAX_LEN] > 64
        assert_not_fused(a, None)
    else:
        assert_fused(a, record)
        if name == "10x8x64":
            assert np.diff(a.ml_level_array(0, "blk_start")).max() == 64
    assert_not_fused(b, None if name in LONG else True)
    assert_not_fused(c, False)


def test_cycle_and_solve(case):
    name, P, builder = case
    a, b, c = three(P, builder)
    with a, b, c:
        assert_paths(name, a, b, c, record=True)
        for other in (b, c):
            assert_same_cycle(a, other, P)
            assert_same_solve(a, other, P)


def test_refresh(case):
    """new values on the same pattern (nkp_refactor): the tile map depends on the pattern only"""
    name, P, builder = case
    a, b, c = three(P, builder)
    with a, b, c:
        before = a.ml_level_array(0, "grp_tile")
        for s in (a, b, c):
            s.refactor(P.other.nzval)
        assert_paths(name, a, b, c)
        assert np.array_equal(before, a.ml_level_array(0, "grp_tile"))
        for other in (b, c):
            assert_same_cycle(a, other, P)
            assert_same_solve(a, other, P)


@pytest.mark.parametrize("nu", [1, 2, 3])
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_sweep_counts(builder, nu):
    """the parity of the buffer ping-pong: 2 nu - 1 fused half sweeps before the coarse correction, 2 nu after"""
    name = "24x20x12"
    P = problem(name)
    a, b, c = three(P, builder, ml_smooth=nu)
    with a, b, c:
        assert_paths(name, a, b, c)
        for other in (b, c):
            assert_same_cycle(a, other, P)
            assert_same_solve(a, other, P)


def test_batch(case):
    """one batched solve of two right-hand sides (CSR and two kernels on every level) gives each the bits of its single solve
    on the new path"""
    name, P, builder = case
    with P.solver(builder, FUSED) as a:
        if name not in LONG:
            assert_fused(a)
        B = np.stack([P.rhs(3), P.rhs(4)])
        X, infos = a.solve_many(B, raise_on_fail=False)
        for k in range(2):
            x, info = a.solve(B[k], raise_on_fail=False)
            assert np.array_equal(X[k], x) and infos[k]["iters"] == info["iters"] and infos[k]["relres"] == info["relres"]


def test_paths_cover():
    """over the cases above (this test runs behind them; on its own it builds what it needs): half bandwidth 1 and 2, a colour of
    one group and of several, a partial last group, groups of fewer than NCH chunks and of NCH"""
    if not _seen:
        for name in SHAPES:
            if name not in LONG:
                with problem(name).solver("device", FUSED) as a:
                    assert_fused(a, record=True)
    seen = sorted(set(_seen))
    print(seen)
    assert {1, 2} <= {P for P, _, _, _ in seen}
    assert any(ngrp == 1 for _, ngrp, _, _ in seen) and any(ngrp > 1 for _, ngrp, _, _ in seen)
    assert any(nb < 32 for _, _, nb, _ in seen) and any(nb == 32 for _, _, nb, _ in seen)
    assert any(nch < NCH for _, _, _, nch in seen) and any(nch == NCH for _, _, _, nch in seen)
