"""Wave-fused half sweeps on per-column diagonals (gs_wave_diag_kernel, csrc/diagop.hip): the bits of everything that runs
through them against the same solver on the CSR kernel (ml_diag = 0, gs_wave_kernel) and on the two-kernel path
(col_wave_max = 0, ml_wave_fused = 0: residual rows + column solves).

On these small grids every level has fewer than col_wave_max columns, so with the default tuning level 0 itself is
wave-fused; a small ml_coarsest_rows gives several levels.  Every case runs with the levels built on the host
(ml_device_min = -1) and by the setup kernels (ml_device_min = 0), and asserts from nkp_ml_level_array (.., "wave_diag"),
"dg_val" and "col_kernel" that each of the three solvers is on the path it is named for.

Shapes (upwind3 + isop unless said otherwise; 12x10x6 with hmix="const", see tests/test_gpu_diag_residual.py):
  12x10x6, 24x20x12   short columns
  40x36x24 seed 4     coarse levels with one-row columns and columns that start below the surface
  tracers2            two coupled tracers: keys to the other tracer's column
  10x8x64 seed 6      the deepest column has exactly 64 rows: groups of one key (17 keys at most, padding 1.31 nnz on level 0,
                      worked out on the host from the low-order twin); cut at max_iters = 150
  10x8x70 seed 5      longest column 67 rows: no level qualifies, the CSR kernel with its descriptors still runs; cut at 150
  noadv               12x10x6 without advection: narrower bands on the coarse levels
test_paths_cover checks over all of them that the new kernel ran with half bandwidth 1 and 2 and on colours whose number of
columns leaves every remainder modulo the 4 waves of a workgroup.

Every comparison is np.array_equal: the kernel sums a row's products in ascending column order from +0.0 like the CSR
kernel, a padded position adds 0.0f * x = +-0, and the substitution sweeps are the same text (wave_band_sweeps).
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
LONG = ("10x8x70",)                      # columns over 64 rows: stays on CSR
BUILDERS = {"host": -1, "device": 0}
TWO_KERNEL = dict(col_wave_max=0, ml_wave_fused=0)
WAVE_FUSED, BAND, MAX_LEN = 1, 5, 7      # positions in "col_kernel"


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

    def solver(self, builder, tuning=None, values=None, **more):
        p = self.p
        tuning = dict(dict(ml_coarsest_rows=self.coarsest, ml_device_min=BUILDERS[builder]), **(tuning or {}))
        return solver.NkpSolver(p.rowptr, p.colind, p.nzval if values is None else values, self.blk, coupled_tracer_cnt=self.cnt,
                                precond=solver.PRECOND_MULTILEVEL, tuning=tuning,
                                **dict(dict(rtol=1e-10, restart=60, **self.coords), **self.options, **more))

    def rhs(self, k=0):
        return np.random.default_rng(47 + k).standard_normal(self.n)


_problems = {}
_seen = []            # (shape, level, half bandwidth, columns of colour 0, of colour 1) of every level the new kernel ran on


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


def wave_diag_levels(s):
    return [l for l in smoothed_levels(s) if s.ml_level_array(l, "wave_diag")[0] == 1]


def assert_on_diagonals(s, name=None):
    """default tuning: the wave-fused levels whose columns fit a wave run the new kernel and have the diagonals"""
    levels = wave_diag_levels(s)
    assert levels and 0 in levels, "level 0 does not run gs_wave_diag_kernel: nothing would be tested"
    for l in smoothed_levels(s):
        ck, cb = s.ml_level_array(l, "col_kernel"), s.ml_level_array(l, "color_blk")
        if l in levels:
            assert ck[WAVE_FUSED] == 1 and ck[MAX_LEN] <= 64 and s.ml_level_array(l, "dg_val").size
            if name:
                _seen.append((name, l, int(ck[BAND]), int(cb[1] - cb[0]), int(cb[2] - cb[1])))
        else:
            assert s.ml_level_array(l, "wave_diag")[0] == 0
    print(f"levels {s.get_int('levels')}, on gs_wave_diag_kernel {levels}, "
          f"(P, columns of colour 0, of colour 1, most keys) "
          f"{[(int(s.ml_level_array(l, 'col_kernel')[BAND]), *np.diff(s.ml_level_array(l, 'color_blk')).tolist(), int(np.diff(s.ml_level_array(l, 'dg_ptr')).max())) for l in levels]}")
    return levels


def assert_on_csr_wave(s, levels=(0,)):
    """no level on the new kernel or with diagonals; the CSR kernel gs_wave_kernel on `levels`"""
    for l in smoothed_levels(s):
        assert s.ml_level_array(l, "wave_diag")[0] == 0 and s.ml_level_array(l, "dg_val").size == 0
    for l in levels:
        assert s.ml_level_array(l, "col_kernel")[WAVE_FUSED] == 1


def assert_two_kernel(s):
    for l in smoothed_levels(s):
        assert s.ml_level_array(l, "wave_diag")[0] == 0 and s.ml_level_array(l, "col_kernel")[WAVE_FUSED] == 0


def one_colour_zeroed(s, r):
    """r with the rows of colour 0 (level-0 rows [0, rows0) in colour-major order) zeroed"""
    perm0, blk, cb = s.ml_level_array(0, "perm0"), s.ml_level_array(0, "blk_start"), s.ml_level_array(0, "color_blk")
    out = r.copy()
    out[perm0[:blk[cb[1]]]] = 0.0
    return out


def end_rows(s):
    """original rows of the first and the last column of each colour of level 0: their x windows are clamped at 0, at the
    colour boundary (split) and at n"""
    perm0, blk, cb = s.ml_level_array(0, "perm0"), s.ml_level_array(0, "blk_start"), s.ml_level_array(0, "color_blk")
    cols = [c for c in (cb[0], cb[1] - 1, cb[1], cb[2] - 1) if 0 <= c < cb[2]]
    return np.concatenate([perm0[blk[c]:blk[c + 1]] for c in cols])


def assert_same_cycle(a, b, P):
    rows = end_rows(a)
    assert rows.size and np.array_equal(np.sort(rows), np.sort(end_rows(b)))
    for r in (P.rhs(), one_colour_zeroed(a, P.rhs(1))):
        za, zb = a.precond_apply(r), b.precond_apply(r)
        assert np.all(np.isfinite(za)) and np.any(za[rows] != 0.0)
        assert np.array_equal(za[rows], zb[rows])              # the array ends
        assert np.array_equal(za, zb)


def assert_same_solve(a, b, P):
    xa, ia = a.solve(P.rhs(2), raise_on_fail=False)
    xb, ib = b.solve(P.rhs(2), raise_on_fail=False)
    assert np.array_equal(xa, xb) and all(ia[k] == ib[k] for k in ("status", "iters", "relres")) and ia["iters"] > 0


def test_cycle_and_solve(case):
    name, P, builder = case
    with P.solver(builder) as a, P.solver(builder, dict(ml_diag=0)) as b, P.solver(builder, TWO_KERNEL) as c:
        if name in LONG:
            # a column of 67 rows on every level: CSR and its descriptors, as before
            assert a.ml_level_array(0, "col_kernel")[MAX_LEN] > 64 and not wave_diag_levels(a)
            levels = (0,)
            assert_on_csr_wave(a, levels)
        else:
            levels = assert_on_diagonals(a, name)
            if name == "10x8x64":
                assert np.diff(a.ml_level_array(0, "blk_start")).max() == 64
                gptr, ptr = a.ml_level_array(0, "dg_gptr"), a.ml_level_array(0, "dg_ptr")
                tall = int(np.argmax(np.diff(a.ml_level_array(0, "blk_start"))))
                assert gptr[tall + 1] - gptr[tall] == ptr[tall + 1] - ptr[tall]          # groups of one key
        assert_on_csr_wave(b, levels)
        assert_two_kernel(c)
        for other in (b, c):
            assert_same_cycle(a, other, P)
            assert_same_solve(a, other, P)


def test_refresh(case):
    """new values on the same pattern: a plain refactor against the CSR solver through the same refactor, a refactor with
    rebuild=True (the fresh create's hierarchy) against a fresh solver"""
    name, P, builder = case
    with P.solver(builder) as a, P.solver(builder, dict(ml_diag=0)) as b:
        before = None if name in LONG else a.ml_level_array(0, "dg_val")
        for s in (a, b):
            s.refactor(P.other.nzval)
        if name not in LONG:
            assert_on_diagonals(a)
            assert not np.array_equal(before, a.ml_level_array(0, "dg_val"))           # the diagonals were refreshed
        assert_on_csr_wave(b)
        assert_same_cycle(a, b, P)
        assert_same_solve(a, b, P)
        a.refactor(P.other.nzval, rebuild=True)
        with P.solver(builder, values=P.other.nzval) as fresh:
            if name not in LONG:
                assert_on_diagonals(a)
                assert_on_diagonals(fresh)
            assert_same_cycle(a, fresh, P)
            assert_same_solve(a, fresh, P)


@pytest.mark.parametrize("nu", [1, 2, 3])
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_sweep_counts(builder, nu):
    """the parity of the buffer ping-pong: 2 nu - 1 fused half sweeps before the coarse correction, 2 nu after"""
    P = problem("24x20x12")
    with P.solver(builder, ml_smooth=nu) as a, P.solver(builder, dict(ml_diag=0), ml_smooth=nu) as b, P.solver(builder, TWO_KERNEL, ml_smooth=nu) as c:
        assert_on_csr_wave(b, assert_on_diagonals(a))
        assert_two_kernel(c)
        for other in (b, c):
            assert_same_cycle(a, other, P)
            assert_same_solve(a, other, P)


@pytest.mark.parametrize("tuning", [dict(ml_diag=8), dict(ml_f32=0)], ids=["cap8", "f64"])
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_fallback(builder, tuning):
    """a cap no column meets, and f64 level operators (no f32 copy to make diagonals of): the CSR kernel, silently, with the
    bits of the same tuning with ml_diag = 0"""
    P = problem("24x20x12")
    with P.solver(builder, tuning) as a, P.solver(builder, dict(tuning, ml_diag=0)) as b:
        assert_on_csr_wave(a)
        assert_on_csr_wave(b)
        assert_same_cycle(a, b, P)
        assert_same_solve(a, b, P)


def test_paths_cover():
    """over the cases above (this test runs behind them; on its own it builds what it needs): the new kernel with half
    bandwidth 1 and 2, and colours whose columns are no multiple of the 4 waves of a workgroup, every remainder"""
    if not _seen:
        for name in SHAPES:
            if name not in LONG:
                with problem(name).solver("device") as a:
                    assert_on_diagonals(a, name)
    print(sorted(set(_seen)))
    assert {1, 2} <= {P for _, _, P, _, _ in _seen}
    assert {1, 2, 3} <= {c % 4 for _, _, _, c0, c1 in _seen for c in (c0, c1)}
