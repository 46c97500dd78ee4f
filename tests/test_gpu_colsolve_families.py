"""Every water-column band-solve kernel at wide bands, long columns and batched, against references that are not kernels.

The matrices, the kernel families (one nkp_tuning dict per kernel), the restated selection rule (expected_kernel) and the case
lists are data in tests/colsolve_cases.py; tests/test_colsolve_cases.py checks their claims without a GPU, among them that the
lists below reach every instantiation a launcher can select; tests/test_col_plan.py holds expected_kernel against the
library's own rule (col_plan, csrc/col_plan.cpp) on the CPU.  Which kernel ran is read back (nkp_ml_level_array "col_kernel",
nkp_get_int "col_*") and compared with expected_kernel on every level, so that a knob combination that silently selects the
default kernel fails here, and every designed fallback (wave with dropped bands, packed at 81 rows or with f64 storage, stream
at 65 rows, the pipelined kernel at P = 4, gs_fused without room in LDS) is asserted as one.

  (a) column-Jacobi against the oracle's band LU and band solve, bit for bit (same operation order, no contraction on either
      side), bands 1, 2, 3, 4 and 6 (dropped), columns of 10 .. 128 rows, under the lanes, stream and LDS-resident layouts
  (b) the multilevel cycle under every family: all families give the bits of the lanes8 family, and that one is within the bound
      of mcr.Reference of the cycle restated in tests/ml_cycle_reference.py on the levels read back from the device.  On a
      level that reports dropped entries the restated half sweep solves the band-capped block (|row - col| <= 4)
  (c) solve_many against solve, column by column and bit for bit, through the packed two- and four-system kernels, the
      wave-per-column batch kernel and the fused batch kernel
  (d) nkp_refactor on the layouts tests/test_gpu_refactor.py never has (sorted and unsorted packed, LDS-resident, streamed; the
      column-Jacobi preconditioner with LDS-resident columns) against a fresh create of the new values, bit for bit.  The new
      values are cc.refactor_values: with the diagonal grown by 50 % the planner picks other coarse cells on these shapes

Tolerances of (b) are those of tests/test_gpu_cycle_options.py, formulas unchanged, from the reference alone on the levels at
hand: f64 storage max (1e-12, 4096 d), d = restated cycle with LU blocks against explicit inverses; f32 storage
min (2e-5, 16 e), e = what f32 rounding of the block factors and of the last level's inverse changes in the restated cycle.
No tolerance was fitted to the device's output.

Found by (b): gs_fused_kernel on the streamed and the LDS-resident layouts (32 columns per group) gave results unrelated to the
other families.  The kernel stages the group's factors in LDS under every layout, but the setup sized its dynamic LDS from the
lane kernel's need, which has no factor area on those two layouts: the factors went past the end of the allocation.  Fixed in
the layout rule, now col_plan of csrc/col_plan.cpp (gs_lds_bytes counts the factors, and gs_ok falls when they do not fit 64 KB).

Measured on an MI355X: ||z - z_ref|| / ||z_ref|| of the lanes8 family, its bound and their ratio, and the measured in-column
half bandwidth of every level with column blocks (level 0 first; 6 = entries beyond the band dropped, on every level of those
hierarchies).  Nothing of this had been measured before:
  12x10 band 2 km 60     f64  1.6e-14  bound 3.8e-11  ratio 0.00042  bands [2, 2, 2, 2, 2]
  12x10 band 2 km 60     f32  4.8e-06  bound 2.0e-05  ratio 0.24  bands [2, 2, 2, 2, 2]
  12x10 band 2 km 80     f64  2.6e-15  bound 8.4e-12  ratio 0.00031  bands [2, 2, 2, 2, 2]
  12x10 band 2 km 80     f32  5.6e-08  bound 1.1e-06  ratio 0.051  bands [2, 2, 2, 2, 2]
  12x10 band 2 km 128    f64  1.4e-14  bound 1.6e-11  ratio 0.00088  bands [2, 2, 2, 2, 2, 2, 2]
  12x10 band 2 km 128    f32  8.6e-08  bound 4.9e-07  ratio 0.18  bands [2, 2, 2, 2, 2, 2, 2]
  12x10 band 4 km 60     f64  3.3e-16  bound 1.0e-12  ratio 0.00033  bands [4, 4, 4, 4, 4]
  12x10 band 4 km 60     f32  1.6e-09  bound 4.0e-08  ratio 0.04  bands [4, 4, 4, 4, 4]
  12x10 band 4 km 80     f64  5.9e-16  bound 1.3e-12  ratio 0.00047  bands [4, 4, 4, 4, 4]
  12x10 band 4 km 80     f32  1.9e-09  bound 2.6e-08  ratio 0.071  bands [4, 4, 4, 4, 4]
  12x10 band 4 km 128    f64  4.2e-16  bound 1.6e-12  ratio 0.00026  bands [4, 4, 4, 4, 4, 4, 4]
  12x10 band 4 km 128    f32  2.9e-09  bound 3.2e-08  ratio 0.092  bands [4, 4, 4, 4, 4, 4, 4]
  12x10 band 6 km 60     f64  1.9e-16  bound 1.0e-12  ratio 0.00019  bands [6, 6, 6, 6, 6]
  12x10 band 6 km 60     f32  2.0e-09  bound 2.7e-08  ratio 0.074  bands [6, 6, 6, 6, 6]
  12x10 band 6 km 80     f64  2.0e-16  bound 1.2e-12  ratio 0.00016  bands [6, 6, 6, 6, 6]
  12x10 band 6 km 80     f32  4.0e-09  bound 4.3e-08  ratio 0.093  bands [6, 6, 6, 6, 6]
  12x10 band 6 km 128    f64  5.5e-16  bound 1.5e-12  ratio 0.00037  bands [6, 6, 6, 6, 6, 6, 6]
  12x10 band 6 km 128    f32  1.6e-09  bound 2.5e-08  ratio 0.062  bands [6, 6, 6, 6, 6, 6, 6]
  12x10 band 1 km 10     f64  4.1e-16  bound 2.0e-12  ratio 0.00021  bands [1, 1, 1]
  12x10 band 1 km 10     f32  1.1e-07  bound 1.2e-06  ratio 0.092  bands [1, 1, 1]
  12x10 band 1 km 96     f64  4.3e-15  bound 2.5e-11  ratio 0.00017  bands [1, 1, 1, 1, 1, 1]
  12x10 band 1 km 96     f32  1.1e-06  bound 1.3e-05  ratio 0.081  bands [1, 1, 1, 1, 1, 1]
  12x10 band 3 km 10     f64  2.1e-16  bound 1.2e-12  ratio 0.00018  bands [3, 3, 3]
  12x10 band 3 km 10     f32  7.1e-10  bound 1.2e-08  ratio 0.061  bands [3, 3, 3]
  12x10 band 3 km 96     f64  5.0e-16  bound 1.4e-12  ratio 0.00036  bands [3, 3, 3, 3, 3]
  12x10 band 3 km 96     f32  3.0e-09  bound 6.4e-08  ratio 0.047  bands [3, 3, 3, 3, 3]
  8x8 band 4 km 60       f64  6.1e-16  bound 1.8e-12  ratio 0.00034  bands [4, 4, 4]
  8x8 band 4 km 60       f32  1.4e-09  bound 1.7e-08  ratio 0.086  bands [4, 4, 4]
  8x8 band 4 km 128      f64  5.5e-16  bound 1.4e-12  ratio 0.0004  bands [4, 4, 4]
  8x8 band 4 km 128      f32  1.1e-09  bound 1.8e-08  ratio 0.064  bands [4, 4, 4]
  12x10 band 1 km 80     f64  4.7e-15  bound 1.8e-11  ratio 0.00027  bands [1, 1, 1, 1, 1]
  12x10 band 1 km 80     f32  1.3e-07  bound 2.3e-06  ratio 0.059  bands [1, 1, 1, 1, 1]
"""
import numpy as np
import pytest

import colsolve_cases as cc
import ml_cycle_reference as mcr
import oracle_binding as ora
from nk_ocn_tracer_jacobian_precond_amd import solver

pytestmark = pytest.mark.gpu

FIELDS = cc.COL_KERNEL_FIELDS


def grid_id(grid):
    return "%dx%d" % grid[:2]


class Case:
    """One matrix with its column blocks, column coordinates and fixed vectors."""

    def __init__(self, grid, band, km):
        self.p = p = cc.problem(grid, km, band)
        self.blk = cc.column_blocks(p)
        ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
        self.coords = dict(col_i=ci, col_j=cj)
        self.r = np.random.default_rng(17).standard_normal(p.flat_len)
        self.B = np.random.default_rng(11).standard_normal((8, p.flat_len))
        self.B[2] *= 1e-3

    def multilevel(self, tuning, val=None, **more):
        p = self.p
        return solver.NkpSolver(p.rowptr, p.colind, p.nzval if val is None else val, self.blk, precond=solver.PRECOND_MULTILEVEL,
                                tuning=tuning, **dict(dict(restart=4, **self.coords), **more))

    def jacobi(self, tuning, val=None, **more):
        p = self.p
        return solver.NkpSolver(p.rowptr, p.colind, p.nzval if val is None else val, self.blk, precond=solver.PRECOND_COLUMN_JACOBI,
                                tuning=tuning, **dict(dict(restart=4), **more))


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(grid, band, km):
        if (grid, band, km) not in cache:
            cache[(grid, band, km)] = Case(grid, band, km)
        return cache[(grid, band, km)]
    return get


def level_shapes(s):
    """Per level with column blocks: (col_kernel as a dict, column lengths per colour in layout order)."""
    out = []
    for l in range(s.get_int("levels")):
        ck = s.ml_level_array(l, "col_kernel")
        blk = s.ml_level_array(l, "blk_start").astype(np.int64)
        if not blk.size:
            assert ck.size == 0
            out.append(None)
            continue
        assert ck.dtype == np.int32 and ck.size == len(FIELDS)
        cb = s.ml_level_array(l, "color_blk")
        lens = np.diff(blk)
        out.append((dict(zip(FIELDS, (int(v) for v in ck))), [lens[cb[0]:cb[1]], lens[cb[1]:cb[2]]]))
    return out


def assert_selection(s, family, f32, shapes, label):
    """Every level's col_kernel equals the restated selection rule on that level's (P, dropped, max_len, columns)."""
    got_kernels = set()
    for l, (shape, got) in enumerate(zip(shapes, level_shapes(s))):
        assert (shape is None) == (got is None), (label, family, l)
        if shape is None:
            continue
        ck0, lens = shape
        ck = got[0]
        want = cc.expected_kernel(family, f32, ck0["P"], ck0["dropped"], ck0["max_len"], sum(x.size for x in lens), lens)
        diff = {f: (ck[f], want[f]) for f in FIELDS if ck[f] != want[f]}
        assert not diff, (label, family, "level", l, diff)
        if l < len(shapes) - 1:
            got_kernels |= want["kernels"]
    return got_kernels


# ================================================================ (a) column-Jacobi against the oracle
@pytest.mark.parametrize("grid,band,km", cc.CASES_JACOBI, ids=["%s_band%d_km%d" % (grid_id(g), b, k) for g, b, k in cc.CASES_JACOBI])
def test_column_jacobi_is_the_oracle_bit_for_bit(grid, band, km, cases):
    c = cases(grid, band, km)
    p, blk = c.p, c.blk
    n = p.flat_len
    bw, _, max_len = ora.colblock_measure(p.rowptr, p.colind, p.nzval, blk)
    assert bw == band
    P = cc.stored_band(bw)
    fac, dropped = ora.colblock_factor(p.rowptr, p.colind, p.nzval, blk, P)
    assert dropped == int(band > cc.MAX_BAND)
    want_z = ora.colblock_apply(n, blk, P, fac, c.r)
    lens = [np.diff(blk.astype(np.int64))]
    seen = set()
    for layout in cc.JACOBI_LAYOUTS:
        e = cc.expected_kernel(layout, 0, P, dropped, max_len, blk.size - 1, lens, multilevel=False)
        with c.jacobi(cc.FAMILIES[layout]) as s:
            assert s.get_int("band") == P and s.get_int("band_dropped") == dropped and s.get_int("nblk") == blk.size - 1
            got = dict(stream=s.get_int("col_stream"), ldsres=s.get_int("col_ldsres"), gw=s.get_int("col_gw"), max_len=s.get_int("col_max_len"),
                       lds_doubles=s.get_int("col_lds_bytes") // 8)
            assert got == {f: e[f] for f in got}, (layout, got, {f: e[f] for f in got})
            z = s.precond_apply(c.r)
        assert np.array_equal(z, want_z), (layout, e["kernels"], np.abs(z - want_z).max())
        seen |= e["kernels"]
    if max_len <= 64:
        assert {k[0] for k in seen} == {"lanes", "stream", "ldsres"}, seen
    else:
        assert {k[0] for k in seen} == {"lanes", "ldsres"}, seen             # stream falls back to the lanes kernel beyond 64 rows


# ================================================================ (b) the cycle under every family
_f64_levels = {}


def f64_levels(c, key, source):
    if key not in _f64_levels:
        with c.multilevel(dict(cc.FAMILIES[source], ml_f32=0)) as s:
            _f64_levels[key] = mcr.levels_from_solver(s)
    return _f64_levels[key]


@pytest.mark.parametrize("grid,band,km,f32", cc.CASES_CYCLE,
                         ids=["%s_band%d_km%d_%s" % (grid_id(g), b, k, "f32" if f else "f64") for g, b, k, f in cc.CASES_CYCLE])
def test_every_family_runs_the_restated_cycle(grid, band, km, f32, cases):
    c = cases(grid, band, km)
    label = "%s band %d km %d" % (grid_id(grid), band, km)
    source = "wave2" if band <= cc.MAX_BAND else "lanes8"
    with c.multilevel(dict(cc.FAMILIES[source], ml_f32=f32)) as s:
        levels = mcr.levels_from_solver(s)
        shapes = level_shapes(s)
    nlev = len(levels)
    assert nlev >= 3 and shapes[0] is not None
    # what the tail family relies on: all levels fit ml_tail_rows = 16000 and the last one is solved densely
    assert nlev <= 8 and sum(lv.n for lv in levels) <= 16000 and levels[-1].coarse_inv is not None
    bands = []
    for l, (lv, shape) in enumerate(zip(levels, shapes)):
        if lv.col_of is None:
            continue
        ck = shape[0]
        bands.append(lv.band)
        assert ck["P"] == cc.stored_band(min(lv.band, cc.MAX_BAND)) and ck["dropped"] == int(lv.band > cc.MAX_BAND), (l, lv.band, ck)
        assert ck["max_len"] == int(np.diff(lv.blk_start).max()), (l, ck)
    assert bands[0] == band                                    # the twin keeps the matrix's in-column band
    if f32:
        levels = mcr.with_exact_blocks(levels, f64_levels(c, (grid, band, km), source))
    ref = mcr.Reference(levels, c.r, f32, {"default": {}})

    z, kernels = {}, set()
    for family, tuning in cc.FAMILIES.items():
        with c.multilevel(dict(tuning, ml_f32=f32)) as s:
            assert [s.ml_level_array(l, "rowptr").size - 1 for l in range(s.get_int("levels"))] == ref.rows, family
            kernels |= assert_selection(s, family, f32, shapes, label)
            z[family] = s.precond_apply(c.r)
    anchor = z[cc.ANCHOR]
    assert np.isfinite(anchor).all() and np.linalg.norm(anchor) > 0
    err, bound = mcr.relative_difference(anchor, ref.z["default"]), ref.bound("default")
    print("MEASURED %-22s %s  %.1e  bound %.1e  ratio %.2g  bands %s" % (label, "f32" if f32 else "f64", err, bound, err / bound, bands))
    for family in cc.FAMILIES:
        assert np.array_equal(anchor, z[family]), (label, f32, family, np.abs(anchor - z[family]).max())
    assert err <= bound, (label, f32, err, bound, ref.yard, bands)
    # the families did not collapse onto one kernel: whatever the level, these three are selected by some family
    assert {"lanes", "ldsres", "tail"} <= {k[0] for k in kernels}, kernels


# ================================================================ (c) batched solves
BATCH_OPTIONS = dict(max_iters=6, rtol=1e-30)


def batch_against_single(make, tuning, B, expect_status=True):
    """solve_many of every width against solve, column by column: solution, iteration count and residual, bit for bit."""
    with make(tuning, **BATCH_OPTIONS) as s:
        single = [s.solve(B[k], raise_on_fail=False) for k in range(B.shape[0])]
    assert all(np.isfinite(x).all() and i["iters"] == 6 for x, i in single), [i for _, i in single]
    if expect_status:
        assert all(i["status"] == solver.NKP_NOT_CONVERGED for _, i in single), [i for _, i in single]
    for rhs_batch in sorted({rb for _, rb in cc.BATCH_WIDTHS}):
        with make(dict(tuning, rhs_batch=rhs_batch), **BATCH_OPTIONS) as s:
            for width in [w for w, rb in cc.BATCH_WIDTHS if rb == rhs_batch]:
                before = s.get_int("batch_steps")
                X, infos = s.solve_many(B[:width], raise_on_fail=False)
                assert s.get_int("batch_steps") > before, (width, "the call fell back to one solve at a time")
                assert s.get_int("batch_width") == cc.batch_groups(width, rhs_batch)[-1], (width, s.get_int("batch_width"))
                for k in range(width):
                    x1, i1 = single[k]
                    assert infos[k]["iters"] == i1["iters"] and infos[k]["relres"] == i1["relres"], (width, k, infos[k], i1)
                    assert np.array_equal(X[k], x1), (width, k, np.abs(X[k] - x1).max())


@pytest.mark.parametrize("grid,band,km,f32", cc.CASES_BATCH,
                         ids=["%s_band%d_km%d_%s" % (grid_id(g), b, k, "f32" if f else "f64") for g, b, k, f in cc.CASES_BATCH])
def test_batched_solves_have_the_bits_of_single_solves(grid, band, km, f32, cases):
    c = cases(grid, band, km)
    label = "%s band %d km %d" % (grid_id(grid), band, km)
    with c.multilevel(dict(cc.FAMILIES[cc.ANCHOR], ml_f32=f32)) as s:
        shapes = level_shapes(s)
    batch_kernels = set()
    for family in cc.BATCH_FAMILIES:
        tuning = dict(cc.FAMILIES[family], ml_f32=f32)
        with c.multilevel(tuning) as s:
            assert_selection(s, family, f32, shapes, label)
        for shape in shapes[:-1]:
            ck0, lens = shape
            e = cc.expected_kernel(family, f32, ck0["P"], ck0["dropped"], ck0["max_len"], sum(x.size for x in lens), lens)
            for K in (2, 4, 8):
                batch_kernels |= e["batch"](K)
        batch_against_single(c.multilevel, tuning, c.B)
    names = {k[0] for k in batch_kernels}
    assert "wave_batch" in names
    if f32 and shapes[0][0]["max_len"] <= 80:
        assert {"ldspack2", "ldspack4"} <= names, names
    if band <= cc.MAX_BAND:
        assert "gs_wave_batch" in names, names


@pytest.mark.parametrize("grid,band,km", cc.CASES_BATCH_JACOBI, ids=["%s_band%d_km%d" % (grid_id(g), b, k) for g, b, k in cc.CASES_BATCH_JACOBI])
def test_batched_column_jacobi_has_the_bits_of_single_solves(grid, band, km, cases):
    c = cases(grid, band, km)
    for layout in ("lanes8", "ldsres"):
        batch_against_single(c.jacobi, cc.FAMILIES[layout], c.B, expect_status=False)


# ================================================================ (d) refactor on the sorted packed and the other layouts
def assert_refactored_equals_fresh(c, make, tuning, new_val, multilevel):
    opts = dict(max_iters=6, rtol=1e-30)
    with make(tuning, **opts) as s, make(tuning, val=new_val, **opts) as t:
        s.solve_many(c.B[:4], raise_on_fail=False)                    # batch vectors exist before the refactor
        s.refactor(new_val)
        assert s.get_int("refactor_rebuilt") == 0 and s.get_int("refactor_count") == 1
        if multilevel:
            assert s.get_int("levels") == t.get_int("levels")
            for l in range(t.get_int("levels") - 1):
                assert np.array_equal(s.ml_level_array(l, "cmap"), t.ml_level_array(l, "cmap")), l
            for l in range(t.get_int("levels")):
                assert np.array_equal(s.ml_level_array(l, "col_kernel"), t.ml_level_array(l, "col_kernel")), l
                assert np.array_equal(s.ml_level_array(l, "fac"), t.ml_level_array(l, "fac")), l
        zs, zt = s.precond_apply(c.r), t.precond_apply(c.r)
        assert np.isfinite(zt).all() and np.array_equal(zs, zt), np.abs(zs - zt).max()
        Xs, infos_s = s.solve_many(c.B[:4], raise_on_fail=False)
        Xt, infos_t = t.solve_many(c.B[:4], raise_on_fail=False)
        assert s.get_int("batch_width") == 4 == t.get_int("batch_width")
        assert np.array_equal(Xs, Xt) and [i["relres"] for i in infos_s] == [i["relres"] for i in infos_t]
        return zt


@pytest.mark.parametrize("f32", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("grid,band,km", cc.CASES_REFACTOR, ids=["%s_band%d_km%d" % (grid_id(g), b, k) for g, b, k in cc.CASES_REFACTOR])
def test_refactor_on_every_layout_equals_a_fresh_create(grid, band, km, f32, cases):
    c = cases(grid, band, km)
    new_val = cc.refactor_values(c.p)
    assert new_val.size == c.p.nzval.size and not np.array_equal(new_val, c.p.nzval)
    with c.multilevel(dict(cc.FAMILIES[cc.ANCHOR], ml_f32=f32)) as s:
        shapes = level_shapes(s)
        z_old = s.precond_apply(c.r)
    z = {}
    for family in cc.REFACTOR_FAMILIES:
        tuning = dict(cc.FAMILIES[family], ml_f32=f32)
        with c.multilevel(tuning) as s:
            assert_selection(s, family, f32, shapes, "refactor")
        z[family] = assert_refactored_equals_fresh(c, c.multilevel, tuning, new_val, True)
        assert not np.array_equal(z[family], z_old)                   # the new values are in use
    for family in cc.REFACTOR_FAMILIES[1:]:
        assert np.array_equal(z[cc.REFACTOR_FAMILIES[0]], z[family]), family


@pytest.mark.parametrize("grid,band,km", cc.CASES_REFACTOR, ids=["%s_band%d_km%d" % (grid_id(g), b, k) for g, b, k in cc.CASES_REFACTOR])
def test_refactor_of_column_jacobi_with_resident_columns(grid, band, km, cases):
    c = cases(grid, band, km)
    p, blk = c.p, c.blk
    new_val = cc.refactor_values(p)
    with c.jacobi(cc.FAMILIES["ldsres"]) as s:
        assert s.get_int("col_ldsres") == 1 and s.get_int("col_gw") == 32
    z = assert_refactored_equals_fresh(c, c.jacobi, cc.FAMILIES["ldsres"], new_val, False)
    fac, _ = ora.colblock_factor(p.rowptr, p.colind, new_val, blk, 4)
    assert np.array_equal(z, ora.colblock_apply(p.flat_len, blk, 4, fac, c.r))
