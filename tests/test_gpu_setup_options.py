"""The hierarchy the setup KERNELS build (csrc/mlsetup.hip, the device branch of ml_setup in csrc/multilevel.hip) at every
option they honour and at every point where they hand over to the host planner (csrc/ml_plan.cpp).  tests/test_gpu_setup.py
pins the two to each other at the default knobs; here the cases of tests/ml_setup_cases.py, which tests/test_ml_plan.py pins
to the scipy restatement tests/ml_reference.py without a GPU.

  (a) device-built (ml_device_min = 0) against host-built (ml_device_min = -1): every array of every level and one
      preconditioner application, bit for bit; the knob cases with f32 and with f64 storage
  (b) the device-built cmap chain against the restatement's coarse cells and columns, and the rows against the case table
  (c) the device-built levels against the identities that define them (ml_structure_checks: the Galerkin bound
      m * 2^-52 * sum |terms| and the 4 * 2^-52 bound on the twin), f64 storage
  (d) every hand-over position: ml_device_min, ml_levels and ml_coarsest_rows around the rows of the default hierarchy
  (e) the options the kernels do not cover fall back to the host planner
  (f) an aggregation that stalls at once (one level) or after one step
  (g) five device builds in one process give the same bytes: the lock-free union-find, the atomic maxima on bit patterns
      and the atomic bucket fills leave no trace of the schedule
  (h) refactor on device-built hierarchies of four option cases
  (i) a Galerkin product with an exactly zero diagonal entry, which both builders must keep

Measured on an MI355X: the 122 tests of this file take 3.7 s together; the slowest is the first one (0.31 s, it starts the
device), every other one stays under 0.1 s.

That the tests can fail was checked on scratch builds with one decision changed each (new tests that then fail / tests of
test_gpu_setup.py, test_gpu_refactor.py, test_gpu_diag_windows.py and the hierarchy cases of test_gpu_cycle_options.py that do):
  agg_edges_kernel<1>, s < pocket for s <= pocket               60 of (a), (b), (d) / 9
  agg_stub_anchor_kernel, first instead of last tied entry      (a) and (b) of ties_none_seed3 / 2, the 100 x 116 x 60 grid
  aggregate, stub block skipped at tau > 0                      56 of (a), (b), (c), (d) / 9
  galerkin_accumulate_kernel, zero diagonals dropped            (i) / none
  ml_setup, l + 3 >= max_levels for l + 2                       (d) levels3 and levels5 / none
  geo_groups of the device path at a constant shift of 1        72 of (a), (b), (c), (d), (g), (h) / 8
"""
import types

import numpy as np
import pytest
import scipy.sparse as sp

import ml_cycle_reference as mcr
import ml_reference as mlr
import ml_setup_cases as msc
from ml_structure_checks import check_structure, check_twin, same_partition
from nk_ocn_tracer_jacobian_precond_amd import solver
from test_gpu_setup import ARRAYS as SETUP_ARRAYS

pytestmark = pytest.mark.gpu

ARRAYS = SETUP_ARRAYS + ("color_blk",)
HOST, DEVICE = -1, 0                             # ml_device_min: negative = the host planner builds every level


def make_solver(case, dev_min, tuning=None, coords=True, **options):
    c = msc.CASES[case]
    p, blk, ci, cj, col_t = msc.problem(case)
    t = dict(ml_coarsest_rows=msc.coarsest_rows(case), ml_device_min=dev_min, **msc.plan_knobs(case))
    t.update(tuning or {})                       # a hand-over case names its own ml_device_min / ml_coarsest_rows
    where = dict(col_i=ci, col_j=cj, col_t=col_t) if coords else {}
    return solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, coupled_tracer_cnt=c.cnt, precond=solver.PRECOND_MULTILEVEL, tuning=t, **where, **options)


def rhs(case):
    return np.random.default_rng(5).standard_normal(msc.problem(case)[0].flat_len)


class Built:
    """what a test needs of a solver after it is closed: every array of every level, one preconditioner application"""

    def __init__(self, s, r, cycle_levels=False):
        self.levels_on_device = s.get_int("ml_levels_on_device")
        self.arrays = [{a: s.ml_level_array(l, a) for a in ARRAYS} for l in range(s.get_int("levels"))]
        self.rows = [a["rowptr"].size - 1 for a in self.arrays]
        self.z = s.precond_apply(r)
        self.cycle_levels = mcr.levels_from_solver(s) if cycle_levels else None

    def ml_level_array(self, l, what):             # for check_structure, which reads the transfer maps of a solver
        return self.arrays[l][what]


def build(case, dev_min, tuning=None, coords=True, cycle_levels=False, **options):
    with make_solver(case, dev_min, tuning, coords, **options) as s:
        return Built(s, rhs(case), cycle_levels)


def assert_same_bytes(a, b, what=""):
    assert a.rows == b.rows, (what, a.rows, b.rows)
    for l, (x, y) in enumerate(zip(a.arrays, b.arrays)):
        for name in ARRAYS:
            assert x[name].shape == y[name].shape, (what, l, name, x[name].shape, y[name].shape)
            assert np.array_equal(x[name].view(np.uint8), y[name].view(np.uint8)), f"{what} level {l}: {name} differs"
    assert np.array_equal(a.z.view(np.uint8), b.z.view(np.uint8)), f"{what}: precond_apply differs"


@pytest.fixture(scope="module")
def built():
    """the hierarchies more than one test looks at, built once: (case, ml_device_min, ml_f32 or None = default)"""
    cache = {}

    def get(case, dev_min, f32=None):
        if (case, dev_min, f32) not in cache:
            cache[(case, dev_min, f32)] = build(case, dev_min, {} if f32 is None else dict(ml_f32=f32), cycle_levels=(dev_min == DEVICE and f32 == 0))
        return cache[(case, dev_min, f32)]
    return get


@pytest.fixture(scope="module")
def restated():
    cache = {}

    def get(case):
        if case not in cache:
            p, blk, ci, cj, _ = msc.problem(case)
            ri, rj, rk, colid, _ = msc.row_arrays(blk, ci, cj)
            cache[case] = mlr.build(p.scipy_csr(), ri, rj, rk, colid, **msc.restatement_knobs(case))
        return cache[case]
    return get


def levels_on_device(case):
    """With ml_device_min = 0 the kernels hand over only a level that is the last one, so they build every level but the last.
    The aggregation of "stall" coarsens nothing at level 0 (ncr >= n): nothing was finalised yet, the host gets level 0, none
    is device-built.  "near_stall" coarsens 383 -> 381 rows, so level 0 is finalised on the device; the aggregation of level 1
    then stalls and level 1 is handed over as the last: one device-built level of two."""
    return len(msc.CASES[case].rows) - 1


# ================================================================ (a) device against host, bit for bit
STORAGE_CASES = [(case, f32) for case in msc.names("knobs") for f32 in (0, 1)] + [(case, None) for case in msc.names() if msc.CASES[case].group != "knobs"]


@pytest.mark.parametrize("case,f32", STORAGE_CASES, ids=["%s-%s" % (c, {0: "f64", 1: "f32", None: "default"}[f]) for c, f in STORAGE_CASES])
def test_device_built_equals_host_built(case, f32, built):
    host, dev = built(case, HOST, f32), built(case, DEVICE, f32)
    print(case, "rows per level", dev.rows, "levels on the device", dev.levels_on_device)
    assert host.levels_on_device == 0
    assert dev.levels_on_device == levels_on_device(case)
    if msc.CASES[case].group != "stall":
        assert dev.levels_on_device >= 2
    assert host.rows == msc.CASES[case].rows
    assert_same_bytes(host, dev, case)
    assert np.isfinite(dev.z).all()


# ================================================================ (b) device against the restatement
@pytest.mark.parametrize("case", msc.names(single_tracer=True))
def test_device_built_cells_match_restatement(case, built, restated):
    f32 = 0 if msc.CASES[case].group == "knobs" else None
    dev, ref = built(case, DEVICE, f32), restated(case)
    assert dev.levels_on_device == levels_on_device(case)
    assert dev.rows == msc.CASES[case].rows == [lv.n for lv in ref]
    # level-0 row i of the device holds original row perm0[i]; further down the restatement's numbering follows the cells
    to_ref = dev.arrays[0]["perm0"].astype(np.int64)
    for l in range(len(ref) - 1):
        ref_of_fine = ref[l].cmap[to_ref]
        cmap = dev.arrays[l]["cmap"].astype(np.int64)
        assert same_partition(cmap, ref_of_fine), f"coarse cells differ on level {l}"
        nxt = np.empty(dev.rows[l + 1], np.int64)
        nxt[cmap] = ref_of_fine
        to_ref = nxt
        blk = dev.arrays[l + 1]["blk_start"].astype(np.int64)
        if blk.size:                                                 # a dense last level keeps no column blocks
            col_of = np.repeat(np.arange(blk.size - 1), np.diff(blk))
            assert same_partition(col_of, ref[l].coarse_colid[to_ref]), f"coarse columns differ on level {l + 1}"


# ================================================================ (c) device-built levels against their defining identities
@pytest.mark.parametrize("case", [n for n in msc.names() if n != "stall"])
def test_device_built_levels_are_galerkin_products_of_the_twin(case, built):
    dev = built(case, DEVICE, 0)
    assert dev.levels_on_device == levels_on_device(case) >= 1
    check_structure(dev.cycle_levels, dev)
    c = msc.CASES[case]
    if c.cnt == 1:
        check_twin(dev.cycle_levels[0], types.SimpleNamespace(p=msc.problem(case)[0]))


# ================================================================ (d) hand-over positions
# The default hierarchy has rows [2813, 889, 275, 100, 13] at ml_coarsest_rows = 60.  ml_setup enters the device path when
# n >= ml_device_min, more than one level is allowed and n > ml_coarsest_rows.  At level l it aggregates to ncr rows; level l + 1
# is the last one (next_last) if l + 2 >= ml_levels or ncr <= ml_coarsest_rows; level l is finalised on the device, and the host
# takes over from level l + 1 if that one is the last or has fewer than ml_device_min rows.  So the number of device-built levels
# is 1 + the number of leading coarse levels that are neither last nor smaller than ml_device_min.
#   (tuning, options, device-built levels, levels)
HAND_OVER = {
    "device_min0": (dict(ml_device_min=0), {}, 4, 5),            # handed over at 13 rows only because that level is the last
    "device_min14": (dict(ml_device_min=14), {}, 4, 5),          # 13 < 14, but that level is the last anyway; 100 >= 14
    "device_min101": (dict(ml_device_min=101), {}, 3, 5),        # 889, 275 >= 101 > 100: levels 0..2 on the device, 3 and 4 on the host
    "device_min276": (dict(ml_device_min=276), {}, 2, 5),        # 889 >= 276 > 275
    "device_min890": (dict(ml_device_min=890), {}, 1, 5),        # 2813 >= 890 > 889: level 0 alone
    "device_min2813": (dict(ml_device_min=2813), {}, 1, 5),      # n >= 2813 still enters the device path
    "device_min2814": (dict(ml_device_min=2814), {}, 0, 5),      # n < 2814: the host builds everything
    "levels1": (dict(ml_device_min=0), dict(ml_levels=1), 0, 1),     # a single level is never built on the device
    "levels2": (dict(ml_device_min=0), dict(ml_levels=2), 1, 2),     # l = 0: 0 + 2 >= 2, level 1 is the last
    "levels3": (dict(ml_device_min=0), dict(ml_levels=3), 2, 3),     # l = 1: 1 + 2 >= 3
    "levels5": (dict(ml_device_min=0), dict(ml_levels=5), 4, 5),     # l = 3: 3 + 2 >= 5 (and 13 <= 60): the limit and the size agree
    "coarsest2813": (dict(ml_device_min=0, ml_coarsest_rows=2813), {}, 0, 1),    # n <= 2813: one level, host
    "coarsest2812": (dict(ml_device_min=0, ml_coarsest_rows=2812), {}, 1, 2),    # n > 2812 >= 889
    "coarsest889": (dict(ml_device_min=0, ml_coarsest_rows=889), {}, 1, 2),      # 889 <= 889: level 1 is the last
    "coarsest888": (dict(ml_device_min=0, ml_coarsest_rows=888), {}, 2, 3),      # 889 > 888 >= 275
}


@pytest.fixture(scope="module")
def host_hand_over():
    """the host-built hierarchy under the ml_levels / ml_coarsest_rows of a hand-over case; most cases share one"""
    cache = {}

    def get(tuning, options):
        t = dict(tuning, ml_device_min=HOST)
        key = (tuple(sorted(t.items())), tuple(sorted(options.items())))
        if key not in cache:
            cache[key] = build("default", HOST, t, **options)
        return cache[key]
    return get


@pytest.mark.parametrize("name", list(HAND_OVER))
def test_hand_over_positions(name, host_hand_over):
    tuning, options, on_device, nlev = HAND_OVER[name]
    dev = build("default", DEVICE, tuning, **options)
    host = host_hand_over(tuning, options)
    assert host.levels_on_device == 0
    assert host.rows == msc.DEFAULT_ROWS[:nlev]
    assert (dev.levels_on_device, len(dev.rows)) == (on_device, nlev)
    assert_same_bytes(host, dev, name)


# ================================================================ (e) fallbacks
FALLBACKS = {
    "theta0.25": (dict(ml_theta=0.25), True),
    "split0": (dict(ml_split=0), True),
    "no_coordinates": (dict(), False),
    "spmv_compress": (dict(spmv_compress=1), True),
    "fused": (dict(ml_fused=1), True),
}


@pytest.mark.parametrize("name", list(FALLBACKS))
def test_options_the_kernels_do_not_cover_build_on_the_host(name):
    tuning, coords = FALLBACKS[name]
    host, dev = build("default", HOST, tuning, coords), build("default", DEVICE, tuning, coords)
    assert host.levels_on_device == 0 and dev.levels_on_device == 0
    assert len(dev.rows) >= 3
    assert_same_bytes(host, dev, name)


# ================================================================ (f) stall and near-stall
@pytest.mark.parametrize("case", msc.names("stall"))
def test_stalled_aggregation(case, built):
    host, dev = built(case, HOST), built(case, DEVICE)
    assert len(host.rows) == len(dev.rows) == len(msc.CASES[case].rows)
    assert dev.levels_on_device == levels_on_device(case)
    assert_same_bytes(host, dev, case)
    # the hierarchy (a single level for "stall") solves; both builds take the same steps
    b = np.random.default_rng(1).standard_normal(msc.problem(case)[0].flat_len)
    out = []
    for dev_min in (HOST, DEVICE):
        with make_solver(case, dev_min, rtol=1e-10) as s:
            x, info = s.solve(b)
            out.append((x, info))
    assert out[0][1]["relres"] <= 1e-10 and out[1][1]["relres"] <= 1e-10
    assert out[0][1]["iters"] == out[1][1]["iters"]
    assert np.array_equal(out[0][0], out[1][0])


# ================================================================ (g) scheduling independence
def test_device_build_does_not_depend_on_scheduling(built):
    case = "larger_40x46x20"
    first = built(case, DEVICE)
    assert first.levels_on_device == levels_on_device(case) >= 2
    for k in range(4):
        assert_same_bytes(first, build(case, DEVICE), "build %d" % (k + 2))


# ================================================================ (h) refactor on these hierarchies
@pytest.mark.parametrize("case", ["pocket0", "big_from1", "tracers3", "deep_12x10x75"])
def test_refactor_on_device_built_option_hierarchies(case):
    """The day_cnt = 180 values have the pattern of the case's own and, in the restatement under the case's knobs, the same
    coarse cells on every level: the refactor keeps its cells (no rebuild) and must give the bits of a fresh device build."""
    p = msc.problem(case)[0]
    p2 = msc.problem(case, day_cnt=180.0)[0]
    assert np.array_equal(p.rowptr, p2.rowptr) and np.array_equal(p.colind, p2.colind) and not np.array_equal(p.nzval, p2.nzval)
    r = rhs(case)
    with make_solver(case, DEVICE) as s:
        assert s.get_int("ml_levels_on_device") == levels_on_device(case)
        z1 = s.precond_apply(r)
        s.refactor(p2.nzval)
        rebuilt = s.get_int("refactor_rebuilt")
        z2 = s.precond_apply(r)
    c = msc.CASES[case]
    _, blk, ci, cj, col_t = msc.problem(case)
    t = dict(ml_coarsest_rows=msc.coarsest_rows(case), ml_device_min=DEVICE, **msc.plan_knobs(case))
    with solver.NkpSolver(p.rowptr, p.colind, p2.nzval, blk, coupled_tracer_cnt=c.cnt, col_i=ci, col_j=cj, col_t=col_t, precond=solver.PRECOND_MULTILEVEL,
                          tuning=t) as fresh:
        assert fresh.get_int("ml_levels_on_device") == levels_on_device(case)
        z3 = fresh.precond_apply(r)
    print(case, "refactor rebuilt the hierarchy:", rebuilt)
    assert rebuilt == 0
    assert not np.array_equal(z1, z2)
    assert np.array_equal(z2.view(np.uint8), z3.view(np.uint8))


# ================================================================ (i) an exactly zero Galerkin diagonal
def zero_diagonal_problem():
    """8 x 6 water columns of 3 cells with small integer entries (every sum is exact, whatever its order): diagonal -10,
    couplings +1 to the cells above, below and beside.  The four surface cells of the group at i, j in 2..3 have diagonal -2:
    their coarse cell gets 4 * (-2) + 8 * 1 = 0 on the diagonal.  No entry is negative off the diagonal, so the twin is A."""
    ni, nj, nk = 8, 6, 3
    row = lambda i, j, k: (j * ni + i) * nk + k
    n = ni * nj * nk
    A = np.zeros((n, n))
    for j in range(nj):
        for i in range(ni):
            for k in range(nk):
                r = row(i, j, k)
                A[r, r] = -2.0 if (k == 0 and i in (2, 3) and j in (2, 3)) else -10.0
                for di, dj, dk in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
                    i2, j2, k2 = i + di, j + dj, k + dk
                    if 0 <= i2 < ni and 0 <= j2 < nj and 0 <= k2 < nk:
                        A[r, row(i2, j2, k2)] = 1.0
    A = sp.csr_matrix(A)
    A.sort_indices()
    blk = np.arange(0, n + 1, nk, dtype=np.int32)
    ci = np.tile(np.arange(ni, dtype=np.int32), nj)
    cj = np.repeat(np.arange(nj, dtype=np.int32), ni)
    return A, blk, ci, cj


def test_zero_galerkin_diagonal_is_kept():
    A, blk, ci, cj = zero_diagonal_problem()
    r = np.random.default_rng(5).standard_normal(A.shape[0])
    out = {}
    for dev_min in (HOST, DEVICE):
        with solver.NkpSolver(A.indptr, A.indices, A.data, blk, col_i=ci, col_j=cj, precond=solver.PRECOND_MULTILEVEL, ml_levels=2,
                              tuning=dict(ml_coarsest_rows=60, ml_device_min=dev_min, ml_f32=0)) as s:
            out[dev_min] = Built(s, r)
    host, dev = out[HOST], out[DEVICE]
    assert host.levels_on_device == 0 and dev.levels_on_device == 1
    assert host.rows == [144, 36]
    # the case means something: exactly one stored diagonal entry of the coarse operator is zero
    last = host.arrays[1]
    rows_of = np.repeat(np.arange(36), np.diff(last["rowptr"]))
    on_diagonal = last["colind"] == rows_of
    assert on_diagonal.sum() == 36 and (last["val"][on_diagonal] == 0.0).sum() == 1
    assert_same_bytes(host, dev, "zero diagonal")
    assert np.isfinite(dev.z).all()
