"""Level operators as per-column diagonals (tuning ml_diag, csrc/diagop.hip): the layout against the CSR arrays it was made
from, and the bits of everything that runs on it against the same solver with ml_diag = 0.

The diagonals serve the residual rows of the two-kernel half sweeps and the residual before the restriction, so every case
runs with col_wave_max = 0 and ml_wave_fused = 0 (small levels then take that path) and a small ml_coarsest_rows (several
levels), once with the levels built on the host (ml_device_min = -1) and once by the setup kernels (ml_device_min = 0).

Shapes: 12x10x6 and 24x20x12 (short columns), 40x36x24 (coarse levels with columns of one row and columns that start below
the surface), 10x8x70 (columns longer than a wave: two tiles per column; its solves take thousands of iterations and are cut
at 150, which compares the same bits in a tenth of the time) and two coupled tracers.  All are upwind3 + isop
except 12x10x6, which has lateral mixing without the isopycnal tensor: with it the columns of that grid, at most 6 rows
between neighbours of other depths, pad their diagonals to 1.51 .. 1.60 times the entries (seeds 0 .. 7, worked out on the
host from the low-order twin), which is over the 1.5 a level may have, and the case would test nothing; without it 1.35,
with 10 keys at most, so the cap of 8 of test_fallback still refuses it.

Every comparison is np.array_equal: the kernel sums a row's products in ascending column order, the order of the CSR
kernels, and a padded position adds 0.0f * x = +-0 to a sum that is never -0.
"""
import ctypes

import numpy as np
import pytest

from nk_ocn_tracer_jacobian_precond_amd import solver, synth

pytestmark = pytest.mark.gpu

SHAPES = {
    "12x10x6": (dict(imt=12, jmt=10, km=6, seed=2, hmix="const"), 1, 200),
    "24x20x12": (dict(imt=24, jmt=20, km=12, seed=2), 1, 200),
    "40x36x24": (dict(imt=40, jmt=36, km=24, seed=4), 1, 300),
    "10x8x70": (dict(imt=10, jmt=8, km=70, seed=5), 1, 200, dict(max_iters=150)),
    "tracers2": (dict(imt=24, jmt=20, km=12, seed=3, coupled_tracer_cnt=2), 2, 200),
}
BUILDERS = {"host": -1, "device": 0}
DG = ("dg_ptr", "dg_key", "dg_voff", "dg_val")


class Problem:
    def __init__(self, name):
        kw, self.cnt, self.coarsest = SHAPES[name][:3]
        self.options = SHAPES[name][3] if len(SHAPES[name]) > 3 else {}
        kw = dict(dict(adv="upwind3", hmix="isop"), **kw)
        self.p = p = synth.generate(**kw)
        self.other = synth.generate(**dict(kw, day_cnt=180.0))          # other values on the same pattern
        assert np.array_equal(p.rowptr, self.other.rowptr) and np.array_equal(p.colind, self.other.colind)
        assert not np.array_equal(p.nzval, self.other.nzval)
        self.blk = solver.column_blocks(p.col_start(), p.tracer_state_len, self.cnt)
        ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), self.cnt)
        self.coords = dict(col_i=ci, col_j=cj)
        self.n = p.flat_len

    def solver(self, builder, ml_diag, **more):
        p = self.p
        tuning = dict(col_wave_max=0, ml_wave_fused=0, ml_coarsest_rows=self.coarsest, ml_device_min=BUILDERS[builder], ml_diag=ml_diag)
        return solver.NkpSolver(p.rowptr, p.colind, p.nzval, self.blk, coupled_tracer_cnt=self.cnt, precond=solver.PRECOND_MULTILEVEL,
                                tuning=tuning, **dict(dict(rtol=1e-10, restart=60, **self.coords), **self.options, **more))

    def rhs(self, k=0):
        return np.random.default_rng(31 + k).standard_normal(self.n)


_problems = {}


@pytest.fixture(params=[(s, b) for s in SHAPES for b in BUILDERS], ids=lambda sb: f"{sb[0]}-{sb[1]}")
def case(request):
    name, builder = request.param
    if name not in _problems:
        _problems[name] = Problem(name)
    return _problems[name], builder


def diag_levels(s):
    return [l for l in range(s.get_int("levels")) if s.ml_level_array(l, "dg_val").size]


def check_layout(s, l):
    """The diagonals of level l hold the level's CSR entries, entry for entry, and exact zeros everywhere else."""
    rowptr, colind, valf, blk = (s.ml_level_array(l, a) for a in ("rowptr", "colind", "valf", "blk_start"))
    ptr, key, voff, val = (s.ml_level_array(l, a) for a in DG)
    n, ncol = rowptr.size - 1, blk.size - 1
    assert ptr.size == ncol + 1 and voff.size == ncol and key.size == ptr[-1] and ptr[0] == 0 and np.all(np.diff(ptr) >= 0)
    length = np.diff(blk).astype(np.int64)
    nk = np.diff(ptr).astype(np.int64)
    assert np.array_equal(voff, np.concatenate(([0], np.cumsum(nk * length)[:-1]))) and val.size == int(np.sum(nk * length))
    # keys strictly ascending inside every column: (column, key) ascending as one number
    span = 2 * n + 1
    ckey = np.repeat(np.arange(ncol, dtype=np.int64), nk) * span + (key.astype(np.int64) + n)
    assert np.all(np.diff(ckey) > 0)
    # every entry's slot
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    col = np.repeat(np.arange(ncol, dtype=np.int64), length)[row]
    kl = row - blk[col]
    want = col * span + (colind.astype(np.int64) - kl + n)
    pos = np.searchsorted(ckey, want)
    assert np.all(pos < ckey.size) and np.array_equal(ckey[np.minimum(pos, ckey.size - 1)], want)      # the entry's key is in its column's list
    assert np.unique(pos).size == key.size                                                            # and no key is idle
    same_row = np.diff(row) == 0
    assert np.all(np.diff(pos)[same_row] > 0)                                                         # slot order = stored order
    idx = voff[col] + (pos - ptr[col]) * length[col] + kl
    assert np.unique(idx).size == idx.size
    expect = np.zeros(val.size, np.float32)
    expect[idx] = valf
    assert np.array_equal(expect.view(np.uint32), val.view(np.uint32))                                # values, and +0.0 in every padded position
    return int(nk.max())


def one_colour_zeroed(s, r):
    """r with the rows of colour 0 (level-0 rows [0, rows0) in colour-major order) zeroed"""
    perm0, blk, cb = s.ml_level_array(0, "perm0"), s.ml_level_array(0, "blk_start"), s.ml_level_array(0, "color_blk")
    out = r.copy()
    out[perm0[:blk[cb[1]]]] = 0.0
    return out


def assert_same_cycle(a, b, P):
    for r in (P.rhs(), one_colour_zeroed(a, P.rhs(1))):
        za, zb = a.precond_apply(r), b.precond_apply(r)
        assert np.all(np.isfinite(za)) and np.array_equal(za, zb)


def assert_same_solve(a, b, P):
    xa, ia = a.solve(P.rhs(2), raise_on_fail=False)
    xb, ib = b.solve(P.rhs(2), raise_on_fail=False)
    assert np.array_equal(xa, xb) and all(ia[k] == ib[k] for k in ("status", "iters", "relres")) and ia["iters"] > 0


def test_layout(case):
    P, builder = case
    with P.solver(builder, 32) as s:
        levels = diag_levels(s)
        assert levels, "no level has the diagonals: nothing would be tested"
        most = max(check_layout(s, l) for l in levels)
        print(f"levels {s.get_int('levels')}, with diagonals {levels}, most keys in a column {most}")
        assert most <= 32
        # the last level has no f32 operator and stays on CSR
        assert s.get_int("levels") - 1 not in levels


def test_cycle_and_solve(case):
    P, builder = case
    with P.solver(builder, 32) as a, P.solver(builder, 0) as b:
        assert diag_levels(a) and not diag_levels(b)
        assert_same_cycle(a, b, P)
        assert_same_solve(a, b, P)


def test_refresh(case):
    P, builder = case
    with P.solver(builder, 32) as a, P.solver(builder, 0) as b:
        before = {l: a.ml_level_array(l, "valf") for l in diag_levels(a)}
        for s in (a, b):
            s.refactor(P.other.nzval)
        print(f"refactor rebuilt the hierarchy: {a.get_int('refactor_rebuilt')}")
        if builder == "device":                    # the default construction keeps its cells: only the values were refreshed
            assert a.get_int("refactor_rebuilt") == 0
        levels = diag_levels(a)
        assert levels
        for l in levels:
            check_layout(a, l)                     # against the new valf: stale diagonals fail here
        assert any(l in before and not np.array_equal(before[l], a.ml_level_array(l, "valf")) for l in levels)
        assert_same_cycle(a, b, P)
        assert_same_solve(a, b, P)


class DeviceVectors:
    """K vectors on the device through the HIP runtime the library links"""

    def __init__(self, B):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.B = np.ascontiguousarray(B, np.float64)
        self.b, self.x = ctypes.c_void_p(), ctypes.c_void_p()
        nbytes = ctypes.c_size_t(self.B.nbytes)
        assert self.hip.hipMalloc(ctypes.byref(self.b), nbytes) == 0 and self.hip.hipMalloc(ctypes.byref(self.x), nbytes) == 0
        assert self.hip.hipMemcpy(self.b, self.B.ctypes.data_as(ctypes.c_void_p), nbytes, 1) == 0
        assert self.hip.hipMemset(self.x, 0, nbytes) == 0

    def solve(self, s):
        K, n = self.B.shape
        infos = s.solve_batch_device(self.b.value, self.x.value, K, n, raise_on_fail=False)
        X = np.empty_like(self.B)
        assert self.hip.hipMemcpy(X.ctypes.data_as(ctypes.c_void_p), self.x, ctypes.c_size_t(X.nbytes), 2) == 0
        return X, [(i["iters"], i["relres"]) for i in infos]

    def close(self):
        self.hip.hipFree(self.b)
        self.hip.hipFree(self.x)


def test_neighbours(case):
    """what shares the hierarchy or is built next to it: the transposed solver, a clone, the K-vector cycle (which stays on CSR)"""
    P, builder = case
    # (rtol: these solves are compared bit for bit with each other, and shorter ones say the same)
    with P.solver(builder, 32, rtol=1e-6) as a, P.solver(builder, 0, rtol=1e-6) as b:
        ta, tb = a.transposed(), b.transposed()
        assert_same_cycle(ta, tb, P)
        assert_same_solve(ta, tb, P)
        ca, cb = a.clone(), b.clone()
        try:
            assert_same_cycle(ca, cb, P)
            assert_same_solve(ca, cb, P)
        finally:
            ca.close()
            cb.close()
        for K in (2, 4):
            d = DeviceVectors(np.stack([P.rhs(10 + k) for k in range(K)]))
            try:
                Xa, ia = d.solve(a)
                Xb, ib = d.solve(b)
            finally:
                d.close()
            assert np.array_equal(Xa, Xb) and ia == ib
        assert_same_cycle(a, b, P)                 # and the one-vector cycle afterwards


def test_fallback(case):
    """a cap that no column of these levels meets: every level on CSR, silently, with the results of ml_diag = 0"""
    P, builder = case
    with P.solver(builder, 8) as a, P.solver(builder, 0) as b:
        for l in range(a.get_int("levels")):
            for name in DG:
                assert a.ml_level_array(l, name).size == 0
        assert_same_cycle(a, b, P)
        assert_same_solve(a, b, P)
