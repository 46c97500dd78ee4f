"""The solver's own matrix A as per-column diagonals (tuning spmv_diag, csrc/diagop.hip, f64 values): the layout against the
CSR arrays the solver was given, and the bits of everything that multiplies with A against the same solver with spmv_diag = 0.

The diagonal kernel sums a row's products from +0.0 in ascending key order = ascending columns, the stored order the CSR
kernels sum in, and a padded position adds +0.0 * x = +-0 to a sum that is never -0: every comparison is np.array_equal.

Shapes: those of tests/test_gpu_diag_residual.py (upwind3 + isop; 12x10x6 also with hmix="const") and 10x8x64 with seed 6,
whose deepest column has exactly 64 rows (one tile of 64 rows: groups of one key; worked out on the host: 20 keys at most,
padding 1.12 nnz).  10x8x70 (longest column 67 rows: two tiles, 34 + 33) and 10x8x64 are cut at max_iters = 150.  The levels
are built by the setup kernels (ml_device_min = 0) with a small ml_coarsest_rows (several levels, as in
tests/test_gpu_diag_residual.py), which keep their coarse cells in a refactor, so a refactor with a live clone is not refused.

test_refactor: after a plain refactor the coarse cells are those of the old values, and a solver created on the new values
may pick others (tests/test_gpu_refactor.py), so dg_val and spmv are compared with the fresh solver after the plain refactor
and the solve after a refactor with rebuild=True, which gives the fresh create's hierarchy; the solver with spmv_diag = 0
goes through the same two refactors and is compared after each.
"""
import numpy as np
import pytest

from nk_ocn_tracer_jacobian_precond_amd import solver, synth

pytestmark = pytest.mark.gpu

SHAPES = {
    "12x10x6-const": (dict(imt=12, jmt=10, km=6, seed=2, hmix="const"), 1, {}),
    "12x10x6": (dict(imt=12, jmt=10, km=6, seed=2), 1, {}),
    "24x20x12": (dict(imt=24, jmt=20, km=12, seed=2), 1, {}),
    "40x36x24": (dict(imt=40, jmt=36, km=24, seed=4), 1, {}),
    "10x8x70": (dict(imt=10, jmt=8, km=70, seed=5), 1, dict(max_iters=150)),
    "tracers2": (dict(imt=24, jmt=20, km=12, seed=3, coupled_tracer_cnt=2), 2, {}),
    "10x8x64": (dict(imt=10, jmt=8, km=64, seed=6), 1, dict(max_iters=150)),
}
DG = ("dg_ptr", "dg_key", "dg_voff", "dg_val", "dg_gptr", "dg_grp")
WAVE, RUN_MAX = 64, 5
SOLVES = {"fgmres": {}, "steps2": dict(precond_steps=2), "equil": dict(equil=1), "bicgstab": dict(krylov=solver.KRYLOV_BICGSTAB)}


class Problem:
    def __init__(self, name):
        kw, self.cnt, self.options = SHAPES[name]
        kw = dict(dict(adv="upwind3", hmix="isop"), **kw)
        self.p = p = synth.generate(**kw)
        self.other = synth.generate(**dict(kw, day_cnt=180.0)).nzval                 # other values on the same pattern
        assert not np.array_equal(p.nzval, self.other)
        self.blk = solver.column_blocks(p.col_start(), p.tracer_state_len, self.cnt)
        ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), self.cnt)
        self.coords = dict(col_i=ci, col_j=cj)
        self.n = p.flat_len
        self.length = np.diff(self.blk).astype(np.int64)
        self._pair = None

    def solver(self, spmv_diag, val=None, blocks=True, tuning=None, **more):
        p = self.p
        val = p.nzval if val is None else val
        tuning = dict(dict(ml_device_min=0, ml_coarsest_rows=300 if self.n > 10000 else 200, spmv_diag=spmv_diag), **(tuning or {}))
        if not blocks:                                    # no water columns given: nothing to build a preconditioner on either
            return solver.NkpSolver(p.rowptr, p.colind, val, precond=solver.PRECOND_NONE, tuning=tuning)
        return solver.NkpSolver(p.rowptr, p.colind, val, self.blk, coupled_tracer_cnt=self.cnt, precond=solver.PRECOND_MULTILEVEL, tuning=tuning,
                                **dict(dict(rtol=1e-10, restart=60, **self.coords), **self.options, **more))

    def pair(self):
        """the plain FGMRES solvers with spmv_diag = 32 and 0, shared by the cases that leave them as they are"""
        if self._pair is None:
            self._pair = (self.solver(32), self.solver(0))
        return self._pair

    def close(self):
        for s in self._pair or ():
            s.close()

    def rhs(self, k=0):
        return np.random.default_rng(31 + k).standard_normal(self.n)

    def vectors(self):
        """x of the product test: normal, with zeros of both signs, and unit vectors around the longest column"""
        rng = np.random.default_rng(7)
        out = [("normal", rng.standard_normal(self.n))]
        z = rng.standard_normal(self.n)
        z[rng.random(self.n) < 0.2] = 0.0
        z[rng.random(self.n) < 0.2] = -0.0
        out.append(("zeros", z))
        c = int(np.argmax(self.length))
        nb = c + 1 if c + 1 < self.length.size else c - 1
        for col in (c, nb):
            r0, ln = int(self.blk[col]), int(self.length[col])
            for r in sorted({r0, r0 + ln // 2, r0 + ln - 1}):
                e = np.zeros(self.n)
                e[r] = 1.0
                out.append((f"unit{r}", e))
        return out


_problems = {}


@pytest.fixture(scope="module", params=list(SHAPES))
def P(request):
    if request.param not in _problems:
        _problems[request.param] = Problem(request.param)
    yield _problems[request.param]
    _problems.pop(request.param).close()


def check_layout(s, P, val):
    """A's diagonals hold the CSR entries the solver was given, entry for entry with their f64 bits, +0.0 everywhere else"""
    rowptr, colind, blk = P.p.rowptr.astype(np.int64), P.p.colind.astype(np.int64), P.blk.astype(np.int64)
    ptr, key, voff, dval = (s.matrix_array(a) for a in DG[:4])
    n, ncol = rowptr.size - 1, blk.size - 1
    assert ptr.size == ncol + 1 and voff.size == ncol and key.size == ptr[-1] and ptr[0] == 0 and np.all(np.diff(ptr) >= 0)
    length, nk = P.length, np.diff(ptr).astype(np.int64)
    assert np.array_equal(voff, np.concatenate(([0], np.cumsum(nk * length)[:-1]))) and dval.size == int(np.sum(nk * length))
    span = 2 * n + 1
    ckey = np.repeat(np.arange(ncol, dtype=np.int64), nk) * span + (key.astype(np.int64) + n)
    assert np.all(np.diff(ckey) > 0)                                                                   # keys strictly ascending per column
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    col = np.repeat(np.arange(ncol, dtype=np.int64), length)[row]
    kl = row - blk[col]
    want = col * span + (colind - kl + n)
    pos = np.searchsorted(ckey, want)
    assert np.all(pos < ckey.size) and np.array_equal(ckey[np.minimum(pos, ckey.size - 1)], want)      # every entry's key is in its column's list
    assert np.unique(pos).size == key.size                                                            # no idle key
    assert np.all(np.diff(pos)[np.diff(row) == 0] > 0)                                                # slot order = stored order
    idx = voff[col] + (pos - ptr[col]) * length[col] + kl
    assert np.unique(idx).size == idx.size
    expect = np.zeros(dval.size, np.float64)
    expect[idx] = val
    assert np.array_equal(expect.view(np.uint64), dval.view(np.uint64))                               # the bits, and +0.0 in every padded position
    return int(nk.max()), dval.size / colind.size


def check_groups(s, P):
    """the rules of tests/test_gpu_diag_windows.py: maximal runs of consecutive keys, at most 5, at most 64 - rows + 1"""
    ptr, key, gptr, grp = (s.matrix_array(a).astype(np.int64) for a in ("dg_ptr", "dg_key", "dg_gptr", "dg_grp"))
    ncol, length = P.length.size, P.length
    tiles = (length + WAVE - 1) // WAVE
    rows = (length + tiles - 1) // tiles
    lim = np.minimum(WAVE - rows + 1, RUN_MAX)
    assert grp.size % 2 == 0
    key0, s0, m = grp[0::2], grp[1::2] & 0xffff, grp[1::2] >> 16
    col = np.repeat(np.arange(ncol, dtype=np.int64), np.diff(gptr))
    nk = np.diff(ptr)
    assert gptr.size == ncol + 1 and gptr[0] == 0 and gptr[-1] == m.size and np.all(np.diff(gptr) > 0) and np.all(nk > 0)
    assert np.all(m >= 1)
    first = np.zeros(m.size, bool)
    first[gptr[:-1]] = True
    assert np.all(s0[first] == 0)
    assert np.array_equal(s0[1:][~first[1:]], (s0 + m)[:-1][~first[1:]])
    last = np.roll(first, -1)
    last[-1] = True
    assert np.array_equal((s0 + m)[last], nk[col[last]])                                              # the groups partition the column's slots in order
    slot = ptr[col] + s0
    assert np.array_equal(key0, key[slot])
    gid = np.repeat(np.arange(m.size), m)
    pos = np.arange(gid.size) - np.repeat(np.cumsum(m) - m, m)
    assert np.array_equal(key[slot[gid] + pos], key0[gid] + pos)                                      # consecutive keys inside a group
    assert np.all(m <= lim[col])
    nxt = key[np.minimum(slot + m, key.size - 1)]
    goes_on = ~last & (nxt == key0 + m)
    assert np.all(m[goes_on] == lim[col][goes_on])                                                    # cut only at 5 keys or at the fit limit
    return rows, col, m


def same_solve(a, b, rhs):
    xa, ia = a.solve(rhs, raise_on_fail=False)
    xb, ib = b.solve(rhs, raise_on_fail=False)
    assert ia["iters"] > 0 and np.all(np.isfinite(xa))
    assert np.array_equal(xa, xb) and all(ia[k] == ib[k] for k in ("status", "iters", "relres"))


def test_layout(P):
    a, b = P.pair()
    assert a.get_int("spmv_diag") == 1 and b.get_int("spmv_diag") == 0
    most, pad = check_layout(a, P, P.p.nzval)
    rows, col, m = check_groups(a, P)
    print(f"columns {P.length.size}, longest {int(P.length.max())}, most keys {most}, padding / nnz {pad:.3f}, group lengths {np.bincount(m)[1:].tolist()}")
    assert most <= 32 and pad <= 1.5
    if int(P.length.max()) == WAVE:                       # 10x8x64: a tile of 64 rows keeps groups of one key
        full = rows[col] == WAVE
        assert np.any(full) and np.all(m[full] == 1)
    if int(P.length.max()) > WAVE:                        # 10x8x70: two tiles
        assert np.any((P.length + WAVE - 1) // WAVE == 2)


def test_product_bits(P):
    a, b = P.pair()
    assert a.get_int("spmv_diag") == 1 and b.get_int("spmv_diag") == 0
    for name, x in P.vectors():
        ya, yb = a.spmv(x), b.spmv(x)
        assert np.array_equal(ya.view(np.uint64), yb.view(np.uint64)), name
    assert np.any(a.spmv(P.vectors()[0][1]) != 0.0)


@pytest.mark.parametrize("variant", list(SOLVES))
def test_solve_bits(P, variant):
    if variant == "fgmres":
        a, b = P.pair()
        assert a.get_int("spmv_diag") == 1 and b.get_int("spmv_diag") == 0
        same_solve(a, b, P.rhs(2))
        return
    with P.solver(32, **SOLVES[variant]) as a, P.solver(0, **SOLVES[variant]) as b:
        assert a.get_int("spmv_diag") == 1 and b.get_int("spmv_diag") == 0
        if variant == "steps2":
            assert a.get_int("precond_steps") == 2
        if variant == "equil":
            assert a.get_int("equil") == 1
        same_solve(a, b, P.rhs(2))


def test_refactor(P):
    x, rhs = P.vectors()[0][1], P.rhs(3)
    with P.solver(32) as a, P.solver(0) as b, P.solver(32, val=P.other) as fresh:
        assert a.get_int("spmv_diag") == 1 and fresh.get_int("spmv_diag") == 1 and b.get_int("spmv_diag") == 0
        old = a.matrix_array("dg_val")
        pattern = [a.matrix_array(w) for w in DG if w != "dg_val"]
        c = a.clone()
        try:
            a.refactor(P.other)
            b.refactor(P.other)
            new = a.matrix_array("dg_val")
            assert not np.array_equal(old, new)
            check_layout(a, P, P.other)                   # stale diagonals fail here
            assert np.array_equal(new.view(np.uint64), fresh.matrix_array("dg_val").view(np.uint64))
            assert all(np.array_equal(w, a.matrix_array(n)) for w, n in zip(pattern, [w for w in DG if w != "dg_val"]))
            assert np.array_equal(a.spmv(x), fresh.spmv(x)) and np.array_equal(a.spmv(x), b.spmv(x))
            same_solve(a, b, rhs)
            assert c.get_int("spmv_diag") == 1
            same_solve(c, a, rhs)                         # the clone made before the refactor multiplies with the new values
        finally:
            c.close()
        a.refactor(P.other, rebuild=True)
        b.refactor(P.other, rebuild=True)
        assert np.array_equal(a.matrix_array("dg_val").view(np.uint64), new.view(np.uint64))
        same_solve(a, fresh, rhs)
        same_solve(a, b, rhs)


def test_fallback(P):
    a, b = P.pair()
    x, rhs = P.vectors()[0][1], P.rhs(2)
    want = b.spmv(x)

    def on_csr(s):
        assert s.get_int("spmv_diag") == 0 and s.get_int("spmv_diag_bytes") == 0
        for w in DG:
            assert s.matrix_array(w).size == 0
        with pytest.raises(solver.NkpError) as e:
            s.time_kernel(8, reps=1)
        assert e.value.code == -1                         # NKP_EINVAL

    with P.solver(8) as capped, P.solver(0) as off, P.solver(32, blocks=False) as noblk:
        for s in (capped, off, noblk):
            on_csr(s)
            assert np.array_equal(s.spmv(x), want)
        same_solve(capped, b, rhs)
        same_solve(off, b, rhs)
    with P.solver(32) as owner:
        t, tb = owner.transposed(), b.transposed()
        assert owner.get_int("spmv_diag") == 1
        on_csr(t)
        assert np.array_equal(t.spmv(x), tb.spmv(x)) and not np.array_equal(t.spmv(x), want)
        same_solve(t, tb, rhs)
        assert np.array_equal(owner.spmv(x), want)        # and the owner still multiplies on its diagonals


def test_bytes(P):
    a, b = P.pair()
    nval, ngrp = a.matrix_array("dg_val").size, a.matrix_array("dg_grp").size // 2
    ntile = int(np.sum((P.length + WAVE - 1) // WAVE))
    assert a.get_int("spmv_diag_bytes") == 8 * nval + 48 * ntile + 8 * ngrp + 16 * P.n
    nnz = P.p.colind.size
    for s in (a, b):
        assert s.get_int("spmv_bytes") == 12 * nnz + 4 * (P.n + 1) + 16 * P.n
    assert a.time_kernel(8, reps=2) > 0.0 and a.time_kernel(0, reps=2) > 0.0


def test_levels_untouched():
    """the level operators keep their own diagonals (f32, y = b - L x) next to A's: small levels take the two-kernel half sweeps
    that read them with col_wave_max = 0 and ml_wave_fused = 0, as in tests/test_gpu_diag_residual.py"""
    Q = Problem("24x20x12")
    r = Q.rhs(5)
    levels = dict(col_wave_max=0, ml_wave_fused=0)
    with Q.solver(32, tuning=levels) as a, Q.solver(0, tuning=levels) as b:
        assert a.get_int("spmv_diag") == 1 and b.get_int("spmv_diag") == 0
        za, zb = a.precond_apply(r), b.precond_apply(r)
        assert np.all(np.isfinite(za)) and np.array_equal(za, zb)
        assert any(a.ml_level_array(l, "dg_val").size for l in range(a.get_int("levels")))
        for l in range(a.get_int("levels")):
            for w in ("dg_key", "dg_val", "dg_grp"):
                assert np.array_equal(a.ml_level_array(l, w), b.ml_level_array(l, w))
