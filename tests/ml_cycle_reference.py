"""The multilevel cycle restated in numpy / scipy (f64) on levels that are GIVEN: read back from a solver
(nkp_ml_level_array) or taken from ml_reference.build.  TEST INFRASTRUCTURE: slow, sequential, never shipped.

Only the cycle is restated here, from the comments of include/nkp.h (nkp_tuning: "cycle"; nkp_ml_level_array), not the
aggregation: so it runs on every hierarchy the planner can build.

  outer step      b0 = r[perm0], x = cyc(0, b0), z[perm0] = x
  half sweep      of colour c: x[R_c] += B_c^-1 (b - L x)[R_c]; R_c the rows of colour c, B_c the entries of L inside each
                  column (block diagonal, one block per column).  No proper 2-colouring is assumed.
  sweep           forward: colour 0 then colour 1; reversed: colour 1 then colour 0
  level l < last  nu_l = nu_coarse if nu_coarse >= 1 and l >= coarse_from else nu.  From x = 0: nu_l forward sweeps; the
                  coarse correction rc = P^T (b - L x), x += omega * P cyc(l + 1, rc), twice if gamma_from <= l < gamma_to;
                  nu_l reversed sweeps
  last level      x = coarse_inv @ b where the level has a dense inverse; else from x = 0 `coarsest_sweeps` sweeps (30 if the
                  knob is <= 0), sweep s forward for even s and reversed for odd s

Two further modes exist only to size tolerances: blocks="inverse" solves the column blocks with explicit dense inverses
instead of LU (the same mathematics in another rounding), factors="f32" rounds the LU factors of every block and the coarsest
inverse to f32 and widens them again (what f32 storage of the factors does to a solve).  With f32 storage the device factors
the blocks of the f64 operator BEFORE it rounds operator and factors to f32, each on its own: a level that carries that f64
operator (with_exact_blocks) factors its blocks likewise in the factors="f32" mode.

Two evaluations of the same half sweep: the per-column one (a Python loop over the water columns; every mode) and, with
grouped=True, one that stacks the blocks of a colour by size and solves each stack in one call (np.linalg.solve, or the
stacked explicit inverses for blocks="inverse"), applied with one scatter -- the same blocks, the same LAPACK routines, for
hierarchies of 10^5 to 10^6 columns (tests/test_gpu_grid_caps.py).  The grouped one has no factors="f32" mode."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

MAX_BAND = 4          # beyond it the device's band factors drop entries: the block solve is then the band-capped one (band_cap)

# The cycle options of tests/test_gpu_cycle_options.py, by the names of nkp_options / nkp_tuning.  "hierarchy": deep = 5 levels
# with a dense last level, iterated = 3 levels with a last level that is relaxed, two = ml_levels = 2.
DEFAULT_KNOBS = dict(ml_smooth=3, ml_smooth_coarse=0, ml_coarse_from=2, ml_gamma_from=0, ml_gamma_to=0, ml_omega=1.1,
                     ml_coarsest_sweeps=30)
COMBINED = dict(ml_smooth=2, ml_smooth_coarse=1, ml_coarse_from=1, ml_gamma_from=1, ml_gamma_to=3, ml_omega=1.0)
OPTION_CASES = [
    ("default", "deep", {}),
    ("nu1", "deep", dict(ml_smooth=1)),
    ("nu2", "deep", dict(ml_smooth=2)),
    ("nu2_coarse1_from1", "deep", dict(ml_smooth=2, ml_smooth_coarse=1, ml_coarse_from=1)),
    ("coarse1_from2", "deep", dict(ml_smooth_coarse=1)),
    ("gamma_0_1", "deep", dict(ml_gamma_from=0, ml_gamma_to=1)),
    ("gamma_1_3", "deep", dict(ml_gamma_from=1, ml_gamma_to=3)),
    ("gamma_0_9", "deep", dict(ml_gamma_from=0, ml_gamma_to=9)),
    ("omega_1.0", "deep", dict(ml_omega=1.0)),
    ("omega_1.35", "deep", dict(ml_omega=1.35)),
    ("sweeps5", "iterated", dict(ml_coarsest_sweeps=5)),
    ("sweeps30", "iterated", dict(ml_coarsest_sweeps=30)),
    ("levels2", "two", {}),
    ("combined", "deep", COMBINED),
]


def cycle_kwargs(**knobs):
    """cycle()'s arguments from knobs named as in nkp_options / nkp_tuning."""
    k = dict(DEFAULT_KNOBS, **knobs)
    return dict(nu=k["ml_smooth"], nu_coarse=k["ml_smooth_coarse"], coarse_from=k["ml_coarse_from"], gamma_from=k["ml_gamma_from"],
                gamma_to=k["ml_gamma_to"], omega=k["ml_omega"], coarsest_sweeps=k["ml_coarsest_sweeps"])


class CycleLevel:
    """L: operator (csr, f64); col_of: column of every row (None on a level that only has an inverse); rows: [R_0, R_1];
    P: piecewise-constant prolongation (None on the last level); coarse_inv: dense inverse (last level) or None.
    band_cap: the half sweep's block solve is built from the in-column entries with |row - col| <= band_cap only (what the
    device's band factors keep on a level that reports dropped entries; the rows of a column must then be contiguous, as they
    are in a level's own colour-major order); the residual b - L x still uses all of L.  None: the whole block."""

    def __init__(self, L, col_of=None, rows=None, P=None, coarse_inv=None, perm0=None, band_cap=None):
        self.L = sp.csr_matrix(L, dtype=np.float64)
        self.L.sort_indices()
        self.n = self.L.shape[0]
        self.col_of, self.rows, self.P, self.coarse_inv, self.perm0 = col_of, rows, P, coarse_inv, perm0
        self._solvers = {}
        self.Bd_unrounded = None
        self.band_cap = band_cap
        if col_of is not None:
            if band_cap is not None:
                assert (np.diff(col_of) >= 0).all()           # contiguous columns: |row - col| is the distance inside the column
            self.band, self.Bd = self._block_diagonal(self.L)

    def _block_diagonal(self, L):
        C = L.tocoo()
        same = self.col_of[C.row] == self.col_of[C.col]
        band = int(np.abs(C.row[same] - C.col[same]).max()) if same.any() else 0
        if self.band_cap is not None:
            same &= np.abs(C.row - C.col) <= self.band_cap
        return band, sp.csr_matrix((C.data[same], (C.row[same], C.col[same])), shape=L.shape)

    def blocks(self, c, Bd):
        """(rows, dense block) of every column of colour c; a column's rows need not be contiguous."""
        R = self.rows[c]
        out = []
        if R.size:
            cols = self.col_of[R]
            o = np.argsort(cols, kind="stable")
            cut = np.flatnonzero(np.diff(cols[o])) + 1
            for idx in np.split(R[o], cut):
                out.append((idx, Bd[idx][:, idx].toarray()))
        return out

    def solver(self, c, blocks, factors):
        """res -> B_c^-1 res on the rows of colour c (res indexed by level row)."""
        key = (c, blocks, factors)
        if key not in self._solvers:
            parts = []
            Bd = self.Bd_unrounded if (factors == "f32" and self.Bd_unrounded is not None) else self.Bd
            for idx, B in self.blocks(c, Bd):
                if blocks == "inverse":
                    parts.append((idx, np.linalg.inv(B)))
                else:
                    lu, piv = sla.lu_factor(B, check_finite=False)
                    if factors == "f32":
                        lu = lu.astype(np.float32).astype(np.float64)
                    parts.append((idx, (lu, piv)))
            self._solvers[key] = parts
        return self._solvers[key]

    def grouped_solver(self, c, blocks):
        """The blocks of colour c stacked by size: [(idx, B)], idx (nb, s) the rows of nb columns of s rows each, B (nb, s, s)
        their dense blocks, or the inverses of those for blocks="inverse".  What blocks() cuts out of Bd, without the loop."""
        key = (c, blocks, "grouped")
        if key not in self._solvers:
            parts = []
            R = self.rows[c]
            if R.size:
                cols = self.col_of[R]
                o = np.argsort(cols, kind="stable")
                Rs = R[o]
                start = np.concatenate([[0], np.flatnonzero(np.diff(cols[o])) + 1])
                size = np.diff(np.concatenate([start, [Rs.size]]))
                blk_of = np.repeat(np.arange(start.size), size)              # of every entry of Rs
                pos = np.full(self.n, -1, np.int64)                          # place of a row inside its block; -1: another colour
                pos[Rs] = np.arange(Rs.size) - start[blk_of]
                blk = np.full(self.n, -1, np.int64)
                blk[Rs] = blk_of
                E = self.Bd.tocoo()
                keep = (blk[E.row] >= 0) & (blk[E.row] == blk[E.col])
                er, ec, ev = E.row[keep], E.col[keep], E.data[keep]
                for s in np.unique(size):
                    which = np.flatnonzero(size == s)
                    slot = np.full(start.size, -1, np.int64)
                    slot[which] = np.arange(which.size)
                    idx = Rs[start[which][:, None] + np.arange(s)[None, :]]
                    B = np.zeros((which.size, s, s))
                    e = slot[blk[er]] >= 0
                    np.add.at(B, (slot[blk[er[e]]], pos[er[e]], pos[ec[e]]), ev[e])      # Bd sums repeated entries too
                    parts.append((idx, np.linalg.inv(B) if blocks == "inverse" else B))
            self._solvers[key] = parts
        return self._solvers[key]


def _half(lv, x, b, c, blocks, factors, grouped=False):
    R = lv.rows[c]
    if not R.size:
        return
    res = b - lv.L @ x                                  # only the rows of colour c are used: they do not change below
    if grouped:
        assert factors == "f64"
        for idx, B in lv.grouped_solver(c, blocks):
            rhs = res[idx][:, :, None]
            x[idx] += ((B @ rhs) if blocks == "inverse" else np.linalg.solve(B, rhs))[:, :, 0]
        return
    for idx, f in lv.solver(c, blocks, factors):
        x[idx] += f @ res[idx] if blocks == "inverse" else sla.lu_solve(f, res[idx], check_finite=False)


def _sweep(lv, x, b, reverse, blocks, factors, grouped=False):
    for c in ((1, 0) if reverse else (0, 1)):
        _half(lv, x, b, c, blocks, factors, grouped)


class Glue:
    """The vector operations between the cycle's sweeps, one method per launch of csrc/mlcycle.hip (launch_gather,
    launch_scatter, launch_restrict_sum, launch_prolong_add, fill_x; l is the FINE level of a transfer), so that a test can
    restate one of them wrongly and see what its tolerance sees (tests/test_gpu_grid_caps.py)."""

    def gather(self, r, perm0):
        return r[perm0]

    def scatter(self, x, perm0):
        z = np.empty_like(x)
        z[perm0] = x
        return z

    def restrict(self, l, P, res):
        return P.T @ res

    def prolong(self, l, P, xc, omega, x):
        x += omega * (P @ xc)

    def fill(self, l, n):
        return np.zeros(n)


def cycle(levels, r, nu=3, nu_coarse=0, coarse_from=2, gamma_from=0, gamma_to=0, omega=1.1, coarsest_sweeps=30, blocks="lu",
          factors="f64", grouped=False, glue=None):
    assert blocks in ("lu", "inverse") and factors in ("f64", "f32") and not (grouped and factors == "f32")
    last = len(levels) - 1
    glue = glue or Glue()

    def cyc(l, b):
        lv = levels[l]
        if l == last and lv.coarse_inv is not None:
            inv = lv.coarse_inv
            if factors == "f32":
                inv = inv.astype(np.float32).astype(np.float64)
            return inv @ b
        x = glue.fill(l, lv.n)
        if l == last:
            for s in range(coarsest_sweeps if coarsest_sweeps > 0 else 30):
                _sweep(lv, x, b, s % 2 == 1, blocks, factors, grouped)
            return x
        nu_l = nu_coarse if (nu_coarse >= 1 and l >= coarse_from) else nu
        for _ in range(nu_l):
            _sweep(lv, x, b, False, blocks, factors, grouped)
        for _ in range(2 if gamma_from <= l < gamma_to else 1):
            rc = glue.restrict(l, lv.P, b - lv.L @ x)
            glue.prolong(l, lv.P, cyc(l + 1, rc), omega, x)
        for _ in range(nu_l):
            _sweep(lv, x, b, True, blocks, factors, grouped)
        return x

    r = np.asarray(r, np.float64)
    perm0 = levels[0].perm0
    if perm0 is None:
        return cyc(0, r.copy())
    return glue.scatter(cyc(0, glue.gather(r, perm0)), perm0)


def relative_difference(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


class Reference:
    """(tests/test_gpu_cycle_options.py, tests/test_gpu_colsolve_families.py)  The restated cycle on the levels of one hierarchy in one storage mode, for a set of option cases: z_ref per case and the
    yardstick of the tolerance (d per case with f64 storage, e over the cases with f32 storage).  Computed once per module."""

    def __init__(self, levels, r, f32, cases, grouped=False):
        assert not (grouped and f32)
        self.levels, self.f32 = levels, f32
        self.rows = [lv.n for lv in levels]
        self.z, self.yard = {}, {}
        for name, knobs in cases.items():
            kw = cycle_kwargs(**knobs)
            self.z[name] = cycle(levels, r, grouped=grouped, **kw)
            other = cycle(levels, r, factors="f32", **kw) if f32 else cycle(levels, r, blocks="inverse", grouped=grouped, **kw)
            self.yard[name] = relative_difference(other, self.z[name])
        self.e = max(self.yard.values())

    def bound(self, name):
        return min(2e-5, 16 * self.e) if self.f32 else max(1e-12, 4096 * self.yard[name])

    def check(self, label, name, z):
        err, bound = relative_difference(z, self.z[name]), self.bound(name)
        print("MEASURED %-34s %s  %.1e  bound %.1e  ratio %.2g" % (label, "f32" if self.f32 else "f64", err, bound, err / bound))
        assert err <= bound, (label, name, self.f32, err, bound, self.yard[name], self.e)


def with_exact_blocks(levels_f32, levels_f64):
    """Levels read from a solver with f32 storage, given the f64 operators their factors were made from (the levels of the same
    hierarchy read from a solver with f64 storage).  Checks that the f32 values are those f64 values rounded."""
    assert len(levels_f32) == len(levels_f64)
    for l, (a, b) in enumerate(zip(levels_f32, levels_f64)):
        assert np.array_equal(a.L.indptr, b.L.indptr) and np.array_equal(a.L.indices, b.L.indices), l
        assert np.array_equal(a.L.data, b.L.data.astype(np.float32).astype(np.float64)) or np.array_equal(a.L.data, b.L.data), l
        if a.col_of is not None:
            a.Bd_unrounded = a._block_diagonal(b.L)[1]
            a._solvers = {}
    return levels_f32


def levels_from_mlr(mlr_levels, dense_last=True):
    """The levels of ml_reference.build (natural row order, colours by grid position)."""
    out = []
    for l, lv in enumerate(mlr_levels):
        is_last = l == len(mlr_levels) - 1
        out.append(CycleLevel(lv.A, col_of=np.asarray(lv.colid), rows=[np.asarray(rows) for rows, _, _ in lv.colours],
                              P=None if is_last else lv.P, coarse_inv=lv.dense_inv if (is_last and dense_last) else None))
    return out


def levels_from_solver(s, band_cap=MAX_BAND):
    """Every level as it sits on the device.  The operator is the one the kernels multiply with: the f32 values widened to f64
    where the level stores them, else the f64 values; the last level multiplies by the device's own inverse if it has one.
    A level whose "col_kernel" reports dropped entries solves its blocks capped at band_cap; lv.band stays the measured one."""
    nlev = s.get_int("levels")
    out = []
    for l in range(nlev):
        rowptr, colind = s.ml_level_array(l, "rowptr"), s.ml_level_array(l, "colind")
        valf = s.ml_level_array(l, "valf")
        val = valf.astype(np.float64) if valf.size else s.ml_level_array(l, "val")
        n = rowptr.size - 1
        assert val.size == colind.size == rowptr[-1], (l, val.size, colind.size, rowptr[-1])
        L = sp.csr_matrix((val, colind, rowptr), shape=(n, n))
        blk = s.ml_level_array(l, "blk_start").astype(np.int64)
        col_of = rows = None
        if blk.size:
            cb = s.ml_level_array(l, "color_blk")
            assert cb.size == 3 and cb[0] == 0 and cb[0] <= cb[1] <= cb[2] == blk.size - 1, (l, cb, blk.size)
            assert blk[0] == 0 and blk[-1] == n and (np.diff(blk) > 0).all(), l
            col_of = np.repeat(np.arange(blk.size - 1), np.diff(blk))
            rows0 = int(blk[cb[1]])
            rows = [np.arange(0, rows0), np.arange(rows0, n)]
        cmap = s.ml_level_array(l, "cmap")
        P = None
        if l < nlev - 1:
            assert cmap.size == n
            nc = s.ml_level_array(l + 1, "rowptr").size - 1
            P = sp.csr_matrix((np.ones(n), (np.arange(n), cmap)), shape=(n, nc))
        inv = s.ml_level_array(l, "coarse_inv") if l == nlev - 1 else np.empty(0)
        ck = s.ml_level_array(l, "col_kernel")
        assert ck.size == (11 if blk.size else 0), (l, ck)
        dropped = bool(blk.size and ck[6])
        lv = CycleLevel(L, col_of=col_of, rows=rows, P=P, coarse_inv=inv.reshape(n, n) if inv.size else None,
                        perm0=s.ml_level_array(0, "perm0").astype(np.int64) if l == 0 else None, band_cap=band_cap if dropped else None)
        lv.blk_start = blk
        lv.dropped = dropped
        if col_of is not None and dropped:
            assert lv.band > band_cap, (l, lv.band)
        elif col_of is not None:
            assert lv.band <= MAX_BAND, (l, lv.band)
        else:
            assert lv.coarse_inv is not None, l
        out.append(lv)
    return out
