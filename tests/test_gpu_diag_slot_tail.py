"""diag_residual_kernel (csrc/diagop.hip) takes a column's keys eight at a time and the rest in one step of exactly that
length.  Same method as tests/test_gpu_diag_residual.py: a solver with ml_diag = 32 against one with ml_diag = 0, both with
col_wave_max = 0, ml_wave_fused = 0 and a small ml_coarsest_rows, so that every level but the last runs its half sweeps and
its residual on the diagonals; np.array_equal on precond_apply of two right-hand sides (one with a colour zeroed) and on a
solve with its iters, relres and status.

What a passing comparison proves depends on the key counts the levels of these grids have, so test_cases_cover works them
out on the host from dg_ptr, blk_start and color_blk of every level that has diagonals and fails unless the cases together
hold: every length 0 .. 7 of the last step, a column of fewer than 8 keys (no full step), one of more than 16 that is no
multiple of 8 (two full steps and a rest), a launch whose tile count is no multiple of the 4 tiles of a workgroup, one of
at least 256 tiles, and a column of two tiles.

Shapes: those of tests/test_gpu_diag_residual.py (12x10x6 with hmix="const", 24x20x12, 40x36x24, 10x8x70 cut at 150
iterations) and 64x48x12, a wider grid of the same kind.
"""
import numpy as np
import pytest

from nk_ocn_tracer_jacobian_precond_amd import solver, synth

pytestmark = pytest.mark.gpu

SHAPES = {
    "12x10x6": (dict(imt=12, jmt=10, km=6, seed=2, hmix="const"), 200, {}),
    "24x20x12": (dict(imt=24, jmt=20, km=12, seed=2), 200, {}),
    "40x36x24": (dict(imt=40, jmt=36, km=24, seed=4), 300, {}),
    "10x8x70": (dict(imt=10, jmt=8, km=70, seed=5), 200, dict(max_iters=150)),
    "64x48x12": (dict(imt=64, jmt=48, km=12, seed=2), 200, {}),
}
WAVE, STEP, WG_TILES = 64, 8, 4


class Pair:
    """the two solvers of one shape and its right-hand sides"""

    def __init__(self, name):
        kw, coarsest, options = SHAPES[name]
        p = synth.generate(**dict(dict(adv="upwind3", hmix="isop"), **kw))
        blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
        ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
        self.n = p.flat_len

        def make(ml_diag):
            tuning = dict(col_wave_max=0, ml_wave_fused=0, ml_coarsest_rows=coarsest, ml_diag=ml_diag)
            return solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, precond=solver.PRECOND_MULTILEVEL, tuning=tuning,
                                    **dict(dict(rtol=1e-10, restart=60, col_i=ci, col_j=cj), **options))
        self.diag, self.csr = make(32), make(0)

    def rhs(self, k):
        return np.random.default_rng(31 + k).standard_normal(self.n)

    def close(self):
        self.diag.close()
        self.csr.close()


@pytest.fixture(scope="module")
def pairs():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Pair(name)
        return made[name]
    yield get
    for p in made.values():
        p.close()


def diag_levels(s):
    return [l for l in range(s.get_int("levels")) if s.ml_level_array(l, "dg_val").size]


@pytest.mark.parametrize("name", list(SHAPES))
def test_cycle_and_solve(name, pairs):
    P = pairs(name)
    a, b = P.diag, P.csr
    assert diag_levels(a) and not diag_levels(b)
    perm0, blk, cb = (a.ml_level_array(0, w) for w in ("perm0", "blk_start", "color_blk"))
    zeroed = P.rhs(1)
    zeroed[perm0[:blk[cb[1]]]] = 0.0                    # the rows of colour 0
    for r in (P.rhs(0), zeroed):
        za, zb = a.precond_apply(r), b.precond_apply(r)
        assert np.all(np.isfinite(za)) and np.array_equal(za, zb)
    xa, ia = a.solve(P.rhs(2), raise_on_fail=False)
    xb, ib = b.solve(P.rhs(2), raise_on_fail=False)
    assert np.array_equal(xa, xb) and all(ia[k] == ib[k] for k in ("status", "iters", "relres")) and ia["iters"] > 0


def test_cases_cover(pairs):
    rests, keys, launches, two_tiles = set(), set(), set(), False
    for name in SHAPES:
        s = pairs(name).diag
        for l in diag_levels(s):
            ptr, blk, cb = (s.ml_level_array(l, w) for w in ("dg_ptr", "blk_start", "color_blk"))
            nk, length = np.diff(ptr), np.diff(blk)
            tiles = (length + WAVE - 1) // WAVE
            rests |= set((nk % STEP).tolist())
            keys |= set(nk.tolist())
            two_tiles = two_tiles or bool(np.any(tiles == 2))
            c0, c1 = int(tiles[:cb[1]].sum()), int(tiles[cb[1]:].sum())
            launches |= {c0, c1, c0 + c1}
            print(f"{name} level {l}: columns {nk.size}, keys per column {np.bincount(nk).nonzero()[0].tolist()}, tiles per launch {c0} {c1} {c0 + c1}")
    assert rests == set(range(STEP)), f"lengths of the last step: {sorted(rests)}"
    assert any(k < STEP for k in keys), "no column without a full step"
    assert any(k > 2 * STEP and k % STEP for k in keys), "no column with two full steps and a rest"
    assert any(c % WG_TILES for c in launches), "every launch fills its last workgroup"
    assert any(c >= 256 for c in launches), "no launch of 256 tiles"
    assert two_tiles, "no column of two tiles"
