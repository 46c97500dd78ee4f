"""Every CSR SpMV kernel, mode and batch width on the ragged row blocks of tests/spmv_shapes.py (what those matrices contain is
asserted on the CPU by tests/test_spmv_shapes.py).

Rows summed in stored order (blocks of at most 2048 entries) must have the bits of the CPU oracle; long rows (a 256-strided
tree sum) must lie within the rounding bound e_i = (len_i + 2) 2^-52 d_i of the exact reference, and every kernel selection must
give the same bits, long rows included.  Modes 1 (b - A x) and 2 (|A||x| + |b|) are read through the public ABI: with
max_iters = 0 and use_guess = 1 a solve is the evaluation of the residual and of the backward error of the guess."""
import ctypes
import math

import numpy as np
import pytest

import oracle_binding as ora
import spmv_shapes as sh
from nk_ocn_tracer_jacobian_precond_amd import solver, synth

pytestmark = pytest.mark.gpu

PIPE = dict(spmv_variant=4, spmv_pipe_min=1)
SELECT = {
    "pipe_run1": dict(PIPE, spmv_run=1, spmv_compress=0),
    "pipe_run4": dict(PIPE, spmv_run=4, spmv_compress=0),
    "pipe_run1_coded": dict(PIPE, spmv_run=1, spmv_compress=1),
    "pipe_run4_coded": dict(PIPE, spmv_run=4, spmv_compress=1),
    "stream_coded": dict(spmv_variant=4, spmv_compress=1),                     # below spmv_pipe_min: variant 4 of the stream kernel
    "stream": dict(spmv_variant=0),
    "pairs": dict(spmv_variant=1),
    "nontemporal": dict(spmv_variant=2),
    "pairs_nontemporal": dict(spmv_variant=3),
    "rows": dict(spmv_variant=9),
}
EVAL_SELECT = ["pipe_run1", "pipe_run4_coded", "stream", "stream_coded", "rows"]
KRYLOV = {"fgmres": solver.KRYLOV_FGMRES, "bicgstab": solver.KRYLOV_BICGSTAB}
SHAPES = {"ragged_empty": sh.ragged_empty, "ragged_dd": sh.ragged_dd}


def _solver(s, tuning=None, rowptr64=False, **opts):
    """ragged_empty without a preconditioner, ragged_dd with point Jacobi (one-row column blocks)."""
    rowptr = s.rowptr.astype(np.int64) if rowptr64 else s.rowptr
    kw = dict(restart=4)
    kw.update(opts)
    if tuning is not None:
        kw["tuning"] = dict(tuning)
    if s.name == "ragged_empty":
        return solver.NkpSolver(rowptr, s.colind, s.val, None, precond=solver.PRECOND_NONE, **kw)
    return solver.NkpSolver(rowptr, s.colind, s.val, np.arange(s.n + 1), precond=solver.PRECOND_COLUMN_JACOBI, **kw)


def _norm(v):
    return math.sqrt(math.fsum((np.asarray(v, np.float64) ** 2).tolist()))


@pytest.fixture(scope="module")
def refs():
    """Per matrix: x0, b, the exact reference of y = A x (E0) and of r, d for b (E1), the oracle's stored-order y."""
    out = {}
    for name, make in SHAPES.items():
        s = make()
        x0, b = sh.vectors(s)
        out[name] = dict(s=s, x0=x0, b=b, E0=sh.exact(s, x0), E1=sh.exact(s, x0, b), y_ora=ora.spmv(s.rowptr, s.colind, s.val, x0))
    return out


# ---------------------------------------------------------------- a. y = A x, every kernel
@pytest.fixture(scope="module")
def products(refs):
    """nkp_spmv on ragged_empty for every kernel selection, once."""
    R = refs["ragged_empty"]
    s, nb = R["s"], sh.row_blocks(R["s"].rowptr).size - 1
    out = {}
    for name, tuning in SELECT.items():
        with _solver(s, tuning) as h:
            assert h.get_int("rowblocks") == nb                                 # the restated partitioner is the library's
            out[name] = h.spmv(R["x0"])
    with _solver(s, SELECT["pipe_run4_coded"], rowptr64=True) as h:
        out["pipe_run4_coded/rowptr64"] = h.spmv(R["x0"])
    return out


def _check_product(y, R, s=None, y_ora=None, E=None):
    s, y_ora, E = s or R["s"], R["y_ora"] if y_ora is None else y_ora, E or R["E0"]
    short = ~s.long
    assert np.all(np.isfinite(y))
    bad = np.flatnonzero(short & (y != y_ora))
    assert bad.size == 0, (bad[:8], y[bad[:8]], y_ora[bad[:8]])                 # stored-order sums: the oracle's bits
    err = np.abs(y - E.y)
    worst = np.flatnonzero(err > E.e)
    assert worst.size == 0, (worst[:8], err[worst[:8]], E.e[worst[:8]])         # every row, the long ones among them


@pytest.mark.parametrize("name", list(SELECT) + ["pipe_run4_coded/rowptr64"])
def test_product_on_ragged_blocks(products, refs, name):
    R = refs["ragged_empty"]
    assert R["s"].long.sum() >= 6 and (R["s"].len == 0).sum() > 300
    _check_product(products[name], R)
    assert np.all(products[name][R["s"].len == 0] == 0.0)                       # empty rows are written, with zero


def test_product_has_the_same_bits_from_every_kernel(products):
    first = products["stream"]
    for name, y in products.items():
        bad = np.flatnonzero(y != first)
        assert bad.size == 0, (name, bad[:8], y[bad[:8]], first[bad[:8]])


# ---------------------------------------------------------------- b. modes 1 and 2 through the public ABI
class _Device:
    """a float64 array on the device, through the HIP runtime the library links (hipMalloc / hipMemcpy / hipFree); a second
    runtime in the process -- the one a later `import torch` brings along -- is what these tests must not load"""

    def __init__(self, a):
        self.hip = ctypes.CDLL("libamdhip64.so")
        a = np.ascontiguousarray(a, np.float64)
        self.size, self.p = a.size, ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(self.p), ctypes.c_size_t(a.nbytes)) == 0
        assert self.hip.hipMemcpy(self.p, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.nbytes), 1) == 0           # host to device
        self.ptr = self.p.value

    def get(self):
        out = np.empty(self.size)
        assert self.hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), self.p, ctypes.c_size_t(out.nbytes), 2) == 0       # device to host
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.hip.hipFree(self.p)


def _evaluate(h, b, x0):
    """relres, berr of the guess x0 (no iteration) and what the call leaves in x."""
    with _Device(b) as db, _Device(x0) as dx:
        info = h.solve_device(db.ptr, dx.ptr, use_guess=True, raise_on_fail=False)
        return info, dx.get()


@pytest.fixture(scope="module")
def evaluations(refs):
    out = {}
    for shape, R in refs.items():
        for kname, krylov in KRYLOV.items():
            for name in EVAL_SELECT:
                with _solver(R["s"], SELECT[name], krylov=krylov, max_iters=0) as h:
                    out[shape, kname, name] = _evaluate(h, R["b"], R["x0"])
    return out


@pytest.mark.parametrize("name", EVAL_SELECT)
@pytest.mark.parametrize("kname", list(KRYLOV))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_residual_and_backward_error_of_a_guess(evaluations, refs, shape, kname, name):
    R = refs[shape]
    s, E = R["s"], R["E1"]
    info, x = evaluations[shape, kname, name]
    assert info["status"] == solver.NKP_NOT_CONVERGED and info["iters"] == 0, info
    assert np.array_equal(x, R["x0"])
    rnorm, bnorm = _norm(E.r), _norm(R["b"])
    berr = float(np.max(np.abs(E.r) / E.d))
    print(f"{shape} {kname} {name}: relres {info['relres']:.17g} exact {rnorm / bnorm:.17g}  berr {info['berr']:.17g} exact {berr:.17g}")
    assert abs(info["relres"] * bnorm - rnorm) <= _norm(E.e) + s.n * sh.U * rnorm, (info, rnorm / bnorm)
    assert abs(info["berr"] - berr) <= (int(s.len.max()) + 3) * sh.U * (1.0 + berr), (info, berr)


@pytest.mark.parametrize("kname", list(KRYLOV))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_residual_and_backward_error_have_the_same_bits_from_every_kernel(evaluations, shape, kname):
    first = evaluations[shape, kname, EVAL_SELECT[0]][0]
    for name in EVAL_SELECT[1:]:
        info = evaluations[shape, kname, name][0]
        assert info["relres"] == first["relres"] and info["berr"] == first["berr"], (name, info, first)


def _probe_rows(s):
    """Rows whose |A||x| + |b| a probe reads back: every long row, the rows at the caps, an empty row inside the block of empty
    rows and at a block's end, a row of each dictionary block and an ordinary row of either stretch."""
    m = s.marks
    rows = np.flatnonzero(s.long).tolist()
    rows += [m["row_2048"], m["row_2047_then_2"], m["row_2047_then_2"] + 1, m["block_2048"] + 2, m["empty_at_block_end"] + 1,
             m["empty_block"] + 100, m["empty_block"] + 299, m["dict_256"] + 84, m["dict_257"] + 85, 1000, 2000]
    return rows


@pytest.mark.parametrize("name", ["pipe_run4_coded", "stream", "rows"])
def test_backward_error_reads_one_row_at_a_time(refs, name):
    """berr = max_i |r_i| / d_i shows d = |A||x| + |b| of the worst row only.  With b = A x0 in stored order the residual of
    every short row is zero and that of a long row at rounding level; moving ONE entry of b by (|A||x|)_t makes row t the worst
    one, so that berr is |r_t| / d_t of a chosen row: mode 2 of the kernel on that row, within the same bound."""
    R = refs["ragged_empty"]
    s, x0 = R["s"], R["x0"]
    absAx = R["E0"].d
    with _solver(s, SELECT[name], max_iters=0) as h:
        for t in _probe_rows(s):
            b = R["y_ora"].copy()
            b[t] += absAx[t] if absAx[t] > 0.0 else 1.0
            E = sh.exact(s, x0, b)
            with np.errstate(invalid="ignore", divide="ignore"):
                q = np.where(E.d > 0.0, np.abs(E.r) / E.d, 0.0)
            assert np.all(E.r[E.d == 0.0] == 0.0) and (E.d == 0.0).sum() > 300          # empty rows with b_i = 0: 0 / 0 counts as 0
            assert int(np.argmax(q)) == t and 0.1 < q[t] <= 1.0 and np.sort(q)[-2] < 1e-12
            info, _ = _evaluate(h, b, x0)
            assert info["iters"] == 0
            assert abs(info["berr"] - q[t]) <= (int(s.len[t]) + 3) * sh.U * (1.0 + q[t]), (name, t, int(s.len[t]), info, q[t])


# ---------------------------------------------------------------- c. batched long rows
BATCH_OPTIONS = {
    "rows_layout": dict(tuning=dict(batch_spmv_rows=1)),
    "products_layout": dict(tuning=dict(batch_spmv_rows=0)),
    "equil": dict(equil=1),
    "chained": dict(precond_steps=2),
    "products_layout+equil+chained": dict(equil=1, precond_steps=2, tuning=dict(batch_spmv_rows=0)),
    "rows_layout+equil+chained": dict(equil=1, precond_steps=2),               # the residual between two cycles reads a split, scaled right-hand side
}


def _assert_column_bits(tag, X, infos, single, cols):
    for q, c in enumerate(cols):
        x1, i1 = single[c]
        assert infos[q]["iters"] == i1["iters"] and infos[q]["relres"] == i1["relres"] and infos[q]["berr"] == i1["berr"], (tag, c, infos[q], i1)
        assert np.array_equal(X[q], x1), (tag, c, np.abs(X[q] - x1).max())


@pytest.mark.parametrize("key", list(BATCH_OPTIONS))
def test_batched_columns_on_long_rows_have_the_bits_of_single_solves(key):
    """ragged_dd, point Jacobi: the long-row branches of both batched SpMV layouts, with the scaling of the row-weighted
    iteration in their epilogue (equil) and the split, scaled right-hand side of the residual between two chained cycles."""
    s = sh.ragged_dd()
    opts = dict(BATCH_OPTIONS[key])
    tuning = opts.pop("tuning", {})
    B = sh.solve_rhs(s, 8)
    common = dict(rtol=1e-10, restart=60, max_iters=4000, **opts)
    with _solver(s, tuning, **common) as h:
        assert h.get_int("equil") == (1 if opts.get("equil", 0) > 0 else 0) and h.get_int("precond_steps") == opts.get("precond_steps", 1)
        single = [h.solve(B[c], raise_on_fail=False) for c in range(8)]
        assert all(i["status"] == 0 and i["iters"] > 0 for _, i in single), [i for _, i in single]
        for nrhs in (2, 3, 4, 5):
            before = h.get_int("batch_steps")
            X, infos = h.solve_many(B[:nrhs], raise_on_fail=False)
            assert h.get_int("batch_steps") > before, (key, nrhs, "the call fell back to one solve at a time")
            if nrhs >= 4:
                assert h.get_int("batch_width") == 4
            _assert_column_bits((key, nrhs), X, infos, single, range(nrhs))
    with _solver(s, dict(tuning, rhs_batch=8), **common) as h:
        before = h.get_int("batch_steps")
        X, infos = h.solve_many(B, raise_on_fail=False)
        assert h.get_int("batch_steps") > before and h.get_int("batch_width") == 8
        _assert_column_bits((key, 8), X, infos, single, range(8))
    for c, (x, info) in enumerate(single):
        E = sh.exact(s, x, B[c])
        print(f"{key} rhs {c}: iters {info['iters']} relres {info['relres']:.3e} exact {_norm(E.r) / _norm(B[c]):.3e}")
        assert _norm(E.r) <= 1e-10 * _norm(B[c]) + _norm(E.e), (key, c, info)


# ---------------------------------------------------------------- d. float and coded kernels on real level operators
ML_SELECT = [{}, dict(spmv_variant=0), dict(spmv_variant=9), dict(PIPE, spmv_run=1), dict(PIPE, spmv_run=4), dict(PIPE, spmv_compress=1)]


@pytest.mark.parametrize("f32", [1, 0])
@pytest.mark.parametrize("case", ["small", "tracers2"])
def test_cycle_has_the_same_bits_from_every_spmv_kernel(case, f32):
    """The residuals of every level of the multilevel cycle come from the SpMV kernels (no fused wave or tail kernels here):
    f32-stored level operators with ml_f32 = 1, f64 ones without."""
    cnt = 2 if case == "tracers2" else 1
    if cnt == 2:
        p = synth.generate(imt=40, jmt=46, km=20, adv="upwind3", hmix="isop", coupled_tracer_cnt=2, seed=3)
    else:
        p = synth.generate(imt=24, jmt=20, km=12, adv="upwind3", hmix="isop", seed=0)
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, cnt)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), cnt)
    r = np.random.default_rng(8).standard_normal(p.flat_len)
    got = []
    for sel in ML_SELECT:
        tuning = dict(sel, col_wave_max=0, ml_tail_rows=0, ml_f32=f32, ml_coarsest_rows=400)            # small grids: several levels all the same
        with solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, coupled_tracer_cnt=cnt, col_i=ci, col_j=cj, restart=4, tuning=tuning) as h:
            assert h.get_int("levels") >= 3
            got.append(h.precond_apply(r))
    assert np.all(np.isfinite(got[0])) and np.linalg.norm(got[0]) > 0
    for sel, z in zip(ML_SELECT[1:], got[1:]):
        assert np.array_equal(z, got[0]), (sel, np.abs(z - got[0]).max())


# ---------------------------------------------------------------- e. use_guess
def test_use_guess():
    s = sh.ragged_dd()
    b = sh.solve_rhs(s)[0]
    noise = np.random.default_rng(4).standard_normal(s.n)
    with _solver(s, rtol=1e-10, restart=60, max_iters=4000) as h, _solver(s, rtol=1e-10, max_iters=0) as h0, _Device(b) as db:
        x, info = h.solve(b)
        assert info["iters"] > 0
        # use_guess = 0: what d_x holds is not read
        with _Device(np.full(s.n, np.nan)) as dx:
            got = h.solve_device(db.ptr, dx.ptr, use_guess=False)
            assert got == info and np.array_equal(dx.get(), x)
        # a converged guess: no iteration, x untouched, the residual that the evaluation of x gives
        with _Device(x) as dx:
            again = h.solve_device(db.ptr, dx.ptr, use_guess=True)
            assert again["status"] == 0 and again["iters"] == 0 and np.array_equal(dx.get(), x)
        ev, _ = _evaluate(h0, b, x)
        assert again["relres"] == ev["relres"] == info["relres"] and again["berr"] == ev["berr"]
        E = sh.exact(s, x, b)
        assert abs(again["relres"] * _norm(b) - _norm(E.r)) <= _norm(E.e) + s.n * sh.U * _norm(E.r)
        # a near guess: fewer iterations than from zero, the same tolerance
        with _Device(x + 1e-6 * noise) as dx:
            near = h.solve_device(db.ptr, dx.ptr, use_guess=True)
            x_near = dx.get()
        assert near["status"] == 0 and 0 < near["iters"] < info["iters"] and near["relres"] <= 1e-10, (near, info)
        E = sh.exact(s, x_near, b)
        assert _norm(E.r) <= 1e-10 * _norm(b) + _norm(E.e)


# ---------------------------------------------------------------- f. coded SpMV after a refactor
def test_coded_product_after_refactor(refs):
    R = refs["ragged_dd"]
    s, x0 = R["s"], R["x0"]
    new = sh.refactored_values(s)
    assert not np.array_equal(new, s.val)
    with _solver(s, dict(PIPE, spmv_compress=1)) as h:
        _check_product(h.spmv(x0), R)
        h.refactor(new)
        y = h.spmv(x0)
    _check_product(y, R, y_ora=ora.spmv(s.rowptr, s.colind, new, x0), E=sh.exact(s, x0, val=new))
