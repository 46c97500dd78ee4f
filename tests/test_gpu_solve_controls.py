"""rtol, atol and max_iters after creation (nkp_set_solve_controls) and per column with initial guesses
(nkp_solve_batch_device_ex).  Every comparison is exact equality of bits against a second solver created with the values in its
nkp_options, so the yardstick is nkp_create's own path and no tolerance is chosen anywhere.

Shapes: synth.generate (12, 10, km), km 6 and 10 (n = 340 and 525), upwind3 + isop; ml_coarsest_rows = 40 gives the hierarchy
several levels, restart = 5 sends every solve through restarts."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from nk_ocn_tracer_jacobian_precond_amd import solver, synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL, NOT_CONVERGED, BREAKDOWN = -1, solver.NKP_NOT_CONVERGED, solver.NKP_BREAKDOWN
BASE = dict(restart=5, rtol=1e-10, atol=0.0, max_iters=300)
TUNING = dict(ml_coarsest_rows=40)
ML, JACOBI = solver.PRECOND_MULTILEVEL, solver.PRECOND_COLUMN_JACOBI
CONFIGS = {
    "multilevel": (10, dict(precond=ML)),
    "jacobi": (6, dict(precond=JACOBI)),
    "bicgstab": (6, dict(precond=ML, krylov=solver.KRYLOV_BICGSTAB)),
    "equil": (10, dict(precond=ML, equil=1)),
    "steps2": (6, dict(precond=ML, precond_steps=2)),
    "basis_f32": (10, dict(precond=ML, basis_f32=1)),
}
# (rtol, atol as a multiple of ||b_0||, max_iters); None = keep what the solver was created with
VALUES = {"loose": (1e-3, 0.0, None), "tight": (1e-12, 0.0, None), "absolute": (0.0, 1e-6, None), "three_iterations": (1e-10, 0.0, 3)}


class Dev:
    """float64 host array on the device, through the HIP runtime the library links"""

    def __init__(self, a):
        a = np.ascontiguousarray(a, np.float64)
        self.shape, self.nbytes, self._bufs = a.shape, a.nbytes, []
        self.ptr = solver._device_array(self._bufs, a)

    def get(self):
        out = np.empty(self.shape)
        solver._hip_check(solver._hip().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(self.ptr), C.c_size_t(self.nbytes), 2))
        return out

    def put(self, a):
        a = np.ascontiguousarray(a, np.float64)
        solver._hip_check(solver._hip().hipMemcpy(C.c_void_p(self.ptr), C.c_void_p(a.ctypes.data), C.c_size_t(self.nbytes), 1))

    def free(self):
        for q in self._bufs:
            solver._hip().hipFree(C.c_void_p(q))
        self._bufs = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


_PROBLEMS = {}


def problem(km):
    if km not in _PROBLEMS:
        p = synth.generate(imt=12, jmt=10, km=km, adv="upwind3", hmix="isop", seed=36)
        blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
        ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
        B = np.random.default_rng(20 + km).standard_normal((5, p.flat_len))
        B[2] *= 1e-3                                        # the systems of a group end at different steps
        _PROBLEMS[km] = (p, blk, ci, cj, B)
    return _PROBLEMS[km]


def make(km, tuning=None, val=None, **opts):
    p, blk, ci, cj, _ = problem(km)
    kw = dict(BASE, **opts)
    if kw.get("precond", ML) == ML:
        kw.update(col_i=ci, col_j=cj)
    return solver.NkpSolver(p.rowptr, p.colind, p.nzval if val is None else val, blk, tuning=dict(TUNING, **(tuning or {})), **kw)


def bits(info):
    """the numbers of an info dict as bytes: NaN compares equal to the same NaN"""
    return (info["status"], info["iters"], np.array([info["relres"], info["berr"]]).tobytes())


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and [bits(i) for i in a[1]] == [bits(i) for i in b[1]]


def every_call(s, B):
    """nkp_solve, nkp_solve_device, nkp_solve_batch_device with 3 and 5 right-hand sides: [(x, [info, ...]), ...]"""
    n = B.shape[1]
    x, info = s.solve(B[0], raise_on_fail=False)
    out = [(x, [info])]
    with Dev(B[1]) as d_b, Dev(np.zeros(n)) as d_x:
        info = s.solve_device(d_b.ptr, d_x.ptr, raise_on_fail=False)
        out.append((d_x.get(), [info]))
    for nrhs in (3, 5):
        with Dev(B[:nrhs]) as d_b, Dev(np.zeros((nrhs, n))) as d_x:
            infos = s.solve_batch_device(d_b.ptr, d_x.ptr, nrhs, n, raise_on_fail=False)
            out.append((d_x.get(), infos))
    return out


def resolved(name, B):
    rtol, atol_rel, max_iters = VALUES[name]
    return rtol, atol_rel * float(np.linalg.norm(B[0])), max_iters


# ---------------------------------------------------------------- 1: the setter against nkp_create with the same values
@pytest.mark.parametrize("values", list(VALUES))
@pytest.mark.parametrize("config", list(CONFIGS))
def test_setter_gives_the_bits_of_a_solver_created_with_the_values(config, values):
    km, opts = CONFIGS[config]
    B = problem(km)[4]
    rtol, atol, max_iters = resolved(values, B)
    created = dict(rtol=rtol, atol=atol, **({} if max_iters is None else dict(max_iters=max_iters)))
    with make(km, **opts) as s, make(km, **dict(opts, **created)) as t:
        if opts["precond"] == ML:
            assert s.get_int("levels") >= 3
        s.set_solve_controls(rtol=rtol, atol=atol, max_iters=max_iters)
        want = dict(rtol=rtol, atol=atol, max_iters=BASE["max_iters"] if max_iters is None else max_iters)
        assert s.get_solve_controls() == want == t.get_solve_controls()
        assert s.get_int("max_iters") == want["max_iters"]
        got, ref = every_call(s, B), every_call(t, B)
        for call, (g, r) in enumerate(zip(got, ref)):
            print(config, values, call, [(i["status"], i["iters"], i["relres"]) for i in r[1]])
            assert same(g, r), (config, values, call, g[1], r[1])
        if values == "three_iterations":
            assert ref[0][1][0]["status"] == NOT_CONVERGED and ref[0][1][0]["iters"] == 3, ref[0][1]
        # a loose and a tight tolerance are different solves: the setter is not a no-op
        if config == "multilevel" and values in ("loose", "tight"):
            with make(km, **opts) as u:
                assert not same(every_call(u, B)[0], ref[0])


# ---------------------------------------------------------------- 2, 3: reset; invalid values change nothing
def test_reset_gives_back_the_bits_of_an_untouched_solver():
    km, opts = CONFIGS["multilevel"]
    B = problem(km)[4]
    with make(km, **opts) as s, make(km, **opts) as u:
        ref = every_call(u, B)
        s.set_solve_controls(rtol=1e-3, atol=1e-9, max_iters=7)
        assert not same(every_call(s, B)[0], ref[0])
        s.reset_solve_controls()
        assert s.get_solve_controls() == dict(rtol=BASE["rtol"], atol=BASE["atol"], max_iters=BASE["max_iters"])
        for g, r in zip(every_call(s, B), ref):
            assert same(g, r)


def test_invalid_values_are_refused_and_change_nothing():
    km, opts = CONFIGS["multilevel"]
    B = problem(km)[4]
    lib = solver.load_library()
    size = C.sizeof(solver.NkpSolveControls)
    with make(km, **opts) as s:
        s.set_solve_controls(rtol=1e-6)
        before, ref = s.get_solve_controls(), every_call(s, B)
        for c in (solver.NkpSolveControls(size, 0, float("nan"), -1.0), solver.NkpSolveControls(size, 0, -1.0, float("nan")),
                  solver.NkpSolveControls(size, 0, float("inf"), -1.0), solver.NkpSolveControls(size, 0, 1e-3, float("inf")),
                  solver.NkpSolveControls(size, 0, float("-inf"), -1.0), solver.NkpSolveControls(size + 8, 5, 1e-3, 1e-3),
                  solver.NkpSolveControls(0, 5, 1e-3, 1e-3), solver.NkpSolveControls(size, -1, 1e-3, 1e-3)):
            assert lib.nkp_set_solve_controls(s._h, C.byref(c)) == EINVAL, (c.struct_size, c.max_iters, c.rtol, c.atol)
            assert "nkp_set_solve_controls" in solver.last_error() and "nothing changed" in solver.last_error()
            assert s.get_solve_controls() == before
        for g, r in zip(every_call(s, B), ref):
            assert same(g, r)


# ---------------------------------------------------------------- 4, 5, 6: per-column controls and guesses
RTOL5 = [1e-3, 1e-10, 1e-6, 1e-12, 1e-4]
GUESS5 = [1, 0, 1, 0, 1]


@pytest.fixture(scope="module")
def columns():
    """the five systems of case 4 solved alone, each on a solver SET to its column's controls, from its column's guess; made once
    and left unchanged"""
    km, opts = CONFIGS["multilevel"]
    p, _, _, _, B = problem(km)
    n = p.flat_len
    xi = np.random.default_rng(77).standard_normal((5, n))
    with make(km, **opts) as r:
        r.set_solve_controls(rtol=1e-12)
        exact = np.stack([r.solve(B[c])[0] for c in range(5)])
        X0 = np.where(np.array(GUESS5)[:, None] != 0, exact * (1.0 + 1e-3 * xi), 0.0)
        single = []
        for c in range(5):
            r.set_solve_controls(rtol=RTOL5[c])
            with Dev(B[c]) as d_b, Dev(X0[c]) as d_x:
                info = r.solve_device(d_b.ptr, d_x.ptr, use_guess=bool(GUESS5[c]), raise_on_fail=False)
                single.append((d_x.get(), info))
        # the guesses matter: a warm start is another solve than a cold one
        r.set_solve_controls(rtol=RTOL5[2])
        cold = r.solve(B[2])
        assert cold[0].tobytes() != single[2][0].tobytes() and cold[1]["status"] == single[2][1]["status"] == 0, (cold[1], single[2][1])
    return dict(km=km, opts=opts, B=B, X0=X0, single=single, n=n)


def run_ex(s, B, X0, raise_on_fail=False, **kw):
    nrhs, n = B.shape
    with Dev(B) as d_b, Dev(X0) as d_x:
        infos = s.solve_batch_device_ex(d_b.ptr, d_x.ptr, nrhs, n, raise_on_fail=raise_on_fail, **kw)
        return d_x.get(), infos, d_b.get()


def assert_columns(X, infos, single, cols, status=None):
    for q, c in enumerate(cols):
        x1, i1 = single[c]
        assert (infos[q]["iters"], np.array([infos[q]["relres"], infos[q]["berr"]]).tobytes()) == bits(i1)[1:], (c, infos[q], i1)
        assert X[q].tobytes() == x1.tobytes(), (c, np.abs(X[q] - x1).max())
    if status is not None:
        assert infos[0]["status"] == status


@pytest.mark.parametrize("path", ["batched", "rhs_batch0", "clone"])
def test_ex_columns_have_the_bits_of_their_single_solves(columns, path):
    k = columns
    with make(k["km"], tuning=dict(rhs_batch=0) if path == "rhs_batch0" else None, **k["opts"]) as owner:
        s = owner.clone() if path == "clone" else owner
        try:
            own = s.get_solve_controls()
            for nrhs in (5, 2):                               # a group of four and a single column; a pair
                steps = owner.get_int("batch_steps")
                X, infos, Bback = run_ex(s, k["B"][:nrhs], k["X0"][:nrhs], rtol=RTOL5[:nrhs], use_guess=GUESS5[:nrhs])
                assert_columns(X, infos, k["single"], range(nrhs), status=0)
                assert np.array_equal(Bback, k["B"][:nrhs])
                assert (owner.get_int("batch_steps") > steps) == (path == "batched")
                assert s.get_solve_controls() == own          # the columns' values are gone when the call returns
            # the converged iteration counts follow the tolerances, so the per-column values were read
            assert len({i[1]["iters"] for i in k["single"]}) > 1, [i[1] for i in k["single"]]
        finally:
            if s is not owner:
                s.close()


@pytest.mark.parametrize("config", ["bicgstab", "basis_f32", "equil", "steps2", "jacobi"])
def test_ex_under_the_other_configurations(config):
    """the fallbacks that are properties of the solver (BiCGStab, an f32 basis: one at a time) and the batched path under row
    equilibration, chained cycles and column Jacobi: columns 0 .. 4 against their single solves on a second solver"""
    km, opts = CONFIGS[config]
    p, _, _, _, B = problem(km)
    xi = np.random.default_rng(78).standard_normal(B.shape)
    with make(km, **opts) as s, make(km, **opts) as r:
        r.set_solve_controls(rtol=1e-12)
        exact = np.stack([r.solve(B[c], raise_on_fail=False)[0] for c in range(5)])
        X0 = np.where(np.array(GUESS5)[:, None] != 0, exact * (1.0 + 1e-3 * xi), 0.0)
        single = []
        for c in range(5):
            r.set_solve_controls(rtol=RTOL5[c])
            with Dev(B[c]) as d_b, Dev(X0[c]) as d_x:
                info = r.solve_device(d_b.ptr, d_x.ptr, use_guess=bool(GUESS5[c]), raise_on_fail=False)
                single.append((d_x.get(), info))
        steps = s.get_int("batch_steps")
        X, infos, _ = run_ex(s, B, X0, rtol=RTOL5, use_guess=GUESS5)
        print(config, [(i[1]["status"], i[1]["iters"]) for i in single])
        assert_columns(X, infos, single, range(5))
        assert (s.get_int("batch_steps") > steps) == (config in ("equil", "steps2", "jacobi"))
        assert s.get_solve_controls() == dict(rtol=BASE["rtol"], atol=BASE["atol"], max_iters=BASE["max_iters"])


def test_ex_arrays_of_every_kind_and_the_worst_status(columns):
    """max_iters and atol per column, "leave as it is" entries and NULL arrays; the return code is the worst column's; the
    host convenience solve_many stages the same call"""
    k = columns
    B, n = k["B"], k["n"]
    nb = float(np.linalg.norm(B[1]))
    with make(k["km"], **k["opts"]) as s, make(k["km"], **k["opts"]) as r:
        s.set_solve_controls(rtol=1e-8)
        want = []
        for c, (rt, at, mi) in enumerate([(1e-8, 0.0, 300), (0.0, 1e-5 * nb, 300), (1e-8, 0.0, 3)]):
            r.set_solve_controls(rtol=rt, atol=at, max_iters=mi)
            want.append(r.solve(B[c], raise_on_fail=False))
        X, infos = s.solve_many(B[:3], raise_on_fail=False, rtol=[None, 0.0, -1.0], atol=[None, 1e-5 * nb, None], max_iters=[0, None, 3])
        assert [i["status"] for i in infos] == [NOT_CONVERGED] * 3 and want[2][1]["status"] == NOT_CONVERGED and want[0][1]["status"] == 0
        assert_columns(X, infos, want, range(3))
        assert s.get_solve_controls() == dict(rtol=1e-8, atol=0.0, max_iters=300)
        # no arrays at all: nkp_solve_batch_device
        X, infos, _ = run_ex(s, B[:3], np.zeros((3, n)))
        with Dev(B[:3]) as d_b, Dev(np.zeros((3, n))) as d_x:
            plain = s.solve_batch_device(d_b.ptr, d_x.ptr, 3, n)
            assert X.tobytes() == d_x.get().tobytes() and [bits(i) for i in infos] == [bits(i) for i in plain]


def test_ex_nan_guess_is_that_columns_breakdown(columns):
    """column 2 of the group of four starts from a guess with one NaN: NKP_BREAKDOWN as nkp_solve_device gives it alone (iters 0,
    relres NaN, berr NaN, x as it was passed -- nothing iterates on a residual that is not a number), the others as in case 4"""
    k = columns
    X0 = k["X0"].copy()
    X0[2, k["n"] // 2] = np.nan
    with make(k["km"], **k["opts"]) as s:
        s.set_solve_controls(rtol=RTOL5[2])
        with Dev(k["B"][2]) as d_b, Dev(X0[2]) as d_x:
            alone = s.solve_device(d_b.ptr, d_x.ptr, use_guess=True, raise_on_fail=False)
            x_alone = d_x.get()
        s.reset_solve_controls()
        assert alone["status"] == BREAKDOWN and alone["iters"] == 0 and np.isnan(alone["relres"]) and np.isnan(alone["berr"])
        X, infos, _ = run_ex(s, k["B"], X0, rtol=RTOL5, use_guess=GUESS5)
        assert infos[0]["status"] == BREAKDOWN                 # the worst of the columns'
        assert infos[2]["iters"] == 0 and np.isnan(infos[2]["relres"]) and np.isnan(infos[2]["berr"]), infos[2]
        assert X[2].tobytes() == x_alone.tobytes() and np.isnan(X[2]).any()
        assert_columns(X[[0, 1, 3, 4]], [infos[c] for c in (0, 1, 3, 4)], k["single"], (0, 1, 3, 4))


def test_ex_refuses_a_guess_in_the_right_hand_sides_own_memory(columns):
    k = columns
    B, n = k["B"][:2], k["n"]
    lib = solver.load_library()
    with make(k["km"], **k["opts"]) as s, Dev(B) as d:
        flags, tol = (C.c_int * 2)(0, 1), (C.c_double * 2)(1e-3, 1e-3)
        steps = s.get_int("batch_steps")
        rc = lib.nkp_solve_batch_device_ex(s._h, 2, C.c_void_p(d.ptr), C.c_void_p(d.ptr), n, tol, None, None, flags, None, None, None)
        assert rc == EINVAL and "d_X == d_B" in solver.last_error() and "use_guess[1]" in solver.last_error()
        assert np.array_equal(d.get(), B) and s.get_int("batch_steps") == steps
        with Dev(np.zeros((2, n))) as d_x:
            for bad, text in (((C.c_double * 2)(1e-3, float("nan")), "rtol[1]"), ((C.c_double * 2)(float("inf"), 1e-3), "rtol[0]")):
                assert lib.nkp_solve_batch_device_ex(s._h, 2, C.c_void_p(d.ptr), C.c_void_p(d_x.ptr), n, bad, None, None, None, None, None, None) == EINVAL
                assert text in solver.last_error()
            assert lib.nkp_solve_batch_device_ex(s._h, 2, C.c_void_p(d.ptr), C.c_void_p(d_x.ptr), n, None, bad, None, None, None, None, None) == EINVAL
            assert "atol[0]" in solver.last_error()
            assert lib.nkp_solve_batch_device_ex(s._h, 2, C.c_void_p(d.ptr), C.c_void_p(d_x.ptr), n, None, None, (C.c_int * 2)(4, -1), None, None, None, None) == EINVAL
            assert "max_iters[1]" in solver.last_error()
            assert lib.nkp_solve_batch_device_ex(s._h, 2, C.c_void_p(d.ptr), C.c_void_p(d_x.ptr), n - 1, None, None, None, None, None, None, None) == EINVAL
            assert "ldb" in solver.last_error()
            assert not d_x.get().any() and s.get_int("batch_steps") == steps
        # without a guess flag the solutions may overwrite the right-hand sides, as in nkp_solve_batch_device
        flags = (C.c_int * 2)(0, 0)
        assert lib.nkp_solve_batch_device_ex(s._h, 2, C.c_void_p(d.ptr), C.c_void_p(d.ptr), n, tol, None, None, flags, None, None, None) == 0
        assert not np.array_equal(d.get(), B)


# ---------------------------------------------------------------- 7: the controls belong to the handle
def test_controls_belong_to_the_handle():
    km, opts = CONFIGS["multilevel"]
    p, _, _, _, B = problem(km)
    n = p.flat_len
    created = dict(rtol=BASE["rtol"], atol=BASE["atol"], max_iters=BASE["max_iters"])
    first = dict(rtol=1e-4, atol=0.0, max_iters=50)
    second = dict(rtol=1e-7, atol=1e-30, max_iters=60)
    with make(km, **opts) as s:
        c0, t0 = s.clone(), s.transposed()
        s.set_solve_controls(**first)
        assert c0.get_solve_controls() == created and t0.get_solve_controls() == created      # nothing propagates
        c1 = s.clone()
        t0.close()
        t1 = s.transposed()
        assert c1.get_solve_controls() == first and t1.get_solve_controls() == first          # a new handle starts with its source's
        s.set_solve_controls(**second)
        c1.set_solve_controls(max_iters=9)
        assert s.get_solve_controls() == second and c0.get_solve_controls() == created and t1.get_solve_controls() == first
        assert c1.get_solve_controls() == dict(first, max_iters=9)
        t1.reset_solve_controls()
        assert t1.get_solve_controls() == first                # what the handle began with
        t1.set_solve_controls(rtol=1e-5)
        # each handle solves at its own values: the bits of solvers created with them
        with make(km, **dict(opts, **dict(first, max_iters=9))) as r:
            for g, w in zip(every_call(c1, B), every_call(r, B)):
                assert same(g, w)
        c0.close()
        c1.close()
        # a refactor keeps them, on the owner and on the transposed handle that follows it
        with Dev(p.nzval * 1.01) as d_val:
            for rebuild in (False, True):
                s.refactor_device(d_val.ptr, rebuild=rebuild)
                assert s.get_int("refactor_rebuilt") == int(rebuild)
                assert s.get_solve_controls() == second and t1.get_solve_controls() == dict(first, rtol=1e-5)
        with make(km, val=p.nzval * 1.01, **dict(opts, **second)) as r:
            for g, w in zip(every_call(s, B), every_call(r, B)):
                assert same(g, w)


def test_tangent_solve_runs_at_the_set_values():
    km, opts = CONFIGS["multilevel"]
    p, _, _, _, B = problem(km)
    n, nrhs = p.flat_len, 3
    rng = np.random.default_rng(5)
    dval = 0.01 * p.nzval * rng.standard_normal(p.nzval.size)
    dB = rng.standard_normal((nrhs, n))
    with make(km, **opts) as s, make(km, **dict(opts, rtol=1e-4)) as t:
        X = np.stack([s.solve(B[c])[0] for c in range(nrhs)])
        default = s.solve_tangent(X, dval=dval, dB=dB)
        s.set_solve_controls(rtol=1e-4)
        got, want = s.solve_tangent(X, dval=dval, dB=dB), t.solve_tangent(X, dval=dval, dB=dB)
        assert same(got, want) and not same(got, default)
        # its iterations are those of nkp_solve_batch_device on its own R = dB - dA X
        with Dev(dval) as d_v, Dev(X) as d_x, Dev(dB) as d_r, Dev(np.zeros((nrhs, n))) as d_o:
            s.values_product_device(d_v.ptr, d_x.ptr, nrhs, n, d_r.ptr, n, alpha=-1.0, accumulate=True)
            infos = s.solve_batch_device(d_r.ptr, d_o.ptr, nrhs, n)
            assert [i["iters"] for i in infos] == [i["iters"] for i in got[1]] and d_o.get().tobytes() == got[0].tobytes()
        assert max(i["iters"] for i in got[1]) < min(i["iters"] for i in default[1])


# ---------------------------------------------------------------- 8: the torch wrapper
def test_torch_solver_sets_forward_and_transposed_handle(tmp_path):
    """torch runs in a process of its own (it brings its own HIP runtime along): tests/torch_solve_controls_worker.py"""
    out = str(tmp_path / "torch.json")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(HERE, "torch_solve_controls_worker.py"), "--out", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.load(open(out))
    want = dict(res["created"], rtol=1e-5, max_iters=77)
    assert res["created"] == dict(rtol=BASE["rtol"], atol=BASE["atol"], max_iters=BASE["max_iters"])
    assert res["before_backward"] == dict(forward=want, transposed=None)
    assert res["after_backward"] == dict(forward=want, transposed=want)
    assert res["grad_equal"] and res["grad_differs_from_default"], res
    want = dict(want, atol=1e-20)
    assert res["after_second_set"] == dict(forward=want, transposed=want)
