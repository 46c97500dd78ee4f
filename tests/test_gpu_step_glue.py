"""Tuning step_glue: what a Krylov step leaves out between its large kernels must leave every stored double as it is.

Every case runs the same matrix through a solver with step_glue = 0 (every launch of its own) and one with the bit(s) under
test, in one process, and compares by np.array_equal:

  bit 4  nkp_precond_apply with the restriction that also zeroes the coarse x and requests a coarse row's fine values together
  bit 8  FGMRES whose Hessenberg column reaches the host from the kernel that completes it, behind an event, and whose next basis
         vector, level-0 right-hand side and level-0 x come from one kernel that is enqueued, with the first column solves,
         before the host waits -- by whole solves: x, iterations, relres, status and berr

and the paths that must not notice the bits: equil, chained cycles, a second Gram-Schmidt pass, the f32 basis, BiCGStab, column
Jacobi, a one-rank row-distributed solver and the batched solve.  (A multi-dot that kept w in LDS measured slower than the grid
of one block per slice and chunk, and the entry kernel alone earned nothing without the early hand-over; bit 1 went with its
tests, bit 2 became part of bit 8: DESIGN.md section 5.)
"""
import ctypes

import numpy as np
import pytest

from nk_ocn_tracer_jacobian_precond_amd import solver, synth

pytestmark = pytest.mark.gpu

# level 0 (about 480 water columns) on the lane-per-column kernels, the levels below it one column per wave, a dense last level
HIERARCHY = dict(ml_coarsest_rows=60, col_wave_max=300, col_ldsres_min=1)
ALL = 12


class System:
    def __init__(self):
        self.p = p = synth.generate(imt=24, jmt=20, km=12, adv="upwind3", hmix="isop", seed=4)
        self.blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
        ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
        self.coords = dict(col_i=ci, col_j=cj)
        rng = np.random.default_rng(23)
        self.b = rng.standard_normal(p.flat_len)
        self.b2 = rng.standard_normal(p.flat_len)

    def solver(self, step_glue, tuning=None, **options):
        p = self.p
        return solver.NkpSolver(p.rowptr, p.colind, p.nzval, self.blk, tuning=dict(HIERARCHY, **(tuning or {}), step_glue=step_glue),
                                **dict(dict(self.coords, precond=solver.PRECOND_MULTILEVEL), **options))


@pytest.fixture(scope="module")
def system():
    return System()


def kernels_of(s):
    """(wave_columns, lane_diag) of every smoothed level, and whether the last level is dense"""
    nlev = s.get_int("levels")
    kinds = []
    for l in range(nlev - 1):
        kinds.append((int(s.ml_level_array(l, "col_kernel")[0]), int(s.ml_level_array(l, "lane_diag")[0])))
    return kinds, s.ml_level_array(nlev - 1, "coarse_inv").size > 0


def test_the_hierarchy_has_the_levels_the_cases_need(system):
    with system.solver(0) as s:
        kinds, dense = kernels_of(s)
        print("levels", s.get_int("levels"), "(wave_columns, lane_diag) per smoothed level", kinds, "dense last", dense)
        assert s.get_int("levels") >= 4 and dense
        assert any(w == 0 for w, _ in kinds) and any(w == 1 for w, _ in kinds)
    with system.solver(0, dict(ml_dense_max=0)) as s:
        assert not kernels_of(s)[1]


def test_default_is_all_bits(monkeypatch):
    monkeypatch.delenv("NKP_STEP_GLUE", raising=False)
    assert solver.default_tuning().step_glue == ALL
    monkeypatch.setenv("NKP_STEP_GLUE", "5")
    assert solver.default_tuning().step_glue == 5


# ================================================================ bit 4: restriction
def test_restriction_meets_short_and_long_coarse_rows(system):
    counts = []
    for tuning in (dict(), dict(ml_huge_from=1)):
        with system.solver(0, tuning) as s:
            for l in range(s.get_int("levels") - 1):
                counts.append(np.diff(s.ml_level_array(l, "rptr")))
    counts = np.concatenate(counts)
    print("fine rows per coarse row: min", counts.min(), "max", counts.max())
    assert counts.min() == 1 and counts.max() > 8


@pytest.mark.parametrize("ml_smooth", [1, 2, 3])
def test_restriction_that_fills_the_coarse_x(system, ml_smooth):
    for f32 in (0, 1):
        for lane in (0, None):
            for wave in (0, 1):
                for extra in (dict(), dict(ml_huge_from=1)):
                    tuning = dict(extra, ml_f32=f32, ml_wave_fused=wave)
                    if lane is not None:
                        tuning["ml_lane_fused"] = lane
                    z = {}
                    for glue in (0, 4):
                        with system.solver(glue, tuning, ml_smooth=ml_smooth, restart=4) as s:
                            z[glue] = s.precond_apply(system.b)
                            z[glue, 2] = s.precond_apply(system.b2)              # a second cycle on the level vectors the first left
                    assert np.isfinite(z[0]).all() and np.abs(z[0]).max() > 0.0
                    assert np.array_equal(z[0], z[4]) and np.array_equal(z[0, 2], z[4, 2]), (ml_smooth, tuning)


def test_restriction_onto_an_iterated_last_level(system):
    z = {}
    for glue in (0, 4, ALL):
        with system.solver(glue, dict(ml_dense_max=0), restart=4) as s:
            z[glue] = s.precond_apply(system.b)
    assert np.array_equal(z[0], z[4]) and np.array_equal(z[0], z[ALL])


# ================================================================ bit 8: whole solves
def bits(v):
    return np.asarray(v, np.float64).tobytes()


def assert_same_solve(a, b, what):
    (xa, ia), (xb, ib) = a, b
    assert np.array_equal(xa, xb, equal_nan=True), (what, np.abs(xa - xb).max())
    assert ia["iters"] == ib["iters"] and ia["status"] == ib["status"], (what, ia, ib)
    assert bits(ia["relres"]) == bits(ib["relres"]) and bits(ia["berr"]) == bits(ib["berr"]), (what, ia, ib)


SOLVES = {
    "default": dict(),
    "restart2": dict(restart=2, max_iters=40),
    "restart3": dict(restart=3, max_iters=40),
    "max_iters1": dict(max_iters=1),
    "max_iters2": dict(max_iters=2),
    "max_iters5": dict(max_iters=5),
    "max_iters5_restart3": dict(max_iters=5, restart=3),
    "one_step": dict(rtol=0.9),
    "iterated_last_level": dict(),
}


@pytest.fixture(scope="module")
def plain_solves(system):
    """the solves with step_glue = 0, once"""
    out = {}
    for name, options in SOLVES.items():
        tuning = dict(ml_dense_max=0) if name == "iterated_last_level" else {}
        with system.solver(0, tuning, **options) as s:
            out[name] = s.solve(system.b, raise_on_fail=False)
            out[name, "zero"] = s.solve(np.zeros_like(system.b), raise_on_fail=False)
    return out


@pytest.mark.parametrize("glue", [8, ALL])
@pytest.mark.parametrize("name", list(SOLVES))
def test_solves_keep_their_bits(system, plain_solves, name, glue):
    tuning = dict(ml_dense_max=0) if name == "iterated_last_level" else {}
    with system.solver(glue, tuning, **SOLVES[name]) as s:
        got = s.solve(system.b, raise_on_fail=False)
        zero = s.solve(np.zeros_like(system.b), raise_on_fail=False)
        again = s.solve(system.b, raise_on_fail=False)              # behind a solve that may have left launches ahead
    ref = plain_solves[name]
    print(name, glue, got[1])
    if name == "default":
        assert ref[1]["status"] == 0 and ref[1]["iters"] > 5
    if name == "one_step":
        assert ref[1]["status"] == 0 and ref[1]["iters"] == 1
    if name.startswith("max_iters"):
        assert ref[1]["iters"] == SOLVES[name]["max_iters"]
    if name.startswith("restart"):
        assert ref[1]["iters"] > 2 * SOLVES[name]["restart"]        # several restart cycles
    assert_same_solve(ref, got, (name, glue))
    assert_same_solve(ref, again, (name, glue, "repeated"))
    assert_same_solve(plain_solves[name, "zero"], zero, (name, glue, "b = 0"))
    assert not zero[0].any() and zero[1]["iters"] == 0


def test_a_handle_solves_one_system_after_another(system):
    with system.solver(0) as s:
        ref = [s.solve(b) for b in (system.b, system.b2)]
    with system.solver(ALL, max_iters=3) as short, system.solver(ALL) as s:
        short.solve(system.b, raise_on_fail=False)                  # ends with the start of a cycle enqueued ahead
        after_short = short.precond_apply(system.b2)
        got = [s.solve(b) for b in (system.b, system.b2, system.b)]
        z = s.precond_apply(system.b2)
        c = s.clone()
        cloned = c.solve(system.b2)
        c.close()
    with system.solver(0) as s:
        z_ref = s.precond_apply(system.b2)
    assert_same_solve(ref[0], got[0], "first")
    assert_same_solve(ref[1], got[1], "second")
    assert_same_solve(ref[0], got[2], "first again")
    assert_same_solve(ref[1], cloned, "clone")
    assert np.array_equal(z, z_ref) and np.array_equal(after_short, z_ref)


def test_timing_entry_runs_the_step(system):
    with system.solver(ALL, restart=8) as s:
        for j in (0, 3, 7):
            assert s.time_kernel(2, reps=2, arg=j) > 0.0
        assert s.time_kernel(1, reps=2) > 0.0
        x, info = s.solve(system.b)                                 # and leaves nothing behind that a solve would notice
    with system.solver(0, restart=8) as s:
        assert s.time_kernel(2, reps=2, arg=7) > 0.0
        assert_same_solve(s.solve(system.b), (x, info), "after time_kernel")


# ================================================================ paths that must ignore the bits
IGNORING = {
    "equil": dict(equil=1),
    "precond_steps2": dict(precond_steps=2),
    "reorth": dict(reorth=1),
    "basis_f32": dict(basis_f32=1),
    "bicgstab": dict(krylov=solver.KRYLOV_BICGSTAB),
    "column_jacobi": dict(precond=solver.PRECOND_COLUMN_JACOBI, max_iters=40),
}


@pytest.mark.parametrize("name", list(IGNORING))
def test_other_paths_keep_their_bits(system, name):
    out = {}
    for glue in (0, ALL):
        with system.solver(glue, **IGNORING[name]) as s:
            out[glue] = s.solve(system.b, raise_on_fail=False)
    print(name, out[0][1])
    assert out[0][1]["iters"] > 0
    assert_same_solve(out[0], out[ALL], name)


def test_one_rank_row_distributed(system, tmp_path):
    p = system.p
    lib = solver.load_library()
    lib.nkp_comm_file_init.argtypes = [ctypes.POINTER(solver.NkpCommOps), ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    lib.nkp_comm_file_free.argtypes = [ctypes.POINTER(solver.NkpCommOps)]
    lib.nkp_comm_file_free.restype = None
    rp = np.ascontiguousarray(p.rowptr, np.int32)
    ci = np.ascontiguousarray(p.colind, np.int32)
    v = np.ascontiguousarray(p.nzval, np.float64)
    blk = np.ascontiguousarray(system.blk, np.int32)
    n = p.flat_len
    out = {}
    for glue in (0, ALL):
        ops = solver.NkpCommOps()
        d = tmp_path / str(glue)
        d.mkdir()
        assert lib.nkp_comm_file_init(ctypes.byref(ops), str(d).encode(), 0, 1) == 0
        opt = solver.default_options(precond=solver.PRECOND_MULTILEVEL)
        tun = solver.default_tuning(**dict(HIERARCHY, force_dist=1, step_glue=glue))
        opt.tuning = ctypes.pointer(tun)
        h = ctypes.c_void_p()
        rc = lib.nkp_create_dist(ctypes.byref(h), ctypes.byref(opt), n, 0, n, ci.size, solver._p(rp, ctypes.c_int32), solver._p(ci, ctypes.c_int32),
                                 solver._p(v, ctypes.c_double), solver._p(blk, ctypes.c_int32), blk.size - 1, 1, ctypes.byref(ops))
        assert rc == 0, lib.nkp_last_error().decode()
        s = solver.NkpSolver._from_handle(lib, h, n, ci.size, opt)
        try:
            out[glue] = s.solve(system.b)
        finally:
            s.close()
            lib.nkp_comm_file_free(ctypes.byref(ops))
    assert out[0][1]["iters"] > 0
    assert_same_solve(out[0], out[ALL], "force_dist")


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
        return X, infos

    def close(self):
        self.hip.hipFree(self.b)
        self.hip.hipFree(self.x)


def test_batched_solve_against_its_single_solves(system):
    B = np.stack([system.b, system.b2])
    dv = DeviceVectors(B)
    try:
        with system.solver(0) as s:
            singles = [s.solve(b) for b in B]
            X0, infos0 = dv.solve(s)
        with system.solver(ALL) as s:
            X, infos = dv.solve(s)
            assert s.get_int("batch_width") == 2
            after = s.solve(system.b)                                # the single driver behind the batched one, same handle
    finally:
        dv.close()
    for c in range(2):
        assert_same_solve(singles[c], (X[c], infos[c]), ("batched", c))
        assert_same_solve((X0[c], infos0[c]), (X[c], infos[c]), ("batched, both settings", c))
    assert_same_solve(singles[0], after, "single after batched")
