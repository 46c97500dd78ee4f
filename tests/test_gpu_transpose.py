"""nkp_transpose: the solver for A^T made from the matrix a solver holds on the device is bit for bit the solver nkp_create
builds from the host transpose (scipy: csr_matrix(...).T.tocsr() + sort_indices()) -- matrix, hierarchy, solves, batched solves --
it follows the refactors of its source, and it is owned by it."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from nk_ocn_tracer_jacobian_precond_amd import dist, nc3, solver, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nk_ocn_tracer_jacobian_precond_amd", "bin")
ARRAYS = ("rowptr", "colind", "valf", "val", "cmap", "rptr", "ridx", "blk_start", "fac", "perm0", "coarse_inv")
GRID = (40, 46, 20)


@pytest.fixture(autouse=True)
def _small_levels(monkeypatch):
    monkeypatch.setenv("NKP_ML_DEVICE_MIN", "0")
    monkeypatch.setenv("NKP_ML_COARSEST_ROWS", "300")


def _transpose(rowptr, colind, val):
    """the reference A^T, and the position in val of every one of its entries"""
    n = len(rowptr) - 1
    T = sp.csr_matrix((val, colind, rowptr), shape=(n, n)).T.tocsr()
    T.sort_indices()
    I = sp.csr_matrix((np.arange(1, len(colind) + 1, dtype=np.float64), colind, rowptr), shape=(n, n)).T.tocsr()
    I.sort_indices()
    src = I.data.astype(np.int64) - 1
    assert np.array_equal(T.indptr, I.indptr) and np.array_equal(T.indices, I.indices) and np.array_equal(T.data, np.asarray(val)[src])
    return T, src


def _gen(**kw):
    a = dict(adv="upwind3", hmix="isop", seed=2, u_scale=3.0, ah=4.0e6, isop_k33=True)
    a.update(kw)
    return synth.generate(imt=GRID[0], jmt=GRID[1], km=GRID[2], **a)


@pytest.fixture(scope="module")
def probs():
    p = _gen()
    same = _gen(day_cnt=180.0)
    differ = _gen(vdc_bg=100.0)
    for q in (same, differ):
        assert np.array_equal(p.rowptr, q.rowptr) and np.array_equal(p.colind, q.colind)
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    T, src = _transpose(p.rowptr, p.colind, p.nzval)
    return dict(rowptr=p.rowptr, colind=p.colind, val=p.nzval, same=same.nzval, differ=differ.nzval, blk=blk, ci=ci, cj=cj, cnt=1, T=T, src=src, n=p.flat_len)


def _golden_prob(g):
    ci, cj = solver.column_coords(g.ind_i, g.ind_j, g.col_start, g.cnt)
    T, src = _transpose(g.rowptr, g.colind, g.val)
    return dict(rowptr=g.rowptr, colind=g.colind, val=g.val, blk=g.blk_start, ci=ci, cj=cj, cnt=g.cnt, T=T, src=src, n=g.n)


def _forward(P, val=None, **kw):
    return solver.NkpSolver(P["rowptr"], P["colind"], P["val"] if val is None else val, P["blk"], P["cnt"], col_i=P["ci"], col_j=P["cj"], **kw)


def _reference(P, val=None, **kw):
    """nkp_create on the host transpose, same options: never the code under test"""
    T = P["T"]
    return solver.NkpSolver(T.indptr, T.indices, T.data if val is None else np.asarray(val)[P["src"]], P["blk"], P["cnt"], col_i=P["ci"], col_j=P["cj"], **kw)


def _arrays(s):
    return [{a: s.ml_level_array(l, a) for a in ARRAYS} for l in range(s.get_int("levels"))]


def _assert_same_hierarchy(s, t):
    ha, hb = _arrays(s), _arrays(t)
    assert len(ha) == len(hb)
    for l, (a, b) in enumerate(zip(ha, hb)):
        for name in ARRAYS:
            assert a[name].shape == b[name].shape, (l, name)
            assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), f"level {l}: {name} differs"


def _rhs(P, k=0):
    return np.random.default_rng(11 + k).standard_normal(P["n"])


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _assert_same_solves(t, u, P, batch=True):
    b = _rhs(P)
    assert _bits(t.spmv(b), u.spmv(b))
    assert _bits(t.precond_apply(b), u.precond_apply(b))
    xt, it = t.solve(b)
    xu, iu = u.solve(b)
    assert _bits(xt, xu) and it["iters"] == iu["iters"] and it["relres"] == iu["relres"]
    if batch:
        B = np.stack([_rhs(P, k) for k in range(4)])
        Xt, _ = t.solve_many(B)
        Xu, _ = u.solve_many(B)
        assert _bits(Xt, Xu)
    return xt, it


def _assert_same_solver(t, u, P, multilevel=True, batch=True):
    assert t.get_int("n") == u.get_int("n") and t.get_int("nnz") == u.get_int("nnz")
    if multilevel:
        _assert_same_hierarchy(t, u)
    return _assert_same_solves(t, u, P, batch)


# ---------------------------------------------------------------- 1. the transpose kernels alone
def test_transpose_kernel_random_matrix():
    """n = 1003, unsorted duplicate-free rows of mixed lengths (one empty, some longer than a wave), column 5 with 700 entries
    (a 700-entry row of A^T), column 17 empty"""
    n, rng = 1003, np.random.default_rng(5)
    lengths = rng.choice([1, 2, 3, 7, 20, 33, 64, 65, 150], size=n)
    lengths[400] = 0
    long_rows = set(rng.choice(n, size=700, replace=False).tolist())
    rows = []
    for r in range(n):
        c = rng.choice(n, size=lengths[r], replace=False)
        c = c[(c != 5) & (c != 17)]
        if r in long_rows:
            c = np.append(c, 5)
        rows.append(rng.permutation(c))
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int32)
    colind = np.concatenate(rows).astype(np.int32)
    val = rng.standard_normal(colind.size)
    assert any(np.any(np.diff(c) < 0) for c in rows)                 # rows of A are not sorted
    T, _ = _transpose(rowptr, colind, val)
    assert np.diff(T.indptr)[5] == 700 and np.diff(T.indptr)[17] == 0
    with solver.NkpSolver(rowptr, colind, val, None, precond=solver.PRECOND_NONE) as s, \
            solver.NkpSolver(T.indptr, T.indices, T.data, None, precond=solver.PRECOND_NONE) as u:
        t = s.transposed()
        assert (t.n, t.nnz) == (u.n, u.nnz)
        assert t.get_int("n") == u.get_int("n") == n and t.get_int("nnz") == u.get_int("nnz") == colind.size
        assert t.get_int("is_transpose") == 1 and s.get_int("is_transpose") == 0 and u.get_int("is_transpose") == 0
        for k in range(2):
            x = rng.standard_normal(n)
            y = t.spmv(x)
            assert _bits(y, u.spmv(x))
            ref = T @ x
            assert np.linalg.norm(y - ref) <= 1e-13 * np.linalg.norm(ref)
        t2 = s.transposed()
        assert t2 is t and t2._h.value == t._h.value
        h = ctypes.c_void_p()
        assert s._lib.nkp_transpose(s._h, ctypes.byref(h)) == 0 and h.value == t._h.value
        assert s.get_int("trans_us") > 0 and 0 < s.get_int("trans_kernel_us") <= s.get_int("trans_us")


# ---------------------------------------------------------------- 2. bit identity with a fresh create of A^T
@pytest.mark.parametrize("case", ["multilevel", "column", "equil", "pair"])
def test_bitwise_equal_to_create_of_host_transpose(case, probs, golden_by_name):
    P = _golden_prob(golden_by_name("pair_8x8x5")) if case == "pair" else probs
    opts = dict(column=dict(precond=solver.PRECOND_COLUMN_JACOBI), equil=dict(equil=1)).get(case, {})
    multilevel = case != "column"
    b = _rhs(P)
    s = _forward(P, **opts)
    x0, i0 = s.solve(b)
    bytes0 = s.get_int("device_bytes")
    t = s.transposed()
    u = _reference(P, **opts)
    x, info = _assert_same_solver(t, u, P, multilevel)
    res = np.linalg.norm(b - P["T"] @ x) / np.linalg.norm(b)
    print(f"{case}: transposed solve {info['iters']} iterations, relres {info['relres']:.3e}, scipy residual {res:.3e}; forward {i0['iters']} iterations")
    assert info["status"] == 0 and res <= 1e-10
    x1, i1 = s.solve(b)
    assert _bits(x0, x1) and i0["iters"] == i1["iters"] and i0["relres"] == i1["relres"]
    assert s.get_int("device_bytes") == bytes0
    for h in (u, s):
        h.close()


# ---------------------------------------------------------------- 3. against the direct solve
def test_transposed_solve_matches_direct_solve(golden):
    P = _golden_prob(golden)
    lu = spla.splu(sp.csc_matrix(P["T"]))
    with _forward(P, rtol=1e-12, restart=150, max_iters=5000) as s:
        t = s.transposed()
        for g in golden.groups():
            b = golden.rhs(g)
            x, info = t.solve(b)
            ref = lu.solve(b)
            err = np.linalg.norm(x - ref) / np.linalg.norm(ref)
            print(f"{golden.name} {g}: {info['iters']} iterations, relres {info['relres']:.3e}, error against splu(A.T) {err:.3e}")
            assert info["status"] == 0 and err <= 1e-7


# ---------------------------------------------------------------- 4. refactor keeps it in step
class _DeviceCopy:
    """a device copy of a float64 array through the HIP runtime the library links (hipMalloc / hipMemcpy / hipFree)"""

    def __init__(self, a):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.a = np.ascontiguousarray(a, np.float64)
        self.p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(self.p), ctypes.c_size_t(self.a.nbytes)) == 0
        assert self.hip.hipMemcpy(self.p, self.a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(self.a.nbytes), 1) == 0     # host to device

    def __enter__(self):
        return self.p.value

    def __exit__(self, *exc):
        self.hip.hipFree(self.p)


@pytest.mark.parametrize("new", ["same", "differ"])
def test_refactor_keeps_transposed_in_step(new, probs):
    P = probs
    s = _forward(P)
    t = s.transposed()
    t.solve_many(np.stack([_rhs(P, k) for k in range(4)]))          # its batch vectors exist before the refactor
    s.refactor(P[new])
    assert s.transposed() is t and t.get_int("is_transpose") == 1
    assert s.get_int("refactor_count") == 1 and t.get_int("refactor_count") == 1
    u = _reference(P)
    u.refactor(np.asarray(P[new])[P["src"]])
    assert t.get_int("refactor_rebuilt") == u.get_int("refactor_rebuilt")
    _assert_same_solver(t, u, P)
    f = _forward(P, P[new])                                          # the source itself is what a refactor alone leaves
    assert _bits(s.spmv(_rhs(P)), f.spmv(_rhs(P)))
    for h in (u, f, s):
        h.close()


def test_refactor_device_and_rebuild(probs):
    P = probs
    s = _forward(P)
    t = s.transposed()
    with _DeviceCopy(P["same"]) as d:
        s.refactor_device(d)
    assert s.transposed() is t and t.get_int("refactor_count") == 1 and t.get_int("refactor_rebuilt") == 0
    u = _reference(P)
    u.refactor(np.asarray(P["same"])[P["src"]])
    _assert_same_solver(t, u, P)
    u.close()
    # rebuild: the transposed solver is not a clone and does not block it; both are then fresh creates of the new matrix
    s.refactor(P["differ"], rebuild=True)
    assert s.transposed() is t and t.get_int("refactor_count") == 2
    assert s.get_int("refactor_rebuilt") == 1 and t.get_int("refactor_rebuilt") == 1
    u = _reference(P, P["differ"])
    _assert_same_solver(t, u, P)
    f = _forward(P, P["differ"])
    _assert_same_hierarchy(s, f)
    for h in (u, f, s):
        h.close()


def test_refactor_under_row_equilibration(probs):
    """equil=1: the row scaling of A^T is recomputed from the gathered (unscaled) values"""
    P = probs
    s = _forward(P, equil=1)
    t = s.transposed()
    s.refactor(P["same"])
    assert s.transposed() is t and t.get_int("refactor_count") == 1 and t.get_int("equil") == 1
    u = _reference(P, equil=1)
    u.refactor(np.asarray(P["same"])[P["src"]])
    _assert_same_solver(t, u, P)
    for h in (u, s):
        h.close()


def test_refused_refactor_leaves_both_solvers(probs):
    P = probs
    b = _rhs(P)
    s = _forward(P)
    t = s.transposed()
    xs, is_ = s.solve(b)
    xt, it = t.solve(b)
    bad = np.array(P["same"], copy=True)
    r = 7
    rp, ci = P["rowptr"], P["colind"]
    bad[rp[r] + np.nonzero(ci[rp[r]:rp[r + 1]] == r)[0][0]] = 0.0
    with pytest.raises(solver.NkpError) as e:
        s.refactor(bad)
    assert e.value.code == -4
    assert s.transposed() is t and s.get_int("refactor_count") == 0 and t.get_int("refactor_count") == 0
    xs1, is1 = s.solve(b)
    xt1, it1 = t.solve(b)
    assert _bits(xs, xs1) and is_["iters"] == is1["iters"] and _bits(xt, xt1) and it["iters"] == it1["iters"]
    s.close()


# ---------------------------------------------------------------- 5. lifetime and refusals
class _FileComm:
    """the library's file transport for one rank, shaped like the transports of dist.py (ops, errors)"""

    def __init__(self, lib, path):
        lib.nkp_comm_file_init.argtypes = [ctypes.POINTER(solver.NkpCommOps), ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
        lib.nkp_comm_file_free.argtypes = [ctypes.POINTER(solver.NkpCommOps)]
        lib.nkp_comm_file_free.restype = None
        self.lib, self.ops, self.errors = lib, solver.NkpCommOps(), []
        assert lib.nkp_comm_file_init(ctypes.byref(self.ops), str(path).encode(), 0, 1) == 0

    def close(self):
        self.lib.nkp_comm_file_free(ctypes.byref(self.ops))


def _refused(fn, fragment):
    with pytest.raises(solver.NkpError) as e:
        fn()
    assert e.value.code == -1 and fragment in str(e.value), str(e.value)


def test_refusals(golden_by_name, tmp_path):
    g = golden_by_name("tri_12x10x6")
    P = _golden_prob(g)
    lib = solver.load_library()
    s = _forward(P)
    c = s.clone()
    h = ctypes.c_void_p(1)
    assert lib.nkp_transpose(c._h, ctypes.byref(h)) == -1 and h.value is None and "clone" in solver.last_error()
    _refused(c.transposed, "clone")
    c.close()
    assert s.get_int("trans_device_bytes") == 0                      # nothing was allocated
    t = s.transposed()
    h = ctypes.c_void_p(1)
    assert lib.nkp_transpose(t._h, ctypes.byref(h)) == -1 and h.value is None
    _refused(t.transposed, "transposed handle")
    _refused(lambda: t.refactor(P["val"][P["src"]]), "refactor the solver it was transposed from")
    with _DeviceCopy(P["val"][P["src"]]) as d:
        _refused(lambda: t.refactor_device(d), "refactor the solver it was transposed from")
    _refused(t.clone, "transposed")
    _refused(lambda: t.set_stream(0), "transposed")
    x, _ = t.solve(g.rhs("IAGE"))                                   # still the solver it was
    s.set_stream(0)                                                 # moves both solvers
    x1, _ = t.solve(g.rhs("IAGE"))
    assert _bits(x, x1)
    s.close()
    # the row-distributed flavour: one rank, distributed code path
    comm = _FileComm(lib, tmp_path)
    loc = dist.local_slice(g.rowptr, g.colind, g.val, g.blk_start, np.array([0, g.n]), 0, P["ci"], P["cj"])
    d = dist.NkpDistSolver(loc, g.n, comm, tuning=dict(force_dist=1))
    try:
        _refused(d.transposed, "distributed")
        assert d.get_int("trans_device_bytes") == 0
    finally:
        d.close()
        comm.close()


def test_ownership_and_detaching(golden_by_name):
    g = golden_by_name("tri_12x10x6")
    P = _golden_prob(g)
    b = g.rhs("IAGE")
    s = _forward(P)
    own = s.get_int("device_bytes")
    assert s.get_int("trans_device_bytes") == 0
    t = s.transposed()
    held = s.get_int("trans_device_bytes")
    assert held >= t.get_int("device_bytes") + 4 * t.nnz > 0 and s.get_int("device_bytes") == own
    x, _ = t.solve(b)
    t.close()                                                       # frees and detaches
    assert t._h.value is None and s.get_int("trans_device_bytes") == 0 and s.get_int("device_bytes") == own
    t2 = s.transposed()                                             # a new one
    assert t2 is not t and s.get_int("trans_device_bytes") > 0 and s.get_int("device_bytes") == own
    x2, _ = t2.solve(b)
    assert _bits(x, x2)
    s.close()                                                       # destroys the transposed solver too
    assert t2._h.value is None
    t2.close()                                                      # a no-op, not a second free


# ---------------------------------------------------------------- 6. executables
def test_cli_transposed_solve(tmp_path, golden_by_name):
    g = golden_by_name("tri_12x10x6")
    P = _golden_prob(g)
    dst = str(tmp_path / "B.nc")
    shutil.copy(g.tracer_path, dst)
    env = dict(os.environ, NKP_RTOL="1e-12", NKP_RESTART="150", NKP_TRANS="1")
    r = subprocess.run([os.path.join(BIN, "solve_ABglobal"), "-D1", "-v", ",".join(g.varnames), g.matrix_path, dst], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "NKP_TRANS" in r.stdout and "trans_us" in r.stdout
    out = nc3.NcFile(dst)
    ocean = np.zeros((g.km, g.jmt, g.imt), bool)
    ocean[g.ind_k, g.ind_j, g.ind_i] = True
    lu = spla.splu(sp.csc_matrix(P["T"]))
    for v in g.varnames:
        f = out.get(v)
        assert np.array_equal(f[~ocean], g.fields[v][~ocean])       # land bytes untouched
        ref = lu.solve(g.rhs(v))
        xt = f[g.ind_k, g.ind_j, g.ind_i]
        assert np.linalg.norm(xt - ref) / np.linalg.norm(ref) <= 1e-7
    # the row-distributed executable refuses the mode on every rank before it does anything else
    shutil.copy(g.tracer_path, dst)
    for rank in ("0", "1"):
        r = subprocess.run([os.path.join(BIN, "solve_ABdist"), "-v", ",".join(g.varnames), g.matrix_path, dst], capture_output=True, text=True,
                           env=dict(env, RANK=rank))
        assert r.returncode != 0 and "NKP_TRANS" in r.stderr and "row-distributed" in r.stderr
    assert open(dst, "rb").read() == open(g.tracer_path, "rb").read()
