"""Batched right-hand sides on the row-distributed solver: what needs no GPU.  The feature adds no entry point and changes no
struct; it is documented in include/nkp.h, reachable through the inherited Python methods, and the executable's NKP_RHS_BLOCK
no longer depends on the flavour."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from nk_ocn_tracer_jacobian_precond_amd import dist as nd
from nk_ocn_tracer_jacobian_precond_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("dist_alltoallv_calls", "dist_allreduce_calls", "batch_steps", "batch_width")


def _header():
    return open(os.path.join(ROOT, "include", "nkp.h")).read()


def test_prototypes_unchanged_and_keys_documented():
    text = _header()
    assert re.search(r"\bint nkp_solve \(nkp_solver \*s, double \*b_in_x_out, int nrhs, int64_t ldb,\s*double \*berr, int \*iters, double \*relres\);", text)
    assert re.search(r"\bint nkp_solve_batch_device \(nkp_solver \*s, int nrhs, const void \*d_B, void \*d_X, int64_t ldb, double \*berr, int \*iters, "
                     r"double \*relres\);", text)
    assert re.search(r"\bint64_t nkp_get_int \(nkp_solver \*s, const char \*key\);", text)
    assert re.search(r"#define NKP_VERSION 1\b", text)
    for key in KEYS:
        assert f'"{key}"' in text, key
    # the contract next to nkp_solve_batch_device: collective use, and where bit identity is not promised
    doc = text.split("int nkp_solve_batch_device")[0].rsplit("/*", 1)[1]
    assert "collective" in doc and "ldb >= m_loc" in doc and "bit identity is not promised" in doc
    assert "the distributed flavour)" not in doc           # no longer listed among the fallbacks
    # the four transport callbacks are the whole interface still
    ops = text.split("typedef struct nkp_comm_ops")[1].split("} nkp_comm_ops;")[0] if "typedef struct nkp_comm_ops" in text else text.split("struct nkp_comm_ops")[1].split("};")[0]
    assert len(re.findall(r"\(\*\w+\)", ops)) == 4, ops


def test_struct_layouts_still_match_the_library():
    lib = solver.load_library()
    sizes = {"nkp_options": solver.NkpOptions, "nkp_tuning": solver.NkpTuning, "nkp_comm_ops": solver.NkpCommOps}
    assert C.sizeof(solver.NkpCommOps) == 2 * C.sizeof(C.c_void_p) + 4 * C.sizeof(C.c_void_p)      # ctx, rank + nranks, four callbacks
    t = solver.default_tuning()
    assert t.rhs_batch == int(os.environ.get("NKP_RHS_BATCH", 1))
    assert all(hasattr(cls, "_fields_") for cls in sizes.values())
    assert lib.nkp_get_int(None, b"batch_steps") == -1


def test_python_surface():
    assert nd.NkpDistSolver.solve_many is not solver.NkpSolver.solve_many and "collective" in nd.NkpDistSolver.solve_many.__doc__
    assert "collective" in nd.NkpDistSolver.solve_batch_device.__doc__
    assert nd.NkpDistSolver.get_int is solver.NkpSolver.get_int
    s = object.__new__(nd.NkpDistSolver)
    s.n = 5
    with pytest.raises(ValueError):
        s.solve_many([[1.0, 2.0, 3.0]])                       # not this rank's m_loc rows: refused before the library


@pytest.mark.skipif(solver.device_count() > 0, reason="CPU-only behaviour")
def test_rhs_block_without_gpu_fails_loudly_and_leaves_file_untouched(tmp_path, golden_by_name):
    g = golden_by_name("penta_12x10x6")
    dst = str(tmp_path / "tracers.nc")
    shutil.copy(g.tracer_path, dst)
    before = open(dst, "rb").read()
    env = dict(os.environ, NKP_RHS_BLOCK="2")
    exe = os.path.join(ROOT, "nk_ocn_tracer_jacobian_precond_amd", "bin", "solve_ABdist")
    r = subprocess.run([exe, "-D1", "-n", "1", "-v", ",".join(g.varnames), g.matrix_path, dst], capture_output=True, text=True, env=env)
    assert r.returncode != 0, r.stdout
    assert open(dst, "rb").read() == before
