"""nkp_values_product / nkp_values_product_device / nkp_solve_tangent_device: declared, exported and bound; the NULL refusals name
the argument and run without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from nk_ocn_tracer_jacobian_precond_amd import dist, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nkp_values_product", "nkp_values_product_device", "nkp_solve_tangent_device")
F64P = C.POINTER(C.c_double)


def test_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "nkp.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", solver.HIP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = solver.load_library()
    assert re.search(r"\bint\s+nkp_values_product_device\s*\(\s*nkp_solver\s*\*\s*s\s*,\s*int\s+nrhs\s*,\s*const\s+void\s*\*\s*d_val\s*,\s*const\s+void\s*\*\s*d_x\s*,"
                     r"\s*int64_t\s+ldx\s*,\s*double\s+alpha\s*,\s*int\s+accumulate\s*,\s*void\s*\*\s*d_y\s*,\s*int64_t\s+ldy\s*\)\s*;", text)
    assert re.search(r"\bint\s+nkp_values_product\s*\(\s*nkp_solver\s*\*\s*s\s*,\s*int\s+nrhs\s*,\s*const\s+double\s*\*\s*val\s*,\s*const\s+double\s*\*\s*x\s*,"
                     r"\s*int64_t\s+ldx\s*,\s*double\s+alpha\s*,\s*int\s+accumulate\s*,\s*double\s*\*\s*y\s*,\s*int64_t\s+ldy\s*\)\s*;", text)
    assert re.search(r"\bint\s+nkp_solve_tangent_device\s*\(\s*nkp_solver\s*\*\s*s\s*,\s*int\s+nrhs\s*,\s*const\s+void\s*\*\s*d_dval\s*,\s*const\s+void\s*\*\s*d_x\s*,"
                     r"\s*int64_t\s+ldx\s*,\s*const\s+void\s*\*\s*d_db\s*,\s*void\s*\*\s*d_dx\s*,\s*int64_t\s+ld\s*,\s*double\s*\*\s*berr\s*,\s*int\s*\*\s*iters\s*,"
                     r"\s*double\s*\*\s*relres\s*\)\s*;", text)
    for name in NAMES:
        assert re.search(rf"\bT {name}\b", out), name
        assert name in solver.ABI_SYMBOLS
        assert getattr(lib, name).argtypes is not None
    for cls in (solver.NkpSolver, dist.NkpDistSolver):
        for method in ("values_product", "values_product_device", "solve_tangent", "solve_tangent_device"):
            assert hasattr(cls, method), (cls, method)


def test_null_handle_needs_no_gpu():
    lib = solver.load_library()
    v = np.ones(4)
    p, q = v.ctypes.data_as(F64P), C.c_void_p(v.ctypes.data)
    assert lib.nkp_values_product(None, 1, p, p, 4, 1.0, 0, p, 4) == -1
    msg = lib.nkp_last_error().decode()
    assert "nkp_values_product:" in msg and "NULL solver" in msg and "argument s" in msg
    assert lib.nkp_values_product_device(None, 1, q, q, 4, 1.0, 0, q, 4) == -1
    msg = lib.nkp_last_error().decode()
    assert "nkp_values_product_device:" in msg and "NULL solver" in msg and "argument s" in msg
    assert lib.nkp_solve_tangent_device(None, 1, q, q, 4, q, q, 4, None, None, None) == -1
    msg = lib.nkp_last_error().decode()
    assert "nkp_solve_tangent_device:" in msg and "NULL solver" in msg and "argument s" in msg
    assert np.array_equal(v, np.ones(4))


@pytest.mark.parametrize("missing", ["val", "x", "y"])
def test_null_pointers_are_refused_before_the_handle_is_looked_at(missing):
    """the handle is a host array, not a solver: a refusal that dereferenced it would read garbage (or fault)"""
    lib = solver.load_library()
    fake = C.c_void_p(np.zeros(64).ctypes.data)
    v = np.ones(4)
    p = v.ctypes.data_as(F64P)
    args = {k: (None if k == missing else p) for k in ("val", "x", "y")}
    assert lib.nkp_values_product(fake, 1, args["val"], args["x"], 4, 1.0, 0, args["y"], 4) == -1
    assert f"NULL argument {missing}" in lib.nkp_last_error().decode()
    q = C.c_void_p(v.ctypes.data)
    args = {k: (None if k == missing else q) for k in ("val", "x", "y")}
    assert lib.nkp_values_product_device(fake, 1, args["val"], args["x"], 4, 1.0, 0, args["y"], 4) == -1
    assert f"NULL argument d_{missing}" in lib.nkp_last_error().decode()


def test_tangent_null_buffers_are_refused_before_the_handle_is_looked_at():
    lib = solver.load_library()
    fake = C.c_void_p(np.zeros(64).ctypes.data)
    q = C.c_void_p(np.ones(4).ctypes.data)
    assert lib.nkp_solve_tangent_device(fake, 1, q, q, 4, q, None, 4, None, None, None) == -1
    assert "NULL argument d_dx" in lib.nkp_last_error().decode()
    assert lib.nkp_solve_tangent_device(fake, 1, q, None, 4, q, q, 4, None, None, None) == -1
    assert "NULL argument d_x" in lib.nkp_last_error().decode()
    assert lib.nkp_solve_tangent_device(fake, 1, None, None, 4, None, q, 4, None, None, None) == -1
    msg = lib.nkp_last_error().decode()
    assert "d_dval" in msg and "d_db" in msg and "both NULL" in msg


def test_kernel_files_do_not_read_the_environment():
    csrc = os.path.join(ROOT, "nk_ocn_tracer_jacobian_precond_amd", "csrc")
    for name in ("valprod.hip", "valprod_api.hip"):
        assert "getenv" not in open(os.path.join(csrc, name)).read(), name
