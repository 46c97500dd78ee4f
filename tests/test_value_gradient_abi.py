"""nkp_value_gradient / nkp_value_gradient_device: declared, exported and bound; the NULL refusals name the argument and run
without a device; the torch wrapper's module imports without a GPU (and without importing torch)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from nk_ocn_tracer_jacobian_precond_amd import dist, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nkp_value_gradient", "nkp_value_gradient_device")


def test_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "nkp.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", solver.HIP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = solver.load_library()
    assert re.search(r"\bint\s+nkp_value_gradient_device\s*\(\s*nkp_solver\s*\*\s*s\s*,\s*int\s+nrhs\s*,\s*const\s+void\s*\*\s*d_lambda\s*,\s*const\s+void\s*\*\s*d_x\s*,"
                     r"\s*int64_t\s+ld\s*,\s*double\s+alpha\s*,\s*int\s+accumulate\s*,\s*void\s*\*\s*d_gval\s*\)\s*;", text)
    assert re.search(r"\bint\s+nkp_value_gradient\s*\(\s*nkp_solver\s*\*\s*s\s*,\s*int\s+nrhs\s*,\s*const\s+double\s*\*\s*lambda\s*,\s*const\s+double\s*\*\s*x\s*,"
                     r"\s*int64_t\s+ld\s*,\s*double\s+alpha\s*,\s*int\s+accumulate\s*,\s*double\s*\*\s*gval\s*\)\s*;", text)
    for name in NAMES:
        assert re.search(rf"\bT {name}\b", out), name
        assert name in solver.ABI_SYMBOLS
        assert getattr(lib, name).argtypes is not None
    for cls in (solver.NkpSolver, dist.NkpDistSolver):
        assert hasattr(cls, "value_gradient") and hasattr(cls, "value_gradient_device")


def test_null_handle_needs_no_gpu():
    lib = solver.load_library()
    v = np.ones(4)
    p = v.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.nkp_value_gradient(None, 1, p, p, 4, -1.0, 0, p) == -1
    msg = lib.nkp_last_error().decode()
    assert "nkp_value_gradient:" in msg and "NULL solver" in msg and "argument s" in msg
    assert lib.nkp_value_gradient_device(None, 1, C.c_void_p(v.ctypes.data), C.c_void_p(v.ctypes.data), 4, -1.0, 0, C.c_void_p(v.ctypes.data)) == -1
    msg = lib.nkp_last_error().decode()
    assert "nkp_value_gradient_device:" in msg and "NULL solver" in msg and "argument s" in msg
    assert np.array_equal(v, np.ones(4))


@pytest.mark.parametrize("missing", ["lambda", "x", "gval"])
def test_null_pointers_are_refused_before_the_handle_is_looked_at(missing):
    """the handle is a host array, not a solver: a refusal that dereferenced it would read garbage (or fault)"""
    lib = solver.load_library()
    fake = C.c_void_p(np.zeros(64).ctypes.data)
    v = np.ones(4)
    p = v.ctypes.data_as(C.POINTER(C.c_double))
    args = {k: (None if k == missing else p) for k in ("lambda", "x", "gval")}
    assert lib.nkp_value_gradient(fake, 1, args["lambda"], args["x"], 4, -1.0, 0, args["gval"]) == -1
    assert f"NULL argument {missing}" in lib.nkp_last_error().decode()
    q = C.c_void_p(v.ctypes.data)
    args = {k: (None if k == missing else q) for k in ("lambda", "x", "gval")}
    assert lib.nkp_value_gradient_device(fake, 1, args["lambda"], args["x"], 4, -1.0, 0, args["gval"]) == -1
    assert f"NULL argument d_{missing}" in lib.nkp_last_error().decode()


def test_torch_op_imports_without_a_gpu_and_without_torch():
    code = ("import sys\n"
            "import nk_ocn_tracer_jacobian_precond_amd\n"
            "assert 'torch' not in sys.modules\n"
            "from nk_ocn_tracer_jacobian_precond_amd import torch_op\n"
            "assert 'torch' not in sys.modules, 'torch_op imported torch at import time'\n"
            "assert hasattr(torch_op, 'NkpTorchSolver') and torch_op.MAX_RHS == 8\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_kernel_files_do_not_read_the_environment():
    csrc = os.path.join(ROOT, "nk_ocn_tracer_jacobian_precond_amd", "csrc")
    for name in ("valgrad.hip", "valgrad_api.hip"):
        assert "getenv" not in open(os.path.join(csrc, name)).read(), name
