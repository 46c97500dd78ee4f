"""nkp_refactor_dist / nkp_refactor_dist_device: declared, exported and bound; argument checks that need no GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from nk_ocn_tracer_jacobian_precond_amd import dist as nd
from nk_ocn_tracer_jacobian_precond_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nkp_refactor_dist", "nkp_refactor_dist_device")


def test_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "nkp.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", solver.HIP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = solver.load_library()
    for name in NAMES:
        assert re.search(rf"\bint {name}\s*\(nkp_solver \*s,", text), name
        assert re.search(rf"\bT {name}\b", out), name
        assert name in solver.ABI_SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    assert "refactor_halo_values" in text


def test_null_arguments_need_no_gpu():
    lib = solver.load_library()
    val = np.ones(4)
    vp = val.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.nkp_refactor_dist(None, vp, 0) == -1
    assert "NULL" in lib.nkp_last_error().decode()
    assert lib.nkp_refactor_dist_device(None, C.c_void_p(val.ctypes.data), 0) == -1
    assert lib.nkp_refactor_dist(None, None, 0) == -1
    # a NULL value array is refused on the calling rank before the solver handle is looked at
    fake = C.c_void_p(val.ctypes.data)
    assert lib.nkp_refactor_dist(fake, None, 0) == -1
    assert lib.nkp_refactor_dist_device(fake, None, 0) == -1
    assert "NULL" in lib.nkp_last_error().decode()


def test_python_methods():
    for name in ("refactor_dist", "refactor_dist_device"):
        assert callable(getattr(nd.NkpDistSolver, name))
    # the inherited single-GPU entry stays (the library refuses it on a distributed solver)
    assert nd.NkpDistSolver.refactor is solver.NkpSolver.refactor


def test_wrong_length_is_refused_before_the_library():
    s = object.__new__(nd.NkpDistSolver)
    s.nnz = 5
    try:
        s.refactor_dist(np.ones(4))
    except ValueError as e:
        assert "expected 5" in str(e)
    else:
        raise AssertionError("a slice of the wrong length reached the library")
