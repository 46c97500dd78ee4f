"""nkp_refactor / nkp_refactor_device: declared, exported and bound; argument checks that need no GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from nk_ocn_tracer_jacobian_precond_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nkp_refactor", "nkp_refactor_device")


def test_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "nkp.h")).read()
    assert re.search(r"#define\s+NKP_REFACTOR_REBUILD\s+1\b", text)
    out = subprocess.run(["nm", "-D", "--defined-only", solver.HIP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = solver.load_library()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert re.search(rf"\bT {name}\b", out), name
        assert name in solver.ABI_SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    assert hasattr(solver.NkpSolver, "refactor") and hasattr(solver.NkpSolver, "refactor_device")


def test_null_arguments_need_no_gpu():
    lib = solver.load_library()
    val = np.ones(4)
    vp = val.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.nkp_refactor(None, vp, 0) == -1
    assert "NULL" in lib.nkp_last_error().decode()
    assert lib.nkp_refactor_device(None, C.c_void_p(val.ctypes.data), 0) == -1
    # a NULL value array is refused before the solver handle is looked at
    fake = C.c_void_p(val.ctypes.data)
    assert lib.nkp_refactor(fake, None, 0) == -1
    assert lib.nkp_refactor_device(fake, None, 0) == -1
