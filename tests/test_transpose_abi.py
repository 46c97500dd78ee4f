"""nkp_transpose: declared, exported and bound; the NULL refusals run without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from nk_ocn_tracer_jacobian_precond_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "nkp.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", solver.HIP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = solver.load_library()
    assert re.search(r"\bint\s+nkp_transpose\s*\(\s*nkp_solver\s*\*\s*s\s*,\s*nkp_solver\s*\*\*\s*out\s*\)\s*;", text)
    assert re.search(r"\bT nkp_transpose\b", out)
    assert "nkp_transpose" in solver.ABI_SYMBOLS
    assert lib.nkp_transpose.argtypes is not None
    assert hasattr(solver.NkpSolver, "transposed")


def test_null_arguments_need_no_gpu():
    lib = solver.load_library()
    h = C.c_void_p(0xdead)                                # must come back NULL
    assert lib.nkp_transpose(None, C.byref(h)) == -1
    assert h.value is None
    assert "NULL" in lib.nkp_last_error().decode()
    # a NULL out is refused before the solver handle is looked at
    fake = C.c_void_p(np.ones(4).ctypes.data)
    assert lib.nkp_transpose(fake, None) == -1
    assert "NULL" in lib.nkp_last_error().decode()
