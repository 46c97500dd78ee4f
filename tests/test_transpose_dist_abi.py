"""nkp_transpose_dist: declared, exported and bound; the NULL refusals run without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from nk_ocn_tracer_jacobian_precond_amd import dist, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "nkp.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", solver.HIP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = solver.load_library()
    assert re.search(r"\bint\s+nkp_transpose_dist\s*\(\s*nkp_solver\s*\*\s*s\s*,\s*nkp_solver\s*\*\*\s*out\s*\)\s*;", text)
    assert re.search(r"\bT nkp_transpose_dist\b", out)
    assert "nkp_transpose_dist" in solver.ABI_SYMBOLS
    assert lib.nkp_transpose_dist.argtypes is not None
    assert callable(getattr(dist.NkpDistSolver, "transposed_dist", None))
    assert dist.NkpDistSolver.transposed is solver.NkpSolver.transposed          # the inherited call stays; the library refuses it


def test_null_arguments_need_no_gpu():
    lib = solver.load_library()
    h = C.c_void_p(0xdead)                                # must come back NULL
    assert lib.nkp_transpose_dist(None, C.byref(h)) == -1
    assert h.value is None
    assert "NULL" in lib.nkp_last_error().decode()
    # a NULL out is refused before the solver handle is looked at
    fake = C.c_void_p(np.ones(4).ctypes.data)
    assert lib.nkp_transpose_dist(fake, None) == -1
    assert "NULL" in lib.nkp_last_error().decode()


def test_header_documents_the_protocol():
    text = open(os.path.join(ROOT, "include", "nkp.h")).read()
    doc = text.split("int nkp_transpose_dist")[0].rsplit("/*", 1)[1]
    for word in ("COLLECTIVE", "allgather_i64_host", "alltoallv_i32_host", "trans_sent_entries", "trans_recv_entries", "NKP_ECOMM"):
        assert word in doc, word
    single = text.split("int nkp_transpose (")[0].rsplit("/*", 1)[1]
    assert "row-distributed" in single and "nkp_transpose_dist" in single


def test_the_device_path_reads_no_environment():
    src = open(os.path.join(ROOT, "nk_ocn_tracer_jacobian_precond_amd", "csrc", "transpose_dist.hip")).read()
    assert "getenv" not in src
