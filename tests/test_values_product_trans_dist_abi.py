"""nkp_values_product_trans_dist / nkp_values_product_trans_dist_device: declared, exported and bound, with their mirror methods on
NkpDistSolver; every NULL argument of both flavours is NKP_EINVAL, the message names the argument, and the refusal is made before
the handle is looked at -- so without a device, without a HIP call and without a collective."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from nk_ocn_tracer_jacobian_precond_amd import dist, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nkp_values_product_trans_dist", "nkp_values_product_trans_dist_device")
F64P = C.POINTER(C.c_double)
NKP_EINVAL = -1


def test_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "nkp.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", solver.HIP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = solver.load_library()
    assert re.search(r"\bint\s+nkp_values_product_trans_dist_device\s*\(\s*nkp_solver\s*\*\s*s\s*,\s*int\s+nrhs\s*,\s*const\s+void\s*\*\s*d_val_loc\s*,\s*const\s+void\s*\*\s*d_x\s*,"
                     r"\s*int64_t\s+ldx\s*,\s*double\s+alpha\s*,\s*int\s+accumulate\s*,\s*void\s*\*\s*d_y\s*,\s*int64_t\s+ldy\s*\)\s*;", text)
    assert re.search(r"\bint\s+nkp_values_product_trans_dist\s*\(\s*nkp_solver\s*\*\s*s\s*,\s*int\s+nrhs\s*,\s*const\s+double\s*\*\s*val_loc\s*,\s*const\s+double\s*\*\s*x\s*,"
                     r"\s*int64_t\s+ldx\s*,\s*double\s+alpha\s*,\s*int\s+accumulate\s*,\s*double\s*\*\s*y\s*,\s*int64_t\s+ldy\s*\)\s*;", text)
    for name in NAMES:
        assert re.search(rf"\bT {name}\b", out), name
        assert name in solver.ABI_SYMBOLS
        assert getattr(lib, name).argtypes is not None
    for method in ("values_product_trans_dist", "values_product_trans_dist_device"):
        assert hasattr(dist.NkpDistSolver, method), method
    assert "still to come" not in text


def test_null_solver_is_refused_and_named():
    lib = solver.load_library()
    v = np.ones(4)
    p, q = v.ctypes.data_as(F64P), C.c_void_p(v.ctypes.data)
    assert lib.nkp_values_product_trans_dist(None, 1, p, p, 4, 1.0, 0, p, 4) == NKP_EINVAL
    msg = lib.nkp_last_error().decode()
    assert "nkp_values_product_trans_dist:" in msg and "NULL solver" in msg and "argument s" in msg
    assert lib.nkp_values_product_trans_dist_device(None, 1, q, q, 4, 1.0, 0, q, 4) == NKP_EINVAL
    msg = lib.nkp_last_error().decode()
    assert "nkp_values_product_trans_dist_device:" in msg and "NULL solver" in msg and "argument s" in msg
    assert np.array_equal(v, np.ones(4))


@pytest.mark.parametrize("missing", ["val_loc", "x", "y"])
def test_null_buffers_are_refused_before_the_handle_is_looked_at(missing):
    """the handle is a host array of zeros, not a solver: a refusal that looked at it would find a single-GPU solver on device 0
    with a NULL stream and go on to HIP calls (or fault); the buffers are host memory in both flavours, so any kernel or copy would
    fail, not return -1 with this message"""
    lib = solver.load_library()
    fake = C.c_void_p(np.zeros(4096).ctypes.data)
    v = np.ones(4)
    p = v.ctypes.data_as(F64P)
    args = {k: (None if k == missing else p) for k in ("val_loc", "x", "y")}
    assert lib.nkp_values_product_trans_dist(fake, 1, args["val_loc"], args["x"], 4, 1.0, 0, args["y"], 4) == NKP_EINVAL
    msg = lib.nkp_last_error().decode()
    assert msg.startswith("nkp_values_product_trans_dist:") and f"NULL argument {missing}" in msg
    q = C.c_void_p(v.ctypes.data)
    args = {k: (None if k == missing else q) for k in ("val_loc", "x", "y")}
    assert lib.nkp_values_product_trans_dist_device(fake, 1, args["val_loc"], args["x"], 4, 1.0, 0, args["y"], 4) == NKP_EINVAL
    msg = lib.nkp_last_error().decode()
    assert msg.startswith("nkp_values_product_trans_dist_device:") and f"NULL argument d_{missing}" in msg
    assert np.array_equal(v, np.ones(4))


def test_the_refusals_make_no_hip_call():
    """in a fresh process with every device hidden from the HIP runtime: a refusal that went on to a HIP call that needs a device
    would come back with another code than NKP_EINVAL"""
    code = (
        "import ctypes as C, numpy as np\n"
        "from nk_ocn_tracer_jacobian_precond_amd import solver\n"
        "lib = solver.load_library()\n"
        "v = np.ones(4); p = v.ctypes.data_as(C.POINTER(C.c_double)); q = C.c_void_p(v.ctypes.data)\n"
        "fake = C.c_void_p(np.zeros(4096).ctypes.data)\n"
        "f, g = lib.nkp_values_product_trans_dist, lib.nkp_values_product_trans_dist_device\n"
        "rc = [f(fake, 1, None, p, 4, 1.0, 0, p, 4), f(fake, 1, p, None, 4, 1.0, 0, p, 4), f(fake, 1, p, p, 4, 1.0, 0, None, 4),\n"
        "      g(fake, 1, None, q, 4, 1.0, 0, q, 4), g(fake, 1, q, None, 4, 1.0, 0, q, 4), g(fake, 1, q, q, 4, 1.0, 0, None, 4),\n"
        "      f(None, 1, p, p, 4, 1.0, 0, p, 4), g(None, 1, q, q, 4, 1.0, 0, q, 4)]\n"
        "print(rc)\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == str([NKP_EINVAL] * 8)
