"""nkp_residual_batch / nkp_residual_batch_device: declared, exported and bound, with their methods on NkpSolver and NkpDistSolver;
a NULL solver, B or X is NKP_EINVAL, the message names the argument, and the refusal is made before the handle is looked at -- so
without a device, without a HIP call and without a collective.  R may be NULL: that is no refusal of its own."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from nk_ocn_tracer_jacobian_precond_amd import dist, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nkp_residual_batch", "nkp_residual_batch_device")
F64P = C.POINTER(C.c_double)
NKP_EINVAL = -1


def test_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "nkp.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", solver.HIP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = solver.load_library()
    assert re.search(r"\bint\s+nkp_residual_batch_device\s*\(\s*nkp_solver\s*\*\s*s\s*,\s*int\s+nrhs\s*,\s*const\s+void\s*\*\s*d_B\s*,\s*int64_t\s+ldb\s*,"
                     r"\s*const\s+void\s*\*\s*d_X\s*,\s*int64_t\s+ldx\s*,\s*void\s*\*\s*d_R\s*,\s*int64_t\s+ldr\s*,\s*double\s*\*\s*rnorm\s*,"
                     r"\s*double\s*\*\s*bnorm\s*,\s*double\s*\*\s*berr\s*\)\s*;", text)
    assert re.search(r"\bint\s+nkp_residual_batch\s*\(\s*nkp_solver\s*\*\s*s\s*,\s*int\s+nrhs\s*,\s*const\s+double\s*\*\s*B\s*,\s*int64_t\s+ldb\s*,"
                     r"\s*const\s+double\s*\*\s*X\s*,\s*int64_t\s+ldx\s*,\s*double\s*\*\s*R\s*,\s*int64_t\s+ldr\s*,\s*double\s*\*\s*rnorm\s*,"
                     r"\s*double\s*\*\s*bnorm\s*,\s*double\s*\*\s*berr\s*\)\s*;", text)
    for name in NAMES:
        assert re.search(rf"\bT {name}\b", out), name
        assert name in solver.ABI_SYMBOLS
        assert getattr(lib, name).argtypes is not None
    for cls in (solver.NkpSolver, dist.NkpDistSolver):
        for method in ("residual_batch", "residual_batch_device"):
            assert hasattr(cls, method), (cls, method)


def test_null_solver_is_refused_and_named():
    lib = solver.load_library()
    v, o = np.ones(4), np.full(3, 7.0)
    p, q = v.ctypes.data_as(F64P), C.c_void_p(v.ctypes.data)
    op = [o[k:].ctypes.data_as(F64P) for k in range(3)]
    assert lib.nkp_residual_batch(None, 1, p, 4, p, 4, None, 0, *op) == NKP_EINVAL
    msg = lib.nkp_last_error().decode()
    assert "nkp_residual_batch:" in msg and "NULL solver" in msg and "argument s" in msg
    assert lib.nkp_residual_batch_device(None, 1, q, 4, q, 4, None, 0, *op) == NKP_EINVAL
    msg = lib.nkp_last_error().decode()
    assert "nkp_residual_batch_device:" in msg and "NULL solver" in msg and "argument s" in msg
    assert np.array_equal(v, np.ones(4)) and np.all(o == 7.0)


@pytest.mark.parametrize("missing", ["B", "X"])
def test_null_buffers_are_refused_before_the_handle_is_looked_at(missing):
    """the handle is a host array of zeros, not a solver: a refusal that looked at it would find a single-GPU solver on device 0
    with a NULL stream and go on to HIP calls (or fault); the buffers are host memory in both flavours, so any kernel or copy would
    fail, not return -1 with this message"""
    lib = solver.load_library()
    fake = C.c_void_p(np.zeros(8192).ctypes.data)
    v, o = np.ones(4), np.full(3, 7.0)
    op = [o[k:].ctypes.data_as(F64P) for k in range(3)]
    p = v.ctypes.data_as(F64P)
    args = {k: (None if k == missing else p) for k in ("B", "X")}
    assert lib.nkp_residual_batch(fake, 1, args["B"], 4, args["X"], 4, None, 0, *op) == NKP_EINVAL
    msg = lib.nkp_last_error().decode()
    assert msg.startswith("nkp_residual_batch:") and f"NULL argument {missing}" in msg
    q = C.c_void_p(v.ctypes.data)
    args = {k: (None if k == missing else q) for k in ("B", "X")}
    assert lib.nkp_residual_batch_device(fake, 1, args["B"], 4, args["X"], 4, None, 0, *op) == NKP_EINVAL
    msg = lib.nkp_last_error().decode()
    assert msg.startswith("nkp_residual_batch_device:") and f"NULL argument d_{missing}" in msg
    assert np.array_equal(v, np.ones(4)) and np.all(o == 7.0)


def test_out_of_range_arguments_are_refused_without_a_hip_call():
    """in a fresh process with every device hidden from the HIP runtime, on a handle of zeros, which reads as a single-GPU solver
    of n = 0 rows: nrhs 0 and 9, each ld below n (-1), R == X, nothing asked for, next to the NULL arguments.  A refusal that went
    on to a HIP call that needs a device would come back with another code than NKP_EINVAL"""
    code = (
        "import ctypes as C, numpy as np\n"
        "from nk_ocn_tracer_jacobian_precond_amd import solver\n"
        "lib = solver.load_library()\n"
        "v = np.ones(4); o = np.zeros(3); p = v.ctypes.data_as(C.POINTER(C.c_double)); q = C.c_void_p(v.ctypes.data)\n"
        "op = [o[k:].ctypes.data_as(C.POINTER(C.c_double)) for k in range(3)]\n"
        "w = np.ones(4); pw = w.ctypes.data_as(C.POINTER(C.c_double)); qw = C.c_void_p(w.ctypes.data)\n"
        "fake = C.c_void_p(np.zeros(8192).ctypes.data)\n"
        "f, g = lib.nkp_residual_batch, lib.nkp_residual_batch_device\n"
        "rc, msgs = [], []\n"
        "def call(fn, *a):\n"
        "    rc.append(fn(*a)); msgs.append(lib.nkp_last_error().decode())\n"
        "for fn, b, x, r in ((f, p, pw, p), (g, q, qw, q)):\n"
        "    call(fn, None, 1, b, 4, x, 4, None, 0, *op)\n"
        "    call(fn, fake, 1, None, 4, x, 4, None, 0, *op)\n"
        "    call(fn, fake, 1, b, 4, None, 4, None, 0, *op)\n"
        "    call(fn, fake, 0, b, 4, x, 4, None, 0, *op)\n"
        "    call(fn, fake, 9, b, 4, x, 4, None, 0, *op)\n"
        "    call(fn, fake, 1, b, -1, x, 4, None, 0, *op)\n"
        "    call(fn, fake, 1, b, 4, x, -1, None, 0, *op)\n"
        "    call(fn, fake, 1, b, 4, x, 4, r, -1, *op)\n"
        "    call(fn, fake, 1, b, 4, x, 4, x, 4, *op)\n"
        "    call(fn, fake, 1, b, 4, x, 4, None, 0, None, None, None)\n"
        "print(rc)\n"
        "print('|'.join(msgs))\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[0] == str([NKP_EINVAL] * 20), out.stdout
    msgs = lines[1].split("|")
    for k, what in enumerate(("NULL solver", "NULL argument", "NULL argument", "nrhs = 0", "nrhs = 9", "ldb =", "ldx =", "ldr =", "same buffer", "nothing is asked")):
        assert what in msgs[k] and what in msgs[10 + k], (k, what, msgs[k], msgs[10 + k])
    assert "call again" in msgs[4]
