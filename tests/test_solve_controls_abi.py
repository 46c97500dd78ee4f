"""nkp_set_solve_controls / nkp_get_solve_controls / nkp_solve_batch_device_ex: declared, exported and bound; the struct has the
library's size; the NULL refusals name the argument and run without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from nk_ocn_tracer_jacobian_precond_amd import dist, solver, torch_op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nkp_set_solve_controls", "nkp_get_solve_controls", "nkp_solve_batch_device_ex")
F64P, I32P = C.POINTER(C.c_double), C.POINTER(C.c_int)


def controls(size=None, max_iters=0, rtol=-1.0, atol=-1.0):
    return solver.NkpSolveControls(C.sizeof(solver.NkpSolveControls) if size is None else size, max_iters, rtol, atol)


def test_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "nkp.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", solver.HIP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = solver.load_library()
    assert re.search(r"\bint\s+nkp_set_solve_controls\s*\(\s*nkp_solver\s*\*\s*s\s*,\s*const\s+nkp_solve_controls\s*\*\s*c\s*\)\s*;", text)
    assert re.search(r"\bint\s+nkp_get_solve_controls\s*\(\s*nkp_solver\s*\*\s*s\s*,\s*nkp_solve_controls\s*\*\s*out\s*\)\s*;", text)
    assert re.search(r"\bint\s+nkp_solve_batch_device_ex\s*\(\s*nkp_solver\s*\*\s*s\s*,\s*int\s+nrhs\s*,\s*const\s+void\s*\*\s*d_B\s*,\s*void\s*\*\s*d_X\s*,\s*int64_t\s+ldb\s*,"
                     r"\s*const\s+double\s*\*\s*rtol\s*,\s*const\s+double\s*\*\s*atol\s*,\s*const\s+int\s*\*\s*max_iters\s*,\s*const\s+int\s*\*\s*use_guess\s*,"
                     r"\s*double\s*\*\s*berr\s*,\s*int\s*\*\s*iters\s*,\s*double\s*\*\s*relres\s*\)\s*;", text)
    assert re.search(r"typedef\s+struct\s+nkp_solve_controls\s*\{\s*int\s+struct_size\s*;[^}]*int\s+max_iters\s*;[^}]*double\s+rtol\s*;[^}]*double\s+atol\s*;[^}]*\}\s*nkp_solve_controls\s*;",
                     text)
    for name in NAMES:
        assert re.search(rf"\bT {name}\b", out), name
        assert name in solver.ABI_SYMBOLS
        assert getattr(lib, name).argtypes is not None
    for cls in (solver.NkpSolver, dist.NkpDistSolver):
        for method in ("set_solve_controls", "reset_solve_controls", "get_solve_controls", "solve_batch_device_ex", "solve_many"):
            assert hasattr(cls, method), (cls, method)
    assert hasattr(torch_op.NkpTorchSolver, "set_solve_controls")


def test_struct_has_the_size_of_the_library():
    """nkp_get_solve_controls checks out->struct_size before it looks at the handle: the right size gets as far as the NULL
    solver, any other is refused with the library's own sizeof in the message."""
    lib = solver.load_library()
    size = C.sizeof(solver.NkpSolveControls)
    assert [f[0] for f in solver.NkpSolveControls._fields_] == ["struct_size", "max_iters", "rtol", "atol"]
    c = controls()
    assert lib.nkp_get_solve_controls(None, C.byref(c)) == -1
    msg = lib.nkp_last_error().decode()
    assert "nkp_get_solve_controls:" in msg and "NULL solver" in msg and "argument s" in msg and "struct_size" not in msg
    for wrong in (size + 8, size - 4, 0):
        c = controls(size=wrong)
        assert lib.nkp_get_solve_controls(None, C.byref(c)) == -1
        msg = lib.nkp_last_error().decode()
        got = re.search(r"struct_size mismatch \((-?\d+) != (\d+)\)", msg)
        assert got and int(got.group(1)) == wrong and int(got.group(2)) == size, msg
    assert lib.nkp_get_solve_controls(None, None) == -1
    assert "NULL argument out" in lib.nkp_last_error().decode()


def test_null_handle_needs_no_gpu():
    lib = solver.load_library()
    c = controls(rtol=1e-3)
    assert lib.nkp_set_solve_controls(None, C.byref(c)) == -1
    msg = lib.nkp_last_error().decode()
    assert "nkp_set_solve_controls:" in msg and "NULL solver" in msg and "argument s" in msg
    assert lib.nkp_set_solve_controls(None, None) == -1
    assert "NULL solver" in lib.nkp_last_error().decode()
    v = np.ones(4)
    q = C.c_void_p(v.ctypes.data)
    assert lib.nkp_solve_batch_device_ex(None, 1, q, q, 4, None, None, None, None, None, None, None) == -1
    msg = lib.nkp_last_error().decode()
    assert "nkp_solve_batch_device_ex:" in msg and "NULL solver" in msg and "argument s" in msg
    assert np.array_equal(v, np.ones(4))


@pytest.mark.parametrize("missing", ["d_B", "d_X"])
def test_null_buffers_are_refused_before_the_handle_is_looked_at(missing):
    """the handle is a host array, not a solver: a refusal that dereferenced it would read garbage (or fault)"""
    lib = solver.load_library()
    fake = C.c_void_p(np.zeros(64).ctypes.data)
    v = np.ones(4)
    args = {k: (None if k == missing else C.c_void_p(v.ctypes.data)) for k in ("d_B", "d_X")}
    tol = (C.c_double * 1)(1e-3)
    assert lib.nkp_solve_batch_device_ex(fake, 1, args["d_B"], args["d_X"], 4, tol, None, None, None, None, None, None) == -1
    assert f"NULL argument {missing}" in lib.nkp_last_error().decode()
    assert np.array_equal(v, np.ones(4))


def test_python_setter_refuses_what_the_struct_cannot_say():
    """None is the only way to say "leave as it is": a negative tolerance or max_iters <= 0 never reaches the library"""
    s = object.__new__(solver.NkpSolver)
    s._lib, s._h = solver.load_library(), C.c_void_p()
    for kw in (dict(rtol=-1.0), dict(atol=-1e-3), dict(max_iters=0), dict(max_iters=-2)):
        with pytest.raises(ValueError):
            s.set_solve_controls(**kw)
    with pytest.raises(solver.NkpError) as e:
        s.set_solve_controls(rtol=1e-3)
    assert e.value.code == -1 and "NULL solver" in str(e.value)


def test_unit_does_not_read_the_environment_or_the_device():
    text = open(os.path.join(ROOT, "nk_ocn_tracer_jacobian_precond_amd", "csrc", "solve_controls.hip")).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert "getenv" not in code
    assert not re.search(r"\bhip[A-Z]\w*\s*\(", code), "the setter and the checks of the _ex entry make no HIP call"
