"""What nkp_transpose costs on the bench's synthetic matrix ("Solves with the transposed matrix").

Creates the bench's solver, then reports -- medians of --reps runs after one warm-up each -- the time of nkp_transpose and its
device part next to create_us, the device bytes of the transposed solver next to the source's, one transposed solve against the
forward solve on the same right-hand side, and a refactor_device with and without a transposed solver attached.  Host wall
clock around calls that synchronise.  One JSON line per grid.

    python tools/probe_transpose.py [--grid 320x384x60] [--reps 5]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nk_ocn_tracer_jacobian_precond_amd import solver, synth  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e6, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="320x384x60")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ml-smooth", type=int, default=3)
    a = ap.parse_args()
    imt, jmt, km = (int(t) for t in a.grid.split("x"))
    p = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=0, isop_k33=True)
    q = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=0, isop_k33=True, day_cnt=180.0)
    assert np.array_equal(p.rowptr, q.rowptr) and np.array_equal(p.colind, q.colind)
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    kw = dict(precond=solver.PRECOND_MULTILEVEL, restart=200, ml_smooth=a.ml_smooth, rtol=1e-10)
    solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, col_i=ci, col_j=cj, **kw).close()      # warm-up: code objects, allocator
    s = solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, col_i=ci, col_j=cj, **kw)
    out = dict(grid=a.grid, n=p.flat_len, nnz=p.nnz, create_us=s.get_int("create_us"), device_bytes=s.get_int("device_bytes"))
    med = lambda v: float(np.median(v))

    hip = ctypes.CDLL("libamdhip64.so")
    dev = []
    for v in (q.nzval, p.nzval):
        d = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(d), ctypes.c_size_t(v.nbytes)) == 0
        assert hip.hipMemcpy(d, v.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(v.nbytes), 1) == 0
        dev.append(d)

    # refactor_device without a transposed solver (the first call builds the value maps)
    s.refactor_device(dev[0].value)
    out["refactor_device_us_without"] = med([timed(lambda k=k: s.refactor_device(dev[(k + 1) % 2].value))[0] for k in range(a.reps)])
    out["refactor_lib_us_without"] = s.get_int("refactor_us")
    s.refactor_device(dev[1].value)                                                # back to the day_cnt = 365 matrix

    # nkp_transpose: build, read the counters, detach, again
    s.transposed().close()                                                          # warm-up
    tot, ker = [], []
    for _ in range(a.reps):
        t = s.transposed()
        tot.append(s.get_int("trans_us"))
        ker.append(s.get_int("trans_kernel_us"))
        t.close()
    out["trans_us"], out["trans_kernel_us"] = med(tot), med(ker)
    t = s.transposed()
    out["trans_device_bytes"] = s.get_int("trans_device_bytes")
    out["trans_levels"], out["levels"] = t.get_int("levels"), s.get_int("levels")

    # one solve each on the same right-hand side
    b = np.random.default_rng(1).standard_normal(p.flat_len)
    s.solve(b)
    t.solve(b)
    fw = [timed(lambda: s.solve(b)) for _ in range(a.reps)]
    tr = [timed(lambda: t.solve(b)) for _ in range(a.reps)]
    out["solve_us"], out["solve_iters"], out["solve_relres"] = med([f[0] for f in fw]), fw[0][1][1]["iters"], fw[0][1][1]["relres"]
    out["trans_solve_us"], out["trans_solve_iters"], out["trans_solve_relres"] = med([f[0] for f in tr]), tr[0][1][1]["iters"], tr[0][1][1]["relres"]

    # refactor_device with the transposed solver attached (its first call builds the transposed solver's maps)
    s.refactor_device(dev[0].value)
    out["refactor_device_us_with"] = med([timed(lambda k=k: s.refactor_device(dev[(k + 1) % 2].value))[0] for k in range(a.reps)])
    out["trans_device_bytes_after_refactor"] = s.get_int("trans_device_bytes")
    out["transposed_still_attached"] = bool(s.transposed() is t and t.get_int("refactor_count") == a.reps + 1)
    for d in dev:
        hip.hipFree(d)
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
