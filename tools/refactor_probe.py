"""nkp_refactor against nkp_create on the bench's synthetic matrix ("New values on the same pattern").

Creates a solver for day_cnt = 365, then refactors it to the day_cnt = 180 Jacobian (same pattern) and back, with host
(nkp_refactor) and device (nkp_refactor_device) values: host wall clock around calls that synchronise, the first call
(builds the value maps) reported apart from the steady state.  One JSON line per grid.

    python tools/refactor_probe.py [--grid 320x384x60] [--reps 5] [--rebuild]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/refactor_probe.py --reps 2     (per-kernel times, separate run)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="320x384x60")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ml-smooth", type=int, default=3)
    ap.add_argument("--rebuild", action="store_true", help="also time NKP_REFACTOR_REBUILD")
    a = ap.parse_args()
    imt, jmt, km = (int(t) for t in a.grid.split("x"))
    p = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=0, isop_k33=True)
    q = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=0, isop_k33=True, day_cnt=180.0)
    assert np.array_equal(p.rowptr, q.rowptr) and np.array_equal(p.colind, q.colind)
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    kw = dict(precond=solver.PRECOND_MULTILEVEL, restart=200, ml_smooth=a.ml_smooth, rtol=1e-10)
    mk = lambda v: solver.NkpSolver(p.rowptr, p.colind, v, blk, col_i=ci, col_j=cj, **kw)
    mk(p.nzval).close()                                        # warm-up: code objects, allocator
    s = mk(p.nzval)
    out = dict(grid=a.grid, n=p.flat_len, nnz=p.nnz, create_us=s.get_int("create_us"), device_MB_create=s.get_int("device_bytes") / 1e6)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e6

    vals = (q.nzval, p.nzval)
    first = timed(lambda: s.refactor(vals[0]))
    out["refactor_first_us"] = first
    out["refactor_first_lib_us"] = s.get_int("refactor_us")
    out["rebuilt_first"] = s.get_int("refactor_rebuilt")
    host = [timed(lambda k=k: s.refactor(vals[(k + 1) % 2])) for k in range(a.reps)]
    out["refactor_us"] = float(np.median(host))
    out["refactor_lib_us"] = s.get_int("refactor_us")
    hip = ctypes.CDLL("libamdhip64.so")
    dev = []
    for v in vals:
        d = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(d), ctypes.c_size_t(v.nbytes)) == 0
        assert hip.hipMemcpy(d, v.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(v.nbytes), 1) == 0
        dev.append(d)
    devt = [timed(lambda k=k: s.refactor_device(dev[k % 2].value)) for k in range(a.reps)]
    out["refactor_device_us"] = float(np.median(devt))
    out["rebuilt_steady"] = s.get_int("refactor_rebuilt")
    out["device_MB_after"] = s.get_int("device_bytes") / 1e6
    if a.rebuild:
        out["rebuild_us"] = timed(lambda: s.refactor(vals[0], rebuild=True))
    b = np.random.default_rng(1).standard_normal(p.flat_len)
    s.refactor(q.nzval)
    x, info = s.solve(b)
    t = mk(q.nzval)
    x2, info2 = t.solve(b)
    out["solve_bitwise_equal_to_create"] = bool(np.array_equal(x, x2))
    out["iters"] = info["iters"]
    out["ratio_device_to_create"] = out["refactor_device_us"] / max(1, out["create_us"])
    for d in dev:
        hip.hipFree(d)
    s.close()
    t.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
