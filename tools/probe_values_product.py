"""The product kernel of nkp_values_product next to the CSR SpMV and next to the composition it replaces, on the bench's
synthetic matrix.

One process.  Kernels: one solver without preconditioner (all of them read the matrix only).  nkp_time_kernel times each piece
alone with HIP events on the solver's stream, `--launches` back-to-back launches after its own warm-up launches; the probe
repeats that `--reps` times, alternating SpMV (which = 0), the product kernel (which = 6) and the composition of SpMV kernels
(which = 7: batched operator product into a temporary, de-interleave, one update pass) at K = 1, 2, 4, 8, and reports the median
and the spread of every series, the ratios, and the fraction of the 8 TB/s HBM peak on the compulsory bytes of a launch:

    SpMV          12 nnz + 4 (n + 1) + 16 n
    product       12 nnz + 4 (n + 1) + 16 K n               (values, columns, row pointers, K-wide x once, y written)
    composition   the product's + 24 K n                    (the temporary written and read twice on its way into y)

Tangent solve: with --solve, a multilevel solver on the same matrix; wall time of one nkp_solve_tangent_device (d_dval and d_db)
against one nkp_solve_batch_device of the same width on the same right-hand sides R, `--solves` times each, alternating.

    python tools/probe_values_product.py [--grid 320x384x60] [--reps 7] [--launches 100] [--solve] [--log profiles/values_product_1deg.log]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nk_ocn_tracer_jacobian_precond_amd import solver, synth  # noqa: E402

HBM_PEAK = 8.0e12


class Device:
    def __init__(self, a):
        self.hip = C.CDLL("libamdhip64.so")
        a = np.ascontiguousarray(a, np.float64)
        self.shape, self.size, self.p = a.shape, a.size, C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(max(a.nbytes, 8))) == 0
        assert self.hip.hipMemcpy(self.p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
        self.ptr = self.p.value

    def get(self):
        out = np.empty(self.size)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(out.nbytes), 2) == 0
        return out.reshape(self.shape)

    def free(self):
        self.hip.hipFree(self.p)


def kernels(p, a):
    n, nnz = p.flat_len, p.nnz
    s = solver.NkpSolver(p.rowptr, p.colind, p.nzval, None, precond=solver.PRECOND_NONE, restart=4)
    widths = (1, 2, 4, 8)
    series = {"spmv": []}
    for K in widths:
        series[f"prod_k{K}"], series[f"comp_k{K}"] = [], []
    for K in widths:                                   # work space and code objects before anything is timed
        s.time_kernel(6, reps=3, arg=K)
        s.time_kernel(7, reps=3, arg=K)
    s.time_kernel(0, reps=3)
    for _ in range(a.reps):
        series["spmv"].append(s.time_kernel(0, reps=a.launches))
        for K in widths:
            series[f"prod_k{K}"].append(s.time_kernel(6, reps=a.launches, arg=K))
            series[f"comp_k{K}"].append(s.time_kernel(7, reps=a.launches, arg=K))
    nbytes = {"spmv": 12 * nnz + 4 * (n + 1) + 16 * n}
    for K in widths:
        nbytes[f"prod_k{K}"] = 12 * nnz + 4 * (n + 1) + 16 * K * n
        nbytes[f"comp_k{K}"] = nbytes[f"prod_k{K}"] + 24 * K * n
    assert nbytes["spmv"] == s.get_int("spmv_bytes") == nbytes["prod_k1"]
    spmv_ms = float(np.median(series["spmv"]))
    out = dict(n=n, nnz=nnz, rowblocks=s.get_int("rowblocks"), launches=a.launches, reps=a.reps)
    for name, v in series.items():
        ms = float(np.median(v))
        out[name] = dict(ms=ms, min_ms=float(min(v)), max_ms=float(max(v)), bytes=nbytes[name], tb_per_s=nbytes[name] / (ms * 1e-3) / 1e12,
                         frac_of_hbm_peak=nbytes[name] / (ms * 1e-3) / HBM_PEAK, ratio_to_spmv=ms / spmv_ms)
    for K in widths:
        out[f"prod_k{K}"]["ratio_to_composition"] = out[f"prod_k{K}"]["ms"] / out[f"comp_k{K}"]["ms"]
    s.close()
    return out, series


def tangent(p, a):
    n = p.flat_len
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    rng = np.random.default_rng(5)
    K = a.width
    s = solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, col_i=ci, col_j=cj, rtol=1e-10, restart=60, max_iters=3000)
    dB, dval = rng.standard_normal((K, n)), p.nzval * rng.standard_normal(p.nnz)
    db, dx, dv, dr, do = Device(dB), Device(np.zeros((K, n))), Device(dval), Device(dB), Device(np.zeros((K, n)))
    s.solve_batch_device(db.ptr, dx.ptr, K, n)                                   # X
    s.values_product_device(dv.ptr, dx.ptr, K, n, dr.ptr, n, alpha=-1.0, accumulate=True)      # R, the right-hand sides of both
    plain, tang = [], []
    s.solve_batch_device(dr.ptr, do.ptr, K, n)
    s.solve_tangent_device(dv.ptr, dx.ptr, n, db.ptr, do.ptr, K, n)
    for _ in range(a.solves):
        t0 = time.perf_counter()
        info = s.solve_batch_device(dr.ptr, do.ptr, K, n)
        t1 = time.perf_counter()
        s.solve_tangent_device(dv.ptr, dx.ptr, n, db.ptr, do.ptr, K, n)
        t2 = time.perf_counter()
        plain.append((t1 - t0) * 1e3)
        tang.append((t2 - t1) * 1e3)
    out = dict(width=K, iters=[i["iters"] for i in info], plain_solve_ms=float(np.median(plain)), tangent_solve_ms=float(np.median(tang)),
               plain_min_max_ms=[min(plain), max(plain)], tangent_min_max_ms=[min(tang), max(tang)], product_us=s.get_int("values_product_us"))
    for d in (db, dx, dv, dr, do):
        d.free()
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="320x384x60")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--solve", action="store_true")
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--width", type=int, default=4)
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    imt, jmt, km = (int(t) for t in a.grid.split("x"))
    p = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=0, isop_k33=True)
    out, series = kernels(p, a)
    out["grid"] = a.grid
    if a.solve:
        out["tangent"] = tangent(p, a)
    line = json.dumps(out)
    print(line)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write(f"# python tools/probe_values_product.py --grid {a.grid} --reps {a.reps} --launches {a.launches}{' --solve' if a.solve else ''}\n")
            for name, v in series.items():
                fh.write(f"# {name}: " + " ".join(f"{t:.4f}" for t in v) + " ms per launch\n")
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
