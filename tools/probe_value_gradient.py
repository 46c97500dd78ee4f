"""The gradient kernel of nkp_value_gradient next to the CSR SpMV on the bench's synthetic matrix.

One process, one solver (no preconditioner: both kernels read the matrix only).  nkp_time_kernel times each kernel alone with
HIP events on the solver's stream, `--launches` back-to-back launches after its own warm-up launches; the probe repeats that
`--reps` times, alternating SpMV (which = 0) and the gradient kernel (which = 5) at K = 1, 2, 4, 8, and reports the median and
the spread of every series, the ratio to the SpMV of the same run, and the fraction of the 8 TB/s HBM peak on the compulsory
bytes of a launch:

    SpMV       12 nnz + 4 (n + 1) + 16 n                 (values, columns, row pointers, x gathered once, y)
    gradient   4 nnz + 8 nnz + 4 (n + 1) + 16 K n        (columns, g written, row pointers, K-wide lambda and x once)

    python tools/probe_value_gradient.py [--grid 320x384x60] [--reps 7] [--launches 100] [--log profiles/value_gradient_1deg.log]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nk_ocn_tracer_jacobian_precond_amd import solver, synth  # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="320x384x60")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    imt, jmt, km = (int(t) for t in a.grid.split("x"))
    p = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=0, isop_k33=True)
    n, nnz = p.flat_len, p.nnz
    s = solver.NkpSolver(p.rowptr, p.colind, p.nzval, None, precond=solver.PRECOND_NONE, restart=4)
    widths = (1, 2, 4, 8)
    series = {"spmv": []}
    series.update({f"grad_k{K}": [] for K in widths})
    for K in widths:                                   # work space and code objects before anything is timed
        s.time_kernel(5, reps=3, arg=K)
    s.time_kernel(0, reps=3)
    for _ in range(a.reps):
        series["spmv"].append(s.time_kernel(0, reps=a.launches))
        for K in widths:
            series[f"grad_k{K}"].append(s.time_kernel(5, reps=a.launches, arg=K))
    nbytes = {"spmv": 12 * nnz + 4 * (n + 1) + 16 * n}
    nbytes.update({f"grad_k{K}": 12 * nnz + 4 * (n + 1) + 16 * K * n for K in widths})
    assert nbytes["spmv"] == s.get_int("spmv_bytes")
    spmv_ms = float(np.median(series["spmv"]))
    out = dict(grid=a.grid, n=n, nnz=nnz, rowblocks=s.get_int("rowblocks"), launches=a.launches, reps=a.reps)
    for name, v in series.items():
        ms = float(np.median(v))
        out[name] = dict(ms=ms, min_ms=float(min(v)), max_ms=float(max(v)), bytes=nbytes[name], tb_per_s=nbytes[name] / (ms * 1e-3) / 1e12,
                         frac_of_hbm_peak=nbytes[name] / (ms * 1e-3) / HBM_PEAK, ratio_to_spmv=ms / spmv_ms)
    s.close()
    line = json.dumps(out)
    print(line)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write(f"# python tools/probe_value_gradient.py --grid {a.grid} --reps {a.reps} --launches {a.launches}\n")
            for name, v in series.items():
                fh.write(f"# {name}: " + " ".join(f"{t:.4f}" for t in v) + " ms per launch\n")
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
