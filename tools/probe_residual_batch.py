"""The kernel of nkp_residual_batch next to the composition it replaces, on the bench's synthetic matrix.

One process, one solver without preconditioner (both read the matrix only).  nkp_time_kernel times each piece with HIP events on
the solver's stream, `--launches` back-to-back repetitions after its own warm-up; the probe repeats that `--reps` times,
alternating the kernel (which = 11) and the composition (which = 12: per column the b - A x and |A||x| + |b| products, the berr
pass and two dots) at K = 1, 2, 4, 8, and reports the median and the spread of every series, the ratio, the factor the compulsory
bytes predict, and the fraction of the 8 TB/s HBM peak on the compulsory bytes of the kernel:

    kernel        12 nnz + 4 (n + 1) + 16 K n                         (values, columns, row pointers, K-wide x and b once)
    composition   K (2 (12 nnz + 4 (n + 1) + 24 n) + 16 n + 24 n)     (two sweeps, each with x, b in and a vector out; berr and the dots)
    predicted     2 K 12 nnz / (12 nnz + 16 K n)                      (the factor the sweeps over A alone give)

    python tools/probe_residual_batch.py [--grid 320x384x60] [--reps 3] [--launches 200] [--log profiles/residual_batch_1deg.log]
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    imt, jmt, km = (int(t) for t in a.grid.split("x"))
    p = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=0, isop_k33=True)
    n, nnz = p.flat_len, p.nnz
    s = solver.NkpSolver(p.rowptr, p.colind, p.nzval, None, precond=solver.PRECOND_NONE, restart=4)
    widths = (1, 2, 4, 8)
    series = {}
    for K in widths:                                   # work space and code objects before anything is timed
        series[f"kernel_k{K}"], series[f"comp_k{K}"] = [], []
        s.time_kernel(11, reps=3, arg=K)
        s.time_kernel(12, reps=3, arg=K)
    for _ in range(a.reps):
        for K in widths:
            series[f"kernel_k{K}"].append(s.time_kernel(11, reps=a.launches, arg=K))
            series[f"comp_k{K}"].append(s.time_kernel(12, reps=a.launches, arg=K))
    out = dict(grid=a.grid, n=n, nnz=nnz, rowblocks=s.get_int("rowblocks"), launches=a.launches, reps=a.reps)
    for K in widths:
        kb = 12 * nnz + 4 * (n + 1) + 16 * K * n
        cb = K * (2 * (12 * nnz + 4 * (n + 1) + 24 * n) + 16 * n + 24 * n)
        k_ms, c_ms = float(np.median(series[f"kernel_k{K}"])), float(np.median(series[f"comp_k{K}"]))
        out[f"k{K}"] = dict(kernel_ms=k_ms, kernel_min_max_ms=[min(series[f"kernel_k{K}"]), max(series[f"kernel_k{K}"])], composition_ms=c_ms,
                            composition_min_max_ms=[min(series[f"comp_k{K}"]), max(series[f"comp_k{K}"])], speedup=c_ms / k_ms,
                            predicted=2 * K * 12 * nnz / (12 * nnz + 16 * K * n), kernel_bytes=kb, composition_bytes=cb,
                            kernel_tb_per_s=kb / (k_ms * 1e-3) / 1e12, kernel_frac_of_hbm_peak=kb / (k_ms * 1e-3) / HBM_PEAK,
                            composition_tb_per_s=cb / (c_ms * 1e-3) / 1e12)
    s.close()
    line = json.dumps(out)
    print(line)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write(f"# python tools/probe_residual_batch.py --grid {a.grid} --reps {a.reps} --launches {a.launches}\n")
            for name, v in series.items():
                fh.write(f"# {name}: " + " ".join(f"{t:.4f}" for t in v) + " ms per repetition\n")
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
