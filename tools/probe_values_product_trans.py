"""The kernel of nkp_values_product_trans next to the non-transposed product kernel and next to the composition it replaces,
on the bench's synthetic matrix.

One process, one solver without preconditioner (all three read the pattern only).  nkp_time_kernel times each piece alone with HIP
events on the solver's stream, `--launches` back-to-back launches after its own warm-up launches; the probe repeats that `--reps`
times, alternating the product kernel (which = 6), the same kernel on the transposed index with gathered values (which = 9) and the
composition that kernel replaces (which = 10: the values gathered into a temporary of nnz doubles, then the product kernel on the
transposed pattern) at K = 1, 2, 4, 8, and reports the median and the min-max of every series and the compulsory bytes of a launch:

    product           12 nnz + 4 (n + 1) + 16 K n
    transposed        12 nnz + 4 nnz (the value map) + 4 (n + 1) + 16 K n
    composition       the transposed product's + 16 nnz              (the temporary of nnz doubles written and read)

    python tools/probe_values_product_trans.py [--grid 320x384x60] [--reps 5] [--launches 100] [--log profiles/values_product_trans_1deg.log]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nk_ocn_tracer_jacobian_precond_amd import solver, synth  # noqa: E402

WHICH = dict(prod=6, trans=9, comp=10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="320x384x60")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    imt, jmt, km = (int(t) for t in a.grid.split("x"))
    p = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=0, isop_k33=True)
    n, nnz = p.flat_len, p.nnz
    s = solver.NkpSolver(p.rowptr, p.colind, p.nzval, None, precond=solver.PRECOND_NONE, restart=4)
    widths = (1, 2, 4, 8)
    series = {f"{name}_k{K}": [] for K in widths for name in WHICH}
    for K in widths:                                   # the index, work space and code objects before anything is timed
        for which in WHICH.values():
            s.time_kernel(which, reps=3, arg=K)
    for _ in range(a.reps):
        for K in widths:
            for name, which in WHICH.items():
                series[f"{name}_k{K}"].append(s.time_kernel(which, reps=a.launches, arg=K))
    out = dict(grid=a.grid, n=n, nnz=nnz, rowblocks=s.get_int("rowblocks"), launches=a.launches, reps=a.reps,
               trans_index_bytes=s.get_int("trans_index_bytes"), trans_index_us=s.get_int("trans_index_us"))
    for K in widths:
        base = 12 * nnz + 4 * (n + 1) + 16 * K * n
        nbytes = dict(prod=base, trans=base + 4 * nnz, comp=base + 20 * nnz)
        for name in WHICH:
            v = series[f"{name}_k{K}"]
            ms = float(np.median(v))
            out[f"{name}_k{K}"] = dict(ms=ms, min_ms=float(min(v)), max_ms=float(max(v)), bytes=nbytes[name], tb_per_s=nbytes[name] / (ms * 1e-3) / 1e12)
        out[f"trans_k{K}"]["ratio_to_product"] = out[f"trans_k{K}"]["ms"] / out[f"prod_k{K}"]["ms"]
        out[f"trans_k{K}"]["ratio_to_composition"] = out[f"trans_k{K}"]["ms"] / out[f"comp_k{K}"]["ms"]
    s.close()
    line = json.dumps(out)
    print(line)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write(f"# python tools/probe_values_product_trans.py --grid {a.grid} --reps {a.reps} --launches {a.launches}\n")
            for name, v in series.items():
                fh.write(f"# {name}: " + " ".join(f"{t:.4f}" for t in v) + " ms per launch\n")
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
