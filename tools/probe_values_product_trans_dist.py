"""What nkp_values_product_trans_dist_device costs on the bench's synthetic matrix cut into latitude bands.

The ranks share ONE GPU over the library's file transport: every collective is staged through host memory and files.  The
numbers are those of a host-staged transport with ranks sharing a GPU, not a multi-GPU result.  Each rank creates a solver
(water-column Jacobi: nothing here solves), builds the transposed index with a first call and reports, per nrhs, the median of
--reps values of "values_product_trans_us" (the library's wall clock around a call, exchange and agreements included), next to
nkp_values_product_device's "values_product_us" on the same operands, the index's bytes and build time and the entries shipped
and received.  One JSON line per rank.

    python tools/probe_values_product_trans_dist.py [--grid 320x384x60] [--reps 5] [--ranks 2]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spawn(a):
    """one child process per rank (the parent never opens the GPU)"""
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for r in range(a.ranks):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(a.ranks), NKP_PROBE_DIR=tmp, NKP_COMM_TIMEOUT="600", OMP_NUM_THREADS="4")
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env))
        return max(p.wait(timeout=1500) for p in procs)


def rank_main(a):
    from nk_ocn_tracer_jacobian_precond_amd import dist as nd
    from nk_ocn_tracer_jacobian_precond_amd import solver, synth

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    lib = solver.load_library()
    assert lib.nkp_set_device(0) == 0
    lib.nkp_comm_file_init.argtypes = [C.POINTER(solver.NkpCommOps), C.c_char_p, C.c_int, C.c_int]
    lib.nkp_comm_file_free.argtypes = [C.POINTER(solver.NkpCommOps)]
    lib.nkp_comm_file_free.restype = None
    ops = solver.NkpCommOps()
    assert lib.nkp_comm_file_init(C.byref(ops), os.environ["NKP_PROBE_DIR"].encode(), rank, world) == 0
    comm = types.SimpleNamespace(ops=ops, errors=[])
    hip = C.CDLL("libamdhip64.so")

    def device(arr):
        arr = np.ascontiguousarray(arr, np.float64)
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(max(arr.nbytes, 8))) == 0
        assert hip.hipMemcpy(p, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes), 1) == 0
        return p

    imt, jmt, km = (int(t) for t in a.grid.split("x"))
    p = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=0, isop_k33=True)
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    starts = nd.snap_partition(blk, world)
    loc = nd.local_slice(p.rowptr, p.colind, p.nzval, blk, starts, rank, ci, cj)
    n, m = p.flat_len, int(loc["m_loc"])
    s = nd.NkpDistSolver(loc, n, comm, precond=solver.PRECOND_COLUMN_JACOBI, restart=4)
    rng = np.random.default_rng(3 + rank)
    dv, dx, dy = device(loc["val"]), device(rng.standard_normal((8, m))), device(np.zeros((8, m)))
    s.values_product_trans_dist_device(dv.value, dx.value, 1, m, dy.value, m)         # builds the index
    out = dict(grid=a.grid, ranks=world, rank=rank, m_loc=m, nnz_loc=int(loc["colind"].size), halo_rows=s.get_int("dist_halo_rows"),
               transport="file transport, host-staged; ranks share one GPU", trans_index_bytes=s.get_int("trans_index_bytes"),
               trans_index_us=s.get_int("trans_index_us"), sent_entries=s.get_int("trans_index_sent_entries"), recv_entries=s.get_int("trans_index_recv_entries"))
    for K in (1, 2, 4, 8):
        s.values_product_trans_dist_device(dv.value, dx.value, K, m, dy.value, m)     # work space of this width
        s.values_product_device(dv.value, dx.value, K, m, dy.value, m)
        t, f = [], []
        for _ in range(a.reps):
            s.values_product_trans_dist_device(dv.value, dx.value, K, m, dy.value, m)
            t.append(s.get_int("values_product_trans_us"))
            s.values_product_device(dv.value, dx.value, K, m, dy.value, m)
            f.append(s.get_int("values_product_us"))
        out[f"values_product_trans_us_K{K}"] = [float(np.median(t)), min(t), max(t)]
        out[f"values_product_us_K{K}"] = [float(np.median(f)), min(f), max(f)]
    out["device_bytes"] = s.get_int("device_bytes")
    out["comm_errors"] = comm.errors
    s.close()
    print(json.dumps(out), flush=True)
    lib.nkp_comm_file_free(C.byref(ops))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="320x384x60")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ranks", type=int, default=2)
    a = ap.parse_args()
    if "RANK" not in os.environ:
        sys.exit(spawn(a))
    rank_main(a)


if __name__ == "__main__":
    main()
