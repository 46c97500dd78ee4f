#!/usr/bin/env python3
"""Run under `rocprofv3 --pmc FETCH_SIZE`, `--pmc WRITE_SIZE` and `--pmc SQ_INSTS_VMEM_RD SQ_WAVES` (separate passes, no
tracing): launches the product with A of the 1 degree bench workload on its per-column diagonals (tuning spmv_diag,
diag_residual_kernel<double, 0>) and on CSR (csr_spmv_pipe_kernel<0, double, false>), plus a 16 B/lane calibration stream
(scale_to_kernel inside one Krylov step), as tools/pmc_spmv.py does for the CSR kernel alone."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nk_ocn_tracer_jacobian_precond_amd import solver, synth
p = synth.generate(imt=320, jmt=384, km=60, adv="upwind3", hmix="isop", seed=0, isop_k33=True)
blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
s = solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, precond=solver.PRECOND_COLUMN_JACOBI, restart=8)
assert s.get_int("spmv_diag") == 1
print("n", p.flat_len, "nnz", p.nnz, "spmv_bytes", s.get_int("spmv_bytes"), "spmv_diag_bytes", s.get_int("spmv_diag_bytes"))
print("columns", s.matrix_array("dg_ptr").size - 1, "keys", s.matrix_array("dg_key").size, "groups", s.matrix_array("dg_grp").size // 2)
print("spmv_diag_ms", s.time_kernel(8, reps=40))
print("spmv_csr_ms", s.time_kernel(0, reps=40))
print("step_ms", s.time_kernel(2, reps=5, arg=3))
