// Entry points of the tests and of timing: the arrays of the hierarchy and of the matrix, single products and preconditioner
// applications (parity / roofline), one kernel at a time under HIP events.  No solve goes through this unit.
#include "solver_impl.h"

#include <string.h>

#include <vector>

// ---------------------------------------------------------------- hierarchy introspection (tests)
extern "C" int64_t nkp_ml_level_array (nkp_solver *s, int level, const char *what, void *dst, int64_t capacity_bytes)
{
   if (!s || !what || s->opt.precond != NKP_PRECOND_MULTILEVEL || level < 0 || level >= (int) s->ml.lev.size ()) return fail (NKP_EINVAL, "nkp_ml_level_array: bad argument");
   const MlLevel &V = s->ml.lev[(size_t) level];
   const bool last = level == (int) s->ml.lev.size () - 1;
   const void *src = nullptr;
   int64_t count = 0;
   size_t elem = 4;
   bool host = false;
   int col_kernel[11];
   if (!strcmp (what, "rowptr")) { src = V.L.rowptr; count = V.n + 1; }
   else if (!strcmp (what, "colind")) { src = V.L.colind; count = V.L.nnz; }
   else if (!strcmp (what, "valf")) { src = V.L.valf; count = V.L.valf ? V.L.nnz : 0; }
   else if (!strcmp (what, "val")) { src = V.L.val; count = V.L.val ? V.L.nnz : 0; elem = 8; }
   else if (!strcmp (what, "dg_ptr")) { src = V.L.dg_ptr; count = src ? V.L.dg_ncol + 1 : 0; }
   else if (!strcmp (what, "dg_key")) { src = V.L.dg_key; count = src ? (int64_t) V.L.dg_nkey : 0; }
   else if (!strcmp (what, "dg_voff")) { src = V.L.dg_voff; count = src ? V.L.dg_ncol : 0; elem = 8; }
   else if (!strcmp (what, "dg_val")) { src = V.L.dg_val; count = src ? V.L.dg_nval : 0; }
   else if (!strcmp (what, "dg_gptr")) { src = V.L.dg_gptr; count = src ? V.L.dg_ncol + 1 : 0; }
   else if (!strcmp (what, "dg_grp")) { src = V.L.dg_grp; count = src ? 2 * (int64_t) V.L.dg_ngrp : 0; }
   else if (!strcmp (what, "cmap")) { src = V.cmap; count = V.cmap ? V.n : 0; }
   else if (!strcmp (what, "rptr")) { src = V.rptr; count = V.rptr ? V.nc + 1 : 0; }
   else if (!strcmp (what, "ridx")) { src = V.ridx; count = V.ridx ? V.n : 0; }
   else if (!strcmp (what, "blk_start")) { src = V.B.blk_start; count = V.B.blk_start ? V.B.nblk + 1 : 0; }
   else if (!strcmp (what, "fac")) { src = V.B.fac; count = V.B.fac ? (int64_t) (2 * V.B.P + 1) * V.n : 0; elem = 8; }
   else if (!strcmp (what, "perm0")) { src = level == 0 ? s->ml.perm0 : nullptr; count = src ? V.n : 0; }
   else if (!strcmp (what, "coarse_inv")) { src = last ? s->ml.coarse_inv : nullptr; count = src ? V.n * V.n : 0; elem = 8; }
   else if (!strcmp (what, "color_blk")) { src = V.B.blk_start ? V.color_blk : nullptr; count = src ? 3 : 0; host = true; }
   else if (!strcmp (what, "col_kernel")) {      // which column-solve kernels the level was given (read-only, host values)
      const ColBlocksDev &B = V.B;
      const int v[11] = { V.wave_columns ? 1 : 0, V.wave_fused ? 1 : 0, B.stream ? 1 : 0, B.ldsres, B.gw, B.P, B.dropped, B.max_len, B.gs_ok, B.ngrp, B.lds_doubles };
      memcpy (col_kernel, v, sizeof v);
      src = B.blk_start ? col_kernel : nullptr; count = src ? 11 : 0; host = true;
   }
   else if (!strcmp (what, "wave_diag")) { src = &V.wave_diag; count = 1; host = true; }      // 1: the half sweeps run gs_wave_diag_kernel
   else if (!strcmp (what, "lane_diag")) { src = &V.lane_diag; count = 1; host = true; }      // 1: the half sweeps run gs_lanes_diag_kernel
   else if (!strcmp (what, "grp_tile")) { src = V.B.grp_tile; count = src ? (int64_t) V.B.ngrp * V.B.gw : 0; }
   else return fail (NKP_EINVAL, "nkp_ml_level_array: unknown array '%s'", what);
   if (!dst) return count;
   if (count * (int64_t) elem > capacity_bytes) return fail (NKP_EINVAL, "nkp_ml_level_array: buffer too small");
   if (host) {                                  // kept on the host: no device call
      if (count) memcpy (dst, src, (size_t) count * elem);
      return count;
   }
   HIPCHK (hipSetDevice (s->device));
   HIPCHK (hipStreamSynchronize (s->stream));
   if (count) HIPCHK (hipMemcpy (dst, src, (size_t) count * elem, hipMemcpyDeviceToHost));
   return count;
}

// the per-column diagonals of the solver's own matrix (tuning spmv_diag), same contract as nkp_ml_level_array
extern "C" int64_t nkp_matrix_array (nkp_solver *s, const char *what, void *dst, int64_t capacity_bytes)
{
   if (!s || !what) return fail (NKP_EINVAL, "nkp_matrix_array: bad argument");
   const CsrDev &A = s->A;
   const bool have = A.dg_vald != nullptr;
   const void *src = nullptr;
   int64_t count = 0;
   size_t elem = 4;
   if (!strcmp (what, "dg_ptr")) { src = A.dg_ptr; count = have ? A.dg_ncol + 1 : 0; }
   else if (!strcmp (what, "dg_key")) { src = A.dg_key; count = have ? (int64_t) A.dg_nkey : 0; }
   else if (!strcmp (what, "dg_voff")) { src = A.dg_voff; count = have ? A.dg_ncol : 0; elem = 8; }
   else if (!strcmp (what, "dg_val")) { src = A.dg_vald; count = have ? A.dg_nval : 0; elem = 8; }
   else if (!strcmp (what, "dg_gptr")) { src = A.dg_gptr; count = have ? A.dg_ncol + 1 : 0; }
   else if (!strcmp (what, "dg_grp")) { src = A.dg_grp; count = have ? 2 * (int64_t) A.dg_ngrp : 0; }
   // A as it sits on the device in CSR (a transposed handle: the device transpose), and the band factors of column Jacobi
   else if (!strcmp (what, "rowptr")) { src = A.rowptr; count = src ? A.n + 1 : 0; }
   else if (!strcmp (what, "colind")) { src = A.colind; count = src ? A.nnz : 0; }
   else if (!strcmp (what, "val")) { src = A.val; count = src ? A.nnz : 0; elem = 8; }
   else if (!strcmp (what, "fac")) { src = s->opt.precond == NKP_PRECOND_COLUMN_JACOBI ? s->B.fac : nullptr; count = src ? (int64_t) (2 * s->B.P + 1) * s->B.n : 0; elem = 8; }
   else return fail (NKP_EINVAL, "nkp_matrix_array: unknown array '%s'", what);
   if (!dst) return count;
   if (count * (int64_t) elem > capacity_bytes) return fail (NKP_EINVAL, "nkp_matrix_array: buffer too small");
   HIPCHK (hipSetDevice (s->device));
   HIPCHK (hipStreamSynchronize (s->stream));
   if (count) HIPCHK (hipMemcpy (dst, src, (size_t) count * elem, hipMemcpyDeviceToHost));
   return count;
}

// ---------------------------------------------------------------- exposed pieces (parity / roofline)
extern "C" int nkp_spmv_device (nkp_solver *s, const void *d_x, void *d_y)
{
   if (!s || !d_x || !d_y) return fail (NKP_EINVAL, "nkp_spmv_device: NULL argument");
   HIPCHK (hipSetDevice (s->device));
   spmv_op (s, (const double *) d_x, (double *) d_y, nullptr, 0);
   HIPCHK (hipStreamSynchronize (s->stream));
   HIPCHK (hipGetLastError ());
   return NKP_OK;
}

extern "C" int nkp_spmv (nkp_solver *s, const double *x, double *y)
{
   if (!s || !x || !y) return fail (NKP_EINVAL, "nkp_spmv: NULL argument");
   HIPCHK (hipSetDevice (s->device));
   const size_t bytes = (size_t) s->n * sizeof (double);
   HIPCHK (hipMemcpyAsync (s->t1, x, bytes, hipMemcpyHostToDevice, s->stream));
   spmv_op (s, s->t1, s->t2, nullptr, 0);
   HIPCHK (hipMemcpyAsync (y, s->t2, bytes, hipMemcpyDeviceToHost, s->stream));
   HIPCHK (hipStreamSynchronize (s->stream));
   HIPCHK (hipGetLastError ());
   return NKP_OK;
}

extern "C" int nkp_precond_apply (nkp_solver *s, const double *r, double *z)
{
   if (!s || !r || !z) return fail (NKP_EINVAL, "nkp_precond_apply: NULL argument");
   if (s->shared->broken) return refactor_broken (s);
   HIPCHK (hipSetDevice (s->device));
   const size_t bytes = (size_t) s->n * sizeof (double);
   HIPCHK (hipMemcpyAsync (s->t1, r, bytes, hipMemcpyHostToDevice, s->stream));
   apply_precond_once (s, s->t1, s->t2);      // one cycle: what the parity tests and the cycle timing mean
   HIPCHK (hipMemcpyAsync (z, s->t2, bytes, hipMemcpyDeviceToHost, s->stream));
   HIPCHK (hipStreamSynchronize (s->stream));
   HIPCHK (hipGetLastError ());
   return NKP_OK;
}

extern "C" int nkp_multi_dot (nkp_solver *s, const double *V, int64_t ld, int k, const double *w, double *out)
{
   if (!s || !V || !w || !out || k < 0 || k > s->m + 1 || ld < s->n) return fail (NKP_EINVAL, "nkp_multi_dot: bad argument (k must be <= restart+1)");
   HIPCHK (hipSetDevice (s->device));
   std::vector<float> vf;
   for (int j = 0; j < k; j++) {
      if (s->vf32) {
         vf.assign (V + (int64_t) j * ld, V + (int64_t) j * ld + s->n);
         HIPCHK (hipMemcpyAsync ((float *) s->V + (int64_t) j * s->ld, vf.data (), (size_t) s->n * sizeof (float), hipMemcpyHostToDevice, s->stream));
         HIPCHK (hipStreamSynchronize (s->stream));        // vf is reused
      } else
         HIPCHK (hipMemcpyAsync (s->V + (int64_t) j * s->ld, V + (int64_t) j * ld, (size_t) s->n * sizeof (double), hipMemcpyHostToDevice, s->stream));
   }
   HIPCHK (hipMemcpyAsync (s->w, w, (size_t) s->n * sizeof (double), hipMemcpyHostToDevice, s->stream));
   launch_multi_dot (s->V, s->vf32, s->ld, k, s->w, s->n, s->partial, s->h_dev (), s->stream);
   allreduce_dev (s, s->h_dev (), k + 1, 0);
   HIPCHK (hipMemcpyAsync (out, s->h_dev (), (size_t) (k + 1) * sizeof (double), hipMemcpyDeviceToHost, s->stream));
   HIPCHK (hipStreamSynchronize (s->stream));
   HIPCHK (hipGetLastError ());
   return NKP_OK;
}

// The kernels of the K-vector calls on the pattern (operand_call.h), each at interleave width arg on scratch operands of its own:
// prepare checks the solver and arg and makes the operands, launch queues the kernel once.  A new kernel adds one row
struct TimedKernel { int which; int (*prepare) (nkp_solver *, int K, int which); void (*launch) (nkp_solver *, int K); };
const TimedKernel timed_kernels[] = {
   { 5, valgrad_time_prepare, valgrad_time_launch },                  // the gradient kernel of nkp_value_gradient
   { 6, valprod_time_prepare, valprod_time_launch },                  // the product kernel of nkp_values_product
   { 7, valprod_time_prepare, valprod_time_composition },             // what it replaces
   { 9, valprod_time_prepare, valprod_time_launch_trans },            // the same kernel on the transposed index with gathered values
   { 10, valprod_time_prepare, valprod_time_composition_trans },      // what that replaces
   { 11, residual_time_prepare, residual_time_launch },               // the kernel of nkp_residual_batch alone, R not written
   { 12, residual_time_prepare, residual_time_composition },          // the composition it replaces
};

extern "C" int nkp_time_kernel (nkp_solver *s, int which, int arg, int reps, double *avg_ms)
{
   if (!s || !avg_ms || reps < 1) return fail (NKP_EINVAL, "nkp_time_kernel: bad argument");
   if (which == 8 && !s->A.dg_vald) return fail (NKP_EINVAL, "nkp_time_kernel: the matrix has no per-column diagonals (tuning spmv_diag)");
   HIPCHK (hipSetDevice (s->device));
   const TimedKernel *tk = nullptr;
   for (const TimedKernel &row : timed_kernels)
      if (row.which == which) tk = &row;
   if (tk)
      if (const int prc = tk->prepare (s, arg, which)) return prc;
   StepEvent step_ev;
   if (which == 2) {
      const int erc = step_ev.make (s);
      if (erc) return erc;
   }
   hipEvent_t e0, e1;
   HIPCHK (hipEventCreate (&e0));
   HIPCHK (hipEventCreate (&e1));
   // operands: whatever is in the work vectors (made finite first)
   launch_fill (s->t1, 1.0, s->n, s->stream);
   if (which == 2) {
      if (arg < 0 || arg >= s->m) return fail (NKP_EINVAL, "nkp_time_kernel: restart position out of range");
      // finite operands in whichever basis precision is active (f32 vectors are filled through their f64 twin)
      for (int j = 0; j <= arg + 1; j++) {
         launch_fill (s->t2, 1.0 / (1.0 + j), s->n, s->stream);
         s->hpin[0] = 1.0;
         HIPCHK (hipMemcpyAsync (s->misc_dev () + 1, s->hpin, sizeof (double), hipMemcpyHostToDevice, s->stream));
         if (s->vf32) launch_scale_to (s->t2, s->misc_dev () + 1, s->vcur, (float *) s->V + (int64_t) j * s->ld, s->n, s->stream);
         else launch_scale_to (s->t2, s->misc_dev () + 1, s->V + (int64_t) j * s->ld, nullptr, s->n, s->stream);
         HIPCHK (hipStreamSynchronize (s->stream));
      }
   }
   for (int pass = 0; pass < 2; pass++) {      // pass 0 = warm-up
      const int cnt = pass == 0 ? (reps < 3 ? reps : 3) : reps;
      HIPCHK (hipEventRecord (e0, s->stream));
      for (int i = 0; i < cnt; i++) {
         if (which == 0 && s->A.dg_vald) launch_csr_spmv (s->A, s->t1, s->t2, nullptr, 0, s->stream);      // 0 stays the CSR kernel
         else if (which == 0) spmv_op (s, s->t1, s->t2, nullptr, 0);
         else if (which == 8) launch_diag_spmv (s->A, s->t1, s->t2, nullptr, 0, s->stream);
         else if (which == 1) apply_precond_once (s, s->t1, s->t2);
         else if (which == 2) {      // the step as fgmres runs it, the hand-over of the Hessenberg column to the host included
            const int src = arnoldi_hand_over (s, arg, step_ev.ev);
            if (src) { s->ml.entered = 0; return src; }
         }
         else if (tk) tk->launch (s, arg);
         else if (s->opt.precond == NKP_PRECOND_MULTILEVEL) ml_time_piece (s->ml, which - 3, s->stream);   // 3: smoother residual rows, 4: column solves (level 0, colour 0)
      }
      HIPCHK (hipEventRecord (e1, s->stream));
      HIPCHK (hipEventSynchronize (e1));
      float ms = 0.f;
      HIPCHK (hipEventElapsedTime (&ms, e0, e1));
      *avg_ms = (double) ms / cnt;
   }
   (void) hipEventDestroy (e0);
   (void) hipEventDestroy (e1);
   s->ml.entered = 0;      // which == 2: the cycle the last step entered ahead is dropped
   HIPCHK (hipGetLastError ());
   return NKP_OK;
}
