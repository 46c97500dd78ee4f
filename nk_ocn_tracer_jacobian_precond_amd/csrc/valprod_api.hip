// nkp_values_product / nkp_values_product_device / nkp_solve_tangent_device (include/nkp.h): the product of caller-supplied values
// on the solver's pattern with K vectors, y_c (+)= alpha * (pattern with val) x_c, and with it the forward mode of a solve,
// dX = A^-1 (dB - dA X).  The kernel is valprod.hip; this unit checks the arguments, keeps the work space, fetches the halo rows
// of x on a row-distributed solver (fetch_x_operand, shared with nkp_value_gradient) and keeps the ranks together.  Only the
// pattern of the solver's matrix is read by the product.
// nkp_values_product_trans*: the same product with the transposed pattern, y_c (+)= alpha * (pattern with val)^T x_c, val still in
// A's order.  Same arguments, work space and kernel text; what it adds is the transposed index (solver_impl.h: vt) it builds at its
// first call, and the refusals of the handles that do not hold A's pattern themselves.
#include "operand_call.h"
#include "transpose.h"

#include <stdlib.h>

namespace {

// ---- the transposed index: the device transpose of the pattern (its values dropped), the row blocks from a host copy of rowptrT --
// those a solver created from the host transpose has.  All four arrays or none: after a failure the solver holds what it held and
// HIP's last error is cleared.  The ranking step of the device transpose reads A.val, which a solver keeps also when broken.
int trans_index_build (nkp_solver *s, const char *who)
{
   auto &I = s->vt;
   if (I.src) return NKP_OK;
   const int64_t n = s->n, nnz = s->A.nnz;
   hipStream_t st = s->stream;
   const Stopwatch watch;
   mls::DBuf<int> rowptrT, colindT, src, rowblk;
   {
      mls::DBuf<double> valT;      // comes along with the transpose; freed here
      const int trc = transpose_device (s->A, n, rowptrT, colindT, valT, src, st);
      if (trc) {
         (void) hipStreamSynchronize (st);
         (void) hipGetLastError ();      // an out-of-memory error is sticky until read
         if (trc == (int) hipErrorOutOfMemory) return fail (NKP_ENOMEM, "%s: no device memory for the transposed index (%lld entries); the solver is unchanged", who, (long long) nnz);
         return fail (NKP_EDEVICE, "%s: the device transpose of the pattern failed (%s)", who, trc >= 1000 ? "inconsistent column counts" : hipGetErrorString ((hipError_t) trc));
      }
   }
   std::vector<int> h_rp ((size_t) n + 1);
   hipError_t e = hipMemcpy (h_rp.data (), rowptrT.p, h_rp.size () * sizeof (int), hipMemcpyDeviceToHost);
   int *h_rb = nullptr;
   int nrb = 0;
   if (e == hipSuccess) {
      build_rowblocks_host (n, h_rp.data (), &h_rb, &nrb);
      e = rowblk.alloc ((size_t) nrb + 1);
      if (e == hipSuccess) e = hipMemcpy (rowblk.p, h_rb, ((size_t) nrb + 1) * sizeof (int), hipMemcpyHostToDevice);
      free (h_rb);
   }
   if (e != hipSuccess) {
      (void) hipGetLastError ();
      return fail (e == hipErrorOutOfMemory ? NKP_ENOMEM : NKP_EDEVICE, "%s: the row blocks of the transposed index failed: %s; the solver is unchanged", who, hipGetErrorString (e));
   }
   // as the allocations were made: a buffer of no element holds one
   I.bytes = (((size_t) n + 1) + 2 * (size_t) (nnz ? nnz : 1) + ((size_t) nrb + 1)) * sizeof (int);
   I.T.n = n;
   I.T.nnz = nnz;
   I.T.rowptr = rowptrT.release ();
   I.T.colind = colindT.release ();
   I.T.rowblk = rowblk.release ();
   I.T.nrowblk = nrb;
   I.src = src.release ();
   s->device_bytes += I.bytes;
   I.build_seconds = watch.seconds ();
   msg (s, 1, "%s: transposed index of %lld entries, %d row blocks, %.1f MB, %.3f s\n", who, (long long) nnz, nrb, (double) I.bytes / 1.0e6, I.build_seconds);
   return NKP_OK;
}

// ---- (b) the operand x (single-GPU: interleaved; row-distributed: the halo rows, all vectors in one exchange), the kernel, and on
// a row-distributed solver the second agreement; the time of a product runs from here.  h_y: the host flavour's result, downloaded
// from Y (ld n) before the agreement.  trans: the product with the transposed pattern (single-GPU only; the index exists)
int product_run (OperandCall &c, const double *val, const double *X, int64_t ldx, double alpha, int accumulate, double *Y, int64_t ldy, double *h_y,
                 int64_t h_ldy, bool trans = false)
{
   nkp_solver *s = c.s;
   hipStream_t st = s->stream;
   c.watch.start ();
   const double *xp[NKP_BATCH_MAX] = {};
   for (int k = 0; k < c.nrhs; k++) xp[k] = X + (size_t) k * (size_t) ldx;
   const double *x_in = X;
   c.rc = fetch_x_operand (s, c.K, xp, s->vp.x, &x_in, c.who);
   hipError_t e = hipSuccess;
   if (!c.rc) {
      if (trans) launch_values_product_trans (c.K, c.nrhs, s->vt.T, s->vt.src, val, x_in, alpha, accumulate, Y, ldy, st);
      else launch_values_product (c.K, c.nrhs, s->A, val, x_in, alpha, accumulate, Y, ldy, st);
      if (h_y) e = download_columns (h_y, h_ldy, Y, c.nrhs, s->n, st);
   }
   return c.finish (e, "product", "exchange and kernel", trans ? s->vt.seconds : s->vp.seconds, trans ? s->vt.calls : s->vp.calls);
}

// Host flavour: h_* given, d_* NULL; device flavour the other way round.  The entry points have refused NULL arguments on the
// calling rank, before the solver is looked at and before any collective.  trans: nkp_values_product_trans*, refused here on the
// handles that do not hold A's pattern themselves and on row-distributed solvers (on the calling rank, no collective)
int values_product (nkp_solver *s, int nrhs, const double *h_val, const double *h_x, const double *d_val, const double *d_x, int64_t ldx, double alpha,
                    int accumulate, double *h_y, double *d_y, int64_t ldy, const char *who, bool trans = false)
{
   if (trans) {
      if (s->borrowed) return fail (NKP_EINVAL, "%s: a clone shares its matrix; call it on the solver it was cloned from", who);
      if (s->trans_of)
         return fail (NKP_EINVAL, "%s: this solver is itself a transposed handle; call it on the solver it was transposed from (or nkp_values_product here, with values in A^T's order)", who);
      if (s->dist.on)
         return fail (NKP_EINVAL, "%s: not available for the row-distributed flavour (the product with the transposed pattern sends products back to the owners of their columns, a collective of its own); call nkp_values_product_trans_dist%s on every rank", who, h_y ? "" : "_device");
   }
   OperandCall c (s, who, nrhs, h_y != nullptr);
   const int64_t n = s->n;

   // ---- (a) this rank's arguments, for the transposed product its index, the work space, the host arrays staged on the device
   int rc = refuse_nrhs (who, nrhs, " (more vectors: call again)");
   if (!rc) rc = refuse_ld (who, "ldx", ldx, "n", n);
   if (!rc) rc = refuse_ld (who, "ldy", ldy, "n", n);
   if (!rc && (c.host ? (const double *) h_y == h_x : (const double *) d_y == d_x)) rc = fail (NKP_EINVAL, "%s: y and x are the same buffer (the product is not done in place)", who);
   if (c.begin (rc)) return c.rc;
   if (!c.rc && trans) c.rc = trans_index_build (s, who);
   ProductOperands o = { d_val, d_x, d_y, ldx, ldy };
   product_stage (c, { &s->vp.x, &s->vp.x_cap, !c.dist && c.K >= 2 ? (size_t) n * (size_t) c.K : 0 },      // K = 1 reads x in place; row-distributed: dist.xe / dist.bxe
                  h_val, h_x, h_y, accumulate, o, true);
   if (c.agree ("arguments and work space")) return c.rc;
   return product_run (c, o.val, o.x, o.ldx, alpha, accumulate, o.y, o.ldy, h_y, ldy, trans);
}

// The first agreement of a tangent solve: every rank learns whether any rank's step failed AND whether all ranks pass d_dval alike
// (a rank without it would not join the exchange of the product, and the others would wait for it)
int tangent_agree (nkp_solver *s, int local_rc, bool has_dval, const char *who)
{
   std::vector<int64_t> all;
   if (const int rc = dist_allgather (s, local_rc, has_dval ? 2 : 1, all, who, "arguments and work space")) return rc;
   const int bad = failed_rank (all);
   if (bad >= 0) return fail (NKP_ECOMM, "%s: rank %d failed (arguments and work space); see its message", who, bad);
   for (int p = 1; p < s->dist.ops.nranks; p++)
      if (all[(size_t) p] != all[0])
         return fail (NKP_EINVAL, "%s: rank %d passes d_dval %s and rank 0 %s: every rank must pass it or every rank NULL", who, p,
                      all[(size_t) p] == 2 ? "non-NULL" : "NULL", all[0] == 2 ? "non-NULL" : "NULL");
   return NKP_OK;
}

}   // namespace

void product_stage (OperandCall &c, Want xbuf, const double *h_val, const double *h_x, const double *h_y, int accumulate, ProductOperands &o, bool fetch)
{
   nkp_solver *s = c.s;
   auto &W = s->vp;
   const int64_t n = s->n;
   const size_t nnz = (size_t) s->A.nnz, vecs = c.rc ? 0 : (size_t) c.nrhs * (size_t) n;
   c.reserve ({ xbuf, { &W.stage, &W.stage_cap, c.host ? nnz + 2 * vecs : 0 } }, fetch);
   if (c.rc || !c.host) return;
   double *sx = W.stage + nnz, *sy = sx + vecs;
   hipError_t e = nnz ? hipMemcpyAsync (W.stage, h_val, nnz * sizeof (double), hipMemcpyHostToDevice, s->stream) : hipSuccess;
   if (e == hipSuccess) e = upload_columns (sx, h_x, o.ldx, c.nrhs, n, s->stream);
   if (e == hipSuccess && accumulate) e = upload_columns (sy, h_y, o.ldy, c.nrhs, n, s->stream);
   c.uploaded (e, "arrays");
   o = { W.stage, sx, sy, n, n };
}

void valprod_release (nkp_solver *s)
{
   auto &W = s->vp;
   auto &I = s->vt;
   release_buffers (s, { { &W.x, &W.x_cap, 0 }, { &W.stage, &W.stage_cap, 0 }, { &W.r, &W.r_cap, 0 }, { &I.xe, &I.xe_cap, 0 }, { &I.send, &I.send_cap, 0 } });
   for (int **p : { &I.T.rowptr, &I.T.colind, &I.T.rowblk, &I.src, &I.ship_e, &I.ship_i })
      if (*p) { (void) hipFree (*p); *p = nullptr; }
   s->device_bytes -= I.bytes;      // the index, counted when it was built
   I.T.nrowblk = 0;
   I.bytes = 0;
   s->vt.n_ship = s->vt.n_recv = 0;
}

int valprod_time_prepare (nkp_solver *s, int K, int which)
{
   if (const int wrc = time_width_ok (s, K, which, "product")) return wrc;
   const size_t kn = (size_t) K * (size_t) s->n, il = K >= 2 ? kn : 0, nnz = (size_t) s->A.nnz;
   if (which == 9 || which == 10) {
      if (s->borrowed || s->trans_of) return fail (NKP_EINVAL, "nkp_time_kernel: which = %d is timed on the solver that owns A's pattern, not on a clone or a transposed handle", which);
      if (const int irc = trans_index_build (s, "nkp_time_kernel")) return irc;
   }
   // values | y, and for the composition | the temporary product, interleaved | the same, one vector after the other (7) or | the
   // gathered values (10)
   const int rc = reserve (s, { { &s->vp.x, &s->vp.x_cap, il }, { &s->vp.stage, &s->vp.stage_cap, nnz + (which == 7 ? 3 : 1) * kn + (which == 10 ? nnz : 0) } }, "nkp_time_kernel");
   if (rc) return rc;
   if (nnz) launch_fill (s->vp.stage, 1.0, (int64_t) nnz, s->stream);
   if (kn) launch_fill (s->vp.stage + nnz, 1.0, (int64_t) kn, s->stream);
   if (il) launch_fill (s->vp.x, 1.0, (int64_t) il, s->stream);
   return NKP_OK;
}

// values = 1 in the staging buffer, y behind them; K = 1 reads the solver's work vector t1 (filled by nkp_time_kernel) as x
void valprod_time_launch (nkp_solver *s, int K)
{
   launch_values_product (K, K, s->A, s->vp.stage, K >= 2 ? s->vp.x : s->t1, -1.0, 0, s->vp.stage + (size_t) s->A.nnz, s->n, s->stream);
}

// which = 7, measurement only: what the product kernel replaces, from the SpMV kernels on the solver's own values -- the (batched)
// operator product into a temporary, its de-interleave, and one update pass y += alpha t over the K vectors
void valprod_time_composition (nkp_solver *s, int K)
{
   const size_t kn = (size_t) K * (size_t) s->n;
   double *y = s->vp.stage + (size_t) s->A.nnz, *til = y + kn, *t = til + kn;
   hipStream_t st = s->stream;
   if (K == 1) launch_csr_spmv (s->A, s->t1, t, nullptr, 0, st);
   else {
      double *cols[NKP_BATCH_MAX] = {};
      for (int c = 0; c < K; c++) cols[c] = t + (size_t) c * (size_t) s->n;
      launch_csr_spmv_batch (K, s->A, 0, s->A.nrowblk, s->vp.x, til, nullptr, 0, st);
      launch_deinterleave (K, til, cols, s->n, st);
   }
   launch_axpby (-1.0, t, 1.0, y, (int64_t) kn, st);
}

// which = 9: values = 1 in A's order, gathered by the kernel; which = 10: gathered into the temporary behind y first
void valprod_time_launch_trans (nkp_solver *s, int K)
{
   launch_values_product_trans (K, K, s->vt.T, s->vt.src, s->vp.stage, K >= 2 ? s->vp.x : s->t1, -1.0, 0, s->vp.stage + (size_t) s->A.nnz, s->n, s->stream);
}

void valprod_time_composition_trans (nkp_solver *s, int K)
{
   const size_t nnz = (size_t) s->A.nnz;
   double *y = s->vp.stage + nnz, *valT = y + (size_t) K * (size_t) s->n;
   launch_tr_gather (s->vp.stage, s->vt.src, (int64_t) nnz, valT, s->stream);
   launch_values_product (K, K, s->vt.T, valT, K >= 2 ? s->vp.x : s->t1, -1.0, 0, y, s->n, s->stream);
}

extern "C" int nkp_values_product_device (nkp_solver *s, int nrhs, const void *d_val, const void *d_x, int64_t ldx, double alpha, int accumulate, void *d_y, int64_t ldy)
{
   if (!s) return fail (NKP_EINVAL, "nkp_values_product_device: NULL solver (argument s)");
   if (!d_val) return fail (NKP_EINVAL, "nkp_values_product_device: NULL argument d_val");
   if (!d_x) return fail (NKP_EINVAL, "nkp_values_product_device: NULL argument d_x");
   if (!d_y) return fail (NKP_EINVAL, "nkp_values_product_device: NULL argument d_y");
   return values_product (s, nrhs, nullptr, nullptr, (const double *) d_val, (const double *) d_x, ldx, alpha, accumulate, nullptr, (double *) d_y, ldy, "nkp_values_product_device");
}

extern "C" int nkp_values_product (nkp_solver *s, int nrhs, const double *val, const double *x, int64_t ldx, double alpha, int accumulate, double *y, int64_t ldy)
{
   if (!s) return fail (NKP_EINVAL, "nkp_values_product: NULL solver (argument s)");
   if (!val) return fail (NKP_EINVAL, "nkp_values_product: NULL argument val");
   if (!x) return fail (NKP_EINVAL, "nkp_values_product: NULL argument x");
   if (!y) return fail (NKP_EINVAL, "nkp_values_product: NULL argument y");
   return values_product (s, nrhs, val, x, nullptr, nullptr, ldx, alpha, accumulate, y, nullptr, ldy, "nkp_values_product");
}

extern "C" int nkp_values_product_trans_device (nkp_solver *s, int nrhs, const void *d_val, const void *d_x, int64_t ldx, double alpha, int accumulate, void *d_y, int64_t ldy)
{
   if (!s) return fail (NKP_EINVAL, "nkp_values_product_trans_device: NULL solver (argument s)");
   if (!d_val) return fail (NKP_EINVAL, "nkp_values_product_trans_device: NULL argument d_val");
   if (!d_x) return fail (NKP_EINVAL, "nkp_values_product_trans_device: NULL argument d_x");
   if (!d_y) return fail (NKP_EINVAL, "nkp_values_product_trans_device: NULL argument d_y");
   return values_product (s, nrhs, nullptr, nullptr, (const double *) d_val, (const double *) d_x, ldx, alpha, accumulate, nullptr, (double *) d_y, ldy,
                          "nkp_values_product_trans_device", true);
}

extern "C" int nkp_values_product_trans (nkp_solver *s, int nrhs, const double *val, const double *x, int64_t ldx, double alpha, int accumulate, double *y, int64_t ldy)
{
   if (!s) return fail (NKP_EINVAL, "nkp_values_product_trans: NULL solver (argument s)");
   if (!val) return fail (NKP_EINVAL, "nkp_values_product_trans: NULL argument val");
   if (!x) return fail (NKP_EINVAL, "nkp_values_product_trans: NULL argument x");
   if (!y) return fail (NKP_EINVAL, "nkp_values_product_trans: NULL argument y");
   return values_product (s, nrhs, val, x, nullptr, nullptr, ldx, alpha, accumulate, y, nullptr, ldy, "nkp_values_product_trans", true);
}

extern "C" int nkp_solve_tangent_device (nkp_solver *s, int nrhs, const void *d_dval, const void *d_x, int64_t ldx, const void *d_db, void *d_dx, int64_t ld,
                                         double *berr, int *iters, double *relres)
{
   const char *who = "nkp_solve_tangent_device";
   if (!s) return fail (NKP_EINVAL, "%s: NULL solver (argument s)", who);
   if (!d_dx) return fail (NKP_EINVAL, "%s: NULL argument d_dx", who);
   if (!d_dval && !d_db) return fail (NKP_EINVAL, "%s: d_dval and d_db are both NULL: there is no tangent to solve for", who);
   if (d_dval && !d_x) return fail (NKP_EINVAL, "%s: NULL argument d_x (needed with d_dval)", who);
   OperandCall c (s, who, nrhs, false);
   const bool has_dval = d_dval != nullptr;
   auto &W = s->vp;
   const int64_t n = s->n;
   hipStream_t st = s->stream;

   // ---- (a) arguments, work space, R = dB (or zero) in the solver's work space
   int rc = refuse_nrhs (who, nrhs, "");
   if (!rc) rc = refuse_ld (who, "ld", ld, "n", n);
   if (!rc && has_dval) rc = refuse_ld (who, "ldx", ldx, "n", n);
   if (c.begin (rc)) return c.rc;
   c.reserve ({ { &W.x, &W.x_cap, has_dval && !c.dist && c.K >= 2 ? (size_t) n * (size_t) c.K : 0 }, { &W.r, &W.r_cap, (size_t) nrhs * (size_t) ld } }, has_dval);
   if (!c.rc) {
      const size_t bytes = (size_t) n * sizeof (double);
      hipError_t e = hipSuccess;
      for (int k = 0; k < nrhs && e == hipSuccess && bytes; k++) {
         double *rk = W.r + (size_t) k * (size_t) ld;
         e = d_db ? hipMemcpyAsync (rk, (const double *) d_db + (size_t) k * (size_t) ld, bytes, hipMemcpyDeviceToDevice, st) : hipMemsetAsync (rk, 0, bytes, st);
      }
      if (e != hipSuccess) c.rc = fail (NKP_EDEVICE, "%s: the copy of dB failed: %s", who, hipGetErrorString (e));
   }
   if (c.agreed (c.dist ? tangent_agree (s, c.rc, has_dval, who) : c.rc)) return c.rc;
   // ---- (b) R -= dA X: nkp_values_product_device (alpha = -1, accumulate = 1) on R; then the batched solve R -> dX
   if (has_dval && product_run (c, (const double *) d_dval, (const double *) d_x, ldx, -1.0, 1, W.r, ld, nullptr, 0)) return c.rc;
   rc = nkp_solve_batch_device (s, nrhs, W.r, d_dx, ld, berr, iters, relres);
   if (rc >= 0) W.tangent_calls++;
   return rc;
}
