// nkp_values_product / nkp_values_product_device / nkp_solve_tangent_device (include/nkp.h): the product of caller-supplied values
// on the solver's pattern with K vectors, y_c (+)= alpha * (pattern with val) x_c, and with it the forward mode of a solve,
// dX = A^-1 (dB - dA X).  The kernel is valprod.hip; this unit checks the arguments, keeps the work space, fetches the halo rows
// of x on a row-distributed solver (fetch_x_operand, shared with nkp_value_gradient) and keeps the ranks together.  Only the
// pattern of the solver's matrix is read by the product.
// nkp_values_product_trans*: the same product with the transposed pattern, y_c (+)= alpha * (pattern with val)^T x_c, val still in
// A's order.  Same arguments, work space and kernel text; what it adds is the transposed index (solver_impl.h: vt) it builds at its
// first call, and the refusals of the handles that do not hold A's pattern themselves.
#include "solver_impl.h"
#include "transpose.h"

#include <stdlib.h>
#include <time.h>

namespace {

double seconds_between (const struct timespec &a, const struct timespec &b) { return (double) (b.tv_sec - a.tv_sec) + 1e-9 * (double) (b.tv_nsec - a.tv_nsec); }

// ---- the transposed index: the device transpose of the pattern (its values dropped), the row blocks from a host copy of rowptrT --
// those a solver created from the host transpose has.  All four arrays or none: after a failure the solver holds what it held and
// HIP's last error is cleared.  The ranking step of the device transpose reads A.val, which a solver keeps also when broken.
int trans_index_build (nkp_solver *s, const char *who)
{
   auto &I = s->vt;
   if (I.src) return NKP_OK;
   const int64_t n = s->n, nnz = s->A.nnz;
   hipStream_t st = s->stream;
   struct timespec t0, t1;
   clock_gettime (CLOCK_MONOTONIC, &t0);
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
   clock_gettime (CLOCK_MONOTONIC, &t1);
   I.build_seconds = seconds_between (t0, t1);
   msg (s, 1, "%s: transposed index of %lld entries, %d row blocks, %.1f MB, %.3f s\n", who, (long long) nnz, nrb, (double) I.bytes / 1.0e6, I.build_seconds);
   return NKP_OK;
}

// ---- (b) the operand x (single-GPU: interleaved; row-distributed: the halo rows, all vectors in one exchange), the kernel, and on
// a row-distributed solver the second agreement.  h_y: the host flavour's result, downloaded from Y (ld n) before the agreement
// trans: the product with the transposed pattern (single-GPU only; the index exists)
int product_run (nkp_solver *s, int nrhs, const double *val, const double *X, int64_t ldx, double alpha, int accumulate, double *Y, int64_t ldy,
                 double *h_y, int64_t h_ldy, const char *who, bool trans = false)
{
   const int K = width_of (nrhs);
   const int64_t n = s->n;
   hipStream_t st = s->stream;
   struct timespec ts0;
   clock_gettime (CLOCK_MONOTONIC, &ts0);
   const double *xp[NKP_BATCH_MAX] = {};
   for (int c = 0; c < nrhs; c++) xp[c] = X + (size_t) c * (size_t) ldx;
   const double *x_in = X;
   int rc = fetch_x_operand (s, K, xp, s->vp.x, &x_in, who);
   if (!rc) {
      if (trans) launch_values_product_trans (K, nrhs, s->vt.T, s->vt.src, val, x_in, alpha, accumulate, Y, ldy, st);
      else launch_values_product (K, nrhs, s->A, val, x_in, alpha, accumulate, Y, ldy, st);
      hipError_t e = hipSuccess;
      for (int c = 0; h_y && c < nrhs && e == hipSuccess && n; c++)
         e = hipMemcpyAsync (h_y + (size_t) c * (size_t) h_ldy, Y + (size_t) c * (size_t) ldy, (size_t) n * sizeof (double), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize (st);
      if (e == hipSuccess) e = hipGetLastError ();
      if (e != hipSuccess) rc = fail (NKP_EDEVICE, "%s: the product kernel or its copies failed: %s", who, hipGetErrorString (e));
   } else
      (void) hipStreamSynchronize (st);
   if (s->dist.on) rc = dist_agree (s, rc, who, "exchange and kernel");
   if (rc) return rc;
   struct timespec ts1;
   clock_gettime (CLOCK_MONOTONIC, &ts1);
   if (trans) {
      s->vt.seconds = seconds_between (ts0, ts1);
      s->vt.calls++;
   } else {
      s->vp.seconds = seconds_between (ts0, ts1);
      s->vp.calls++;
   }
   return NKP_OK;
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
   const bool host = h_y != nullptr;
   const bool dist = s->dist.on;
   auto &W = s->vp;
   const int64_t n = s->n, nnz = s->A.nnz;
   hipStream_t st = s->stream;

   // ---- (a) this rank's arguments (no HIP call), its work space, the host arrays staged on the device
   int rc = NKP_OK;
   if (nrhs < 1 || nrhs > NKP_BATCH_MAX) rc = fail (NKP_EINVAL, "%s: nrhs = %d, must be 1 .. %d (more vectors: call again)", who, nrhs, NKP_BATCH_MAX);
   else if (ldx < n) rc = fail (NKP_EINVAL, "%s: ldx = %lld < n = %lld", who, (long long) ldx, (long long) n);
   else if (ldy < n) rc = fail (NKP_EINVAL, "%s: ldy = %lld < n = %lld", who, (long long) ldy, (long long) n);
   else if (host ? (const double *) h_y == h_x : (const double *) d_y == d_x) rc = fail (NKP_EINVAL, "%s: y and x are the same buffer (the product is not done in place)", who);
   if (rc && !dist) return rc;
   const int K = width_of (nrhs);
   if (!rc && hipSetDevice (s->device) != hipSuccess) rc = fail (NKP_EDEVICE, "%s: hipSetDevice (%d) failed", who, s->device);
   const size_t vecs = rc ? 0 : (size_t) nrhs * (size_t) n;
   if (!rc && trans) rc = trans_index_build (s, who);
   if (!rc)
      rc = reserve (s, { { &W.x, &W.x_cap, !dist && K >= 2 ? (size_t) n * (size_t) K : 0 },      // K = 1 reads x in place; row-distributed: dist.xe / dist.bxe
                         { &W.stage, &W.stage_cap, host ? (size_t) nnz + 2 * vecs : 0 } }, who);
   if (!rc && dist && K >= 2 && s->dist.bK < K) rc = batch_prepare_exchange (s, K);
   const double *V = d_val, *X = d_x;
   double *Y = d_y;
   int64_t lx = ldx, ly = ldy;
   if (!rc && host) {
      const size_t bytes = (size_t) n * sizeof (double);
      double *sx = W.stage + (size_t) nnz, *sy = sx + vecs;
      hipError_t e = hipSuccess;
      if (nnz) e = hipMemcpyAsync (W.stage, h_val, (size_t) nnz * sizeof (double), hipMemcpyHostToDevice, st);
      for (int c = 0; c < nrhs && e == hipSuccess && bytes; c++) {
         e = hipMemcpyAsync (sx + (size_t) c * (size_t) n, h_x + (size_t) c * (size_t) ldx, bytes, hipMemcpyHostToDevice, st);
         if (e == hipSuccess && accumulate) e = hipMemcpyAsync (sy + (size_t) c * (size_t) n, h_y + (size_t) c * (size_t) ldy, bytes, hipMemcpyHostToDevice, st);
      }
      if (e != hipSuccess) rc = fail (NKP_EDEVICE, "%s: upload of the host arrays failed: %s", who, hipGetErrorString (e));
      V = W.stage; X = sx; Y = sy;
      lx = ly = n;
   }
   if (dist && (rc = dist_agree (s, rc, who, "arguments and work space"))) {
      // a rank whose K-wide exchange buffers are gone is not a rank "known to have buffers": the next batched solve agrees anew
      s->dist.agreed_K = 0;
      return rc;
   }
   if (rc) return rc;
   return product_run (s, nrhs, V, X, lx, alpha, accumulate, Y, ly, host ? h_y : nullptr, ldy, who, trans);
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

void valprod_release (nkp_solver *s)
{
   for (double **p : { &s->vp.x, &s->vp.stage, &s->vp.r })
      if (*p) { (void) hipFree (*p); *p = nullptr; }
   s->vp.x_cap = s->vp.stage_cap = s->vp.r_cap = 0;
   for (int **p : { &s->vt.T.rowptr, &s->vt.T.colind, &s->vt.T.rowblk, &s->vt.src, &s->vt.ship_e, &s->vt.ship_i })
      if (*p) { (void) hipFree (*p); *p = nullptr; }
   for (double **p : { &s->vt.xe, &s->vt.send })
      if (*p) { (void) hipFree (*p); *p = nullptr; }
   s->vt.T.nrowblk = 0;
   s->vt.bytes = s->vt.xe_cap = s->vt.send_cap = 0;
   s->vt.n_ship = s->vt.n_recv = 0;
}

int valprod_time_prepare (nkp_solver *s, int K, int which)
{
   if (s->dist.on) return fail (NKP_EINVAL, "nkp_time_kernel: the product kernel (which = %d) is timed on single-GPU solvers only", which);
   if (K != 1 && K != 2 && K != 4 && K != 8) return fail (NKP_EINVAL, "nkp_time_kernel: which = %d takes arg = K in {1, 2, 4, 8}", which);
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
   const bool dist = s->dist.on, has_dval = d_dval != nullptr;
   auto &W = s->vp;
   const int64_t n = s->n;
   hipStream_t st = s->stream;

   // ---- (a) arguments (no HIP call), work space, R = dB (or zero) in the solver's work space
   int rc = NKP_OK;
   if (nrhs < 1 || nrhs > NKP_BATCH_MAX) rc = fail (NKP_EINVAL, "%s: nrhs = %d, must be 1 .. %d", who, nrhs, NKP_BATCH_MAX);
   else if (ld < n) rc = fail (NKP_EINVAL, "%s: ld = %lld < n = %lld", who, (long long) ld, (long long) n);
   else if (has_dval && ldx < n) rc = fail (NKP_EINVAL, "%s: ldx = %lld < n = %lld", who, (long long) ldx, (long long) n);
   if (rc && !dist) return rc;
   const int K = width_of (nrhs);
   if (!rc && hipSetDevice (s->device) != hipSuccess) rc = fail (NKP_EDEVICE, "%s: hipSetDevice (%d) failed", who, s->device);
   if (!rc)
      rc = reserve (s, { { &W.x, &W.x_cap, has_dval && !dist && K >= 2 ? (size_t) n * (size_t) K : 0 }, { &W.r, &W.r_cap, (size_t) nrhs * (size_t) ld } }, who);
   if (!rc && has_dval && dist && K >= 2 && s->dist.bK < K) rc = batch_prepare_exchange (s, K);
   if (!rc) {
      const size_t bytes = (size_t) n * sizeof (double);
      hipError_t e = hipSuccess;
      for (int c = 0; c < nrhs && e == hipSuccess && bytes; c++) {
         double *rc_ = W.r + (size_t) c * (size_t) ld;
         e = d_db ? hipMemcpyAsync (rc_, (const double *) d_db + (size_t) c * (size_t) ld, bytes, hipMemcpyDeviceToDevice, st) : hipMemsetAsync (rc_, 0, bytes, st);
      }
      if (e != hipSuccess) rc = fail (NKP_EDEVICE, "%s: the copy of dB failed: %s", who, hipGetErrorString (e));
   }
   if (dist && (rc = tangent_agree (s, rc, has_dval, who))) {
      s->dist.agreed_K = 0;
      return rc;
   }
   if (rc) return rc;
   // ---- (b) R -= dA X: nkp_values_product_device (alpha = -1, accumulate = 1) on R; then the batched solve R -> dX
   if (has_dval && (rc = product_run (s, nrhs, (const double *) d_dval, (const double *) d_x, ldx, -1.0, 1, W.r, ld, nullptr, 0, who))) return rc;
   rc = nkp_solve_batch_device (s, nrhs, W.r, d_dx, ld, berr, iters, relres);
   if (rc >= 0) W.tangent_calls++;
   return rc;
}
