// nkp_residual_batch / nkp_residual_batch_device (include/nkp.h): for nrhs given solutions X of A X = B under the matrix the handle
// solves with now, the residuals R = B - A X (when asked), ||r_c||, ||b_c|| and the componentwise backward error of every column, all
// from ONE pass over A.  The kernel is residual.hip; this unit checks the arguments, keeps the work space, fetches the halo rows of X
// on a row-distributed solver (fetch_x_operand, shared with nkp_value_gradient and nkp_values_product), reduces the norms and the
// backward errors across the ranks and keeps the ranks together.  A.val is the unscaled matrix whatever equil is: the row scaling of
// the row-weighted iteration lives in vectors of its own (rscale, rinv) and is applied to vectors only.
#include "operand_call.h"

#include <math.h>

namespace {

// Host flavour: h_* given, d_* NULL; device flavour the other way round.  The entry points have refused NULL B and X on the calling
// rank, before the solver is looked at and before any collective
int residual_batch (nkp_solver *s, int nrhs, const double *h_B, const double *h_X, double *h_R, const double *d_B, const double *d_X, double *d_R, int64_t ldb,
                    int64_t ldx, int64_t ldr, double *rnorm, double *bnorm, double *berr, const char *who)
{
   OperandCall c (s, who, nrhs, h_B != nullptr);
   const bool host = c.host, dist = c.dist;
   const bool want_r = host ? h_R != nullptr : d_R != nullptr;
   auto &W = s->rb;
   const int64_t n = s->n;
   hipStream_t st = s->stream;

   // ---- (a) this rank's arguments, its work space, the host arrays staged on the device (B | X | R, ld n)
   int rc = refuse_nrhs (who, nrhs, " (more vectors: call again)");
   if (!rc) rc = refuse_ld (who, "ldb", ldb, "n", n);
   if (!rc) rc = refuse_ld (who, "ldx", ldx, "n", n);
   if (!rc && want_r) rc = refuse_ld (who, "ldr", ldr, "n", n);
   if (!rc && want_r && (host ? (const double *) h_R == h_X : (const double *) d_R == d_X))
      rc = fail (NKP_EINVAL, "%s: R and X are the same buffer (other rows still gather x; R may be B)", who);
   if (!rc && !want_r && !rnorm && !bnorm && !berr) rc = fail (NKP_EINVAL, "%s: R, rnorm, bnorm and berr are all NULL: nothing is asked for", who);
   if (!rc && s->shared->broken) rc = refactor_broken (s);
   if (c.begin (rc)) return c.rc;
   const int K = c.K;
   const size_t vecs = c.rc ? 0 : (size_t) nrhs * (size_t) n, nrb = (size_t) (s->A.nrowblk > 0 ? s->A.nrowblk : 0);
   c.reserve ({ { &W.x, &W.x_cap, !dist && K >= 2 ? (size_t) n * (size_t) K : 0 },      // K = 1 reads x in place; row-distributed: dist.xe / dist.bxe
                { &W.partial, &W.partial_cap, 3 * (size_t) K * (nrb + 1) }, { &W.stage, &W.stage_cap, host ? (want_r ? 3 : 2) * vecs : 0 } }, true);
   const double *B = d_B, *X = d_X;
   double *R = d_R;
   int64_t lb = ldb, lx = ldx, lr = ldr;
   if (!c.rc && host) {
      double *sb = W.stage, *sx = sb + vecs;
      B = sb; X = sx; R = want_r ? sx + vecs : nullptr;
      lb = lx = lr = n;
      hipError_t e = upload_columns (sb, h_B, ldb, nrhs, n, st);
      if (e == hipSuccess) e = upload_columns (sx, h_X, ldx, nrhs, n, st);
      c.uploaded (e, "arrays");
   }
   if (c.agree ("arguments, work space, staging")) return c.rc;

   // ---- (b) the operand x (single-GPU: interleaved; row-distributed: the halo rows, all vectors in one exchange), the kernel, the
   // reductions across the ranks, the results; on a row-distributed solver every callback is reached whatever happened locally
   double *out = W.partial + 3 * (size_t) K * nrb;
   const double *xp[NKP_BATCH_MAX] = {};
   for (int k = 0; k < nrhs; k++) xp[k] = X + (size_t) k * (size_t) lx;
   const double *x_in = X;
   c.rc = fetch_x_operand (s, K, xp, W.x, &x_in, who);
   if (!c.rc) launch_residual_batch (K, nrhs, s->A, x_in, B, lb, R, lr, W.partial, out, st);
   if (dist) {
      // like allreduce_dev, but a failure is this call's alone (not sticky): the solver's later solves reduce anew
      auto &ops = s->dist.ops;
      s->shared->allreduce_calls++;
      const int c1 = ops.allreduce (ops.ctx, out, 2 * K, 0, (void *) st);
      s->shared->allreduce_calls++;
      const int c2 = ops.allreduce (ops.ctx, out + 2 * K, K, 1, (void *) st);
      if (!c.rc && (c1 || c2)) c.rc = fail (NKP_ECOMM, "%s: the allreduce of the %s failed", who, c1 ? "squared norms" : "backward errors");
   }
   double res[3 * NKP_BATCH_MAX] = {};
   hipError_t e = hipSuccess;
   if (!c.rc) {
      e = hipMemcpyAsync (res, out, 3 * (size_t) K * sizeof (double), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess && host && want_r) e = download_columns (h_R, ldr, R, nrhs, n, st);
   }
   if (c.finish (e, "residual", "exchange, kernel, reductions", W.seconds, W.calls)) return c.rc;
   for (int k = 0; k < nrhs; k++) {
      if (rnorm) rnorm[k] = sqrt (res[k]);
      if (bnorm) bnorm[k] = sqrt (res[K + k]);
      if (berr) berr[k] = res[2 * K + k];
   }
   return NKP_OK;
}

}   // namespace

void residual_release (nkp_solver *s)
{
   auto &W = s->rb;
   release_buffers (s, { { &W.x, &W.x_cap, 0 }, { &W.partial, &W.partial_cap, 0 }, { &W.stage, &W.stage_cap, 0 } });
}

// B (K vectors) in the staging buffer, for the composition the K plain vectors of X behind them; the kernel reads the interleaved
// copy, K = 1 the solver's work vector t1 (filled by nkp_time_kernel)
int residual_time_prepare (nkp_solver *s, int K, int which)
{
   if (const int rc = time_width_ok (s, K, which, "residual")) return rc;
   const size_t kn = (size_t) K * (size_t) s->n, il = K >= 2 ? kn : 0, nrb = (size_t) (s->A.nrowblk > 0 ? s->A.nrowblk : 0);
   const int rc = reserve (s, { { &s->rb.x, &s->rb.x_cap, il }, { &s->rb.partial, &s->rb.partial_cap, 3 * (size_t) K * (nrb + 1) },
                                { &s->rb.stage, &s->rb.stage_cap, 2 * kn } }, "nkp_time_kernel");
   if (rc) return rc;
   if (kn) launch_fill (s->rb.stage, 1.0, (int64_t) (2 * kn), s->stream);
   if (il) launch_fill (s->rb.x, 1.0, (int64_t) il, s->stream);
   return NKP_OK;
}

void residual_time_launch (nkp_solver *s, int K)
{
   const size_t nrb = (size_t) (s->A.nrowblk > 0 ? s->A.nrowblk : 0);
   launch_residual_batch (K, K, s->A, K >= 2 ? s->rb.x : s->t1, s->rb.stage, s->n, nullptr, 0, s->rb.partial, s->rb.partial + 3 * (size_t) K * nrb, s->stream);
}

// which = 12, measurement only: what a caller could do before, column by column -- the two products of backward_error (krylov.hip),
// its berr pass, and the two dots of the norms
void residual_time_composition (nkp_solver *s, int K)
{
   const size_t kn = (size_t) K * (size_t) s->n;
   hipStream_t st = s->stream;
   for (int c = 0; c < K; c++) {
      const double *b = s->rb.stage + (size_t) c * (size_t) s->n, *x = s->rb.stage + kn + (size_t) c * (size_t) s->n;
      spmv_op (s, x, s->r, b, 1);
      spmv_op (s, x, s->t2, b, 2);
      launch_berr (s->r, s->t2, s->n, s->partial, s->misc_dev () + 3, st);
      launch_dot (s->r, s->r, s->n, s->partial, s->misc_dev () + 2, st);
      launch_dot (b, b, s->n, s->partial, s->misc_dev () + 4, st);
   }
}

extern "C" int nkp_residual_batch_device (nkp_solver *s, int nrhs, const void *d_B, int64_t ldb, const void *d_X, int64_t ldx, void *d_R, int64_t ldr, double *rnorm,
                                          double *bnorm, double *berr)
{
   if (!s) return fail (NKP_EINVAL, "nkp_residual_batch_device: NULL solver (argument s)");
   if (!d_B) return fail (NKP_EINVAL, "nkp_residual_batch_device: NULL argument d_B");
   if (!d_X) return fail (NKP_EINVAL, "nkp_residual_batch_device: NULL argument d_X");
   return residual_batch (s, nrhs, nullptr, nullptr, nullptr, (const double *) d_B, (const double *) d_X, (double *) d_R, ldb, ldx, ldr, rnorm, bnorm, berr,
                          "nkp_residual_batch_device");
}

extern "C" int nkp_residual_batch (nkp_solver *s, int nrhs, const double *B, int64_t ldb, const double *X, int64_t ldx, double *R, int64_t ldr, double *rnorm,
                                   double *bnorm, double *berr)
{
   if (!s) return fail (NKP_EINVAL, "nkp_residual_batch: NULL solver (argument s)");
   if (!B) return fail (NKP_EINVAL, "nkp_residual_batch: NULL argument B");
   if (!X) return fail (NKP_EINVAL, "nkp_residual_batch: NULL argument X");
   return residual_batch (s, nrhs, B, X, R, nullptr, nullptr, nullptr, ldb, ldx, ldr, rnorm, bnorm, berr, "nkp_residual_batch");
}
