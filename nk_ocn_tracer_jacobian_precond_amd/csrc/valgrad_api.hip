// nkp_value_gradient / nkp_value_gradient_device (include/nkp.h): the sensitivity of a solve to the stored matrix values,
// g[e] (+)= alpha * sum_c lambda_c[row of e] * x_c[colind[e]], on single-GPU and row-distributed solvers.  The kernel is
// valgrad.hip; this unit checks the arguments, keeps the work space, fetches the halo rows of x on a row-distributed solver
// and keeps the ranks together.  Only the pattern of the solver's matrix is read.
#include "operand_call.h"

namespace {

// Host flavour: h_* given, d_* NULL; device flavour the other way round.  The entry points have refused NULL arguments on the
// calling rank, before the solver is looked at and before any collective.
int value_gradient (nkp_solver *s, int nrhs, const double *h_lam, const double *h_x, const double *d_lam, const double *d_x, int64_t ld, double alpha,
                    int accumulate, double *h_g, double *d_g, const char *who)
{
   OperandCall c (s, who, nrhs, h_g != nullptr);
   auto &W = s->vg;
   const int64_t n = s->n, nnz = s->A.nnz;
   hipStream_t st = s->stream;

   // ---- (a) this rank's arguments, its work space, the host vectors staged on the device (lambda | x, ld n)
   int rc = refuse_nrhs (who, nrhs, " (more right-hand sides: call again with accumulate = 1)");
   if (!rc) rc = refuse_ld (who, "ld", ld, "n", n);
   if (c.begin (rc)) return c.rc;
   const int K = c.K;
   const size_t il = K >= 2 ? (size_t) n * (size_t) K : 0;      // K = 1 reads the vectors in place
   c.reserve ({ { &W.lam, &W.lam_cap, il }, { &W.x, &W.x_cap, c.dist ? 0 : il },      // row-distributed: x interleaved is dist.bxe
                { &W.stage, &W.stage_cap, c.host ? 2 * (size_t) nrhs * (size_t) n : 0 }, { &W.g, &W.g_cap, c.host ? (size_t) nnz : 0 } }, true);
   const double *L = d_lam, *X = d_x;
   double *G = d_g;
   int64_t ldv = ld;
   if (!c.rc && c.host) {
      L = W.stage;
      X = W.stage + (size_t) nrhs * (size_t) n;
      G = W.g;
      ldv = n;
      hipError_t e = upload_columns (W.stage, h_lam, ld, nrhs, n, st);
      if (e == hipSuccess) e = upload_columns (W.stage + (size_t) nrhs * (size_t) n, h_x, ld, nrhs, n, st);
      if (e == hipSuccess && accumulate && nnz) e = hipMemcpyAsync (W.g, h_g, (size_t) nnz * sizeof (double), hipMemcpyHostToDevice, st);
      c.uploaded (e, "vectors");
   }
   if (c.agree ("arguments and work space")) return c.rc;

   // ---- (b) the halo rows of x, all K vectors in one exchange; then the kernel
   const double *lp[NKP_BATCH_MAX] = {}, *xp[NKP_BATCH_MAX] = {};
   for (int k = 0; k < nrhs; k++) { lp[k] = L + (size_t) k * (size_t) ldv; xp[k] = X + (size_t) k * (size_t) ldv; }
   const double *lam_in = L, *x_in = X;
   if (K >= 2) {
      launch_interleave (K, lp, W.lam, n, st);
      lam_in = W.lam;
   }
   c.rc = fetch_x_operand (s, K, xp, W.x, &x_in, who);
   hipError_t e = hipSuccess;
   if (!c.rc) {
      launch_value_gradient (K, nrhs, s->A, lam_in, x_in, alpha, accumulate, G, st);
      if (c.host && nnz) e = hipMemcpyAsync (h_g, W.g, (size_t) nnz * sizeof (double), hipMemcpyDeviceToHost, st);
   }
   return c.finish (e, "gradient", "exchange and kernel", W.seconds, W.calls);
}

}   // namespace

int fetch_x_operand (nkp_solver *s, int K, const double *const *xp, double *il, const double **x_in, const char *who)
{
   auto &D = s->dist;
   if (!D.on) {
      *x_in = xp[0];
      if (K >= 2) { launch_interleave (K, xp, il, s->n, s->stream); *x_in = il; }
      return NKP_OK;
   }
   // as spmv_op fetches them; a failure is this call's alone (not sticky): the solver's later solves exchange anew
   *x_in = K == 1 ? D.xe : D.bxe;
   if (halo_fetch (s, K, nullptr, xp, s->stream, false)) return fail (NKP_ECOMM, "%s: the exchange of the halo rows of x failed", who);
   return NKP_OK;
}

void valgrad_release (nkp_solver *s)
{
   auto &W = s->vg;
   release_buffers (s, { { &W.lam, &W.lam_cap, 0 }, { &W.x, &W.x_cap, 0 }, { &W.stage, &W.stage_cap, 0 }, { &W.g, &W.g_cap, 0 } });
}

int valgrad_time_prepare (nkp_solver *s, int K, int which)
{
   if (const int rc = time_width_ok (s, K, which, "gradient")) return rc;
   const size_t il = K >= 2 ? (size_t) s->n * (size_t) K : 0;
   if (const int rc = reserve (s, { { &s->vg.lam, &s->vg.lam_cap, il }, { &s->vg.x, &s->vg.x_cap, il }, { &s->vg.g, &s->vg.g_cap, (size_t) s->A.nnz } }, "nkp_time_kernel")) return rc;
   if (il) {
      launch_fill (s->vg.lam, 1.0, (int64_t) il, s->stream);
      launch_fill (s->vg.x, 1.0, (int64_t) il, s->stream);
   }
   return NKP_OK;
}

// K = 1 reads the solver's work vector t1 (filled by nkp_time_kernel) as lambda and as x
void valgrad_time_launch (nkp_solver *s, int K)
{
   launch_value_gradient (K, K, s->A, K >= 2 ? s->vg.lam : s->t1, K >= 2 ? s->vg.x : s->t1, -1.0, 0, s->vg.g, s->stream);
}

extern "C" int nkp_value_gradient_device (nkp_solver *s, int nrhs, const void *d_lambda, const void *d_x, int64_t ld, double alpha, int accumulate, void *d_gval)
{
   if (!s) return fail (NKP_EINVAL, "nkp_value_gradient_device: NULL solver (argument s)");
   if (!d_lambda) return fail (NKP_EINVAL, "nkp_value_gradient_device: NULL argument d_lambda");
   if (!d_x) return fail (NKP_EINVAL, "nkp_value_gradient_device: NULL argument d_x");
   if (!d_gval) return fail (NKP_EINVAL, "nkp_value_gradient_device: NULL argument d_gval");
   return value_gradient (s, nrhs, nullptr, nullptr, (const double *) d_lambda, (const double *) d_x, ld, alpha, accumulate, nullptr, (double *) d_gval, "nkp_value_gradient_device");
}

extern "C" int nkp_value_gradient (nkp_solver *s, int nrhs, const double *lambda, const double *x, int64_t ld, double alpha, int accumulate, double *gval)
{
   if (!s) return fail (NKP_EINVAL, "nkp_value_gradient: NULL solver (argument s)");
   if (!lambda) return fail (NKP_EINVAL, "nkp_value_gradient: NULL argument lambda");
   if (!x) return fail (NKP_EINVAL, "nkp_value_gradient: NULL argument x");
   if (!gval) return fail (NKP_EINVAL, "nkp_value_gradient: NULL argument gval");
   return value_gradient (s, nrhs, lambda, x, nullptr, nullptr, ld, alpha, accumulate, gval, nullptr, "nkp_value_gradient");
}
