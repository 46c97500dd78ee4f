// The solve of one right-hand side: host-orchestrated, device-resident Krylov drivers.
//
// Replaces the pdgssvx_ABglobal / pdgssvx calls of the reference (src/solve_ABglobal.c:353,395;
// src/solve_ABdist.c:518,571): setup once (nkp_create), then one solve per right-hand side
// with B overwritten by X.  All vectors live in HBM for the whole solve; the host only sees
// one Hessenberg column (<= m+2 doubles) per iteration for the Givens recurrences (krylov_host.cpp).
//
// There is NO CPU fallback in this library: every entry point that computes needs a gfx950
// device and fails with NKP_EDEVICE otherwise.
#include "solver_impl.h"

#include <math.h>

// ---------------------------------------------------------------- the operators of a solve
void apply_precond_once (nkp_solver *s, const double *rin, double *zout)
{
   if (s->opt.precond == NKP_PRECOND_NONE) launch_copy (rin, zout, s->n, s->stream);
   else if (s->opt.precond == NKP_PRECOND_MULTILEVEL && s->dist.ras) {
      // the residual on the overlap rows comes from their owners: alone and straight into place (several rings), or as the SpMV's halo
      RowExchange &X = s->dist.ras_sep ? s->dist.x_ras : s->dist.x_halo;
      if (X.nsend) launch_gather (X.send_idx, rin, X.send, X.nsend, s->stream);
      exchange_rows (s, X, 1, X.send, s->dist.ras_sep ? s->dist.rext + s->n : halo_rows_of (s, 1), s->stream);
      launch_copy (rin, s->dist.rext, s->n, s->stream);
      if (!s->dist.ras_sep && s->dist.n_sel) launch_gather (s->dist.sel_idx, s->dist.xe + s->n, s->dist.rext + s->n, s->dist.n_sel, s->stream);
      ml_apply (s->ml, s->dist.rext, s->dist.zext, s->stream, smooth_hook_of (s));      // (tuning dist_smooth_exchange: + 4 nu - 1 exchanges)
      launch_copy (s->dist.zext, zout, s->n, s->stream);
   } else if (s->opt.precond == NKP_PRECOND_MULTILEVEL) ml_apply (s->ml, rin, zout, s->stream);
   else launch_colblock_apply_lanes (s->B, 0, s->B.ngrp, rin, zout, 0, s->stream);
}

void apply_precond (nkp_solver *s, const double *rin, double *zout)
{
   apply_precond_once (s, rin, zout);
   for (int k = 1; k < s->steps_now && s->p1 && s->p2; k++) {
      spmv_op (s, zout, s->p1, rin, 1);
      apply_precond_once (s, s->p1, s->p2);
      launch_axpby (1.0, s->p2, 1.0, zout, s->n, s->stream);
   }
}

void spmv_op (nkp_solver *s, const double *x, double *y, const double *b, int mode)
{
   const double *xin = x;
   if (s->dist.on) {
      xin = s->dist.xe;
      if (s->dist.overlap) {
         halo_product_overlapped (s, 1, x, [&] (int rb0, int rb1) { launch_csr_spmv_range (s->A, rb0, rb1, xin, y, b, mode, s->stream); });
         return;
      }
      halo_fetch (s, 1, x, nullptr, s->stream);
   }
   if (mode == 2) launch_csr_abs_spmv (s->A, xin, b, y, s->stream);
   else if (s->A.dg_vald) launch_diag_spmv (s->A, xin, y, b, mode, s->stream);      // tuning spmv_diag: same bits, no column indices
   else launch_csr_spmv (s->A, xin, y, b, mode, s->stream);
}

// ---------------------------------------------------------------- device-side building blocks
static int dot_host (nkp_solver *s, const double *x, const double *y, double *out)
{
   launch_dot (x, y, s->n, s->partial, s->misc_dev () + 2, s->stream);
   allreduce_dev (s, s->misc_dev () + 2, 1, 0);
   HIPCHK (hipMemcpyAsync (s->hpin, s->misc_dev () + 2, sizeof (double), hipMemcpyDeviceToHost, s->stream));
   HIPCHK (hipStreamSynchronize (s->stream));
   // a collective that failed on this rank leaves stale halo rows / partial sums behind: no host decision may be taken
   // on them (the ranks' decisions would diverge and their collective sequences with them)
   if (s->comm_failed) return fail (NKP_ECOMM, "nkp_solve: a collective of the distributed solve failed");
   *out = s->hpin[0];
   return NKP_OK;
}

void arnoldi_apply (nkp_solver *s, int j)
{
   const int64_t ld = s->ld;
   double *zj = s->Z + (int64_t) j * ld;
   const double *vj = s->vf32 ? s->vcur : s->V + (int64_t) j * ld;
   if (s->ml.entered) {
      // v_j went into level 0 of the hierarchy with the kernel that stored it (arnoldi_hand_over): the rest of that cycle
      ml_finish (s->ml, zj, s->stream);
      spmv_op (s, zj, s->w, nullptr, 0);
      return;
   }
   if (s->equil) {
      // row-weighted iteration: the basis lives in the scaled space, operator R A M R^-1
      launch_vmul (vj, s->rinv, s->eqtmp, s->n, s->stream);
      apply_precond (s, s->eqtmp, zj);
      spmv_op (s, zj, s->w, nullptr, 0);
      launch_vmul (s->w, s->rscale, s->w, s->n, s->stream);
   } else {
      apply_precond (s, vj, zj);
      spmv_op (s, zj, s->w, nullptr, 0);
   }
}

// orthogonalise w against V[0..j]: the Hessenberg column h[0..j+1] in s->h_dev () is final, 1 / h[j+1] in misc_dev ()[1].
// host_col (tuning step_glue bit 8, never row-distributed): the kernel that completes the column adds up ||w||^2 itself and
// stores the column to that pinned host buffer too
static void arnoldi_column (nkp_solver *s, int j, double *host_col = nullptr)
{
   const int64_t ld = s->ld;
   launch_multi_dot (s->V, s->vf32, ld, j + 1, s->w, s->n, s->partial, s->h_dev (), s->stream);
   allreduce_dev (s, s->h_dev (), j + 2, 0);                 // one allreduce per Gram-Schmidt pass
   launch_update_w (s->V, s->vf32, ld, j + 1, s->h_dev (), s->w, s->n, s->partial, host_col && !s->opt.reorth ? nullptr : s->misc_dev (), s->stream);
   if (s->opt.reorth) {
      launch_multi_dot (s->V, s->vf32, ld, j + 1, s->w, s->n, s->partial, s->h2_dev (), s->stream);
      allreduce_dev (s, s->h2_dev (), j + 2, 0);
      launch_update_w (s->V, s->vf32, ld, j + 1, s->h2_dev (), s->w, s->n, s->partial, host_col ? nullptr : s->misc_dev (), s->stream);
      allreduce_dev (s, s->misc_dev (), 1, 0);
      if (host_col) launch_finish_column_host (s->h_dev (), s->h2_dev (), j + 1, s->partial, s->n, s->misc_dev (), s->misc_dev () + 1, host_col, s->stream);
      else launch_finish_column (s->h_dev (), s->h2_dev (), j + 1, s->misc_dev (), s->misc_dev () + 1, s->stream);
   } else if (s->dist.on && s->tune.dist_one_reduce) {
      // ||w||^2 after the update from the message that is already reduced (w.w rode along with the dots): one allreduce per step
      launch_finish_column_pythagoras (s->h_dev (), j + 1, s->misc_dev () + 1, s->stream);
   } else if (host_col) launch_finish_column_host (s->h_dev (), nullptr, j + 1, s->partial, s->n, s->misc_dev (), s->misc_dev () + 1, host_col, s->stream);
   else {
      allreduce_dev (s, s->misc_dev (), 1, 0);
      launch_finish_column (s->h_dev (), nullptr, j + 1, s->misc_dev (), s->misc_dev () + 1, s->stream);
   }
}

// v_{j+1} = w / ||w||
static void arnoldi_normalise (nkp_solver *s, int j)
{
   const int64_t ld = s->ld;
   if (s->vf32) launch_scale_to (s->w, s->misc_dev () + 1, s->vcur, (float *) s->V + (int64_t) (j + 1) * ld, s->n, s->stream);
   else launch_scale_to (s->w, s->misc_dev () + 1, s->V + (int64_t) (j + 1) * ld, nullptr, s->n, s->stream);
}

void arnoldi_orthogonalise (nkp_solver *s, int j)
{
   arnoldi_column (s, j);
   arnoldi_normalise (s, j);
}

// Tuning step_glue bit 8, second half: the preconditioner of step j + 1 is applied to v_{j+1} itself -- f64 basis, no row weights,
// one plain cycle of this solver's own hierarchy -- so the kernel that stores v_{j+1} can be the one that enters the cycle (ml_enter).
static bool step_enters_cycle (const nkp_solver *s)
{
   return s->opt.precond == NKP_PRECOND_MULTILEVEL && !s->dist.on && !s->vf32 && !s->equil && s->steps_now == 1 &&
          !s->ml.lev.empty () && s->ml.lev[0].n == s->n;
}

// One Arnoldi step of FGMRES and its hand-over: on return column j of the Hessenberg matrix is in s->hpin[0 .. j+1].
// Without step_glue bit 8: the step, the copy, hipStreamSynchronize.  With it (ev; not row-distributed, no row weights, one cycle
// per iteration, and a slot j + 1 in the restart cycle): the kernel that completes the column also stores it to s->hpin, which is
// pinned host memory, and the host waits on the event behind that kernel while the stream goes on with v_{j+1} -- where
// step_enters_cycle, with one kernel that writes it to the basis and into level 0 of the hierarchy, and with the first half sweep
// of the next cycle.  No copy command stands between the column and those launches.  If the host then ends the restart cycle, the launches enqueued ahead have written v_{j+1} and scratch of
// the hierarchy only, and fg_end_cycle follows them in stream order.
int arnoldi_hand_over (nkp_solver *s, int j, hipEvent_t ev)
{
   const bool early = ev && (s->tune.step_glue & 8) && j + 1 < s->m && !s->dist.on && !s->equil && s->steps_now == 1;
   arnoldi_apply (s, j);
   arnoldi_column (s, j, early ? s->hpin : nullptr);
   if (early) HIPCHK (hipEventRecord (ev, s->stream));
   if (early && step_enters_cycle (s)) ml_enter (s->ml, s->w, s->misc_dev () + 1, s->V + (int64_t) (j + 1) * s->ld, s->stream);
   else arnoldi_normalise (s, j);
   if (early) HIPCHK (hipEventSynchronize (ev));
   else {
      HIPCHK (hipMemcpyAsync (s->hpin, s->h_dev (), (size_t) (j + 2) * sizeof (double), hipMemcpyDeviceToHost, s->stream));
      HIPCHK (hipStreamSynchronize (s->stream));
   }
   return NKP_OK;
}

int StepEvent::make (const nkp_solver *s)
{
   if (!ev && (s->tune.step_glue & 8) && !s->dist.on) HIPCHK (hipEventCreateWithFlags (&ev, hipEventDisableTiming | hipEventReleaseToSystem));
   return NKP_OK;
}

StepEvent::~StepEvent ()
{
   if (ev) (void) hipEventDestroy (ev);
}

// ---------------------------------------------------------------- FGMRES as a state machine
// The device work around the host arithmetic of krylov_host.cpp, which takes every decision (FgmresState: krylov_host.h).

// what nkp_last_error says of a right-hand side that was not solved (solver_impl.h)
int rhs_refused (int verdict, const char *what)
{
   if (verdict == RHS_NONFINITE) return fail (NKP_BREAKDOWN, "%s holds a non-finite entry (NaN or Inf): not solved, x is NaN", what);
   return fail (NKP_BREAKDOWN, "%s is outside the range of the solve (||b||^2 finite in f64 and max (rtol ||b||, atol) >= 2^-480 = 3.2e-145): "
                               "not solved, x is NaN; scale the system", what);
}

// The verdict on the right-hand side in s->b (rhs_verdict of krylov_host.cpp; nkp.h at nkp_solve), kept in s->rhs_class for
// the message of the solve.  b = 0 leaves x = 0, a right-hand side that is not solved leaves x = NaN.  Only outside the range
// in which ||b||^2 and the target decide alone are the entries of b counted; row-distributed, ||b||^2 is global, so all ranks
// take that path together and the two counts are added across them.
static int classify_rhs (nkp_solver *s, double bnorm2, double target, int *verdict)
{
   double nonfinite = 0.0, nonzero = 0.0;
   if (rhs_needs_counts (bnorm2, target)) {
      launch_count_entries (s->b, s->n, s->partial, s->misc_dev () + 4, s->stream);
      allreduce_dev (s, s->misc_dev () + 4, 2, 0);
      HIPCHK (hipMemcpyAsync (s->hpin, s->misc_dev () + 4, 2 * sizeof (double), hipMemcpyDeviceToHost, s->stream));
      HIPCHK (hipStreamSynchronize (s->stream));
      if (s->comm_failed) return fail (NKP_ECOMM, "nkp_solve: a collective of the distributed solve failed");
      nonfinite = s->hpin[0];
      nonzero = s->hpin[1];
   }
   s->rhs_class = *verdict = rhs_verdict (bnorm2, target, nonfinite, nonzero);
   if (*verdict == RHS_ZERO) launch_fill (s->x, 0.0, s->n, s->stream);
   else if (*verdict != RHS_ORDINARY) launch_fill (s->x, NAN, s->n, s->stream);
   return NKP_OK;
}

int fg_begin (nkp_solver *s, FgmresState &F)
{
   fg_init (F, s->m);
   double bnorm2 = 0.0;
   int rc = dot_host (s, s->b, s->b, &bnorm2);
   if (rc) return rc;
   F.bnorm = sqrt (bnorm2);
   F.target = fmax (s->opt.rtol * F.bnorm, s->opt.atol);
   s->stagnated = false;
   s->steps_now = s->precond_steps;      // the run-time guard of fg_restart lowers it for this solve only
   int verdict = RHS_ORDINARY;
   if ((rc = classify_rhs (s, bnorm2, F.target, &verdict))) return rc;
   if (verdict != RHS_ORDINARY) {
      F.finished = true;
      F.status = verdict == RHS_ZERO ? NKP_OK : NKP_BREAKDOWN;
      F.relres = verdict == RHS_ZERO ? 0.0 : NAN;
   }
   return NKP_OK;
}

int fg_restart (nkp_solver *s, FgmresState &F)
{
   hipStream_t st = s->stream;
   const int64_t n = s->n;
   int rc;
   s->ml.entered = 0;      // a cycle entered ahead of a step that never came (arnoldi_hand_over) is dropped
   // true residual (unscaled: the stopping test is ||b - A x||_2 <= rtol ||b||_2 whatever norm the iteration minimises)
   spmv_op (s, s->x, s->r, s->b, 1);
   double r2 = 0.0;
   if ((rc = dot_host (s, s->r, s->r, &r2))) return rc;
   const double beta = sqrt (r2);
   const int todo = fg_restart_verdict (F, beta, s->opt.max_iters, s->steps_now);
   msg (s, 2, "fgmres: its = %d, true relres = %.3e\n", F.its, F.relres);
   if (s->comm_failed) return fail (NKP_ECOMM, "nkp_solve: a collective of the distributed solve failed");
   if (todo & FG_LOWER_STEPS) {
      msg (s, 1, "fgmres: no progress over a restart cycle with %d preconditioner cycles per iteration; continuing with one\n", s->steps_now);
      s->steps_now = 1;
   }
   if (todo & FG_STAGNATED) s->stagnated = true;
   if (todo & FG_STOP) return NKP_OK;
   // v0 = r / beta; in the row-weighted iteration v0 = R r / ||R r|| and the inner target is the same relative
   // reduction in that norm (the inner_scale logic of the verdict corrects it from what the next true residual shows)
   if (s->equil) {
      launch_vmul (s->r, s->rscale, s->r, n, st);
      double q2 = 0.0;
      if ((rc = dot_host (s, s->r, s->r, &q2))) return rc;
      F.beta_it = sqrt (q2);
      if (!(F.beta_it > 0.0)) { F.status = NKP_BREAKDOWN; F.finished = true; return NKP_OK; }
      F.target_it = F.target * (F.beta_it / beta);
   }
   s->hpin[0] = 1.0 / F.beta_it;
   HIPCHK (hipMemcpyAsync (s->misc_dev () + 1, s->hpin, sizeof (double), hipMemcpyHostToDevice, st));
   if (s->vf32) launch_scale_to (s->r, s->misc_dev () + 1, s->vcur, (float *) s->V, n, st);
   else launch_scale_to (s->r, s->misc_dev () + 1, s->V, nullptr, n, st);
   HIPCHK (hipStreamSynchronize (st));      // hpin is reused below
   fg_start_cycle (F);
   return NKP_OK;
}

bool fg_post_step (nkp_solver *s, FgmresState &F)
{
   const bool ends = fg_column_step (F, s->hpin, s->opt.max_iters);
   if (!F.breakdown_in_cycle) msg (s, 3, "fgmres: its = %d, est relres = %.3e\n", F.its, F.est / F.bnorm);
   return ends;
}

int fg_end_cycle (nkp_solver *s, FgmresState &F)
{
   const int k = F.j;
   hipStream_t st = s->stream;
   fg_back_substitute (F);
   for (int i = 0; i < k; i++) s->hpin[i] = F.y[i];
   HIPCHK (hipMemcpyAsync (s->y_dev (), s->hpin, (size_t) k * sizeof (double), hipMemcpyHostToDevice, st));
   launch_axpy_multi (s->Z, s->ld, k, s->y_dev (), s->x, s->n, st);
   HIPCHK (hipStreamSynchronize (st));
   if (F.breakdown_in_cycle) {
      // report the true residual of what we have
      int rc;
      double r2 = 0.0;
      spmv_op (s, s->x, s->r, s->b, 1);
      if ((rc = dot_host (s, s->r, s->r, &r2))) return rc;
      F.relres = is_finite (r2) ? sqrt (r2) / F.bnorm : NAN;
      F.status = sqrt (r2) <= F.target ? NKP_OK : NKP_BREAKDOWN;
      F.finished = true;
   }
   return NKP_OK;
}

static int fgmres (nkp_solver *s, int *iters_out, double *relres_out)
{
   FgmresState F;
   StepEvent ev;
   int rc = fg_begin (s, F);
   if (rc) return rc;
   if ((rc = ev.make (s))) return rc;
   while (!F.finished) {
      if ((rc = fg_restart (s, F))) return rc;
      if (F.finished) break;
      for (;;) {
         if ((rc = arnoldi_hand_over (s, F.j, ev.ev))) { s->ml.entered = 0; return rc; }
         if (s->comm_failed) return fail (NKP_ECOMM, "nkp_solve: a collective of the distributed solve failed (Arnoldi step %d)", F.its + 1);
         if (fg_post_step (s, F)) break;
      }
      if ((rc = fg_end_cycle (s, F))) return rc;
   }
   s->ml.entered = 0;
   HIPCHK (hipGetLastError ());
   *iters_out = F.its;
   *relres_out = F.relres;
   return F.status;
}

// right-preconditioned BiCGStab; every inner product is a deterministic two-stage reduction
static int bicgstab (nkp_solver *s, int *iters_out, double *relres_out)
{
   const int64_t n = s->n, ld = s->ld;
   hipStream_t st = s->stream;
   if (s->m < 2) return fail (NKP_EINVAL, "bicgstab needs restart >= 2 (it borrows the Krylov basis storage)");
   double *r = s->r, *r0 = s->V, *p = s->V + ld, *v = s->V + 2 * ld;
   double *ph = s->Z, *sh = s->Z + ld, *t = s->t2, *sv = s->t1;
   int rc;
   double bnorm2, rho = 1.0, alpha = 1.0, omega = 1.0, tmp;
   if ((rc = dot_host (s, s->b, s->b, &bnorm2))) return rc;
   const double bnorm = sqrt (bnorm2);
   const double target = fmax (s->opt.rtol * bnorm, s->opt.atol);
   int verdict = RHS_ORDINARY;
   if ((rc = classify_rhs (s, bnorm2, target, &verdict))) return rc;
   if (verdict != RHS_ORDINARY) {
      *iters_out = 0;
      *relres_out = verdict == RHS_ZERO ? 0.0 : NAN;
      return verdict == RHS_ZERO ? NKP_OK : NKP_BREAKDOWN;
   }
   spmv_op (s, s->x, r, s->b, 1);
   launch_copy (r, r0, n, st);
   launch_fill (p, 0.0, n, st);
   launch_fill (v, 0.0, n, st);
   int its = 0, status = NKP_NOT_CONVERGED;
   double rn2;
   if ((rc = dot_host (s, r, r, &rn2))) return rc;
   double relres = sqrt (rn2) / bnorm;
   while (its < s->opt.max_iters) {
      if (!is_finite (rn2)) { status = NKP_BREAKDOWN; break; }      // a non-finite start vector, an overflow on the way
      if (sqrt (rn2) <= target) { status = NKP_OK; break; }
      double rho_new;
      if ((rc = dot_host (s, r0, r, &rho_new))) return rc;
      if (rho_new == 0.0 || !(rho_new == rho_new)) { status = NKP_BREAKDOWN; break; }
      const double beta = (rho_new / rho) * (alpha / omega);
      // p = r + beta (p - omega v)
      launch_axpby (-omega, v, 1.0, p, n, st);
      launch_axpby (1.0, r, beta, p, n, st);
      apply_precond (s, p, ph);
      spmv_op (s, ph, v, nullptr, 0);
      if ((rc = dot_host (s, r0, v, &tmp))) return rc;
      if (tmp == 0.0 || !(tmp == tmp)) { status = NKP_BREAKDOWN; break; }
      alpha = rho_new / tmp;
      // s = r - alpha v
      launch_copy (r, sv, n, st);
      launch_axpby (-alpha, v, 1.0, sv, n, st);
      apply_precond (s, sv, sh);
      spmv_op (s, sh, t, nullptr, 0);
      double ts, tt;
      if ((rc = dot_host (s, t, sv, &ts))) return rc;
      if ((rc = dot_host (s, t, t, &tt))) return rc;
      if (tt == 0.0 || !(tt == tt)) { status = NKP_BREAKDOWN; break; }
      omega = ts / tt;
      // x += alpha ph + omega sh ; r = s - omega t
      launch_axpby (alpha, ph, 1.0, s->x, n, st);
      launch_axpby (omega, sh, 1.0, s->x, n, st);
      launch_copy (sv, r, n, st);
      launch_axpby (-omega, t, 1.0, r, n, st);
      rho = rho_new;
      its++;
      if ((rc = dot_host (s, r, r, &rn2))) return rc;
      relres = sqrt (rn2) / bnorm;
      msg (s, 3, "bicgstab: its = %d, recurrence relres = %.3e\n", its, relres);
      if (omega == 0.0) { status = NKP_BREAKDOWN; break; }
   }
   // true residual
   spmv_op (s, s->x, r, s->b, 1);
   if ((rc = dot_host (s, r, r, &rn2))) return rc;
   relres = sqrt (rn2) / bnorm;
   if (!is_finite (rn2)) { relres = NAN; status = NKP_BREAKDOWN; }
   else if (sqrt (rn2) <= target * 1.0001) status = NKP_OK;
   else if (status == NKP_OK) status = NKP_NOT_CONVERGED;
   HIPCHK (hipGetLastError ());
   *iters_out = its;
   *relres_out = relres;
   return status;
}

int backward_error (nkp_solver *s, double *berr)
{
   spmv_op (s, s->x, s->r, s->b, 1);
   spmv_op (s, s->x, s->t1, s->b, 2);
   launch_berr (s->r, s->t1, s->n, s->partial, s->misc_dev () + 3, s->stream);
   allreduce_dev (s, s->misc_dev () + 3, 1, 1);
   HIPCHK (hipMemcpyAsync (s->hpin, s->misc_dev () + 3, sizeof (double), hipMemcpyDeviceToHost, s->stream));
   HIPCHK (hipStreamSynchronize (s->stream));
   *berr = s->hpin[0];
   return NKP_OK;
}

static int solve_resident (nkp_solver *s, double *berr, int *iters, double *relres)
{
   if (s->shared->broken) return refactor_broken (s);
   int it = 0;
   double rr = 0.0;
   s->stagnated = false;
   int status = (s->opt.krylov == NKP_KRYLOV_BICGSTAB) ? bicgstab (s, &it, &rr) : fgmres (s, &it, &rr);
   if (status < 0) return status;
   double be = 0.0;
   if (berr || s->stagnated) {
      int rc = backward_error (s, &be);
      if (rc) return rc;
      if (berr) *berr = be;
   }
   // the reference's only accuracy measure is SuperLU's componentwise backward error: a solve that has reached
   // the attainable accuracy with berr at rounding level, or two orders below the requested tolerance (berr bounds
   // the normwise backward error), is as converged as f64 allows, whatever ||r||/||b|| is
   if (s->comm_failed) return fail (NKP_ECOMM, "nkp_solve: a collective of the distributed solve failed");
   if (status == NKP_NOT_CONVERGED && s->stagnated && be <= fmax (NKP_BERR_ROUNDING_LEVEL, 1.0e-2 * s->opt.rtol)) {
      msg (s, 1, "nkp_solve: residual stagnated at %.3e (rtol %.1e) with backward error %.3e: NKP_OK_BERR\n", rr, s->opt.rtol, be);
      status = NKP_OK_BERR;
   }
   if (iters) *iters = it;
   if (relres) *relres = rr;
   msg (s, 1, "nkp_solve: %s after %d iterations, ||b-Ax||/||b|| = %.3e\n", status == NKP_OK ? "converged" : status == NKP_OK_BERR ? "at the attainable accuracy (backward error accepted)" : status == NKP_BREAKDOWN ? "breakdown" : "NOT converged", it, rr);
   if (s->rhs_class == RHS_NONFINITE || s->rhs_class == RHS_OUT_OF_RANGE) rhs_refused (s->rhs_class, "nkp_solve: the right-hand side");
   else if (status == NKP_OK_BERR) fail (status, "nkp_solve: ||b-Ax||/||b|| = %.3e stopped above rtol %.1e at the attainable accuracy after %d iterations; componentwise backward error %.3e", rr, s->opt.rtol, it, be);
   else if (status != NKP_OK) fail (status, "nkp_solve: %s after %d iterations (relres %.3e, rtol %.1e)", status == NKP_BREAKDOWN ? "breakdown" : s->stagnated ? "stagnated at the attainable accuracy, not converged" : "not converged", it, rr, s->opt.rtol);
   return status;
}

extern "C" int nkp_solve_device (nkp_solver *s, const void *d_b, void *d_x, int use_guess, double *berr, int *iters, double *relres)
{
   if (!s || !d_b || !d_x) return fail (NKP_EINVAL, "nkp_solve_device: NULL argument");
   HIPCHK (hipSetDevice (s->device));
   const size_t bytes = (size_t) s->n * sizeof (double);
   if (use_guess) HIPCHK (hipMemcpyAsync (s->x, d_x, bytes, hipMemcpyDeviceToDevice, s->stream));
   else HIPCHK (hipMemsetAsync (s->x, 0, bytes, s->stream));
   HIPCHK (hipMemcpyAsync (s->b, d_b, bytes, hipMemcpyDeviceToDevice, s->stream));
   int status = solve_resident (s, berr, iters, relres);
   if (status < 0) return status;
   HIPCHK (hipMemcpyAsync (d_x, s->x, bytes, hipMemcpyDeviceToDevice, s->stream));
   HIPCHK (hipStreamSynchronize (s->stream));
   return status;
}

extern "C" int nkp_solve (nkp_solver *s, double *b_in_x_out, int nrhs, int64_t ldb, double *berr, int *iters, double *relres)
{
   if (!s || (nrhs > 0 && !b_in_x_out)) return fail (NKP_EINVAL, "nkp_solve: NULL argument");
   if (nrhs < 0 || (nrhs > 0 && ldb < s->n)) return fail (NKP_EINVAL, "nkp_solve: bad nrhs/ldb");
   HIPCHK (hipSetDevice (s->device));
   const size_t bytes = (size_t) s->n * sizeof (double);
   int worst = NKP_OK;
   if (nrhs >= 2 && s->tune.rhs_batch && !batch_unsupported (s)) {
      // several right-hand sides share the sweeps over the matrix and the hierarchy (same bits per column as one at a time)
      double *dB = nullptr;
      const int64_t ldd = s->ld;
      int status = NKP_OK;
      if (hipMalloc ((void **) &dB, (size_t) ldd * (size_t) nrhs * sizeof (double)) != hipSuccess) {
         dB = nullptr;
         (void) hipGetLastError ();
         status = fail (NKP_ENOMEM, "nkp_solve: device memory for %d right-hand sides", nrhs);
      }
      for (int c = 0; c < nrhs && status == NKP_OK; c++)
         if (hipMemcpy (dB + (size_t) c * (size_t) ldd, b_in_x_out + (size_t) c * (size_t) ldb, bytes, hipMemcpyHostToDevice) != hipSuccess) status = fail (NKP_EDEVICE, "nkp_solve: upload of right-hand side %d failed", c);
      // row-distributed: a rank that could not stage its right-hand sides must not leave the others alone in the collectives
      if (s->dist.on) status = dist_agree (s, status, "nkp_solve", "staging the right-hand sides on the device");
      if (status != NKP_OK) { if (dB) (void) hipFree (dB); return status; }
      if (status == NKP_OK) status = nkp_solve_batch_device (s, nrhs, dB, dB, ldd, berr, iters, relres);
      if (status >= 0)
         for (int c = 0; c < nrhs; c++)
            if (hipMemcpy (b_in_x_out + (size_t) c * (size_t) ldb, dB + (size_t) c * (size_t) ldd, bytes, hipMemcpyDeviceToHost) != hipSuccess) status = fail (NKP_EDEVICE, "nkp_solve: download of solution %d failed", c);
      (void) hipFree (dB);
      return status;
   }
   if (nrhs >= 2 && s->tune.rhs_batch) note_fallback (s, "nkp_solve", batch_unsupported (s), nrhs);
   for (int c = 0; c < nrhs; c++) {          // nrhs = 0 is the reference's factor-only call: nothing to do
      double *col = b_in_x_out + (size_t) c * (size_t) ldb;
      HIPCHK (hipMemcpyAsync (s->b, col, bytes, hipMemcpyHostToDevice, s->stream));
      HIPCHK (hipMemsetAsync (s->x, 0, bytes, s->stream));
      int status = solve_resident (s, berr ? berr + c : nullptr, iters ? iters + c : nullptr, relres ? relres + c : nullptr);
      if (status < 0) return status;
      HIPCHK (hipMemcpyAsync (col, s->x, bytes, hipMemcpyDeviceToHost, s->stream));
      HIPCHK (hipStreamSynchronize (s->stream));
      // severity: OK < OK_BERR < NOT_CONVERGED < BREAKDOWN
      if (sev_of (status) > sev_of (worst)) worst = status;
   }
   return worst;
}
