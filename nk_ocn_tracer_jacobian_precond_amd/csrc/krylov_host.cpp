// The host arithmetic of restarted FGMRES (krylov_host.h): pure f64, no device, no solver object.
#include "krylov_host.h"

#include <math.h>

bool rhs_needs_counts (double bnorm2, double target)
{
   return !is_finite (bnorm2) || !(target >= NKP_TARGET_FLOOR);
}

int rhs_verdict (double bnorm2, double target, double n_nonfinite, double n_nonzero)
{
   if (!rhs_needs_counts (bnorm2, target)) return bnorm2 > 0.0 ? RHS_ORDINARY : RHS_ZERO;
   if (!(n_nonfinite == 0.0)) return RHS_NONFINITE;
   return n_nonzero == 0.0 ? RHS_ZERO : RHS_OUT_OF_RANGE;
}

void fg_init (FgmresState &F, int m)
{
   F = FgmresState ();
   F.m = m;
   F.H.assign ((size_t) (m + 1) * m, 0.0);
   F.cs.assign (m, 0.0); F.sn.assign (m, 0.0); F.g.assign (m + 1, 0.0); F.y.assign (m, 0.0);
}

int fg_restart_verdict (FgmresState &F, double beta, int max_iters, int steps_now)
{
   int todo = FG_GO;
   F.beta = beta;
   F.relres = beta / F.bnorm;
   // a residual that is not a number (a non-finite start vector, an overflow on the way) measures nothing: neither does relres
   if (!is_finite (beta)) { F.relres = NAN; F.status = NKP_BREAKDOWN; F.finished = true; return FG_STOP; }
   if (beta <= F.target) { F.status = NKP_OK; F.finished = true; return FG_STOP; }
   if (F.its >= max_iters) { F.status = NKP_NOT_CONVERGED; F.finished = true; return FG_STOP; }
   // a whole restart cycle without progress: the chained cycles are not helping on this right-hand side
   if (steps_now > 1 && F.its > 0 && !(beta < F.beta_prev)) todo |= FG_LOWER_STEPS;
   F.stalled_cycles = (F.cycle_ended_on_estimate && beta > 0.7 * F.beta_prev) ? F.stalled_cycles + 1 : 0;
   if (F.stalled_cycles >= 3) { F.status = NKP_NOT_CONVERGED; F.finished = true; return todo | FG_STOP | FG_STAGNATED; }
   if (F.cycle_ended_on_estimate && F.est_at_exit > 0.0) F.inner_scale = fmax (1e-3, fmin (F.inner_scale, 0.5 * F.est_at_exit / beta));
   F.beta_prev = beta;
   F.cycle_ended_on_estimate = false;
   F.beta_it = beta;
   F.target_it = F.target;
   return todo;
}

void fg_start_cycle (FgmresState &F)
{
   F.g[0] = F.beta_it;
   F.j = 0;
   F.breakdown_in_cycle = false;
}

bool fg_column_step (FgmresState &F, const double *h, int max_iters)
{
   const int m = F.m, j = F.j;
   double *hc = &F.H[(size_t) j * (m + 1)];
   for (int i = 0; i <= j + 1; i++) hc[i] = h[i];
   // a negative sub-diagonal entry is finish_column_pythagoras_kernel's mark: its magnitude is short of digits, the cycle ends here
   const bool weak_norm = hc[j + 1] < 0.0;
   if (weak_norm) hc[j + 1] = -hc[j + 1];
   for (int i = 0; i < j; i++) {
      const double t = F.cs[i] * hc[i] + F.sn[i] * hc[i + 1];
      hc[i + 1] = -F.sn[i] * hc[i] + F.cs[i] * hc[i + 1];
      hc[i] = t;
   }
   const double hjj = hc[j], hj1 = hc[j + 1];
   const double d = hypot (hjj, hj1);
   if (!(d > 0.0) || !(d == d)) { F.status = NKP_BREAKDOWN; F.breakdown_in_cycle = true; return true; }     // column j is unusable: keep k = j
   F.cs[j] = hjj / d;
   F.sn[j] = hj1 / d;
   hc[j] = d;
   hc[j + 1] = 0.0;
   F.g[j + 1] = -F.sn[j] * F.g[j];
   F.g[j] = F.cs[j] * F.g[j];
   F.its++;
   const double est = fabs (F.g[j + 1]);
   F.est = est;
   F.j = j + 1;
   if (est <= F.target_it * F.inner_scale || hj1 == 0.0) {
      F.cycle_ended_on_estimate = true;
      F.est_at_exit = est * (F.beta / F.beta_it);
      return true;
   }
   return weak_norm || F.j >= m || F.its >= max_iters;
}

void fg_back_substitute (FgmresState &F)
{
   const int m = F.m, k = F.j;
   for (int i = k - 1; i >= 0; i--) {
      double t = F.g[i];
      for (int c = i + 1; c < k; c++) t -= F.H[(size_t) c * (m + 1) + i] * F.y[c];
      F.y[i] = t / F.H[(size_t) i * (m + 1) + i];
   }
}
