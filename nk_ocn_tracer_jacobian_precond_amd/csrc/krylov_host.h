// The host arithmetic of restarted FGMRES (krylov_host.cpp): plain C++, no HIP, no solver object.  These routines decide
// `iterations`, `status` and, through the coefficients y, the bits of x; krylov.hip wraps them between its device calls (fg_begin,
// fg_restart, fg_post_step, fg_end_cycle) and tests/krylov_host_main.cpp runs them alone.  Private to the library.
#pragma once
#include "tuning.h"

#include <vector>

// One right-hand side's restarted FGMRES, cut at the points where the host looks at device results, so that the same code
// drives one system (fgmres) or K of them in lockstep around batched operator applications (fgmres_batch).
//
// The recurrence's residual estimate assumes an orthonormal basis; with one Gram-Schmidt pass it can run ahead of the true
// residual.  When a cycle stops on the estimate and the true residual disagrees, the next cycle aims lower by the observed
// factor (inner_scale).  Attainable-accuracy guard: three such cycles in a row that gain less than 30 % mean rounding has
// decoupled the two for good, and the iteration is stopped instead of spinning to max_iters.
struct FgmresState {
   std::vector<double> H, cs, sn, g, y;
   int m = 0;                              // restart length: column c of H is H[c * (m + 1) ...]
   double bnorm = 0.0, target = 0.0, relres = 0.0;
   double beta = 0.0, beta_prev = 0.0, est_at_exit = 0.0, inner_scale = 1.0, beta_it = 0.0, target_it = 0.0;
   double est = 0.0;                       // the recurrence's residual estimate after the newest column
   int its = 0, status = NKP_NOT_CONVERGED, stalled_cycles = 0;
   int j = 0;                              // columns of the running restart cycle
   bool cycle_ended_on_estimate = false;
   bool finished = false;                  // the solve is over (status says how)
   bool breakdown_in_cycle = false;
};

// ---- the right-hand side, before anything iterates (nkp.h at nkp_solve: "Vectors the solve refuses")
// Below this target a sum of squares at the target loses digits to underflow: target^2 < 2^-960 is 62 binary orders above the
// smallest normal number, so every term of such a sum keeps all but 2^-62 of itself.  Derived, not measured.
#define NKP_TARGET_FLOOR 0x1p-480
enum { RHS_ORDINARY = 0,       // iterate
       RHS_ZERO = 1,           // b = 0 (or, with atol > 0, every square of b underflowed: ||b|| < atol): x = 0, NKP_OK
       RHS_NONFINITE = 2,      // b holds a NaN or an Inf: not solved
       RHS_OUT_OF_RANGE = 3 }; // b is finite but ||b||^2 overflows or the target is below NKP_TARGET_FLOOR: not solved
inline bool is_finite (double v) { return v - v == 0.0; }
// Whether ||b||^2 and target = max (rtol ||b||, atol) leave the range in which they decide alone: only then are the entries of b
// counted (launch_count_entries and one more allreduce, on this rare path alone; ordinary solves keep their launches).
NKP_PRIVATE bool rhs_needs_counts (double bnorm2, double target);
// The verdict, from ||b||^2, the target and the two counts (non-finite entries, entries != 0; both ignored unless
// rhs_needs_counts).  Every driver takes it from here: fg_begin (so the batched members too) and bicgstab.
NKP_PRIVATE int rhs_verdict (double bnorm2, double target, double n_nonfinite, double n_nonzero);

// a fresh state for restart length m
NKP_PRIVATE void fg_init (FgmresState &F, int m);

// What the caller of fg_restart_verdict must do, as bits: stop (F.finished and F.status are set), lower the cycles per
// preconditioner application to one for the rest of this solve, record that the attainable-accuracy guard stopped the solve.
enum { FG_GO = 0, FG_STOP = 1, FG_LOWER_STEPS = 2, FG_STAGNATED = 4 };
// The verdict on the true residual norm beta at a restart, with steps_now cycles per application in use.  Without FG_STOP the
// next cycle iterates from beta_it = beta towards target_it = target (the row-weighted iteration replaces both).
NKP_PRIVATE int fg_restart_verdict (FgmresState &F, double beta, int max_iters, int steps_now);
// v_0 is in place: the recurrence starts from g[0] = beta_it
NKP_PRIVATE void fg_start_cycle (FgmresState &F);
// Column j = F.j of the Hessenberg matrix is h[0 .. j + 1]: Givens rotations, the residual estimate.  Returns true when this
// system's restart cycle ends here (estimate met, breakdown, column budget).
NKP_PRIVATE bool fg_column_step (FgmresState &F, const double *h, int max_iters);
// y = H^-1 g (upper triangular, size F.j)
NKP_PRIVATE void fg_back_substitute (FgmresState &F);
