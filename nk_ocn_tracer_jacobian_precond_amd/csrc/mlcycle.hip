// Multilevel water-column preconditioner: the V(nu, nu) cycle on the hierarchy ml_setup built (multilevel.hip), written once
// for one right-hand side (K = 1) and for K interleaved ones, and the measurement helpers of bench.py and the probes.  The
// skeleton (ml_cycle) knows levels, colours and sweeps; the helpers before it say which kernel serves each operation at which
// width, on the level's vectors of that width (MlLevel::vec).  Launchers only: the kernels are colblock.hip, col_lanes.hip,
// col_packed.hip, col_gs_fused.hip, col_gs_lanes.hip, diagop.hip, spmv.hip, blas1.hip, batch.hip, dense.hip and mltail.hip.
// The owner of the hierarchy may hang a hook behind the half sweeps of level 0 (MlSmoothHook in multilevel.h); without one --
// every single-GPU cycle -- it is one pointer test per half sweep.
#include "nkp_dev.h"
#include "multilevel.h"

// started: what of level l's cycle is already done -- ML_FILLED: x = 0 (with b); ML_SOLVED: the first half sweep too (level 0,
// smoothed, no hook: ml_enter).  K = 1 only: a cycle on K >= 2 always starts fresh
enum { ML_FRESH = 0, ML_FILLED = 1, ML_SOLVED = 2 };

// level l starts its cycle with a fill of x that whoever wrote its b may do in the same pass (tuning step_glue bit 4): every level
// but a dense last one and the head of a single-launch tail
static inline bool ml_level_fills_x (const MlHierarchy &H, int l)
{
   if (l == H.tail_from) return false;
   return !(l == (int) H.lev.size () - 1 && H.coarse_inv);
}

// ================================================================ which kernel serves (operation, level, K)
// Every operation of the cycle once, both widths in its body.  K = 1 picks among the kernel families ml_setup planned for the
// level; K >= 2 has one kernel per operation, which gives every column the bits any of those families gives it alone.

// the level's half sweeps are one launch each at this width, ping-pong between the two x buffers; else residual rows of the
// colour, then its column solves accumulate into x in place
static bool half_sweep_is_one_launch (const MlHierarchy &H, const MlLevel &V, int K) { return K == 1 ? ml_level_fused (H, V) : V.wave_fused != 0; }

// column solves of colour c.  K = 1: levels with few columns run one column per WAVE (colblock_apply_kernel: one round trip for
// the column's right-hand side and factors, the substitution by lane broadcasts) -- with thousands of idle wave slots its
// ~5 us beat the 12-16 us latency floor of the lane-per-column kernels, which only win when the chip is full.  K >= 2: the
// packed lane layout has kernels of its own; every other level takes the wave-per-column kernel (which reads the f64 factors
// and rounds them like the f32 layouts store them: same values).  V.B.kern says which (col_plan.cpp)
static void column_solves (const MlHierarchy &H, MlLevel &V, int K, int c, const double *rhs, double *x, int accumulate, hipStream_t st)
{
   if (K != 1) {
      if (launch_colblock_apply_lanes_batch (K, V.B, V.color_grp[c], V.color_grp[c + 1], rhs, x, accumulate, st) != 0)
         launch_colblock_apply_wave_batch (K, V.B, V.color_blk[c], V.color_blk[c + 1], rhs, x, accumulate, H.f32, st);
   } else if (V.wave_columns) {
      if (H.f32) launch_colblock_apply_range_r32 (V.B, V.color_blk[c], V.color_blk[c + 1], rhs, x, accumulate, st);
      else launch_colblock_apply_range (V.B, V.color_blk[c], V.color_blk[c + 1], rhs, x, accumulate, st);
   } else
      launch_colblock_apply_lanes (V.B, V.color_grp[c], V.color_grp[c + 1], rhs, x, accumulate, st);
}

// r = b - L x on the rows of colour c (K >= 2 reads CSR even where K = 1 reads the per-column diagonals)
static void colour_residual (MlLevel &V, int K, int c, hipStream_t st)
{
   MlVecs &W = V.vec (K);
   if (K != 1) launch_csr_spmv_batch (K, V.L, V.color_rb[c], V.color_rb[c + 1], W.x, W.r, W.b, 1, st);
   else if (V.L.dg_val) launch_diag_residual (V.L, V.color_tile[c], V.color_tile[c + 1], W.x, W.b, W.r, st);
   else launch_csr_residual_range (V.L, V.color_rb[c], V.color_rb[c + 1], W.x, W.b, W.r, st);
}

// the half sweep of colour c in one launch: reads each colour from the buffer that holds it, writes colour c to buffer `out`
// (the launchers cannot refuse: ml_setup clears gs_ok / wave_fused for a level whose storage they do not serve)
static void one_launch_half_sweep (const MlHierarchy &H, MlLevel &V, int K, int c, int out, hipStream_t st)
{
   MlVecs &W = V.vec (K);
   const double *x0 = W.buf (W.cur[0]), *x1 = W.buf (W.cur[1]);
   const int rows0 = (int) V.rows0;
   if (K != 1) launch_gs_wave_batch (K, V.L, V.B, V.color_blk[c], V.color_blk[c + 1], x0, x1, rows0, W.b, W.buf (out), H.f32, st);
   else if (V.wave_diag) launch_gs_wave_diag (V.L, V.B, V.color_tile[c], V.color_tile[c + 1], x0, x1, rows0, W.b, W.buf (out), H.f32, st);
   else if (V.lane_diag) launch_gs_lanes_diag (V.L, V.B, V.color_grp[c], V.color_grp[c + 1], x0, x1, rows0, W.b, W.buf (out), st);
   else if (V.wave_fused) launch_gs_wave (V.L, V.B, V.color_blk[c], V.color_blk[c + 1], x0, x1, rows0, W.b, W.buf (out), H.f32, st);
   else (void) launch_gs_fused (V.L, V.B, V.color_grp[c], V.color_grp[c + 1], x0, x1, rows0, W.b, W.buf (out), st);
}

// r = b - L x on every row, before the restriction
static void full_residual (MlLevel &V, int K, hipStream_t st)
{
   MlVecs &W = V.vec (K);
   if (K != 1) launch_csr_spmv_batch (K, V.L, 0, V.L.nrowblk, W.now (), W.r, W.b, 1, st);
   else if (V.L.dg_val) launch_diag_residual (V.L, V.color_tile[0], V.color_tile[2], W.now (), W.b, W.r, st);
   else launch_csr_spmv (V.L, W.now (), W.r, W.b, 1, st);
}

// the coarse right-hand side from level l's residual; returns what of level l + 1's cycle that has done already.  K = 1, tuning
// step_glue bit 4: the restriction zeroes the coarse x where the coarse cycle would start with that fill
static int restrict_residual (MlHierarchy &H, int l, int K, hipStream_t st)
{
   MlLevel &V = H.lev[l];
   MlVecs &W = V.vec (K), &WC = H.lev[l + 1].vec (K);
   if (K != 1) {
      launch_restrict_sum_batch (K, V.rptr, V.ridx, W.r, WC.b, V.nc, st);
      return ML_FRESH;
   }
   const bool fill = (H.tune->step_glue & 4) && ml_level_fills_x (H, l + 1);
   launch_restrict_sum (V.rptr, V.ridx, W.r, WC.b, V.nc, st, fill ? WC.x : nullptr);
   return fill ? ML_FILLED : ML_FRESH;
}

// x += omega P x_coarse
static void prolong_correction (MlHierarchy &H, int l, int K, hipStream_t st)
{
   MlLevel &V = H.lev[l];
   MlVecs &W = V.vec (K), &WC = H.lev[l + 1].vec (K);
   if (K != 1) launch_prolong_add_batch (K, V.cmap, WC.now (), W.now (), V.n, H.omega, st);
   else launch_prolong_add (V.cmap, WC.now (), W.now (), V.n, H.omega, st);
}

static void fill_x (MlLevel &V, int K, hipStream_t st) { launch_fill (V.vec (K).x, 0.0, V.n * K, st); }

// x = L^-1 b by the dense inverse of the last level
static void dense_last_level (const MlHierarchy &H, MlLevel &V, int K, hipStream_t st)
{
   MlVecs &W = V.vec (K);
   if (K != 1) {
      if (H.coarse_invf) launch_dense_matvec_f32_batch (K, H.coarse_invf, H.coarse_ldf, W.b, W.x, (int) V.n, st);
      else launch_dense_matvec_batch (K, H.coarse_inv, W.b, W.x, (int) V.n, st);
   } else if (H.coarse_invf) launch_dense_matvec_f32 (H.coarse_invf, H.coarse_ldf, W.b, W.x, (int) V.n, st);
   else launch_dense_matvec (H.coarse_inv, W.b, W.x, (int) V.n, st);
}

// ================================================================ the cycle
// The per-level hook behind a half sweep (MlSmoothHook): x holds the new values of colour c.  Level 0 only, and only while the
// running cycle has level-0 half sweeps to come; nothing without a hook (every single-GPU cycle).
static inline void after_half_sweep (MlHierarchy &H, const MlLevel &V, int c, double *x, int K, hipStream_t st)
{
   if (!H.hook || &V != &H.lev[0] || H.hook_left <= 0) return;
   if (--H.hook_left > 0) H.hook->refresh (H.hook->ctx, c, x, K, st);
}

// one Gauss-Seidel half sweep over colour c.  One launch: the new values of colour c go where the other colour's current values
// are if the level is incoherent, else to the other buffer.  Two kernels: in place in x.
static void gs_half (MlHierarchy &H, MlLevel &V, int K, int c, bool fused, hipStream_t st)
{
   MlVecs &W = V.vec (K);
   if (fused) {
      const int out = (W.cur[0] != W.cur[1]) ? W.cur[1 - c] : 1 - W.cur[c];
      one_launch_half_sweep (H, V, K, c, out, st);
      W.cur[c] = out;
      after_half_sweep (H, V, c, W.buf (out), K, st);      // the buffer the next half sweep reads colour c from
      return;
   }
   colour_residual (V, K, c, st);
   column_solves (H, V, K, c, W.r, W.x, 1, st);
   after_half_sweep (H, V, c, W.x, K, st);
}

// colour 0 then 1 before the coarse correction, 1 then 0 (reverse) after it
static void gs_sweep (MlHierarchy &H, MlLevel &V, int K, bool reverse, bool fused, hipStream_t st)
{
   for (int step = 0; step < 2; step++) gs_half (H, V, K, reverse ? 1 - step : step, fused, st);
}

// the first half sweep of a smoothed level from x = 0: the column solves of colour 0 straight from b (r = b there)
static void first_half_sweep (MlHierarchy &H, MlLevel &V, int K, bool fused, hipStream_t st)
{
   MlVecs &W = V.vec (K);
   // one-launch half sweeps: colour 0's first values go to the second buffer -- the level starts incoherent, and the odd number
   // of such half sweeps that follows (colour 1, then nu - 1 full sweeps) ends coherent
   double *x = fused ? W.x2 : W.x;
   // a level with one-launch half sweeps that is not wave_fused (K = 1 only) is a lane-per-column level
   if (fused && !V.wave_fused) launch_colblock_apply_lanes (V.B, V.color_grp[0], V.color_grp[1], W.b, x, 0, st);
   else column_solves (H, V, K, 0, W.b, x, 0, st);
   if (fused) W.cur[0] = 1;
   after_half_sweep (H, V, 0, x, K, st);
}

static void ml_cycle (MlHierarchy &H, int K, int l, hipStream_t st, int started = ML_FRESH)
{
   MlLevel &V = H.lev[l];
   MlVecs &W = V.vec (K);
   if (started != ML_SOLVED) W.cur[0] = W.cur[1] = 0;
   if (l == 0) H.hook_left = 0;
   // levels >= tail_from in one single-workgroup launch: K = 1 only
   if (K == 1 && l == H.tail_from && H.coarse_inv && H.gamma_to <= H.gamma_from && ml_tail_launch (H, l, st) == 0) return;
   const bool last = l == (int) H.lev.size () - 1;
   if (last && H.coarse_inv) {
      dense_last_level (H, V, K, st);
      return;
   }
   // every other level smooths from x = 0: its first half sweep needs no SpMV (r = b on colour 0)
   if (started == ML_FRESH) fill_x (V, K, st);
   if (last) {
      // no dense inverse: many sweeps of the column smoother (what is left here is diagonally dominant)
      const int sweeps = H.tune->ml_coarsest_sweeps > 0 ? H.tune->ml_coarsest_sweeps : 30;
      column_solves (H, V, K, 0, W.b, W.x, 0, st);
      gs_half (H, V, K, 1, false, st);
      for (int s = 1; s < sweeps; s++) gs_sweep (H, V, K, s & 1, false, st);
      return;
   }
   const bool fused = half_sweep_is_one_launch (H, V, K);
   const int nu = (l >= H.coarse_from) ? H.nu_coarse : H.nu;
   if (l == 0 && H.hook) H.hook_left = 4 * nu;      // 2 nu half sweeps before and 2 nu after the coarse correction
   if (started != ML_SOLVED) first_half_sweep (H, V, K, fused, st);
   gs_half (H, V, K, 1, fused, st);
   for (int s = 1; s < nu; s++) gs_sweep (H, V, K, false, fused, st);
   // coarse-grid correction; levels in [gamma_from, gamma_to) repeat it on the updated residual, which by the
   // Galerkin property is the second coarse iteration of a W-cycle (NKP_ML_GAMMA_FROM / NKP_ML_GAMMA_TO, default off)
   const int gamma = (l >= H.gamma_from && l < H.gamma_to) ? 2 : 1;
   for (int g = 0; g < gamma; g++) {
      full_residual (V, K, st);
      const int coarse_started = restrict_residual (H, l, K, st);
      ml_cycle (H, K, l + 1, st, coarse_started);
      prolong_correction (H, l, K, st);
   }
   for (int s = 0; s < nu; s++) gs_sweep (H, V, K, true, fused, st);
}

// ================================================================ entry points: gather, cycle, scatter
void ml_apply (MlHierarchy &H, const double *r, double *z, hipStream_t st, const MlSmoothHook *hook)
{
   MlLevel &V = H.lev[0];
   launch_gather (H.perm0, r, V.one.b, V.n, st);
   H.hook = hook;
   ml_cycle (H, 1, 0, st);
   H.hook = nullptr;
   launch_scatter (H.perm0, V.one.now (), z, V.n, st);
}

// The same cycle entered from the Krylov step (tuning step_glue bit 8): r = w * inv[0] is never stored on its own -- one kernel
// writes it to vnext (original row order) and to level 0's b, and zeroes level 0's x; the first half sweep of level 0 follows
// where the cycle has one of its own (a smoothed level 0).  ml_finish runs the rest of the cycle and scatters z.  Between the
// two calls nothing else may run on this hierarchy's vectors; single-GPU cycles only (no hook).
void ml_enter (MlHierarchy &H, const double *w, const double *inv, double *vnext, hipStream_t st)
{
   MlLevel &V = H.lev[0];
   launch_cycle_entry (H.perm0, w, inv, vnext, V.one.b, V.one.x, V.n, st);
   H.entered = ML_FILLED;
   if (H.lev.size () >= 2 && H.tail_from != 0) {
      V.one.cur[0] = V.one.cur[1] = 0;
      H.hook_left = 0;
      first_half_sweep (H, V, 1, half_sweep_is_one_launch (H, V, 1), st);
      H.entered = ML_SOLVED;
   }
}

void ml_finish (MlHierarchy &H, double *z, hipStream_t st)
{
   MlLevel &V = H.lev[0];
   const int started = H.entered;
   H.entered = ML_FRESH;
   ml_cycle (H, 1, 0, st, started);
   launch_scatter (H.perm0, V.one.now (), z, V.n, st);
}

// the level vectors for K interleaved right-hand sides (MlLevel::wide); K = 2, 4 or 8
int ml_batch_prepare (MlHierarchy &H, int K)
{
   if (K != 2 && K != 4 && K != 8) return -1;
   if (H.batch_K >= K) return 0;
   // all or nothing: the narrower vectors go first, and a failure leaves none behind (batch_K = 0 says so to the retry)
   auto drop = [&H] () {
      for (MlLevel &V : H.lev)
         for (double **p : { &V.wide.x, &V.wide.x2, &V.wide.b, &V.wide.r })
            if (*p) {
               (void) hipFree (*p);
               *p = nullptr;
               H.device_bytes -= (size_t) (V.n ? V.n : 1) * (size_t) H.batch_K * sizeof (double);
            }
      H.batch_K = 0;
   };
   drop ();
   for (MlLevel &V : H.lev) {
      for (double **p : { &V.wide.x, &V.wide.x2, &V.wide.b, &V.wide.r }) {
         const size_t bytes = (size_t) (V.n ? V.n : 1) * (size_t) K * sizeof (double);
         void *q = nullptr;
         if (hipMalloc (&q, bytes) != hipSuccess || hipMemset (q, 0, bytes) != hipSuccess) {
            if (q) (void) hipFree (q);
            // the vectors made so far were sized for K
            H.batch_K = K;
            drop ();
            (void) hipGetLastError ();      // the out-of-memory error is answered here, not by the next call that looks
            return -2;
         }
         *p = (double *) q;
         H.device_bytes += bytes;
      }
   }
   H.batch_K = K;
   return 0;
}

// the cycle on K interleaved right-hand sides from / to per-system vectors: src[k] = residual of system k (NULL: zeros), z = the
// K corrections interleaved, dst[k] (may be NULL) = a plain copy of column k; src_scale (row-weighted iteration): the residuals
// are src[k] times it, row by row.  A Krylov step with chained cycles comes here several times: a cycle starts from its
// right-hand side alone (x is filled, the buffer selectors reset), so nothing of the previous application is read.
void ml_apply_batch_split (MlHierarchy &H, int K, const double *const *src, double *z, double *const *dst, hipStream_t st, const double *src_scale)
{
   MlLevel &V = H.lev[0];
   launch_gather_interleave (K, H.perm0, src, V.wide.b, V.n, st, src_scale);
   ml_cycle (H, K, 0, st);
   launch_scatter_split (K, H.perm0, V.wide.now (), z, dst, V.n, st);
}

// the same on the extended rows of a rank of the row-distributed flavour: level 0 has n_own own rows followed by the overlap
// rows, whose residuals are the K-interleaved halo rows halo[sel[.] * K + k] (sel NULL: halo is the K-interleaved block of the
// overlap rows in their own order); z and dst receive the own rows only
void ml_apply_batch_split_ext (MlHierarchy &H, int K, const double *const *src, const double *halo, const int *sel, int64_t n_own, double *z,
                               double *const *dst, hipStream_t st, const MlSmoothHook *hook)
{
   MlLevel &V = H.lev[0];
   launch_gather_interleave_ext (K, H.perm0, src, halo, sel, n_own, V.wide.b, V.n, st);
   H.hook = hook;
   ml_cycle (H, K, 0, st);
   H.hook = nullptr;
   launch_scatter_split_own (K, H.perm0, V.wide.now (), z, dst, n_own, V.n, st);
}

// ================================================================ measurement helpers (bench.py, probes)
// one half sweep of level 0, colour 0: the residual rows (which = 0) or the column solves (which = 1)
void ml_time_piece (MlHierarchy &H, int which, hipStream_t st)
{
   MlLevel &V = H.lev[0];
   MlVecs &W = V.one;
   if (H.lev.size () < 2) return;
   if (which == 0) {
      if (V.L.dg_val) launch_diag_residual (V.L, V.color_tile[0], V.color_tile[1], W.x, W.b, W.r, st);
      else launch_csr_residual_range (V.L, V.color_rb[0], V.color_rb[1], W.x, W.b, W.r, st);
   }
   else launch_colblock_apply_lanes (V.B, V.color_grp[0], V.color_grp[1], W.r, W.x, 1, st);
}

// compulsory HBM bytes (every array element counted once per kernel that must touch it):
//  which 0: residual rows of level 0, colour 0: its entries (value + column), row pointers, b in, r out, x once; with the
//           per-column diagonals its padded slots (value only), groups of keys and tiles instead of entries and row pointers
//  which 1: column solves of level 0, colour 0: factors, r in, x in and out
//  which 2: one whole V(nu, nu) cycle
int64_t ml_bytes (const MlHierarchy &H, int which)
{
   if (H.lev.size () < 2) return 0;
   auto level_piece = [&] (const MlLevel &V, int colour, int what) -> int64_t {
      const int64_t rows = colour == 0 ? V.rows0 : V.n - V.rows0;
      const int64_t vb = V.L.valf ? 4 : 8, fb = V.B.fac_tf ? 4 : 8;
      if (what == 0 && V.L.dg_val) {
         // the colour's share of the slots, groups and tiles by its share of the rows (as below)
         const double share = V.n ? (double) rows / (double) V.n : 0.0;
         return (int64_t) (share * ((double) V.L.dg_nval * 4.0 + (double) V.L.dg_ntile * (double) sizeof (DgTile) + (double) V.L.dg_ngrp * (double) sizeof (DgGroup))) + rows * (8 + 8) + V.n * 8;
      }
      if (what == 0) {
         // entries of the colour's rows: the colour-major CSR keeps them contiguous; split nnz by rows as an estimate is not
         // needed -- the host knows the exact count only at setup, so use the level's average row length
         const double per_row = V.n ? (double) V.L.nnz / (double) V.n : 0.0;
         return (int64_t) (per_row * (double) rows * (double) (vb + 4)) + rows * (4 + 8 + 8) + V.n * 8;
      }
      return rows * ((2 * V.B.P + 1) * fb + 8 + 8 + 8);
   };
   if (which == 0 || which == 1) return level_piece (H.lev[0], 0, which);
   int64_t total = 0;
   for (size_t l = 0; l + 1 < H.lev.size (); l++) {
      const MlLevel &V = H.lev[l];
      const int nu = ((int) l >= H.coarse_from) ? H.nu_coarse : H.nu;
      for (int c = 0; c < 2; c++) {
         total += (int64_t) (2 * nu) * level_piece (V, c, 1);                       // column solves: nu pre + nu post sweeps
         total += (int64_t) (2 * nu - (c == 0 ? 1 : 0)) * level_piece (V, c, 0);    // residual rows (the first half sweep needs none)
         // one launch per half sweep (gs_lanes_diag_kernel): r is neither written nor read; the tile map of the colour's groups is
         if (V.lane_diag) {
            const int64_t rows = c == 0 ? V.rows0 : V.n - V.rows0, slots = (int64_t) (V.color_grp[c + 1] - V.color_grp[c]) * V.B.gw;
            total -= (int64_t) (2 * nu - (c == 0 ? 1 : 0)) * (rows * (8 + 8) - slots * 4);
         }
      }
      if (V.L.dg_val) total += V.L.dg_nval * 4 + (int64_t) V.L.dg_ntile * (int64_t) sizeof (DgTile) + (int64_t) V.L.dg_ngrp * (int64_t) sizeof (DgGroup) + V.n * (8 + 8 + 8);
      else total += V.L.nnz * ((V.L.valf ? 4 : 8) + 4) + V.n * (4 + 8 + 8 + 8);    // full residual before the restriction
      total += V.n * (8 + 4) + V.nc * (8 + 4);                                      // restriction
      total += V.n * (8 + 8 + 4) + V.nc * 8;                                        // prolongation
   }
   const int64_t ncoarse = H.lev.back ().n;
   total += ncoarse * ncoarse * 8 + 2 * ncoarse * 8;                                // dense coarsest solve
   total += H.lev[0].n * (8 + 8 + 4) * 2;                                           // gather in, scatter out
   return total;
}
