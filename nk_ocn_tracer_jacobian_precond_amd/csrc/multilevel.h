// Multilevel water-column preconditioner: data structures, setup (multilevel.hip) and cycle (mlcycle.hip).
#pragma once
#include "nkp_dev.h"

#include <vector>

// One set of a level's vectors: the iterate, the right-hand side and the residual, n doubles each (n * K, element (row, k) at
// row * K + k, in the set for K interleaved right-hand sides).  Half sweeps that are one launch ping-pong between x and x2:
// buf (k) is buffer k, cur[c] the buffer that holds the current values of colour c's rows; the level's x is coherent (one
// buffer) whenever cur[0] == cur[1].
struct MlVecs {
   double *x = nullptr, *x2 = nullptr, *b = nullptr, *r = nullptr;
   int cur[2] = { 0, 0 };
   double *buf (int k) { return k ? x2 : x; }
   double *now () { return buf (cur[0]); }        // valid when coherent
};

struct MlLevel {
   int64_t n = 0;
   CsrDev L;                    // level operator, colour-major row order
   ColBlocksDev B;              // factored water-column blocks of L (absent on the coarsest level)
   int color_rb[3] = { 0, 0, 0 };    // SpMV row blocks of colour c: [color_rb[c], color_rb[c+1])
   int color_blk[3] = { 0, 0, 0 };   // column blocks of colour c
   int color_grp[3] = { 0, 0, 0 };   // lane-per-column groups of colour c
   int color_tile[3] = { 0, 0, 0 };  // tiles of colour c in L's per-column diagonals (all 0: the level runs on CSR)
   int64_t rows0 = 0;           // rows of colour 0 (they come first)
   int wave_columns = 0;        // few columns: solve them one per wave (colblock_apply_kernel) instead of one per lane
   int wave_fused = 0;          // ... and run every half sweep as one launch (gs_wave_kernel: residual rows + band solve per wave)
   int wave_diag = 0;           // ... on L's per-column diagonals (gs_wave_diag_kernel: every column one tile, no B.wave_desc)
   int lane_diag = 0;           // a lane-per-column level (packed layout) whose half sweeps are one launch each on L's diagonals (gs_lanes_diag_kernel)
   int64_t nc = 0;              // rows of the next coarser level
   int *cmap = nullptr;         // fine row -> coarse row                 (prolongation)
   int *rptr = nullptr, *ridx = nullptr;   // coarse row -> its fine rows (restriction)
   MlVecs one, wide;            // the level's vectors for one right-hand side, and for K interleaved ones (ml_batch_prepare)
   MlVecs &vec (int K) { return K == 1 ? one : wide; }
   // host: natural row of this level -> its colour-major row (levels >= 1; level 0 has perm0).  nkp_refactor sums the
   // Galerkin products in the natural order of the fine level, the order the setup used.
   std::vector<int> nat_inv;
};

// What the owner of a hierarchy may hang on one application of the cycle: `refresh` runs after every Gauss-Seidel half sweep of
// level 0 except the cycle's last, with the colour just swept and the level-0 vector (K interleaved ones) that holds that colour's
// new values -- the buffer the next half sweep reads the colour from.  A row-distributed solver overwrites the overlap rows of
// that colour with their owners' values there (smooth_exchange.hip); the hierarchy itself knows nothing of ranks or transports.
struct MlSmoothHook {
   void (*refresh) (void *ctx, int colour, double *x, int K, hipStream_t st);
   void *ctx;
};

struct MlHierarchy {
   std::vector<MlLevel> lev;
   const MlSmoothHook *hook = nullptr;   // set by ml_apply / ml_apply_batch_split_ext for the one application they run
   int hook_left = 0;           // level-0 half sweeps of the running cycle still to come
   int entered = 0;             // ml_enter has started a cycle that ml_finish completes: 1 = level 0's b and x are set, 2 = its first half sweep is launched
   int *perm0 = nullptr;        // level-0 row i holds original row perm0[i]
   double *coarse_inv = nullptr;   // dense inverse of the coarsest operator (row-major)
   float *coarse_invf = nullptr;   // f32 storage mode: the copy the cycle multiplies with (rows padded to coarse_ldf)
   int coarse_ldf = 0;
   int nu = 1;                  // Gauss-Seidel sweeps before and after the coarse correction
   int nu_coarse = 1;           // ... on levels >= coarse_from
   int coarse_from = 2;
   int f32 = 1;                 // store level operators / factors in f32 (arithmetic stays f64)
   int fused = 1;               // one launch per Gauss-Seidel half sweep (gs_fused_kernel) where the level allows it
   int tail_from = -1;          // levels >= tail_from run in ONE single-workgroup launch (mltail.hip); -1 = none
   int gamma_from = 0, gamma_to = 0;   // levels [from, to) apply the coarse-grid correction twice (W-cycle there)
   double omega = 1.1;          // weight of the coarse-grid correction
   const nkp_tuning *tune = nullptr;   // the owning solver's knobs (set by ml_setup)
   size_t device_bytes = 0;
   double setup_seconds = 0.0;  // wall time of ml_setup
   int levels_on_device = 0;    // levels whose operator was built by the kernels of mlsetup.hip
   int inverse_pivoted = 0;     // coarse_inv came from the pivoted routine (ml_coarse_inverse returned 1); 0: blocked elimination or the host routine
   int batch_K = 0;             // every level's wide vectors (MlLevel::wide, ml_batch_prepare) hold this many right-hand sides
   int default_build = 0;       // built by the default construction (the one the setup kernels cover): nkp_refactor may keep the cells
};

// the level's half sweeps are one launch each (gs_wave_kernel, gs_lanes_diag_kernel or gs_fused_kernel) instead of residual rows + column solves
inline bool ml_level_fused (const MlHierarchy &H, const MlLevel &V)
{
   // ml_fused_max_cols: the fused half sweep only on levels with at most that many columns (the launch-bound end)
   const int fused_max = H.tune->ml_fused_max_cols;
   return V.wave_fused || V.lane_diag || (H.fused && V.B.gs_ok && (fused_max <= 0 || V.color_grp[2] * V.B.gw <= fused_max));
}

// returns 0, or a negative nkp error code with a message in err
int ml_setup (MlHierarchy &H, int64_t n, const int *rowptr, const int *colind, const double *val,
              const int *blk_start, int64_t nblk, const int *col_i, const int *col_j, const int *col_t /* tracer of every column, or NULL = positional */,
              int tracer_cnt, int max_levels, int nu, int coarsest_rows, int verbose, int rank,
              hipStream_t st, char *err, size_t errlen, const nkp_tuning &tune, const CsrDev *A_dev = nullptr /* device copy of the same matrix, if the caller has one */);
void ml_free (MlHierarchy &H);
// dense inverse of the coarsest operator (colour-major host CSR) exactly as ml_setup computes it (blocked elimination, the
// pivoted routine when a pivot is too small for it); new device buffers, *invf only in f32 storage mode.  0 (blocked), 1 (pivoted
// routine), -2 (no memory), -4 (singular)
int ml_coarse_inverse (const MlHierarchy &H, int n, const int *prow, const int *pcol, const double *pval, double **inv, float **invf,
                       int *ldf, size_t *bytes, hipStream_t st);
// the level-0 sweeps before (and after) the coarse correction, and whether level 0 runs the half sweeps a hook follows (it is
// neither the last level nor part of the single-launch tail)
inline int ml_level0_sweeps (const MlHierarchy &H) { return 0 >= H.coarse_from ? H.nu_coarse : H.nu; }
inline bool ml_level0_hookable (const MlHierarchy &H) { return H.lev.size () >= 2 && H.tail_from != 0 && ml_level0_sweeps (H) > 0; }
// z = V-cycle(r) in the ORIGINAL row order; hook: see MlSmoothHook (NULL = none)
void ml_apply (MlHierarchy &H, const double *r, double *z, hipStream_t st, const MlSmoothHook *hook = nullptr);
// the same cycle for r = w * inv[0] (a device scalar), entered in one kernel that also stores r to vnext, with the first half sweep
// of level 0 behind it (tuning step_glue bit 8).  ml_finish (H, z, st) runs what is left.  No hook: single-GPU cycles.
void ml_enter (MlHierarchy &H, const double *w, const double *inv, double *vnext, hipStream_t st);
void ml_finish (MlHierarchy &H, double *z, hipStream_t st);
// the same cycle on K interleaved right-hand sides (r, z: n * K doubles, element (row, k) at row * K + k; K = 2 or 4); every
// column gets the bits ml_apply gives it alone.  ml_batch_prepare allocates the level vectors (0, or -2 = out of device memory).
int ml_batch_prepare (MlHierarchy &H, int K);
void ml_apply_batch_split (MlHierarchy &H, int K, const double *const *src, double *z, double *const *dst, hipStream_t st, const double *src_scale = nullptr);
void ml_apply_batch_split_ext (MlHierarchy &H, int K, const double *const *src, const double *halo, const int *sel, int64_t n_own, double *z,
                               double *const *dst, hipStream_t st, const MlSmoothHook *hook = nullptr);
// measurement helpers: launch one piece of a level-0 half sweep (0 residual rows, 1 column solves); compulsory HBM bytes of
// that piece or of the whole cycle (2)
void ml_time_piece (MlHierarchy &H, int which, hipStream_t st);
int64_t ml_bytes (const MlHierarchy &H, int which);
// the sub-cycle of the levels >= l0 in one single-workgroup launch (mltail.hip); 0 = launched
int ml_tail_launch (MlHierarchy &H, int l0, hipStream_t st);
