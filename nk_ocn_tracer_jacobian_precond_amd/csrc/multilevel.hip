// Multilevel water-column preconditioner (NKP_PRECOND_MULTILEVEL): setup and teardown of the device-resident hierarchy.
//
// The algorithm and the host planner are ml_plan.cpp; the kernels that build the large levels are mlsetup.hip; the cycle is
// mlcycle.hip.  Here: ml_setup decides which levels the kernels build and which the planner builds, and turns either kind
// into an MlLevel -- colour-major operator, row blocks, f32 copy, band factors and lane layouts of the column blocks
// (colblock.hip), transfer maps, the dense inverse of the last level (dense.hip).
#include "nkp_dev.h"
#include "multilevel.h"
#include "mlsetup.h"
#include "ml_plan.h"
#include "../../include/nkp.h"

#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <vector>

using namespace mlp;

namespace {

template <class T>
bool upload (T **dst, const T *src, size_t count, size_t *bytes)
{
   void *q = nullptr;
   const size_t b = (count ? count : 1) * sizeof (T);
   if (hipMalloc (&q, b) != hipSuccess) return false;
   if (count && src && hipMemcpy (q, src, count * sizeof (T), hipMemcpyHostToDevice) != hipSuccess) { (void) hipFree (q); return false; }
   *dst = (T *) q;
   *bytes += b;
   return true;
}

// same with `pad` zeroed extra elements (the SpMV reads matrix entries in aligned pairs)
template <class T>
bool upload_padded (T **dst, const T *src, size_t count, size_t pad, size_t *bytes)
{
   void *q = nullptr;
   const size_t b = (count + pad) * sizeof (T);
   if (hipMalloc (&q, b) != hipSuccess) return false;
   if (hipMemset (q, 0, b) != hipSuccess) { (void) hipFree (q); return false; }
   if (count && hipMemcpy (q, src, count * sizeof (T), hipMemcpyHostToDevice) != hipSuccess) { (void) hipFree (q); return false; }
   *dst = (T *) q;
   *bytes += b;
   return true;
}

// ================================================================ setup
using setup_clk = std::chrono::steady_clock;
inline double secs_since (setup_clk::time_point a) { return std::chrono::duration<double> (setup_clk::now () - a).count (); }

struct DevTimes { double rb = 0.0, up = 0.0, fac = 0.0, lay = 0.0, map = 0.0, perm = 0.0, dev = 0.0, twin = 0.0, agg = 0.0, galerkin = 0.0; };

#define ML_FAIL(code, ...) do { snprintf (err, errlen, __VA_ARGS__); return (code); } while (0)

// Column blocks of a level whose colour-major operator is on the device (V.L with f64 values): half bandwidth, band LU of
// every column, lane layouts; then the f64 values are dropped if the cycle reads the f32 copy.  pblk = row offsets of the
// columns in colour-major order (host).
int finish_level_columns (MlHierarchy &H, MlLevel &V, int l, const std::vector<int> &pblk, int ncol, int ncol0, const int *h_prow, hipStream_t st,
                          char *err, size_t errlen, DevTimes &T)
{
   const int64_t nl = V.n;
   V.B.n = nl;
   V.B.nblk = ncol;
   V.B.tune = H.tune;
   V.B.ml_level = 1;
   if (!upload (&V.B.blk_start, pblk.data (), pblk.size (), &H.device_bytes)) ML_FAIL (-2, "multilevel setup: device allocation failed");
   int *dint = nullptr;
   size_t dummy = 0;
   std::vector<int> zeros (8, 0);
   auto t_fac0 = setup_clk::now ();
   if (!upload (&dint, zeros.data (), 8, &dummy)) ML_FAIL (-2, "multilevel setup: device allocation failed");
   launch_colblock_measure (V.L, V.B, dint, st);
   int meas[3];
   (void) hipMemcpyAsync (meas, dint, sizeof meas, hipMemcpyDeviceToHost, st);
   (void) hipStreamSynchronize (st);
   if (meas[1] > 0) { (void) hipFree (dint); ML_FAIL (-4, "multilevel setup: level %d has %d rows without a diagonal entry", l, meas[1]); }
   V.B.max_len = meas[2];
   V.B.P = meas[0] <= 1 ? 1 : meas[0] <= 2 ? 2 : 4;
   if (!upload (&V.B.fac, (const double *) nullptr, (size_t) (2 * V.B.P + 1) * (size_t) nl, &H.device_bytes)) { (void) hipFree (dint); ML_FAIL (-2, "multilevel setup: device allocation failed"); }
   (void) hipMemsetAsync (dint, 0, 8 * sizeof (int), st);
   launch_colblock_factor (V.L, V.B, dint, st);
   int st2[2];
   (void) hipMemcpyAsync (st2, dint, sizeof st2, hipMemcpyDeviceToHost, st);
   (void) hipStreamSynchronize (st);
   (void) hipFree (dint);
   if (st2[0] != 0) ML_FAIL (-4, "multilevel setup: zero pivot in a column block of level %d (row %d)", l, st2[0] - 1);
   V.B.dropped = st2[1];
   T.fac += secs_since (t_fac0);
   {
      auto t_lay0 = setup_clk::now ();
      const int ranges[3] = { 0, ncol0, ncol };
      const int lrc = colblock_build_lane_layout (V.B, pblk.data (), ranges, 2, V.color_grp, &H.device_bytes, st, H.f32, H.fused ? h_prow : nullptr);
      if (lrc != 0) ML_FAIL (-3, "multilevel setup: lane layout of level %d failed (HIP error %d)", l, lrc);
      // few columns: one per wave, and their half sweeps one launch each (residual of the column's rows + its band solve, gs_wave_kernel)
      V.wave_columns = V.B.kern.wave_columns;
      V.wave_fused = V.B.kern.wave_fused;
      // the block-per-group fused kernel serves matching storage only (f32 operator with f32 factors, or f64 with f64)
      if (V.B.gs_ok && !((V.B.fac_tf && V.L.valf) || (V.B.fac_t && !V.L.valf))) V.B.gs_ok = 0;
      T.lay += secs_since (t_lay0);
   }
   // per-column diagonals (ml_diag = most keys a column may need; 0 = off) for the residual rows of the two-kernel half sweeps,
   // for the wave-fused half sweeps of a level whose columns are one tile each (gs_wave_diag_kernel) and for the full residual
   // of both, and for the one-launch half sweeps of a packed lane-per-column level (gs_lanes_diag_kernel, kern.lane_fused).  A level
   // that does not qualify stays on CSR (and on two kernels); a level that runs gs_fused_kernel is not asked.
   if (H.tune->ml_diag > 0 && V.L.valf && (V.wave_fused ? V.B.max_len <= NKP_WAVE : V.B.kern.lane_fused || !ml_level_fused (H, V))) {
      auto t_dg0 = setup_clk::now ();
      (void) diag_build (V.L, pblk.data (), V.B.blk_start, ncol, ncol0, V.B.max_len, H.tune->ml_diag, V.color_tile, &H.device_bytes, st);
      T.lay += secs_since (t_dg0);
   }
   V.wave_diag = V.wave_fused && V.L.dg_val;
   // the tile map counts one tile per column that has rows, which is what diag_build makes of columns of at most 64 rows
   V.lane_diag = V.B.kern.lane_fused && V.L.dg_val && V.B.grp_tile && V.B.fac_tf && V.B.grp_tile_cnt == V.L.dg_ntile;
   if (V.wave_fused && !V.wave_diag) {
      // the CSR kernel's descriptors
      if (!upload (&V.B.wave_desc, (const int *) nullptr, (size_t) 4 * (size_t) ncol, &H.device_bytes)) ML_FAIL (-2, "multilevel setup: device allocation failed");
      launch_build_wave_desc (V.L, V.B, st);
   }
   // f32 storage mode: the f64 copy of the level operator was only needed to factor the column blocks
   if (V.L.valf && V.L.val) {
      (void) hipStreamSynchronize (st);
      (void) hipFree (V.L.val);
      V.L.val = nullptr;
      H.device_bytes -= ((size_t) V.L.nnz + 2) * sizeof (double);
   }
   return 0;
}

// one level from host arrays (natural order in N, next level in C or NULL): uploads of the planner's colour-major level,
// column blocks, dense inverse of the last level
int finalize_host_level (MlHierarchy &H, int l, int nlev, Nat &N, Nat *Cn, const PlanKnobs &K, int verbose, int rank, hipStream_t st, char *err,
                         size_t errlen, DevTimes &T)
{
   MlLevel &V = H.lev[l];
   const int64_t nl = N.L.n;
   const int ncol = (int) N.blk_start.size () - 1;
   V.n = nl;
   auto t_perm0 = setup_clk::now ();
   ColourMajorLevel P;
   colour_major_operator (N, K.threads, P);
   const std::vector<int> &prow = P.prow, &pblk = N.pblk;
   const RawInts &pcol = P.pcol;
   const RawDoubles &pval = P.pval;
   T.perm += secs_since (t_perm0);
   auto t_dev0 = setup_clk::now ();
   V.color_blk[0] = 0;
   V.color_blk[1] = N.ncol0;
   V.color_blk[2] = ncol;
   const int rows0 = pblk[N.ncol0];
   V.rows0 = rows0;
   // row blocks per colour (must not straddle the colour boundary)
   int *rb0 = nullptr, *rb1 = nullptr, nrb0 = 0, nrb1 = 0;
   auto t_rb0 = setup_clk::now ();
   build_rowblocks_host (rows0, prow.data (), &rb0, &nrb0);
   {
      std::vector<int> shifted (nl - rows0 + 1);
      for (int64_t i = rows0; i <= nl; i++) shifted[i - rows0] = prow[i] - prow[rows0];
      build_rowblocks_host (nl - rows0, shifted.data (), &rb1, &nrb1);
   }
   std::vector<int> rb (nrb0 + nrb1 + 1);
   for (int i = 0; i <= nrb0; i++) rb[i] = rb0[i];
   for (int i = 1; i <= nrb1; i++) rb[nrb0 + i] = rows0 + rb1[i];
   if (nl - rows0 == 0) nrb1 = 0;
   if (rows0 == 0) { nrb0 = 0; }
   free (rb0);
   free (rb1);
   V.color_rb[0] = 0;
   V.color_rb[1] = nrb0;
   V.color_rb[2] = nrb0 + nrb1;
   V.L.n = nl;
   V.L.nnz = prow[nl];
   V.L.nrowblk = nrb0 + nrb1;
   V.L.tune = H.tune;
   T.rb += secs_since (t_rb0);
   auto t_up0 = setup_clk::now ();
   bool ok = upload (&V.L.rowptr, prow.data (), (size_t) nl + 1, &H.device_bytes) &&
             upload_padded (&V.L.colind, pcol.data (), (size_t) prow[nl], 2, &H.device_bytes) &&
             upload_padded (&V.L.val, pval.data (), (size_t) prow[nl], 2, &H.device_bytes) &&
             upload (&V.L.rowblk, rb.data (), rb.size (), &H.device_bytes) &&
             upload (&V.one.x, (const double *) nullptr, (size_t) nl, &H.device_bytes) &&
             upload (&V.one.x2, (const double *) nullptr, (size_t) nl, &H.device_bytes) &&
             upload (&V.one.b, (const double *) nullptr, (size_t) nl, &H.device_bytes) &&
             upload (&V.one.r, (const double *) nullptr, (size_t) nl, &H.device_bytes);
   if (ok) ok = attach_spmv_codes (V.L, prow.data (), pcol.data (), rb.data (), &H.device_bytes) == 0;
   if (ok && H.f32 && l < nlev - 1) {
      std::vector<float, RawAlloc<float>> vf;
      vf.resize ((size_t) prow[nl]);
      for_row_chunks (nl, K.threads, [&] (int, int64_t i0, int64_t i1) {
         for (int64_t e = prow[i0]; e < prow[i1]; e++) vf[(size_t) e] = (float) pval[(size_t) e];
      });
      ok = upload_padded (&V.L.valf, vf.data (), vf.size (), 2, &H.device_bytes);
   }
   T.up += secs_since (t_up0);
   if (!ok) ML_FAIL (-2, "multilevel setup: device allocation failed at level %d", l);
   if (l == 0 && !upload (&H.perm0, N.perm.data (), (size_t) nl, &H.device_bytes)) ML_FAIL (-2, "multilevel setup: device allocation failed");
   if (l > 0) V.nat_inv = N.inv;

   const int dense_max = H.tune->ml_dense_max;
   // the last level is solved with a dense inverse when it is small enough; otherwise (rough bathymetry can leave
   // thousands of pocket stubs that nothing absorbs) it is relaxed like the others, with many sweeps
   const bool dense_last = (l == nlev - 1) && nl <= dense_max;
   if (!dense_last) {
      const int frc = finish_level_columns (H, V, l, pblk, ncol, N.ncol0, prow.data (), st, err, errlen, T);
      if (frc) return frc;
   }
   if (l < nlev - 1) {
      // transfer operators in permuted orders
      auto t_map0 = setup_clk::now ();
      const int64_t nc = Cn->L.n;
      V.nc = nc;
      colour_major_transfers (N, *Cn, P);
      if (!(upload (&V.cmap, P.cmap.data (), (size_t) nl, &H.device_bytes) && upload (&V.rptr, P.rptr.data (), (size_t) nc + 1, &H.device_bytes) &&
            upload (&V.ridx, P.ridx.data (), (size_t) nl, &H.device_bytes)))
         ML_FAIL (-2, "multilevel setup: device allocation failed");
      T.map += secs_since (t_map0);
   }
   if (dense_last) {
      // coarsest level: dense inverse (permuted order)
      std::vector<double> dense;
      auto fill_dense = [&] () {
         dense.assign ((size_t) nl * nl, 0.0);
         for (int64_t i = 0; i < nl; i++)
            for (int e = prow[i]; e < prow[i + 1]; e++) dense[(size_t) i * nl + pcol[e]] = pval[e];
      };
      if (H.tune->ml_host_inverse) {
         fill_dense ();
         if (!dense_inverse ((int) nl, dense)) ML_FAIL (-4, "multilevel setup: coarsest operator is singular");
         if (!upload (&H.coarse_inv, dense.data (), dense.size (), &H.device_bytes)) ML_FAIL (-2, "multilevel setup: device allocation failed");
      } else {
         // blocked elimination on the matrix cores (dense.hip); a pivot it does not trust sends the level to the pivoted routine
         auto t_inv0 = setup_clk::now ();
         const int brc = ml_coarse_inverse (H, (int) nl, prow.data (), pcol.data (), pval.data (), &H.coarse_inv, &H.coarse_invf, &H.coarse_ldf, &H.device_bytes, st);
         if (brc == -2) ML_FAIL (-2, "multilevel setup: device allocation failed (dense inverse of %lld rows)", (long long) nl);
         if (brc == -4) ML_FAIL (-4, "multilevel setup: coarsest operator is singular (or the device is out of memory)");
         H.inverse_pivoted = brc == 1;
         if (verbose) printf ("(%d) multilevel: dense inverse of %lld rows: %s, %.3f s\n", rank, (long long) nl, brc == 0 ? "blocked elimination" : "a pivot too small for it, pivoted routine instead", secs_since (t_inv0));
      }
   }
   if (verbose)
      printf ("(%d) multilevel: level %d: %lld rows, %lld entries, %d columns (%d + %d by colour)%s\n", rank, l, (long long) nl,
              (long long) prow[nl], ncol, N.ncol0, ncol - N.ncol0, l < nlev - 1 ? "" : dense_last ? ", dense solve" : ", relaxed (too large for a dense inverse)");
   T.dev += secs_since (t_dev0);
   return 0;
}

// ---- levels whose operator is built on the device (mlsetup.hip)
struct DevLevel {
   mls::DevCsr L;                                                     // natural order
   int *blk_start = nullptr, *col_of = nullptr, *ktop = nullptr;      // per column / per row / per column
   int *perm = nullptr, *inv = nullptr;                               // colour-major maps
   int *cmap = nullptr;                                               // natural row -> natural row of the next level
   std::vector<int> newstart;                                         // host: colour-major start row of every column
   void free_all ()
   {
      L.free_all ();
      for (int **p : { &blk_start, &col_of, &ktop, &perm, &inv, &cmap })
         if (*p) { (void) hipFree (*p); *p = nullptr; }
   }
};

// column arrays of a level on the device + its colour-major maps; N holds the host column arrays (blk_start, ktop, gi, gj)
int dev_level_columns (DevLevel &D, Nat &N, int64_t n, hipStream_t st)
{
   const int ncol = (int) N.blk_start.size () - 1;
   size_t dummy = 0;
   N.colour.resize (ncol);
   for (int c = 0; c < ncol; c++) N.colour[c] = (N.gi[c] + N.gj[c]) & 1;
   colour_major_columns (N, D.newstart);
   int *d_newstart = nullptr;
   bool ok = upload (&D.blk_start, N.blk_start.data (), (size_t) ncol + 1, &dummy) && upload (&D.ktop, N.ktop.data (), (size_t) ncol, &dummy) &&
             upload (&D.col_of, (const int *) nullptr, (size_t) n, &dummy) && upload (&D.perm, (const int *) nullptr, (size_t) n, &dummy) &&
             upload (&D.inv, (const int *) nullptr, (size_t) n, &dummy) && upload (&d_newstart, D.newstart.data (), (size_t) ncol, &dummy);
   if (!ok) { if (d_newstart) (void) hipFree (d_newstart); return 1; }
   mls::rows_to_cols (D.blk_start, ncol, D.col_of, st);
   mls::colour_major_maps (D.blk_start, D.col_of, d_newstart, n, D.perm, D.inv, st);
   const hipError_t e = hipStreamSynchronize (st);
   (void) hipFree (d_newstart);
   return e == hipSuccess ? 0 : 1;
}

// a level that has a coarser one, from its device-resident natural operator: colour-major operator, row blocks, f32 copy,
// column blocks, transfer maps.  inv_next = colour-major map of the next level (device).
int finalize_device_level (MlHierarchy &H, int l, DevLevel &D, Nat &N, const int *inv_next, int64_t nc, int verbose, int rank, hipStream_t st,
                           char *err, size_t errlen, DevTimes &T)
{
   MlLevel &V = H.lev[l];
   const int64_t nl = D.L.n;
   const int ncol = (int) N.blk_start.size () - 1;
   V.n = nl;
   auto t0 = setup_clk::now ();
   int *prow = nullptr, *pcol = nullptr;
   double *pval = nullptr;
   int rc = mls::permute_operator (D.L, D.perm, D.inv, &prow, &pcol, &pval, 2, st);
   if (rc) ML_FAIL (-2, "multilevel setup: colour-major operator of level %d failed on the device (HIP error %d)", l, rc);
   V.L.n = nl;
   V.L.nnz = D.L.nnz;
   V.L.tune = H.tune;
   V.L.rowptr = prow;
   V.L.colind = pcol;
   V.L.val = pval;
   H.device_bytes += ((size_t) nl + 1) * sizeof (int) + ((size_t) D.L.nnz + 2) * (sizeof (int) + sizeof (double));
   T.perm += secs_since (t0);
   t0 = setup_clk::now ();
   V.color_blk[0] = 0;
   V.color_blk[1] = N.ncol0;
   V.color_blk[2] = ncol;
   const int rows0 = N.pblk[N.ncol0];
   V.rows0 = rows0;
   {
      // row blocks per colour (must not straddle the colour boundary)
      int *rb0 = nullptr, *rb1 = nullptr, nrb0 = 0, nrb1 = 0;
      if ((rc = mls::row_blocks (prow, 0, rows0, &rb0, &nrb0, st)) || (rc = mls::row_blocks (prow, rows0, nl, &rb1, &nrb1, st))) {
         if (rb0) (void) hipFree (rb0);
         ML_FAIL (-2, "multilevel setup: row blocks of level %d failed on the device (HIP error %d)", l, rc);
      }
      int *rb = nullptr;
      bool ok = hipMalloc ((void **) &rb, (size_t) (nrb0 + nrb1 + 1) * sizeof (int)) == hipSuccess;
      if (ok && nrb0) ok = hipMemcpyAsync (rb, rb0, (size_t) nrb0 * sizeof (int), hipMemcpyDeviceToDevice, st) == hipSuccess;
      if (ok && nrb1) ok = hipMemcpyAsync (rb + nrb0, rb1, (size_t) (nrb1 + 1) * sizeof (int), hipMemcpyDeviceToDevice, st) == hipSuccess;
      if (ok && !nrb1) { const int last = (int) nl; ok = hipMemcpyAsync (rb + nrb0, &last, sizeof (int), hipMemcpyHostToDevice, st) == hipSuccess; }
      if (ok) ok = hipStreamSynchronize (st) == hipSuccess;
      if (rb0) (void) hipFree (rb0);
      if (rb1) (void) hipFree (rb1);
      if (!ok) { if (rb) (void) hipFree (rb); ML_FAIL (-2, "multilevel setup: device allocation failed at level %d", l); }
      V.L.rowblk = rb;
      V.L.nrowblk = nrb0 + nrb1;
      V.color_rb[0] = 0;
      V.color_rb[1] = nrb0;
      V.color_rb[2] = nrb0 + nrb1;
      H.device_bytes += (size_t) (nrb0 + nrb1 + 1) * sizeof (int);
   }
   T.rb += secs_since (t0);
   t0 = setup_clk::now ();
   bool ok = upload (&V.one.x, (const double *) nullptr, (size_t) nl, &H.device_bytes) && upload (&V.one.x2, (const double *) nullptr, (size_t) nl, &H.device_bytes) &&
             upload (&V.one.b, (const double *) nullptr, (size_t) nl, &H.device_bytes) && upload (&V.one.r, (const double *) nullptr, (size_t) nl, &H.device_bytes);
   if (ok && H.f32) {
      ok = upload (&V.L.valf, (const float *) nullptr, (size_t) D.L.nnz + 2, &H.device_bytes) &&
           hipMemsetAsync (V.L.valf + D.L.nnz, 0, 2 * sizeof (float), st) == hipSuccess;
      if (ok) mls::to_float (pval, V.L.valf, D.L.nnz, st);
   }
   if (!ok) ML_FAIL (-2, "multilevel setup: device allocation failed at level %d", l);
   if (l == 0) {
      // level-0 row i holds original row perm0[i]
      if (!upload (&H.perm0, (const int *) nullptr, (size_t) nl, &H.device_bytes) ||
          hipMemcpyAsync (H.perm0, D.perm, (size_t) nl * sizeof (int), hipMemcpyDeviceToDevice, st) != hipSuccess)
         ML_FAIL (-2, "multilevel setup: device allocation failed");
   }
   if (l > 0) {
      V.nat_inv.resize ((size_t) nl);
      if (hipMemcpyAsync (V.nat_inv.data (), D.inv, (size_t) nl * sizeof (int), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize (st) != hipSuccess)
         ML_FAIL (-3, "multilevel setup: download of the colour-major order of level %d failed", l);
   }
   T.up += secs_since (t0);
   const int frc = finish_level_columns (H, V, l, N.pblk, ncol, N.ncol0, nullptr, st, err, errlen, T);
   if (frc) return frc;
   {
      // transfer operators in colour-major orders
      t0 = setup_clk::now ();
      V.nc = nc;
      if (!upload (&V.cmap, (const int *) nullptr, (size_t) nl, &H.device_bytes)) ML_FAIL (-2, "multilevel setup: device allocation failed");
      mls::permuted_cmap (D.cmap, D.perm, inv_next, nl, V.cmap, st);
      if ((rc = mls::inverse_map (V.cmap, nl, nc, &V.rptr, &V.ridx, st))) ML_FAIL (-2, "multilevel setup: transfer maps of level %d failed on the device (HIP error %d)", l, rc);
      H.device_bytes += ((size_t) nc + 1 + (size_t) nl) * sizeof (int);
      T.map += secs_since (t0);
   }
   if (verbose)
      printf ("(%d) multilevel: level %d: %lld rows, %lld entries, %d columns (%d + %d by colour), built on the device\n", rank, l, (long long) nl,
              (long long) D.L.nnz, ncol, N.ncol0, ncol - N.ncol0);
   return 0;
}

}  // namespace

int ml_setup (MlHierarchy &H, int64_t n, const int *rowptr, const int *colind, const double *val,
              const int *blk_start_in, int64_t nblk, const int *col_i, const int *col_j, const int *col_t, int tracer_cnt, int max_levels, int nu, int coarsest_rows, int verbose, int rank,
              hipStream_t st, char *err, size_t errlen, const nkp_tuning &tune, const CsrDev *A_dev)
{
   DevTimes T;
   SetupTimes TH;
   H.tune = &tune;                                // the caller's (solver's) copy outlives the hierarchy
   H.nu = nu < 1 ? 1 : nu;
   H.f32 = tune.ml_f32 != 0;                      // level operators and factors stored in f32, arithmetic in f64
   // one launch per half sweep (gs_fused_kernel): bit-identical, but measured slower than the two tuned kernels -- 1 degree
   // cycle 3.62 against 2.65 ms, 3 degree 1.56 against 1.26 ms: a workgroup walks its group's 2-3 row blocks one after the
   // other, each exposing the stream -> gather -> row-sum latency chain that the standalone SpMV hides with one block per
   // workgroup and hundreds of workgroups in flight -- so it stays off (ml_fused = 1 turns it on)
   H.fused = tune.ml_fused != 0;
   H.nu_coarse = tune.ml_smooth_coarse >= 1 ? tune.ml_smooth_coarse : H.nu;
   if (tune.ml_coarse_from >= 1) H.coarse_from = tune.ml_coarse_from;
   // 1.1: the Galerkin operators of piecewise-constant cells are too stiff where lateral mixing matters, so a slightly
   // over-weighted coarse correction helps (1 degree: 0.9 -> 77 iterations, 1.0 -> 69, 1.1 -> 64, 1.2 -> 68, 1.35 -> 95)
   H.omega = tune.ml_omega > 0.0 ? tune.ml_omega : 1.1;
   H.gamma_from = tune.ml_gamma_from;
   H.gamma_to = tune.ml_gamma_to;
   if (max_levels <= 0) max_levels = 12;
   const PlanKnobs K = plan_knobs (tune);
   const auto t_begin = setup_clk::now ();

   // Levels with at least dev_min rows are built by the kernels of mlsetup.hip, the rest by the planner of ml_plan.cpp (a
   // level of a few 10^4 rows costs less on the host than the launches and round trips of the device passes); both build
   // the same hierarchy entry for entry.  The device passes cover the default construction only: geometric groups with
   // connectivity-aware cells, no edge threshold, no 2-byte column codes, no fused half sweeps.
   const int64_t dev_min = tune.ml_device_min;
   const bool device_ok = col_i && col_j && K.split && K.theta == 0.0 && !tune.spmv_compress && !H.fused && dev_min >= 0;

   std::vector<Nat> hnat;              // host-built levels (the first of them may have been handed over by the device path)
   int l0 = 0;                         // index of hnat[0] in the hierarchy
   int ndev_levels = 0;
   if (device_ok && n >= dev_min && !((1 >= max_levels) || (n <= coarsest_rows) || nblk <= 4)) {
      // ---------------- device path
      DevLevel D;
      Nat N;
      init_first_nat (N, n, rowptr, colind, val, blk_start_in, nblk, col_i, col_j, col_t, tracer_cnt, false, K, TH);
      N.L.n = n;
      size_t dummy = 0;
      {
         // the matrix: the caller's device copy when there is one, else a temporary upload
         auto t0 = setup_clk::now ();
         int *a_row = nullptr, *a_col = nullptr;
         double *a_val = nullptr;
         const int nnz = rowptr[n];
         if (!A_dev) {
            if (!(upload (&a_row, rowptr, (size_t) n + 1, &dummy) && upload (&a_col, colind, (size_t) nnz, &dummy) && upload (&a_val, val, (size_t) nnz, &dummy))) {
               for (void *p : { (void *) a_row, (void *) a_col, (void *) a_val }) if (p) (void) hipFree (p);
               ML_FAIL (-2, "multilevel setup: device allocation failed");
            }
         }
         int rc = dev_level_columns (D, N, n, st);
         if (!rc) rc = mls::twin (n, A_dev ? A_dev->rowptr : a_row, A_dev ? A_dev->colind : a_col, A_dev ? A_dev->val : a_val, D.col_of, D.L, st);
         for (void *p : { (void *) a_row, (void *) a_col, (void *) a_val }) if (p) (void) hipFree (p);
         if (rc) { D.free_all (); ML_FAIL (-2, "multilevel setup: low-order twin failed on the device (HIP error %d)", rc); }
         T.twin += secs_since (t0);
      }
      for (int l = 0;; l++) {
         // D / N = level l, resident on the device, with a coarser level to come unless the aggregation stalls
         const int ncol = (int) N.blk_start.size () - 1;
         std::vector<int> cgi, cgj, cgt;
         const int ng = geo_groups (N, group_shift (K, l, (int) nblk, tracer_cnt), N.agg, cgi, cgj, cgt);
         N.nagg = ng;
         auto t0 = setup_clk::now ();
         mls::AggregateIn ain;
         ain.n = D.L.n; ain.ncol = ncol;
         ain.rowptr = D.L.rowptr; ain.colind = D.L.colind; ain.val = D.L.val;
         ain.blk_start = D.blk_start; ain.col_of = D.col_of; ain.ktop = D.ktop;
         ain.h_blk_start = N.blk_start.data (); ain.h_ktop = N.ktop.data (); ain.h_group = N.agg.data (); ain.h_col_t = N.gt.data ();
         ain.pocket = K.pocket; ain.tau = K.tau;
         mls::AggregateOut aout;
         int rc = mls::aggregate (ain, aout, st);
         if (rc) { D.free_all (); ML_FAIL (-2, "multilevel setup: aggregation of level %d failed on the device (HIP error %d)", l, rc); }
         T.agg += secs_since (t0);
         D.cmap = aout.cmap;
         const int64_t ncr = aout.blk_start.back ();
         Nat C;
         DevLevel DC;
         bool stalled = ncr >= D.L.n;                  // no coarsening possible: level l is the last one
         if (!stalled) {
            if (verbose)
               printf ("(%d) multilevel: level %d -> %d: %d columns in %d groups -> %d coarse columns (%d stubs), %d leaf stubs absorbed\n", rank, l, l + 1, ncol, ng,
                       (int) aout.blk_start.size () - 1, aout.stubs, aout.absorbed);
            const int ncc = (int) aout.blk_start.size () - 1;
            C.blk_start.swap (aout.blk_start);
            C.ktop.swap (aout.ktop);
            C.gi.resize (ncc); C.gj.resize (ncc); C.gt.resize (ncc);
            for (int q = 0; q < ncc; q++) { const int g = aout.group[q]; C.gi[q] = cgi[g]; C.gj[q] = cgj[g]; C.gt[q] = cgt[g]; }
            t0 = setup_clk::now ();
            rc = mls::galerkin (D.L, D.cmap, ncr, DC.L, st);
            if (!rc) rc = dev_level_columns (DC, C, ncr, st);
            if (rc) { D.free_all (); DC.free_all (); ML_FAIL (-2, "multilevel setup: Galerkin product of level %d failed on the device (HIP error %d)", l, rc); }
            C.L.n = ncr;
            T.galerkin += secs_since (t0);
         }
         // what becomes of the next level (or of this one, if it is the last): handed to the host routines when it is small
         // or final
         const bool next_last = stalled || (l + 2 >= max_levels) || (ncr <= coarsest_rows) || (int) C.blk_start.size () - 1 <= 4;
         const bool hand_over = stalled || next_last || ncr < dev_min;
         if (!stalled) {
            H.lev.resize ((size_t) l + 1);
            const int frc = finalize_device_level (H, l, D, N, DC.inv, ncr, verbose, rank, st, err, errlen, T);
            if (frc) { D.free_all (); DC.free_all (); return frc; }
            ndev_levels = l + 1;
         }
         if (hand_over) {
            // download the natural operator of the level the host continues from
            DevLevel &S = stalled ? D : DC;
            Nat &M = stalled ? N : C;
            M.L.n = S.L.n;
            M.L.rowptr.resize ((size_t) S.L.n + 1);
            M.L.colind.resize ((size_t) S.L.nnz);
            M.L.val.resize ((size_t) S.L.nnz);
            bool ok = hipMemcpy (M.L.rowptr.data (), S.L.rowptr, ((size_t) S.L.n + 1) * sizeof (int), hipMemcpyDeviceToHost) == hipSuccess;
            if (ok && S.L.nnz) ok = hipMemcpy (M.L.colind.data (), S.L.colind, (size_t) S.L.nnz * sizeof (int), hipMemcpyDeviceToHost) == hipSuccess &&
                                    hipMemcpy (M.L.val.data (), S.L.val, (size_t) S.L.nnz * sizeof (double), hipMemcpyDeviceToHost) == hipSuccess;
            const int ncm = (int) M.blk_start.size () - 1;
            M.col_of.resize ((size_t) S.L.n);
            for (int c = 0; c < ncm; c++)
               for (int r = M.blk_start[c]; r < M.blk_start[c + 1]; r++) M.col_of[r] = c;
            M.colour.clear (); M.agg.clear ();
            l0 = stalled ? l : l + 1;
            hnat.clear ();
            hnat.push_back (std::move (M));
            D.free_all ();
            DC.free_all ();
            if (!ok) ML_FAIL (-3, "multilevel setup: download of level %d failed", l0);
            if (!stalled && !next_last) extend_nat_levels (hnat, l0, (int) nblk, tracer_cnt, max_levels, coarsest_rows, verbose, rank, K, TH);
            else {
               // a final level: only its colour-major order is missing
               std::vector<Nat> one;
               one.push_back (std::move (hnat[0]));
               extend_nat_levels (one, l0, (int) nblk, tracer_cnt, l0 + 1, coarsest_rows, verbose, rank, K, TH);
               hnat.swap (one);
            }
            break;
         }
         D.free_all ();
         D = DC;                    // plain struct of pointers + two vectors
         DC = DevLevel ();
         N = std::move (C);
      }
   } else {
      hnat.resize (1);
      init_first_nat (hnat[0], n, rowptr, colind, val, blk_start_in, nblk, col_i, col_j, col_t, tracer_cnt, true, K, TH);
      extend_nat_levels (hnat, 0, (int) nblk, tracer_cnt, max_levels, coarsest_rows, verbose, rank, K, TH);
   }
   const double t_plan = secs_since (t_begin);

   // ---- host-built levels in colour-major order
   const int nlev = l0 + (int) hnat.size ();
   H.lev.resize (nlev);
   for (int l = l0; l < nlev; l++) {
      const int frc = finalize_host_level (H, l, nlev, hnat[(size_t) (l - l0)], l + 1 < nlev ? &hnat[(size_t) (l - l0 + 1)] : nullptr, K, verbose, rank, st, err, errlen, T);
      if (frc) return frc;
   }
   {
      // the small end of the cycle in one single-workgroup launch: the last levels whose rows add up to <= NKP_ML_TAIL_ROWS
      const int64_t cap = tune.ml_tail_rows;   // 0 = off: measured 1.7-5x SLOWER (1 degree cycle 4.57 against 2.68 ms) -- one workgroup is latency-bound on a single CU
      H.tail_from = -1;
      int64_t rows = 0;
      for (int l = nlev - 1; l >= 0 && nlev - l <= 8; l--) {
         rows += H.lev[l].n;
         if (rows > cap) break;
         if (l < nlev - 1) H.tail_from = l;           // at least two levels, else there is nothing to merge
      }
      if (verbose && H.tail_from >= 0) printf ("(%d) multilevel: levels %d..%d run as one single-workgroup launch\n", rank, H.tail_from, nlev - 1);
   }
   H.setup_seconds = secs_since (t_begin);
   H.levels_on_device = ndev_levels;
   H.default_build = device_ok && !tune.ml_host_inverse;
   if (verbose) {
      printf ("(%d) multilevel setup: %d of %d levels built on the device (%.3f s twin, %.3f s coarse cells, %.3f s Galerkin products); host levels: %.3f s twin, %.3f s "
              "column graphs + coarse cells, %.3f s Galerkin products; colour-major operators %.3f s, row blocks %.3f, uploads + f32 copies %.3f, column factors %.3f, "
              "lane layouts %.3f, transfer maps %.3f; hierarchy construction as a whole %.3f s, everything %.3f s\n",
              rank, ndev_levels, nlev, T.twin, T.agg, T.galerkin, TH.low, TH.graph, TH.galerkin, T.perm, T.rb, T.up, T.fac, T.lay, T.map, t_plan, H.setup_seconds);
      fflush (stdout);
   }
   return 0;
}
#undef ML_FAIL

int ml_coarse_inverse (const MlHierarchy &H, int n, const int *prow, const int *pcol, const double *pval, double **inv, float **invf,
                       int *ldf, size_t *bytes, hipStream_t st)
{
   *inv = nullptr;
   *invf = nullptr;
   // blocked elimination on the matrix cores (dense.hip); a pivot it does not trust sends the level to the pivoted routine
   const int brc = dense_inverse_blocked_device (n, prow, pcol, pval, inv, H.f32 ? invf : nullptr, ldf, bytes, st);
   if (brc < 0) return -2;
   if (brc == 0) return 0;
   std::vector<double> dense ((size_t) n * n, 0.0);
   for (int64_t i = 0; i < n; i++)
      for (int e = prow[i]; e < prow[i + 1]; e++) dense[(size_t) i * n + pcol[e]] = pval[e];
   return dense_inverse_device (n, dense, inv, bytes, st) ? 1 : -4;
}

void ml_free (MlHierarchy &H)
{
   for (MlLevel &V : H.lev) {
      void *ptrs[] = { V.L.rowptr, V.L.colind, V.L.val, V.L.valf, V.B.fac_tf, V.L.rowblk, V.L.codes, V.L.dict, V.L.dict_ptr, V.L.dg_ptr, V.L.dg_key, V.L.dg_voff, V.L.dg_val, V.L.dg_tile, V.L.dg_gptr, V.L.dg_grp, V.B.blk_start, V.B.fac, V.B.grp_b0, V.B.grp_nb, V.B.grp_maxlen, V.B.grp_base, V.B.grp_row0, V.B.col_slot, V.B.fac_t, V.B.gs_rb_ptr, V.B.gs_rb, V.B.wave_desc, V.B.grp_tile, V.cmap, V.rptr, V.ridx, V.one.x, V.one.x2, V.one.b, V.one.r, V.wide.x, V.wide.x2, V.wide.b, V.wide.r };
      for (void *p : ptrs)
         if (p) (void) hipFree (p);
      delete V.B.grp_cols;
   }
   H.lev.clear ();
   if (H.perm0) (void) hipFree (H.perm0);
   if (H.coarse_inv) (void) hipFree (H.coarse_inv);
   if (H.coarse_invf) (void) hipFree (H.coarse_invf);
   H.coarse_invf = nullptr;
   H.perm0 = nullptr;
   H.coarse_inv = nullptr;
}
