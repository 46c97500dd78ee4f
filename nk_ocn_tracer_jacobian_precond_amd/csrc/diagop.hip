// Operators as per-column diagonals (CsrDev::dg_*, nkp_dev.h): the residual rows of the Gauss-Seidel half sweeps and the full
// residual before the restriction on the level operators (f32 values), the wave-fused half sweeps of the small levels
// (gs_wave_diag_kernel: residual rows + band solve per wave), and the solver's own products with A (f64 values, tuning
// spmv_diag), without a per-entry column index.  One residual text serves both value types, y = L x and y = b - L x, and x
// from one buffer or from two.
//
// Rows of a water column are contiguous and depth-ordered on every level.  For a row at position kl of its column and an
// entry in column j, key = j - kl is the same for every row of the column that couples to the same neighbour column at the
// same depth offset, so a column needs a short sorted list of keys and one dense diagonal of values per key.  With one lane
// per row the value loads and the x loads of a slot are both contiguous runs.  Ascending keys are ascending columns within
// every row -- the stored order the CSR kernels sum in -- and a padded position adds 0.0f * x = +-0 to a sum that is never
// -0, which leaves it as it is: same bits as csr_spmv_pipe_kernel / csr_spmv_stream_kernel for finite x (a padded zero times
// a non-finite x is NaN, where CSR never touches that x).
#include "nkp_dev.h"
#include "diag_rows.h"
#include "mlsetup.h"

#include <limits.h>

#include <vector>

#define DG_THREADS 256
#define DG_WAVES (DG_THREADS / NKP_WAVE)
#define DG_RPL 4                 // rows per lane of the key kernel: columns of up to 256 rows
#define DG_UNROLL 8              // the zeros behind dg_key

// ---------------------------------------------------------------- setup: the keys of every column
// One wave per column, lane l walks rows l, l + 64, ..: every round takes the smallest key any row still has to offer (rows
// are sorted by column, so by key) and every row that offers it steps on.  Rounds = distinct keys; cnt[c] = their number, or
// cap + 1 when there are more or a row is not strictly ascending.
__global__ __launch_bounds__ (DG_THREADS)
void diag_keys_kernel (int ncol, const int *__restrict__ blk_start, const int *__restrict__ rowptr, const int *__restrict__ colind, int cap,
                       int *__restrict__ tmpkey, int *__restrict__ cnt)
{
   const int c = blockIdx.x * DG_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & (NKP_WAVE - 1);
   if (c >= ncol) return;
   const int r0 = blk_start[c], len = blk_start[c + 1] - r0;
   int p[DG_RPL], e1[DG_RPL], key[DG_RPL];
#pragma unroll
   for (int j = 0; j < DG_RPL; j++) {
      const int kl = lane + j * NKP_WAVE;
      p[j] = e1[j] = 0;
      if (kl < len) { p[j] = rowptr[r0 + kl]; e1[j] = rowptr[r0 + kl + 1]; }
      key[j] = p[j] < e1[j] ? colind[p[j]] - kl : INT_MAX;
   }
   int n = 0;
   bool bad = false;
   for (;;) {
      int m = key[0];
#pragma unroll
      for (int j = 1; j < DG_RPL; j++) m = min (m, key[j]);
#pragma unroll
      for (int off = NKP_WAVE / 2; off > 0; off >>= 1) m = min (m, __shfl_xor (m, off));
      if (m == INT_MAX) break;
      if (n < cap && lane == 0) tmpkey[(size_t) c * cap + n] = m;
      if (++n > cap) break;
#pragma unroll
      for (int j = 0; j < DG_RPL; j++)
         if (key[j] == m) {
            p[j]++;
            key[j] = p[j] < e1[j] ? colind[p[j]] - (lane + j * NKP_WAVE) : INT_MAX;
            if (key[j] <= m) bad = true;
         }
   }
   if (__any (bad)) n = cap + 1;
   if (lane == 0) cnt[c] = n;
}

__global__ __launch_bounds__ (DG_THREADS)
void diag_compact_kernel (int ncol, int cap, const int *__restrict__ tmpkey, const int *__restrict__ dg_ptr, int *__restrict__ dg_key)
{
   const int64_t t = (int64_t) blockIdx.x * DG_THREADS + threadIdx.x;
   const int c = (int) (t / cap), i = (int) (t % cap);
   if (c >= ncol) return;
   const int k0 = dg_ptr[c];
   if (i < dg_ptr[c + 1] - k0) dg_key[k0 + i] = tmpkey[t];
}

// ---------------------------------------------------------------- values (setup and refresh)
// One wave per tile, one lane per row: the row's entries and the column's keys are both ascending, so one walk over the keys
// places every value and writes +0.0 everywhere else -- each position of the value block is written once, by its own row.
template <class VT>
__global__ __launch_bounds__ (DG_THREADS)
void diag_fill_kernel (int ntile, const DgTile *__restrict__ tile, const int *__restrict__ rowptr, const int *__restrict__ colind,
                       const VT *__restrict__ valf, const int *__restrict__ dg_key, VT *__restrict__ dg_val)
{
   const int t = blockIdx.x * DG_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & (NKP_WAVE - 1);
   if (t >= ntile) return;
   const DgTile T = tile[t];
   if (lane >= T.rows) return;
   const int kl = T.kl0 + lane;
   int p = rowptr[T.row0 + lane];
   const int e1 = rowptr[T.row0 + lane + 1];
   VT *dst = dg_val + T.voff + kl;
   for (int s = 0; s < T.nk; s++) {
      VT v = (VT) 0;
      if (p < e1 && colind[p] - kl == dg_key[T.k0 + s]) v = valf[p++];
      dst[(size_t) s * T.len] = v;
   }
}

// ---------------------------------------------------------------- y_rows = b_rows - (L x)_rows (MODE 1), y_rows = (L x)_rows (MODE 0)
// One wave per tile, lane l < rows owns row row0 + l (the lanes behind the tile's end repeat its last row and store nothing,
// so every load stays inside the arrays).  The tile and the groups are wave-uniform: scalar loads.  Per slot one contiguous
// load of the diagonal in its stored type VT (float: the level operators, double: A); f64 product and sum, each rounded, in
// slot order, from acc = +0.0.
//
// Groups: the keys of a neighbour column's rows at depth -1, 0, +1 are consecutive, and for the key behind one a lane would
// load the x its upper neighbour lane loaded for the key before.  So x is loaded once per group of consecutive keys (DgGroup,
// nkp_dev.h), by all 64 lanes with their true lane number: lane i holds x[key0 + kl0 + i], clamped into [0, n) -- out of
// range only where every value that meets it is a padded zero --, and row l takes the x of the group's d-th key from lane
// l + d <= 63 (the groups are cut to fit).  dg_lane_up moves the window one lane down per key: no LDS, no further load.  The
// launch is bound by the vector loads it issues, not by their bytes (a last step filled up with repeated loads cost 9.5 %
// more of them and 5 % of the launch): the 1 degree levels have 14.8 keys in 5.3 groups per column, 29.5 loads per lane
// with one x load per key and 20 with one per group.
//
// dg_step: G groups, their G + (keys of the groups) loads requested before the first is consumed.  Both halves are straight
// lines with wave-uniform exits: the loads (dg_vals) and the sums (dg_sums) of a group of m keys are the first m stages of
// the text for DG_RUN_MAX keys.  The kernel takes a column's groups DG_GROUPS at a time and the rest in one step of exactly
// that length.  The f64 instantiation holds twice the value registers per group (48 VGPRs against 32, both 8 waves per SIMD).
// (dg_lane_up .. dg_row_sum are diag_rows.h: gs_lanes_diag_kernel of col_gs_lanes.hip calls them too.)
template <class VT, int MODE>
__global__ __launch_bounds__ (DG_THREADS)
void diag_residual_kernel (const DgTile *__restrict__ tile, int ntile, const DgGroup *__restrict__ dg_grp, const VT *__restrict__ dg_val,
                           const double *__restrict__ x, const double *__restrict__ b, double *__restrict__ y, int n)
{
   const int t = __builtin_amdgcn_readfirstlane (blockIdx.x * DG_WAVES + (threadIdx.x >> 6));
   if (t >= ntile) return;
   const DgTile T = tile[t];
   const int lane = threadIdx.x & (NKP_WAVE - 1);
   const int lr = min (lane, T.rows - 1);
   double bv = 0.0;
   if constexpr (MODE == 1) bv = b[T.row0 + lr];
   const double acc = dg_row_sum<VT, false> (T, dg_grp, dg_val, lane, lr, x, n);
   if (lane < T.rows) y[T.row0 + lane] = MODE == 1 ? bv - acc : acc;
}

// ---------------------------------------------------------------- one Gauss-Seidel half sweep of a wave-fused level
// gs_wave_kernel (colblock.hip) on the diagonals, for levels whose columns are one tile each (at most 64 rows): one wave per
// column, lane = row.  xout_rows = x_rows + M^-1 (b - L x)_rows with x from two buffers (rows < split from xa, the others from
// xb) like the CSR kernel, whose chain of dependent memory trips -- descriptor, (column, value) stretch into LDS, row pointers,
// LDS reads, gathered x -- becomes two: the tile (scalar), then everything else at once.  The row's b, old x and 2P + 1
// factors (f64 in fac, rounded to f32 on load when R32, as there) depend on the tile alone and are requested in front of the
// first step's value and x loads; the lanes behind the column's end load its last row's and take zeros, which is what
// wave_band_sweeps wants there.  Same products in the same order, a padded position adds +-0: the bits of gs_wave_kernel.
template <int P, bool R32>
__global__ __launch_bounds__ (DG_THREADS)
void gs_wave_diag_kernel (const DgTile *__restrict__ tile, int ntile, const DgGroup *__restrict__ dg_grp, const float *__restrict__ dg_val, int64_t n,
                          const double *__restrict__ fac, const double *__restrict__ xa, const double *__restrict__ xb, int split,
                          const double *__restrict__ b, double *__restrict__ xout)
{
   const int t = __builtin_amdgcn_readfirstlane (blockIdx.x * DG_WAVES + (threadIdx.x >> 6));
   if (t >= ntile) return;
   const DgTile T = tile[t];
   const int lane = threadIdx.x & (NKP_WAVE - 1);
   const bool own = lane < T.rows;
   const int lr = min (lane, T.rows - 1);
   const int64_t r = T.row0 + lr;
   const double bv = b[r];
   const double xold = r < split ? xa[r] : xb[r];
   double f[2 * P + 1];
#pragma unroll
   for (int d = 0; d <= 2 * P; d++) {
      f[d] = fac[(int64_t) d * n + r];
      if (R32) f[d] = (double) (float) f[d];
   }
   const double acc = dg_row_sum<float, true> (T, dg_grp, dg_val, lane, lr, xa, (int) n, xb, split);
   double y[1][1], invd[1], L[1][P], U[1][P];
   y[0][0] = own ? bv - acc : 0.0;
   invd[0] = own ? f[P] : 0.0;
#pragma unroll
   for (int q = 1; q <= P; q++) {
      L[0][q - 1] = own ? f[P - q] : 0.0;      // l(r, r-q)
      U[0][q - 1] = own ? f[P + q] : 0.0;      // u(r, r+q)
   }
   wave_band_sweeps<P, 1, 1> (T.rows, lane, y, invd, L, U);
   if (own) xout[T.row0 + lane] = xold + y[0][0];
}

// ---------------------------------------------------------------- host side
static void diag_drop (CsrDev &L, size_t *device_bytes, size_t held)
{
   for (void **p : { (void **) &L.dg_ptr, (void **) &L.dg_key, (void **) &L.dg_voff, (void **) &L.dg_val, (void **) &L.dg_vald, (void **) &L.dg_tile, (void **) &L.dg_gptr, (void **) &L.dg_grp })
      if (*p) { (void) hipFree (*p); *p = nullptr; }
   L.dg_ntile = L.dg_ncol = L.dg_nkey = L.dg_ngrp = 0;
   L.dg_nval = 0;
   *device_bytes -= held;
   (void) hipGetLastError ();      // an out-of-memory error is answered here: the level stays on CSR
}

// tiles of a column of len rows: ceil (len / 64) of equal heights (the first len % tiles one row taller)
static inline int dg_col_tiles (int len) { return (len + NKP_WAVE - 1) / NKP_WAVE; }

// The groups of a column with the ascending keys key[0 .. nk), whose tallest tile has rows rows: maximal runs of consecutive
// keys, cut to at most DG_RUN_MAX and at most 64 - rows + 1 keys.
static void dg_groups (const int *key, int nk, int rows, std::vector<DgGroup> &out)
{
   const int fit = NKP_WAVE - rows + 1, lim = fit < DG_RUN_MAX ? fit : DG_RUN_MAX;
   for (int s = 0; s < nk;) {
      int m = 1;
      while (s + m < nk && m < lim && key[s + m] == key[s + m - 1] + 1) m++;
      DgGroup R;
      R.key0 = key[s];
      R.slots = s | m << 16;
      out.push_back (R);
      s += m;
   }
}

int diag_build (CsrDev &L, const int *h_blk_start, const int *d_blk_start, int ncol, int ncol0, int max_len, int cap, int color_tile[3],
                size_t *device_bytes, hipStream_t st)
{
   color_tile[0] = color_tile[1] = color_tile[2] = 0;
   const bool f64 = !L.valf;         // no f32 copy: the diagonals hold L.val as it is (the solver's own A)
   if (cap <= 0 || (f64 && !L.val) || ncol <= 0 || L.nnz <= 0 || max_len > DG_RPL * NKP_WAVE) return 0;
   if (cap > 4096) cap = 4096;
   if ((int64_t) ncol * cap > INT_MAX) return 0;
   mls::DBuf<int> tmpkey, dcnt;
   if (tmpkey.alloc ((size_t) ncol * cap) != hipSuccess || dcnt.alloc ((size_t) ncol) != hipSuccess) { (void) hipGetLastError (); return 0; }
   hipLaunchKernelGGL (diag_keys_kernel, dim3 ((ncol + DG_WAVES - 1) / DG_WAVES), dim3 (DG_THREADS), 0, st, ncol, d_blk_start, (const int *) L.rowptr,
                       (const int *) L.colind, cap, tmpkey.p, dcnt.p);
   std::vector<int> cnt ((size_t) ncol);
   if (hipMemcpyAsync (cnt.data (), dcnt.p, (size_t) ncol * sizeof (int), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize (st) != hipSuccess) {
      (void) hipGetLastError ();
      return 0;
   }
   std::vector<int> ptr ((size_t) ncol + 1, 0);
   std::vector<long long> voff ((size_t) ncol);
   long long nval = 0, ntile = 0;
   for (int c = 0; c < ncol; c++) {
      if (cnt[c] > cap) return 0;
      const int len = h_blk_start[c + 1] - h_blk_start[c];
      ptr[c + 1] = ptr[c] + cnt[c];
      voff[c] = nval;
      nval += (long long) cnt[c] * len;
      ntile += dg_col_tiles (len);
   }
   if (2 * nval > 3 * (long long) L.nnz || ntile == 0 || ntile > INT_MAX) return 0;
   size_t held = 0;
   auto put = [&] (void **dst, const void *src, size_t bytes) {
      void *q = nullptr;
      if (hipMalloc (&q, bytes ? bytes : 1) != hipSuccess) return false;
      *dst = q;
      held += bytes ? bytes : 1;
      *device_bytes += bytes ? bytes : 1;
      return !src || !bytes || hipMemcpyAsync (q, src, bytes, hipMemcpyHostToDevice, st) == hipSuccess;
   };
   auto give_up = [&] () {
      (void) hipStreamSynchronize (st);
      diag_drop (L, device_bytes, held);
      color_tile[0] = color_tile[1] = color_tile[2] = 0;
      return 0;
   };
   if (!(put ((void **) &L.dg_ptr, ptr.data (), ptr.size () * sizeof (int)) && put ((void **) &L.dg_key, nullptr, ((size_t) ptr[ncol] + DG_UNROLL) * sizeof (int)) &&
         put ((void **) &L.dg_voff, voff.data (), voff.size () * sizeof (long long)) && (f64 ? put ((void **) &L.dg_vald, nullptr, (size_t) nval * sizeof (double)) : put ((void **) &L.dg_val, nullptr, (size_t) nval * sizeof (float)))))
      return give_up ();
   (void) hipMemsetAsync (L.dg_key + ptr[ncol], 0, DG_UNROLL * sizeof (int), st);
   const int64_t slots = (int64_t) ncol * cap;
   hipLaunchKernelGGL (diag_compact_kernel, dim3 ((unsigned) ((slots + DG_THREADS - 1) / DG_THREADS)), dim3 (DG_THREADS), 0, st, ncol, cap, (const int *) tmpkey.p,
                       (const int *) L.dg_ptr, L.dg_key);
   // the groups and the tiles want the keys on the host
   std::vector<int> key ((size_t) ptr[ncol]);
   if (hipMemcpyAsync (key.data (), L.dg_key, key.size () * sizeof (int), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize (st) != hipSuccess)
      return give_up ();
   std::vector<int> gptr ((size_t) ncol + 1, 0);
   std::vector<DgGroup> grp;
   std::vector<DgTile> tiles;
   grp.reserve (key.size ());
   tiles.reserve ((size_t) ntile);
   for (int c = 0; c < ncol; c++) {
      const int len = h_blk_start[c + 1] - h_blk_start[c], nt = dg_col_tiles (len);
      if (c == ncol0) color_tile[1] = (int) tiles.size ();
      if (nt) dg_groups (key.data () + ptr[c], cnt[c], (len + nt - 1) / nt, grp);
      gptr[c + 1] = (int) grp.size ();
      for (int t = 0, kl0 = 0; t < nt; t++) {
         DgTile T;
         T.rows = len / nt + (t < len % nt ? 1 : 0);
         T.row0 = h_blk_start[c] + kl0;
         T.kl0 = kl0; T.len = len; T.k0 = ptr[c]; T.nk = cnt[c]; T.g0 = gptr[c]; T.ng = gptr[c + 1] - gptr[c]; T.voff = voff[c];
         tiles.push_back (T);
         kl0 += T.rows;
      }
   }
   if (ncol0 >= ncol) color_tile[1] = (int) tiles.size ();
   color_tile[2] = (int) tiles.size ();
   if (!(put ((void **) &L.dg_gptr, gptr.data (), gptr.size () * sizeof (int)) && put ((void **) &L.dg_grp, grp.data (), grp.size () * sizeof (DgGroup)) &&
         put ((void **) &L.dg_tile, tiles.data (), tiles.size () * sizeof (DgTile))))
      return give_up ();
   L.dg_ntile = (int) tiles.size ();
   L.dg_ncol = ncol;
   L.dg_nkey = ptr[ncol];
   L.dg_ngrp = (int) grp.size ();
   L.dg_nval = nval;
   launch_diag_fill (L, st);
   // the host arrays and the scratch buffers go when this returns
   if (hipStreamSynchronize (st) != hipSuccess) return give_up ();
   return 1;
}

void launch_diag_fill (const CsrDev &L, hipStream_t st)
{
   if (!(L.dg_val || L.dg_vald) || L.dg_ntile <= 0) return;
   const dim3 grid ((L.dg_ntile + DG_WAVES - 1) / DG_WAVES);
   if (L.dg_vald)
      hipLaunchKernelGGL (diag_fill_kernel<double>, grid, dim3 (DG_THREADS), 0, st, L.dg_ntile, (const DgTile *) L.dg_tile, (const int *) L.rowptr,
                          (const int *) L.colind, (const double *) L.val, (const int *) L.dg_key, L.dg_vald);
   else
      hipLaunchKernelGGL (diag_fill_kernel<float>, grid, dim3 (DG_THREADS), 0, st, L.dg_ntile, (const DgTile *) L.dg_tile, (const int *) L.rowptr,
                          (const int *) L.colind, (const float *) L.valf, (const int *) L.dg_key, L.dg_val);
}

void launch_diag_residual (const CsrDev &L, int tile0, int tile1, const double *x, const double *b, double *y, hipStream_t st)
{
   const int cnt = tile1 - tile0;
   if (cnt <= 0) return;
   hipLaunchKernelGGL ((diag_residual_kernel<float, 1>), dim3 ((cnt + DG_WAVES - 1) / DG_WAVES), dim3 (DG_THREADS), 0, st, (const DgTile *) L.dg_tile + tile0, cnt,
                       (const DgGroup *) L.dg_grp, (const float *) L.dg_val, x, b, y, (int) L.n);
}

// tiles [tile0, tile1) of one colour of a level whose columns are one tile each (ml_setup sets MlLevel::wave_diag only there)
void launch_gs_wave_diag (const CsrDev &L, const ColBlocksDev &B, int tile0, int tile1, const double *xa, const double *xb, int split, const double *b,
                          double *xout, int r32, hipStream_t st)
{
   const int cnt = tile1 - tile0;
   if (cnt <= 0) return;
   with_band (B.P, [&] (auto p) {
      with_bool (r32, [&] (auto r32_) {
         hipLaunchKernelGGL ((gs_wave_diag_kernel<decltype (p)::value, decltype (r32_)::value>), dim3 ((cnt + DG_WAVES - 1) / DG_WAVES), dim3 (DG_THREADS), 0, st,
                             (const DgTile *) L.dg_tile + tile0, cnt, (const DgGroup *) L.dg_grp, (const float *) L.dg_val, B.n, (const double *) B.fac, xa, xb,
                             split, b, xout);
      });
   });
}

void launch_diag_spmv (const CsrDev &A, const double *x, double *y, const double *b, int mode, hipStream_t st)
{
   if (A.dg_ntile <= 0 || !A.dg_vald) return;
   const dim3 grid ((A.dg_ntile + DG_WAVES - 1) / DG_WAVES);
   with_bool (mode == 1, [&] (auto residual) {
      hipLaunchKernelGGL ((diag_residual_kernel<double, decltype (residual)::value ? 1 : 0>), grid, dim3 (DG_THREADS), 0, st, (const DgTile *) A.dg_tile, A.dg_ntile,
                          (const DgGroup *) A.dg_grp, (const double *) A.dg_vald, x, b, y, (int) A.n);
   });
}
