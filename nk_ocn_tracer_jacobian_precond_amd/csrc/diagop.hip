// Level operators as per-column diagonals (CsrDev::dg_*, nkp_dev.h): the residual rows of the Gauss-Seidel half sweeps and the
// full residual before the restriction without a per-entry column index.
//
// Rows of a water column are contiguous and depth-ordered on every level.  For a row at position kl of its column and an
// entry in column j, key = j - kl is the same for every row of the column that couples to the same neighbour column at the
// same depth offset, so a column needs a short sorted list of keys and one dense diagonal of values per key.  With one lane
// per row the value loads and the x loads of a slot are both contiguous runs.  Ascending keys are ascending columns within
// every row -- the stored order the CSR kernels sum in -- and a padded position adds 0.0f * x = +-0 to a sum that is never
// -0, which leaves it as it is: same bits as csr_spmv_pipe_kernel / csr_spmv_stream_kernel for finite x.
#include "nkp_dev.h"
#include "mlsetup.h"

#include <limits.h>

#include <vector>

#define DG_THREADS 256
#define DG_WAVES (DG_THREADS / NKP_WAVE)
#define DG_RPL 4                 // rows per lane of the key kernel: columns of up to 256 rows
#define DG_UNROLL 8              // slots whose loads are in flight together (and the zeros behind dg_key)

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
// places every value and writes 0.0f everywhere else -- each position of the value block is written once, by its own row.
__global__ __launch_bounds__ (DG_THREADS)
void diag_fill_kernel (int ntile, const DgTile *__restrict__ tile, const int *__restrict__ rowptr, const int *__restrict__ colind,
                       const float *__restrict__ valf, const int *__restrict__ dg_key, float *__restrict__ dg_val)
{
   const int t = blockIdx.x * DG_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & (NKP_WAVE - 1);
   if (t >= ntile) return;
   const DgTile T = tile[t];
   if (lane >= T.rows) return;
   const int kl = T.kl0 + lane;
   int p = rowptr[T.row0 + lane];
   const int e1 = rowptr[T.row0 + lane + 1];
   float *dst = dg_val + T.voff + kl;
   for (int s = 0; s < T.nk; s++) {
      float v = 0.0f;
      if (p < e1 && colind[p] - kl == dg_key[T.k0 + s]) v = valf[p++];
      dst[(size_t) s * T.len] = v;
   }
}

// ---------------------------------------------------------------- y_rows = b_rows - (L x)_rows
// One wave per tile, lane l < rows owns row row0 + l (the lanes behind the tile's end repeat its last row and store nothing,
// so every load stays inside the arrays).  The tile and the keys are wave-uniform: scalar loads.  Per slot one contiguous
// f32 load of the diagonal and one contiguous load of x at key + kl, clamped into [0, n) -- out of range only where the
// value is a padded zero.  f64 product and sum, each rounded, in slot order.
//
// dg_slots: M slots from slot s on, all 2 M loads requested before the first is consumed.  The kernel takes a column's nk
// slots DG_UNROLL at a time and the nk % DG_UNROLL behind them in one step of exactly that length: the launch is bound by
// the vector loads it issues, not by their bytes, and a last step filled up to DG_UNROLL with repeated loads cost 9.5 % more
// of them on the 1 degree levels (keys per column 13 .. 17, mean 14.8: two steps, 16 slots).
template <int M>
__device__ __forceinline__ void dg_slots (const int *__restrict__ key, const float *__restrict__ val, const double *__restrict__ x, int s, int len, int kl,
                                          int n, double &acc)
{
   float v[M];
   double xv[M];
#pragma unroll
   for (int u = 0; u < M; u++) {
      const int j = min (max (key[s + u] + kl, 0), n - 1);
      v[u] = (val + (size_t) (s + u) * len)[kl];
      xv[u] = x[j];
   }
#pragma unroll
   for (int u = 0; u < M; u++) acc += (double) v[u] * xv[u];
}

__global__ __launch_bounds__ (DG_THREADS)
void diag_residual_kernel (const DgTile *__restrict__ tile, int ntile, const int *__restrict__ dg_key, const float *__restrict__ dg_val,
                           const double *__restrict__ x, const double *__restrict__ b, double *__restrict__ y, int n)
{
   const int t = __builtin_amdgcn_readfirstlane (blockIdx.x * DG_WAVES + (threadIdx.x >> 6));
   if (t >= ntile) return;
   const DgTile T = tile[t];
   const int lane = threadIdx.x & (NKP_WAVE - 1);
   const int lr = min (lane, T.rows - 1);
   const int kl = T.kl0 + lr;
   const double bv = b[T.row0 + lr];
   const int *__restrict__ key = dg_key + T.k0;
   const float *__restrict__ val = dg_val + T.voff;
   double acc = 0.0;
   int s = 0;
   for (; s + DG_UNROLL <= T.nk; s += DG_UNROLL) dg_slots<DG_UNROLL> (key, val, x, s, T.len, kl, n, acc);
   static_assert (DG_UNROLL == 8, "one case per length of the last step");
   switch (T.nk - s) {
      case 1: dg_slots<1> (key, val, x, s, T.len, kl, n, acc); break;
      case 2: dg_slots<2> (key, val, x, s, T.len, kl, n, acc); break;
      case 3: dg_slots<3> (key, val, x, s, T.len, kl, n, acc); break;
      case 4: dg_slots<4> (key, val, x, s, T.len, kl, n, acc); break;
      case 5: dg_slots<5> (key, val, x, s, T.len, kl, n, acc); break;
      case 6: dg_slots<6> (key, val, x, s, T.len, kl, n, acc); break;
      case 7: dg_slots<7> (key, val, x, s, T.len, kl, n, acc); break;
      default: break;
   }
   if (lane < T.rows) y[T.row0 + lane] = bv - acc;
}

// ---------------------------------------------------------------- host side
static void diag_drop (CsrDev &L, size_t *device_bytes, size_t held)
{
   for (void **p : { (void **) &L.dg_ptr, (void **) &L.dg_key, (void **) &L.dg_voff, (void **) &L.dg_val, (void **) &L.dg_tile })
      if (*p) { (void) hipFree (*p); *p = nullptr; }
   L.dg_ntile = L.dg_ncol = L.dg_nkey = 0;
   L.dg_nval = 0;
   *device_bytes -= held;
   (void) hipGetLastError ();      // an out-of-memory error is answered here: the level stays on CSR
}

int diag_build (CsrDev &L, const int *h_blk_start, const int *d_blk_start, int ncol, int ncol0, int max_len, int cap, int color_tile[3],
                size_t *device_bytes, hipStream_t st)
{
   color_tile[0] = color_tile[1] = color_tile[2] = 0;
   if (cap <= 0 || !L.valf || ncol <= 0 || L.nnz <= 0 || max_len > DG_RPL * NKP_WAVE) return 0;
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
   std::vector<DgTile> tiles;
   tiles.reserve ((size_t) ncol);
   long long nval = 0;
   for (int c = 0; c < ncol; c++) {
      if (cnt[c] > cap) { color_tile[1] = 0; return 0; }
      const int len = h_blk_start[c + 1] - h_blk_start[c];
      if (c == ncol0) color_tile[1] = (int) tiles.size ();
      ptr[c + 1] = ptr[c] + cnt[c];
      voff[c] = nval;
      nval += (long long) cnt[c] * len;
      for (int kl0 = 0; kl0 < len; kl0 += NKP_WAVE) {
         DgTile T;
         T.row0 = h_blk_start[c] + kl0;
         T.rows = len - kl0 < NKP_WAVE ? len - kl0 : NKP_WAVE;
         T.kl0 = kl0; T.len = len; T.k0 = ptr[c]; T.nk = cnt[c]; T.voff = voff[c];
         tiles.push_back (T);
      }
   }
   if (ncol0 >= ncol) color_tile[1] = (int) tiles.size ();
   color_tile[2] = (int) tiles.size ();
   if (2 * nval > 3 * (long long) L.nnz || tiles.empty ()) { color_tile[0] = color_tile[1] = color_tile[2] = 0; return 0; }
   size_t held = 0;
   auto put = [&] (void **dst, const void *src, size_t bytes) {
      void *q = nullptr;
      if (hipMalloc (&q, bytes ? bytes : 1) != hipSuccess) return false;
      *dst = q;
      held += bytes ? bytes : 1;
      *device_bytes += bytes ? bytes : 1;
      return !src || !bytes || hipMemcpyAsync (q, src, bytes, hipMemcpyHostToDevice, st) == hipSuccess;
   };
   const bool ok = put ((void **) &L.dg_ptr, ptr.data (), ptr.size () * sizeof (int)) && put ((void **) &L.dg_key, nullptr, ((size_t) ptr[ncol] + DG_UNROLL) * sizeof (int)) &&
                   put ((void **) &L.dg_voff, voff.data (), voff.size () * sizeof (long long)) && put ((void **) &L.dg_val, nullptr, (size_t) nval * sizeof (float)) &&
                   put ((void **) &L.dg_tile, tiles.data (), tiles.size () * sizeof (DgTile));
   if (!ok) {
      (void) hipStreamSynchronize (st);
      diag_drop (L, device_bytes, held);
      color_tile[0] = color_tile[1] = color_tile[2] = 0;
      return 0;
   }
   L.dg_ntile = (int) tiles.size ();
   L.dg_ncol = ncol;
   L.dg_nkey = ptr[ncol];
   L.dg_nval = nval;
   (void) hipMemsetAsync (L.dg_key + ptr[ncol], 0, DG_UNROLL * sizeof (int), st);
   const int64_t slots = (int64_t) ncol * cap;
   hipLaunchKernelGGL (diag_compact_kernel, dim3 ((unsigned) ((slots + DG_THREADS - 1) / DG_THREADS)), dim3 (DG_THREADS), 0, st, ncol, cap, (const int *) tmpkey.p,
                       (const int *) L.dg_ptr, L.dg_key);
   launch_diag_fill (L, st);
   // the host arrays and the scratch buffers go when this returns
   if (hipStreamSynchronize (st) != hipSuccess) {
      diag_drop (L, device_bytes, held);
      color_tile[0] = color_tile[1] = color_tile[2] = 0;
      return 0;
   }
   return 1;
}

void launch_diag_fill (const CsrDev &L, hipStream_t st)
{
   if (!L.dg_val || L.dg_ntile <= 0) return;
   hipLaunchKernelGGL (diag_fill_kernel, dim3 ((L.dg_ntile + DG_WAVES - 1) / DG_WAVES), dim3 (DG_THREADS), 0, st, L.dg_ntile, (const DgTile *) L.dg_tile,
                       (const int *) L.rowptr, (const int *) L.colind, (const float *) L.valf, (const int *) L.dg_key, L.dg_val);
}

void launch_diag_residual (const CsrDev &L, int tile0, int tile1, const double *x, const double *b, double *y, hipStream_t st)
{
   const int cnt = tile1 - tile0;
   if (cnt <= 0) return;
   hipLaunchKernelGGL (diag_residual_kernel, dim3 ((cnt + DG_WAVES - 1) / DG_WAVES), dim3 (DG_THREADS), 0, st, (const DgTile *) L.dg_tile + tile0, cnt,
                       (const int *) L.dg_key, (const float *) L.dg_val, x, b, y, (int) L.n);
}
