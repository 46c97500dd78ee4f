// Sensitivity of a solve to the stored matrix values: a sampled outer product on the CSR pattern (nkp_value_gradient).
//
// With x = A^-1 b and the adjoint solution lambda = A^-T g, dL/da_ij = - lambda_i x_j on the pattern.  For every stored entry e
// of row i with column j = colind[e], and K pairs of vectors,
//    s = lam_0[i] * x_0[j];  s = s + lam_c[i] * x_c[j]  (c = 1 .. K - 1, ascending);  g[e] = (g[e] +) alpha * s
// every product and every sum rounded on its own (no contraction), so the result can be restated bit for bit on the host.
//
// The kernel is the SpMV's stream with the value read turned into a value write: one workgroup per CSR-stream row block
// (at most 256 rows and 2048 entries, a longer row alone in its block), coalesced colind loads and g stores, and two gathers --
// x at the entry's column (the SpMV's gather, mostly L2 hits) and lambda at the entry's row.  The row is found in the block's
// slice of rowptr, staged in LDS: an upper-bound search of eight steps whatever the row lengths (a lane per row stamping its
// entries would serialise on one long row and collide on the banks for uniform ones).  A block of one row -- the long-row case
// -- needs no search and is walked in chunks; a block without entries returns after its two rowptr loads.
// K >= 2: lambda and x are K-interleaved (X[i * K + c]), so the K values of a row come with one or a few 16-byte loads; columns
// c >= nk of a width-K buffer are never read, so a width may serve fewer vectors (3 in 4, 5 .. 7 in 8) with unchanged bits.
#include "nkp_dev.h"

#define VG_THREADS 256

template <int K>
__global__ __launch_bounds__ (VG_THREADS)
void value_gradient_kernel (const int *__restrict__ rowblk, int nrowblk, int per_xcd, const int *__restrict__ rowptr, const int *__restrict__ colind,
                            const double *__restrict__ lam, const double *__restrict__ x, int nk, double alpha, int accumulate, double *__restrict__ g)
{
   __shared__ int sp[NKP_SPMV_MAX_ROWS + 1];
   constexpr int GU = K >= 8 ? 2 : K == 4 ? 4 : 8;      // entries per lane in flight (GU * 2 K gathered doubles in registers)
   const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
   const int lb = xcd * per_xcd + idx;
   if (idx >= per_xcd || lb >= nrowblk) return;
   const int tid = threadIdx.x;
   const int r0 = rowblk[lb], r1 = rowblk[lb + 1], nr = r1 - r0;
   const int e0 = rowptr[r0], e1 = rowptr[r1];
   if (e1 <= e0) return;                                 // empty rows only: nothing read, nothing written
   if (nr > 1) {
      for (int i = tid; i <= nr && i <= NKP_SPMV_MAX_ROWS; i += VG_THREADS) sp[i] = rowptr[r0 + i] - e0;
      __syncthreads ();
   }
   for (int64_t base = e0; base < e1; base += VG_THREADS * GU) {
      int col[GU], row[GU];
#pragma unroll
      for (int u = 0; u < GU; u++) {
         const int64_t e = base + tid + u * VG_THREADS;
         col[u] = e < e1 ? colind[e] : 0;
      }
#pragma unroll
      for (int u = 0; u < GU; u++) {
         // the last row whose first entry is not behind entry k: rows without entries share their successor's start and lose
         int pos = 0;
         if (nr > 1) {
            const int64_t k = base + tid + u * VG_THREADS - e0;
#pragma unroll
            for (int step = NKP_SPMV_MAX_ROWS / 2; step > 0; step >>= 1) {
               const int p = pos + step;
               if (p < nr && sp[p] <= k) pos = p;
            }
         }
         row[u] = r0 + pos;
      }
      double lv[GU][K], xv[GU][K];
#pragma unroll
      for (int u = 0; u < GU; u++) {
         const double *lr = lam + (int64_t) row[u] * K, *xr = x + (int64_t) col[u] * K;
         if constexpr (K == 1) { lv[u][0] = lr[0]; xv[u][0] = xr[0]; }
         else {
#pragma unroll
            for (int h = 0; h < K / 2; h++) {
               const double2 a = *reinterpret_cast<const double2 *> (lr + 2 * h), b = *reinterpret_cast<const double2 *> (xr + 2 * h);
               lv[u][2 * h] = a.x; lv[u][2 * h + 1] = a.y;
               xv[u][2 * h] = b.x; xv[u][2 * h + 1] = b.y;
            }
         }
      }
#pragma unroll
      for (int u = 0; u < GU; u++) {
         const int64_t e = base + tid + u * VG_THREADS;
         if (e < e1) {
            double s = __dmul_rn (lv[u][0], xv[u][0]);
#pragma unroll
            for (int c = 1; c < K; c++)
               if (c < nk) s = __dadd_rn (s, __dmul_rn (lv[u][c], xv[u][c]));
            double v = __dmul_rn (alpha, s);
            if (accumulate) v = __dadd_rn (g[e], v);
            g[e] = v;
         }
      }
   }
}

// g (+)= alpha * sum_c lam_c[row] x_c[col] on the pattern of A; K in {1, 2, 4, 8} is the interleave width of lam and x (1: plain
// vectors), nk <= K the number of pairs summed.  x is indexed by A's columns (row-distributed: [own | halo] like the SpMV's input)
void launch_value_gradient (int K, int nk, const CsrDev &A, const double *lam, const double *x, double alpha, int accumulate, double *g, hipStream_t st)
{
   if (A.nrowblk <= 0 || A.nnz <= 0) return;
   const int per_xcd = (A.nrowblk + 7) / 8;
   with_int<1, 2, 4, 8> (K, [&] (auto k) {
      hipLaunchKernelGGL (value_gradient_kernel<decltype (k)::value>, dim3 (per_xcd * 8), dim3 (VG_THREADS), 0, st, A.rowblk, A.nrowblk, per_xcd, A.rowptr, A.colind,
                          lam, x, nk < K ? nk : K, alpha, accumulate, g);
   });
}
