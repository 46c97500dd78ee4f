// K right-hand sides through ONE sweep of the matrix: the operator and the multilevel cycle on K interleaved vectors.
//
// The reference solves its tracers one after the other against one factorisation (RHS loop, reference
// src/solve_ABglobal.c:370-409).  Every kernel of a solve here is bound by the matrix / factor streams (12 bytes per entry of
// A, 8 per entry of a level operator, 20 per row of column factors) or, on the small levels, by launch latency -- both are
// per SWEEP, not per right-hand side.  So K systems share the sweeps: vectors are interleaved, X[i * K + k] = row i of system
// k (K = 2 or 4: one or two 16-byte loads per gathered row), and every kernel below does for the K columns exactly what its
// single-vector twin (spmv.hip, colblock.hip, blas1.hip) does for one -- same products, same summation and substitution
// order -- so every column of a batched solve has the bits of the solve done alone (tests/test_gpu_batch.py).
// The Krylov recurrences stay per system (their basis vectors are not shared: nothing to amortise); batch_solve.hip drives K
// of them in lockstep around these kernels.
#include "nkp_dev.h"

#define BT_THREADS 256
#define BT_WAVES (BT_THREADS / NKP_WAVE)

static inline int bt_grid (int64_t n) { int64_t g = (n + BT_THREADS - 1) / BT_THREADS; return (int) (g < 1 ? 1 : g > 65535 * 16 ? 65535 * 16 : g); }

// ---------------------------------------------------------------- interleave / de-interleave
// X[i * K + k] = src_k[i]; systems without a vector (src_k == NULL) contribute zeros
struct BatchPtrs { const double *p[NKP_BATCH_MAX]; };
struct BatchOutPtrs { double *p[NKP_BATCH_MAX]; };

template <int K>
__global__ __launch_bounds__ (BT_THREADS)
void interleave_kernel (BatchPtrs src, double *__restrict__ X, int64_t n)
{
   const int64_t stride = (int64_t) gridDim.x * BT_THREADS;
   for (int64_t i = (int64_t) blockIdx.x * BT_THREADS + threadIdx.x; i < n; i += stride) {
#pragma unroll
      for (int k = 0; k < K; k++) X[i * K + k] = src.p[k] ? src.p[k][i] : 0.0;
   }
}

// row-weighted iteration: X[i * K + k] = src_k[i] * scale[i], the product rounded like launch_vmul rounds it
template <int K>
__global__ __launch_bounds__ (BT_THREADS)
void interleave_scaled_kernel (BatchPtrs src, const double *__restrict__ scale, double *__restrict__ X, int64_t n)
{
   const int64_t stride = (int64_t) gridDim.x * BT_THREADS;
   for (int64_t i = (int64_t) blockIdx.x * BT_THREADS + threadIdx.x; i < n; i += stride) {
      const double sc = scale[i];
#pragma unroll
      for (int k = 0; k < K; k++) X[i * K + k] = src.p[k] ? __dmul_rn (src.p[k][i], sc) : 0.0;
   }
}

template <int K>
__global__ __launch_bounds__ (BT_THREADS)
void deinterleave_kernel (const double *__restrict__ X, BatchOutPtrs dst, int64_t n)
{
   const int64_t stride = (int64_t) gridDim.x * BT_THREADS;
   for (int64_t i = (int64_t) blockIdx.x * BT_THREADS + threadIdx.x; i < n; i += stride) {
#pragma unroll
      for (int k = 0; k < K; k++)
         if (dst.p[k]) dst.p[k][i] = X[i * K + k];
   }
}

void launch_interleave (int K, const double *const *src, double *X, int64_t n, hipStream_t st, const double *scale)
{
   BatchPtrs P;
   for (int k = 0; k < NKP_BATCH_MAX; k++) P.p[k] = k < K ? src[k] : nullptr;
   with_k (K, [&] (auto k) {
      if (scale) hipLaunchKernelGGL (interleave_scaled_kernel<decltype (k)::value>, dim3 (bt_grid (n)), dim3 (BT_THREADS), 0, st, P, scale, X, n);
      else hipLaunchKernelGGL (interleave_kernel<decltype (k)::value>, dim3 (bt_grid (n)), dim3 (BT_THREADS), 0, st, P, X, n);
   });
}

void launch_deinterleave (int K, const double *X, double *const *dst, int64_t n, hipStream_t st)
{
   BatchOutPtrs P;
   for (int k = 0; k < NKP_BATCH_MAX; k++) P.p[k] = k < K ? dst[k] : nullptr;
   with_k (K, [&] (auto k) { hipLaunchKernelGGL (deinterleave_kernel<decltype (k)::value>, dim3 (bt_grid (n)), dim3 (BT_THREADS), 0, st, X, P, n); });
}

// ---------------------------------------------------------------- CSR SpMV, K columns
// csr_spmv_stream_kernel (spmv.hip) with the (value, column) stream of a row block read ONCE into registers and K / 2 passes
// over it: a pass gathers the 16-byte pair (x[c][2g], x[c][2g + 1]), parks both products in LDS and sums every row's segment
// in stored order.  MODE 0: y = A x   1: y = b - A x
// SCALED (MODE 0, row-weighted iteration): every finished sum times scale[row], one rounded multiplication like launch_vmul's
template <int MODE, class VT, int K, bool SCALED = false>
__global__ __launch_bounds__ (BT_THREADS)
void csr_spmv_batch_kernel (const int *__restrict__ rowblk_all, int rb0, int nrowblk, int per_xcd, const int *__restrict__ rowptr,
                            const int *__restrict__ colind, const VT *__restrict__ val, const double *__restrict__ x,
                            double *__restrict__ y, const double *__restrict__ b, const double *__restrict__ scale = nullptr)
{
   __shared__ double2 prod[NKP_SPMV_LDS_NNZ];
   __shared__ double2 wsum[BT_WAVES];
   constexpr int SLOTS = NKP_SPMV_LDS_NNZ / BT_THREADS;
   const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
   const int lb = xcd * per_xcd + idx;
   if (idx >= per_xcd || lb >= nrowblk) return;
   const int tid = threadIdx.x;
   const int *rowblk = rowblk_all + rb0;
   const int r0 = rowblk[lb], r1 = rowblk[lb + 1];
   const int e0 = rowptr[r0], e1 = rowptr[r1];
   const int cnt = e1 - e0;
   int seg0 = 0, seg1 = 0;
   if (r0 + tid < r1) { seg0 = rowptr[r0 + tid]; seg1 = rowptr[r0 + tid + 1]; }
   if (cnt > NKP_SPMV_LDS_NNZ) {
      // a single long row: strided accumulate + block reduction in the order of the single-vector kernel
      for (int g = 0; g < K / 2; g++) {
         double2 acc = make_double2 (0.0, 0.0);
         for (int e = e0 + tid; e < e1; e += BT_THREADS) {
            const double v = (double) val[e];
            const double2 xv = *reinterpret_cast<const double2 *> (x + (int64_t) colind[e] * K + 2 * g);
            acc.x += v * xv.x;
            acc.y += v * xv.y;
         }
         for (int off = NKP_WAVE / 2; off > 0; off >>= 1) { acc.x += __shfl_down (acc.x, off); acc.y += __shfl_down (acc.y, off); }
         if ((tid & (NKP_WAVE - 1)) == 0) wsum[tid / NKP_WAVE] = acc;
         __syncthreads ();
         if (tid == 0) {
            double2 s = make_double2 (0.0, 0.0);
            for (int w = 0; w < BT_WAVES; w++) { s.x += wsum[w].x; s.y += wsum[w].y; }
            if (MODE == 1) { const double2 bv = *reinterpret_cast<const double2 *> (b + (int64_t) r0 * K + 2 * g); s.x = bv.x - s.x; s.y = bv.y - s.y; }
            if (SCALED) { const double sc = scale[r0]; s.x = __dmul_rn (s.x, sc); s.y = __dmul_rn (s.y, sc); }
            *reinterpret_cast<double2 *> (y + (int64_t) r0 * K + 2 * g) = s;
         }
         __syncthreads ();
      }
      return;
   }
   VT v[SLOTS];
   int c[SLOTS];
#pragma unroll
   for (int u = 0; u < SLOTS; u++) {
      const int k = tid + u * BT_THREADS;
      v[u] = k < cnt ? val[e0 + k] : (VT) 0;
      c[u] = k < cnt ? colind[e0 + k] : 0;
   }
   // all K values of a gathered row are requested together: the two 16-byte halves of a row of x sit in one cache line, so
   // the second load rides on the first one's L2 request (first version: one pass per pair = twice the L2 requests, and the
   // batched kernel was L2-request-bound at 1.9 TB/s)
   double2 xg[K / 2][SLOTS];
#pragma unroll
   for (int u = 0; u < SLOTS; u++) {
      const double *xr = x + (int64_t) c[u] * K;
#pragma unroll
      for (int g = 0; g < K / 2; g++) xg[g][u] = *reinterpret_cast<const double2 *> (xr + 2 * g);
   }
#pragma unroll
   for (int g = 0; g < K / 2; g++) {
#pragma unroll
      for (int u = 0; u < SLOTS; u++) {
         const int k = tid + u * BT_THREADS;
         if (k < cnt) prod[k] = make_double2 ((double) v[u] * xg[g][u].x, (double) v[u] * xg[g][u].y);
      }
      __syncthreads ();
      const int r = r0 + tid;
      if (r < r1) {
         const int s0 = seg0 - e0, s1 = seg1 - e0;
         double2 acc = make_double2 (0.0, 0.0);
#pragma unroll 4
         for (int k = s0; k < s1; k++) { acc.x += prod[k].x; acc.y += prod[k].y; }
         if (MODE == 1) { const double2 bv = *reinterpret_cast<const double2 *> (b + (int64_t) r * K + 2 * g); acc.x = bv.x - acc.x; acc.y = bv.y - acc.y; }
         if (SCALED) { const double sc = scale[r]; acc.x = __dmul_rn (acc.x, sc); acc.y = __dmul_rn (acc.y, sc); }
         *reinterpret_cast<double2 *> (y + (int64_t) r * K + 2 * g) = acc;
      }
      if (g + 1 < K / 2) __syncthreads ();
   }
}

// The other way round: the workgroup stages the row block's (value, column) stream in LDS with coalesced loads (8 bytes per
// entry instead of 16 K of products: 16 KB per workgroup, twice the workgroups per CU), then every row's lane walks its own
// segment, gathers the K-wide rows of x itself (GU entries in flight) and accumulates its K sums in registers -- same
// products, same stored order, one pass for any K.
// SPLIT: the K results of a row go to K separate vectors (split.p[k][r]; NULL = dropped) instead of the interleaved y -- the
// operator product at the end of an Arnoldi step writes every system's w directly.  With MODE 1 the right-hand side is split
// too (bsplit.p[k][r]; NULL = zero): the residual between two chained cycles, p1_k = v_k - A z_k, from and to per-system vectors.
// SCALED (row-weighted iteration): MODE 0 multiplies every finished sum by scale[row]; MODE 1 + SPLIT multiplies the right-hand
// side it reads by scale[row].  Either is ONE rounded multiplication of a finished value, which is what launch_vmul does.
template <int MODE, class VT, int K, bool SPLIT = false, bool SCALED = false>
__global__ __launch_bounds__ (BT_THREADS)
void csr_spmv_batch_rows_kernel (const int *__restrict__ rowblk_all, int rb0, int nrowblk, int per_xcd, const int *__restrict__ rowptr,
                                 const int *__restrict__ colind, const VT *__restrict__ val, const double *__restrict__ x,
                                 double *__restrict__ y, const double *__restrict__ b, BatchOutPtrs split = BatchOutPtrs (),
                                 BatchPtrs bsplit = BatchPtrs (), const double *__restrict__ scale = nullptr)
{
   __shared__ VT sv[NKP_SPMV_LDS_NNZ];
   __shared__ int sc[NKP_SPMV_LDS_NNZ];
   __shared__ double2 wsum[BT_WAVES];
   constexpr int SLOTS = NKP_SPMV_LDS_NNZ / BT_THREADS, GU = 16 / K;
   const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
   const int lb = xcd * per_xcd + idx;
   if (idx >= per_xcd || lb >= nrowblk) return;
   const int tid = threadIdx.x;
   const int *rowblk = rowblk_all + rb0;
   const int r0 = rowblk[lb], r1 = rowblk[lb + 1];
   const int e0 = rowptr[r0], e1 = rowptr[r1];
   const int cnt = e1 - e0;
   if (cnt > NKP_SPMV_LDS_NNZ) {
      for (int g = 0; g < K / 2; g++) {
         double2 acc = make_double2 (0.0, 0.0);
         for (int e = e0 + tid; e < e1; e += BT_THREADS) {
            const double v = (double) val[e];
            const double2 xv = *reinterpret_cast<const double2 *> (x + (int64_t) colind[e] * K + 2 * g);
            acc.x += v * xv.x;
            acc.y += v * xv.y;
         }
         for (int off = NKP_WAVE / 2; off > 0; off >>= 1) { acc.x += __shfl_down (acc.x, off); acc.y += __shfl_down (acc.y, off); }
         if ((tid & (NKP_WAVE - 1)) == 0) wsum[tid / NKP_WAVE] = acc;
         __syncthreads ();
         if (tid == 0) {
            double2 s = make_double2 (0.0, 0.0);
            for (int w = 0; w < BT_WAVES; w++) { s.x += wsum[w].x; s.y += wsum[w].y; }
            if (MODE == 1) {
               double2 bv;
               if (SPLIT) {
                  bv.x = bsplit.p[2 * g] ? bsplit.p[2 * g][r0] : 0.0;
                  bv.y = bsplit.p[2 * g + 1] ? bsplit.p[2 * g + 1][r0] : 0.0;
                  if (SCALED) { const double sc = scale[r0]; bv.x = __dmul_rn (bv.x, sc); bv.y = __dmul_rn (bv.y, sc); }
               } else bv = *reinterpret_cast<const double2 *> (b + (int64_t) r0 * K + 2 * g);
               s.x = bv.x - s.x; s.y = bv.y - s.y;
            } else if (SCALED) { const double sc = scale[r0]; s.x = __dmul_rn (s.x, sc); s.y = __dmul_rn (s.y, sc); }
            if (SPLIT) { if (split.p[2 * g]) split.p[2 * g][r0] = s.x; if (split.p[2 * g + 1]) split.p[2 * g + 1][r0] = s.y; }
            else *reinterpret_cast<double2 *> (y + (int64_t) r0 * K + 2 * g) = s;
         }
         __syncthreads ();
      }
      return;
   }
   const int r = r0 + tid;
   int s0 = 0, s1 = 0;
   if (r < r1) { s0 = rowptr[r] - e0; s1 = rowptr[r + 1] - e0; }
   {
      VT v[SLOTS];
      int c[SLOTS];
#pragma unroll
      for (int u = 0; u < SLOTS; u++) {
         const int k = tid + u * BT_THREADS;
         v[u] = k < cnt ? val[e0 + k] : (VT) 0;
         c[u] = k < cnt ? colind[e0 + k] : 0;
      }
#pragma unroll
      for (int u = 0; u < SLOTS; u++) {
         const int k = tid + u * BT_THREADS;
         if (k < cnt) { sv[k] = v[u]; sc[k] = c[u]; }
      }
   }
   double2 bv[K / 2];
#pragma unroll
   for (int g = 0; g < K / 2; g++) {
      bv[g] = make_double2 (0.0, 0.0);
      if (MODE == 1 && r < r1) {
         if (SPLIT) {
            if (bsplit.p[2 * g]) bv[g].x = bsplit.p[2 * g][r];
            if (bsplit.p[2 * g + 1]) bv[g].y = bsplit.p[2 * g + 1][r];
            if (SCALED) { const double sc = scale[r]; bv[g].x = __dmul_rn (bv[g].x, sc); bv[g].y = __dmul_rn (bv[g].y, sc); }
         } else bv[g] = *reinterpret_cast<const double2 *> (b + (int64_t) r * K + 2 * g);
      }
   }
   __syncthreads ();
   if (r >= r1) return;
   double2 acc[K / 2];
#pragma unroll
   for (int g = 0; g < K / 2; g++) acc[g] = make_double2 (0.0, 0.0);
   for (int k = s0; k < s1; k += GU) {
      double vv[GU];
      double2 xg[GU][K / 2];
#pragma unroll
      for (int u = 0; u < GU; u++) {
         const int kk = k + u < s1 ? k + u : s1 - 1;
         vv[u] = (double) sv[kk];
         const double *xr = x + (int64_t) sc[kk] * K;
#pragma unroll
         for (int g = 0; g < K / 2; g++) xg[u][g] = *reinterpret_cast<const double2 *> (xr + 2 * g);
      }
#pragma unroll
      for (int u = 0; u < GU; u++)
         if (k + u < s1) {
#pragma unroll
            for (int g = 0; g < K / 2; g++) { acc[g].x += vv[u] * xg[u][g].x; acc[g].y += vv[u] * xg[u][g].y; }
         }
   }
#pragma unroll
   for (int g = 0; g < K / 2; g++) {
      if (MODE == 1) { acc[g].x = bv[g].x - acc[g].x; acc[g].y = bv[g].y - acc[g].y; }
      else if (SCALED) { const double sc = scale[r]; acc[g].x = __dmul_rn (acc[g].x, sc); acc[g].y = __dmul_rn (acc[g].y, sc); }
      if (SPLIT) { if (split.p[2 * g]) split.p[2 * g][r] = acc[g].x; if (split.p[2 * g + 1]) split.p[2 * g + 1][r] = acc[g].y; }
      else *reinterpret_cast<double2 *> (y + (int64_t) r * K + 2 * g) = acc[g];
   }
}

// csr_spmv_batch_rows_kernel<MODE, storage of A, K, SPLIT, SCALED> on the row blocks [rb0, rb0 + cnt) of A
template <int MODE, bool SPLIT, bool SCALED>
static void launch_batch_rows (int K, const CsrDev &A, int rb0, int cnt, const double *x, double *y, const double *b, const BatchOutPtrs &split,
                               const BatchPtrs &bsplit, const double *scale, hipStream_t st)
{
   const int per_xcd = (cnt + 7) / 8;
   with_storage (A.valf, A.val, [&] (auto val) {
      with_k (K, [&] (auto k) {
         hipLaunchKernelGGL ((csr_spmv_batch_rows_kernel<MODE, elem_t<decltype (val)>, decltype (k)::value, SPLIT, SCALED>), dim3 (per_xcd * 8), dim3 (BT_THREADS), 0, st,
                             A.rowblk, rb0, cnt, per_xcd, A.rowptr, A.colind, val, x, y, b, split, bsplit, scale);
      });
   });
}

void launch_csr_spmv_batch (int K, const CsrDev &A, int rb0, int rb1, const double *x, double *y, const double *b, int mode, hipStream_t st, const double *scale)
{
   const int cnt = rb1 - rb0;
   if (cnt <= 0) return;
   const nkp_tuning &T = A.tune ? *A.tune : nkp_builtin_tuning ();
   const bool scaled = scale && mode == 0;          // y = R (A x): the same kernels with the scaling in their epilogue
   if (K == 8 || T.batch_spmv_rows) {               // (the products-in-LDS variant stops at four)
      if (scaled) launch_batch_rows<0, false, true> (K, A, rb0, cnt, x, y, b, BatchOutPtrs (), BatchPtrs (), scale, st);
      else if (mode == 0) launch_batch_rows<0, false, false> (K, A, rb0, cnt, x, y, b, BatchOutPtrs (), BatchPtrs (), nullptr, st);
      else launch_batch_rows<1, false, false> (K, A, rb0, cnt, x, y, b, BatchOutPtrs (), BatchPtrs (), nullptr, st);
      return;
   }
   const int per_xcd = (cnt + 7) / 8;
   with_storage (A.valf, A.val, [&] (auto val) {
      using VT = elem_t<decltype (val)>;
      with_int<2, 4> (K, [&] (auto k) {
         constexpr int KK = decltype (k)::value;
         const auto products = [&] (auto kernel, const double *sc) {
            hipLaunchKernelGGL (kernel, dim3 (per_xcd * 8), dim3 (BT_THREADS), 0, st, A.rowblk, rb0, cnt, per_xcd, A.rowptr, A.colind, val, x, y, b, sc);
         };
         if (scaled) products (csr_spmv_batch_kernel<0, VT, KK, true>, scale);
         else if (mode == 0) products (csr_spmv_batch_kernel<0, VT, KK, false>, nullptr);
         else products (csr_spmv_batch_kernel<1, VT, KK, false>, nullptr);
      });
   });
}

// y_k = A x_k for the K interleaved columns of x, every result in its own vector (dst[k] NULL: not wanted); row blocks
// [rb0, rb1) only (the row-distributed flavour multiplies its interior rows while the halo of x travels)
void launch_csr_spmv_batch_split_range (int K, const CsrDev &A, int rb0, int rb1, const double *x, double *const *dst, hipStream_t st, const double *scale)
{
   if (rb1 <= rb0) return;
   BatchOutPtrs P;
   for (int k = 0; k < NKP_BATCH_MAX; k++) P.p[k] = k < K ? dst[k] : nullptr;
   if (scale) launch_batch_rows<0, true, true> (K, A, rb0, rb1 - rb0, x, nullptr, nullptr, P, BatchPtrs (), scale, st);
   else launch_batch_rows<0, true, false> (K, A, rb0, rb1 - rb0, x, nullptr, nullptr, P, BatchPtrs (), nullptr, st);
}

void launch_csr_spmv_batch_split (int K, const CsrDev &A, const double *x, double *const *dst, hipStream_t st, const double *scale)
{
   launch_csr_spmv_batch_split_range (K, A, 0, A.nrowblk, x, dst, st, scale);
}

// dst_k = b_k - A x_k (b_k, times bscale when given, and dst_k per system; NULL: system takes no part), row blocks [rb0, rb1)
void launch_csr_residual_batch_split_range (int K, const CsrDev &A, int rb0, int rb1, const double *x, const double *const *b, const double *bscale,
                                            double *const *dst, hipStream_t st)
{
   if (rb1 <= rb0) return;
   BatchOutPtrs P;
   BatchPtrs Q;
   for (int k = 0; k < NKP_BATCH_MAX; k++) { P.p[k] = k < K ? dst[k] : nullptr; Q.p[k] = k < K ? b[k] : nullptr; }
   if (bscale) launch_batch_rows<1, true, true> (K, A, rb0, rb1 - rb0, x, nullptr, nullptr, P, Q, bscale, st);
   else launch_batch_rows<1, true, false> (K, A, rb0, rb1 - rb0, x, nullptr, nullptr, P, Q, bscale, st);
}

// ---------------------------------------------------------------- grid transfer / permutation / coarsest solve, K columns
template <int K>
__global__ __launch_bounds__ (BT_THREADS)
void restrict_sum_batch_kernel (const int *__restrict__ rptr, const int *__restrict__ ridx, const double *__restrict__ fine, double *__restrict__ coarse, int64_t nc)
{
   const int64_t stride = (int64_t) gridDim.x * BT_THREADS;
   for (int64_t t = (int64_t) blockIdx.x * BT_THREADS + threadIdx.x; t < nc * K; t += stride) {
      const int64_t I = t / K;
      const int k = (int) (t % K);
      double acc = 0.0;
      for (int q = rptr[I]; q < rptr[I + 1]; q++) acc += fine[(int64_t) ridx[q] * K + k];
      coarse[t] = acc;
   }
}

template <int K>
__global__ __launch_bounds__ (BT_THREADS)
void prolong_add_batch_kernel (const int *__restrict__ cmap, const double *__restrict__ coarse, double *__restrict__ fine, int64_t nf, double omega)
{
   const int64_t stride = (int64_t) gridDim.x * BT_THREADS;
   for (int64_t t = (int64_t) blockIdx.x * BT_THREADS + threadIdx.x; t < nf * K; t += stride)
      fine[t] += omega * coarse[(int64_t) cmap[t / K] * K + (t % K)];
}

template <int K>
__global__ __launch_bounds__ (BT_THREADS)
void gather_batch_kernel (const int *__restrict__ perm, const double *__restrict__ in, double *__restrict__ out, int64_t n)
{
   const int64_t stride = (int64_t) gridDim.x * BT_THREADS;
   for (int64_t t = (int64_t) blockIdx.x * BT_THREADS + threadIdx.x; t < n * K; t += stride)
      out[t] = in[(int64_t) perm[t / K] * K + (t % K)];
}

// the entry and the exit of a batched cycle application, fused with the (de-)interleave of the per-system vectors:
//   entry: out[i * K + k] = src_k[perm[i]]        exit: z[perm[i] * K + k] = dst_k[perm[i]] = in[i * K + k]
template <int K>
__global__ __launch_bounds__ (BT_THREADS)
void gather_interleave_kernel (const int *__restrict__ perm, BatchPtrs src, double *__restrict__ out, int64_t n)
{
   const int64_t stride = (int64_t) gridDim.x * BT_THREADS;
   for (int64_t i = (int64_t) blockIdx.x * BT_THREADS + threadIdx.x; i < n; i += stride) {
      const int64_t pi = perm[i];
#pragma unroll
      for (int k = 0; k < K; k++) out[i * K + k] = src.p[k] ? src.p[k][pi] : 0.0;
   }
}

// the entry in the row-weighted iteration: out[i * K + k] = src_k[perm[i]] * scale[perm[i]] (launch_vmul's product, then the gather)
template <int K>
__global__ __launch_bounds__ (BT_THREADS)
void gather_interleave_scaled_kernel (const int *__restrict__ perm, BatchPtrs src, const double *__restrict__ scale, double *__restrict__ out, int64_t n)
{
   const int64_t stride = (int64_t) gridDim.x * BT_THREADS;
   for (int64_t i = (int64_t) blockIdx.x * BT_THREADS + threadIdx.x; i < n; i += stride) {
      const int64_t pi = perm[i];
      const double sc = scale[pi];
#pragma unroll
      for (int k = 0; k < K; k++) out[i * K + k] = src.p[k] ? __dmul_rn (src.p[k][pi], sc) : 0.0;
   }
}

// z_k += p_k between two chained cycles, on the interleaved z that feeds the operator and on the systems' own vectors at once:
// z[i * K + k] = dst_k[i] = z[i * K + k] + p[i * K + k] for the systems that take part (dst_k != NULL); the others keep their z
template <int K>
__global__ __launch_bounds__ (BT_THREADS)
void add_split_kernel (const double *__restrict__ p, double *__restrict__ z, BatchOutPtrs dst, int64_t n)
{
   const int64_t stride = (int64_t) gridDim.x * BT_THREADS;
   for (int64_t i = (int64_t) blockIdx.x * BT_THREADS + threadIdx.x; i < n; i += stride) {
#pragma unroll
      for (int k = 0; k < K; k++)
         if (dst.p[k]) {
            const double v = z[i * K + k] + p[i * K + k];
            z[i * K + k] = v;
            dst.p[k][i] = v;
         }
   }
}

template <int K>
__global__ __launch_bounds__ (BT_THREADS)
void scatter_split_kernel (const int *__restrict__ perm, const double *__restrict__ in, double *__restrict__ z, BatchOutPtrs dst, int64_t n)
{
   const int64_t stride = (int64_t) gridDim.x * BT_THREADS;
   for (int64_t i = (int64_t) blockIdx.x * BT_THREADS + threadIdx.x; i < n; i += stride) {
      const int64_t pi = perm[i];
#pragma unroll
      for (int k = 0; k < K; k++) {
         const double v = in[i * K + k];
         z[pi * K + k] = v;
         if (dst.p[k]) dst.p[k][pi] = v;
      }
   }
}

// ---------------------------------------------------------------- row-distributed flavour: K-wide messages and the overlap rows
// One message row carries the K systems' values of one matrix row (8 K bytes, consecutive lanes write consecutive rows:
// coalesced 16- / 32- / 64-byte stores), so that ONE alltoallv with K times the plan's counts serves the whole group and
// the receiver's halo part is K-interleaved as it arrives.
//   out[i * K + k] = src_k[idx[i]]   (a system without a vector sends zeros)
template <int K>
__global__ __launch_bounds__ (BT_THREADS)
void pack_rows_split_kernel (const int *__restrict__ idx, BatchPtrs src, double *__restrict__ out, int64_t nrows)
{
   const int64_t stride = (int64_t) gridDim.x * BT_THREADS;
   for (int64_t i = (int64_t) blockIdx.x * BT_THREADS + threadIdx.x; i < nrows; i += stride) {
      const int64_t r = idx[i];
#pragma unroll
      for (int k = 0; k < K; k++) out[i * K + k] = src.p[k] ? src.p[k][r] : 0.0;
   }
}

// gather_interleave_kernel on the extended rows [own rows | overlap rows] of a rank's hierarchy: row perm[i] < n_own comes
// from the systems' own vectors, the others from the K-interleaved halo rows that have just arrived (sel[.] = halo position)
template <int K>
__global__ __launch_bounds__ (BT_THREADS)
void gather_interleave_ext_kernel (const int *__restrict__ perm, BatchPtrs src, const double *__restrict__ halo, const int *__restrict__ sel,
                                   int64_t n_own, double *__restrict__ out, int64_t n)
{
   const int64_t stride = (int64_t) gridDim.x * BT_THREADS;
   for (int64_t i = (int64_t) blockIdx.x * BT_THREADS + threadIdx.x; i < n; i += stride) {
      const int64_t pi = perm[i];
      if (pi < n_own) {
#pragma unroll
         for (int k = 0; k < K; k++) out[i * K + k] = src.p[k] ? src.p[k][pi] : 0.0;
      } else {
         const double *h = halo + (int64_t) sel[pi - n_own] * K;
#pragma unroll
         for (int k = 0; k < K; k++) out[i * K + k] = src.p[k] ? h[k] : 0.0;
      }
   }
}

// the same when the overlap rows arrive on their own, in the hierarchy's order (two or more rings): row perm[i] >= n_own is
// row perm[i] - n_own of the K-interleaved receive block
template <int K>
__global__ __launch_bounds__ (BT_THREADS)
void gather_interleave_ext_block_kernel (const int *__restrict__ perm, BatchPtrs src, const double *__restrict__ recv, int64_t n_own,
                                         double *__restrict__ out, int64_t n)
{
   const int64_t stride = (int64_t) gridDim.x * BT_THREADS;
   for (int64_t i = (int64_t) blockIdx.x * BT_THREADS + threadIdx.x; i < n; i += stride) {
      const int64_t pi = perm[i];
      if (pi < n_own) {
#pragma unroll
         for (int k = 0; k < K; k++) out[i * K + k] = src.p[k] ? src.p[k][pi] : 0.0;
      } else {
         const double *h = recv + (pi - n_own) * K;
#pragma unroll
         for (int k = 0; k < K; k++) out[i * K + k] = src.p[k] ? h[k] : 0.0;
      }
   }
}

// scatter_split_kernel that keeps the own rows only (the correction on the overlap rows belongs to their owners)
template <int K>
__global__ __launch_bounds__ (BT_THREADS)
void scatter_split_own_kernel (const int *__restrict__ perm, const double *__restrict__ in, double *__restrict__ z, BatchOutPtrs dst, int64_t n_own, int64_t n)
{
   const int64_t stride = (int64_t) gridDim.x * BT_THREADS;
   for (int64_t i = (int64_t) blockIdx.x * BT_THREADS + threadIdx.x; i < n; i += stride) {
      const int64_t pi = perm[i];
      if (pi >= n_own) continue;
#pragma unroll
      for (int k = 0; k < K; k++) {
         const double v = in[i * K + k];
         z[pi * K + k] = v;
         if (dst.p[k]) dst.p[k][pi] = v;
      }
   }
}

// one wave per output row, the K columns one after the other (each summed like dense_matvec_kernel sums its one)
template <int K>
__global__ __launch_bounds__ (BT_THREADS)
void dense_matvec_batch_kernel (const double *__restrict__ M, const double *__restrict__ x, double *__restrict__ y, int n)
{
   const int row = (int) ((blockIdx.x * BT_THREADS + threadIdx.x) / NKP_WAVE);
   const int lane = threadIdx.x & (NKP_WAVE - 1);
   if (row >= n) return;
   const double *m = M + (int64_t) row * n;
   double acc[K];
#pragma unroll
   for (int k = 0; k < K; k++) acc[k] = 0.0;
   for (int c = lane; c < n; c += NKP_WAVE) {
      const double mv = m[c];
#pragma unroll
      for (int k = 0; k < K; k++) acc[k] += mv * x[(int64_t) c * K + k];
   }
#pragma unroll
   for (int k = 0; k < K; k++) {
      double v = acc[k];
      for (int off = NKP_WAVE / 2; off > 0; off >>= 1) v += __shfl_down (v, off);
      if (lane == 0) y[(int64_t) row * K + k] = v;
   }
}

void launch_restrict_sum_batch (int K, const int *rptr, const int *ridx, const double *fine, double *coarse, int64_t nc, hipStream_t st)
{
   if (nc > 0) with_k (K, [&] (auto k) { hipLaunchKernelGGL (restrict_sum_batch_kernel<decltype (k)::value>, dim3 (bt_grid (nc * K)), dim3 (BT_THREADS), 0, st, rptr, ridx, fine, coarse, nc); });
}
void launch_prolong_add_batch (int K, const int *cmap, const double *coarse, double *fine, int64_t nf, double omega, hipStream_t st)
{
   if (nf > 0) with_k (K, [&] (auto k) { hipLaunchKernelGGL (prolong_add_batch_kernel<decltype (k)::value>, dim3 (bt_grid (nf * K)), dim3 (BT_THREADS), 0, st, cmap, coarse, fine, nf, omega); });
}
void launch_gather_batch (int K, const int *perm, const double *in, double *out, int64_t n, hipStream_t st)
{
   if (n > 0) with_k (K, [&] (auto k) { hipLaunchKernelGGL (gather_batch_kernel<decltype (k)::value>, dim3 (bt_grid (n * K)), dim3 (BT_THREADS), 0, st, perm, in, out, n); });
}
void launch_gather_interleave (int K, const int *perm, const double *const *src, double *out, int64_t n, hipStream_t st, const double *scale)
{
   BatchPtrs P;
   for (int k = 0; k < NKP_BATCH_MAX; k++) P.p[k] = k < K ? src[k] : nullptr;
   if (n <= 0) return;
   if (scale) with_k (K, [&] (auto k) { hipLaunchKernelGGL (gather_interleave_scaled_kernel<decltype (k)::value>, dim3 (bt_grid (n)), dim3 (BT_THREADS), 0, st, perm, P, scale, out, n); });
   else with_k (K, [&] (auto k) { hipLaunchKernelGGL (gather_interleave_kernel<decltype (k)::value>, dim3 (bt_grid (n)), dim3 (BT_THREADS), 0, st, perm, P, out, n); });
}
void launch_add_split (int K, const double *p, double *z, double *const *dst, int64_t n, hipStream_t st)
{
   BatchOutPtrs P;
   for (int k = 0; k < NKP_BATCH_MAX; k++) P.p[k] = k < K ? dst[k] : nullptr;
   if (n > 0) with_k (K, [&] (auto k) { hipLaunchKernelGGL (add_split_kernel<decltype (k)::value>, dim3 (bt_grid (n)), dim3 (BT_THREADS), 0, st, p, z, P, n); });
}
void launch_scatter_split (int K, const int *perm, const double *in, double *z, double *const *dst, int64_t n, hipStream_t st)
{
   BatchOutPtrs P;
   for (int k = 0; k < NKP_BATCH_MAX; k++) P.p[k] = k < K ? dst[k] : nullptr;
   if (n > 0) with_k (K, [&] (auto k) { hipLaunchKernelGGL (scatter_split_kernel<decltype (k)::value>, dim3 (bt_grid (n)), dim3 (BT_THREADS), 0, st, perm, in, z, P, n); });
}
void launch_pack_rows_split (int K, const int *idx, const double *const *src, double *out, int64_t nrows, hipStream_t st)
{
   BatchPtrs P;
   for (int k = 0; k < NKP_BATCH_MAX; k++) P.p[k] = k < K ? src[k] : nullptr;
   if (nrows > 0) with_k (K, [&] (auto k) { hipLaunchKernelGGL (pack_rows_split_kernel<decltype (k)::value>, dim3 (bt_grid (nrows)), dim3 (BT_THREADS), 0, st, idx, P, out, nrows); });
}
void launch_gather_interleave_ext (int K, const int *perm, const double *const *src, const double *halo, const int *sel, int64_t n_own, double *out, int64_t n,
                                   hipStream_t st)
{
   BatchPtrs P;
   for (int k = 0; k < NKP_BATCH_MAX; k++) P.p[k] = k < K ? src[k] : nullptr;
   if (n > 0) with_k (K, [&] (auto k) { hipLaunchKernelGGL (gather_interleave_ext_kernel<decltype (k)::value>, dim3 (bt_grid (n)), dim3 (BT_THREADS), 0, st, perm, P, halo, sel, n_own, out, n); });
}
void launch_gather_interleave_ext_block (int K, const int *perm, const double *const *src, const double *recv, int64_t n_own, double *out, int64_t n, hipStream_t st)
{
   BatchPtrs P;
   for (int k = 0; k < NKP_BATCH_MAX; k++) P.p[k] = k < K ? src[k] : nullptr;
   if (n > 0) with_k (K, [&] (auto k) { hipLaunchKernelGGL (gather_interleave_ext_block_kernel<decltype (k)::value>, dim3 (bt_grid (n)), dim3 (BT_THREADS), 0, st, perm, P, recv, n_own, out, n); });
}
void launch_scatter_split_own (int K, const int *perm, const double *in, double *z, double *const *dst, int64_t n_own, int64_t n, hipStream_t st)
{
   BatchOutPtrs P;
   for (int k = 0; k < NKP_BATCH_MAX; k++) P.p[k] = k < K ? dst[k] : nullptr;
   if (n > 0) with_k (K, [&] (auto k) { hipLaunchKernelGGL (scatter_split_own_kernel<decltype (k)::value>, dim3 (bt_grid (n)), dim3 (BT_THREADS), 0, st, perm, in, z, P, n_own, n); });
}
void launch_dense_matvec_batch (int K, const double *Minv, const double *x, double *y, int n, hipStream_t st)
{
   if (n > 0) with_k (K, [&] (auto k) { hipLaunchKernelGGL (dense_matvec_batch_kernel<decltype (k)::value>, dim3 ((n + BT_WAVES - 1) / BT_WAVES), dim3 (BT_THREADS), 0, st, Minv, x, y, n); });
}

// ---------------------------------------------------------------- water columns, one per wave, K columns of right-hand sides
__device__ __forceinline__ double bt_readlane_f64 (double v, int lane)
{
   int lo = __double2loint (v), hi = __double2hiint (v);
   lo = __builtin_amdgcn_readlane (lo, lane);
   hi = __builtin_amdgcn_readlane (hi, lane);
   return __hiloint2double (hi, lo);
}

// band substitution of colblock_apply_kernel on K right-hand sides held in y[s][k] (lane = level, s = second register set of
// columns longer than a wave); identical operations per column, the K chains interleave in the pipeline
template <int P, int RPL, int K>
__device__ __forceinline__ void wave_band_solve (int len, int lane, double (&y)[RPL][K], const double (&invd)[RPL], const double (&L)[RPL][P], const double (&U)[RPL][P])
{
   for (int k = 0; k < len - 1; k++) {
      const int ks = k >> 6, kl = k & (NKP_WAVE - 1);
      double yk[K];
#pragma unroll
      for (int q = 0; q < K; q++) yk[q] = 0.0;
#pragma unroll
      for (int s = 0; s < RPL; s++)
         if (ks == s) {
#pragma unroll
            for (int q = 0; q < K; q++) yk[q] = bt_readlane_f64 (y[s][q], kl);
         }
#pragma unroll
      for (int s = 0; s < RPL; s++) {
         const int rel = s * NKP_WAVE + lane - k;
#pragma unroll
         for (int d = 1; d <= P; d++)
            if (rel == d) {
#pragma unroll
               for (int q = 0; q < K; q++) y[s][q] -= L[s][d - 1] * yk[q];
            }
      }
   }
   for (int k = len - 1; k >= 0; k--) {
      const int ks = k >> 6, kl = k & (NKP_WAVE - 1);
      double xk[K];
#pragma unroll
      for (int q = 0; q < K; q++) xk[q] = 0.0;
#pragma unroll
      for (int s = 0; s < RPL; s++)
         if (ks == s) {
#pragma unroll
            for (int q = 0; q < K; q++) {
               if (lane == kl) y[s][q] *= invd[s];
               xk[q] = bt_readlane_f64 (y[s][q], kl);
            }
         }
#pragma unroll
      for (int s = 0; s < RPL; s++) {
         const int rel = k - (s * NKP_WAVE + lane);
#pragma unroll
         for (int d = 1; d <= P; d++)
            if (rel == d) {
#pragma unroll
               for (int q = 0; q < K; q++) y[s][q] -= U[s][d - 1] * xk[q];
            }
      }
   }
}

template <int P, int RPL, bool R32>
__device__ __forceinline__ void wave_load_factors (int64_t n, int64_t r0, int len, int lane, const double *__restrict__ fac, double (&invd)[RPL], double (&L)[RPL][P], double (&U)[RPL][P])
{
#pragma unroll
   for (int s = 0; s < RPL; s++) {
      const int li = s * NKP_WAVE + lane;
      invd[s] = 0.0;
#pragma unroll
      for (int q = 0; q < P; q++) { L[s][q] = 0.0; U[s][q] = 0.0; }
      if (li < len) {
         const int64_t r = r0 + li;
         invd[s] = fac[(int64_t) P * n + r];
         if (R32) invd[s] = (double) (float) invd[s];
#pragma unroll
         for (int q = 1; q <= P; q++) {
            L[s][q - 1] = fac[(int64_t) (P - q) * n + r];
            U[s][q - 1] = fac[(int64_t) (P + q) * n + r];
            if (R32) { L[s][q - 1] = (double) (float) L[s][q - 1]; U[s][q - 1] = (double) (float) U[s][q - 1]; }
         }
      }
   }
}

// z (+)= M^-1 rhs on the blocks [b_first, b_end), K columns
template <int P, int RPL, bool R32, int K>
__global__ __launch_bounds__ (BT_THREADS)
void colblock_apply_wave_batch_kernel (const int *__restrict__ blk_start, int b_first, int b_end, int64_t n, const double *__restrict__ fac,
                                       const double *__restrict__ rhs, double *__restrict__ z, int accumulate)
{
   const int blk = __builtin_amdgcn_readfirstlane ((int) ((blockIdx.x * BT_THREADS + threadIdx.x) / NKP_WAVE)) + b_first;
   if (blk >= b_end) return;
   const int lane = threadIdx.x & (NKP_WAVE - 1);
   const int r0 = blk_start[blk], len = blk_start[blk + 1] - r0;
   double y[RPL][K], invd[RPL], L[RPL][P], U[RPL][P];
   wave_load_factors<P, RPL, R32> (n, r0, len, lane, fac, invd, L, U);
#pragma unroll
   for (int s = 0; s < RPL; s++) {
      const int li = s * NKP_WAVE + lane;
#pragma unroll
      for (int q = 0; q < K; q++) y[s][q] = li < len ? rhs[((int64_t) r0 + li) * K + q] : 0.0;
   }
   wave_band_solve<P, RPL, K> (len, lane, y, invd, L, U);
#pragma unroll
   for (int s = 0; s < RPL; s++) {
      const int li = s * NKP_WAVE + lane;
      if (li < len) {
#pragma unroll
         for (int q = 0; q < K; q++) {
            if (accumulate) z[((int64_t) r0 + li) * K + q] += y[s][q];
            else z[((int64_t) r0 + li) * K + q] = y[s][q];
         }
      }
   }
}

// gs_wave_kernel (colblock.hip) on K columns: residual of the column's rows, band solve, xout = x + z in one launch
#define BGS_UNROLL (K >= 8 ? 8 : 16)          // entries (x K values each) requested together
#define BGS_CAP 1536
template <int P, int RPL, class VT, bool R32, int K>
__global__ __launch_bounds__ (BT_THREADS)
void gs_wave_batch_kernel (const int *__restrict__ rowptr, const int *__restrict__ colind, const VT *__restrict__ val, const int *__restrict__ blk_start,
                           int b_first, int b_end, int64_t n, const double *__restrict__ fac, const double *__restrict__ xa, const double *__restrict__ xb,
                           int split, const double *__restrict__ b, double *__restrict__ xout, const int4 *__restrict__ desc)
{
   // the column's entries through LDS with coalesced loads, like gs_wave_kernel (colblock.hip)
   extern __shared__ unsigned char bgs_lds[];
   const int wv = threadIdx.x / NKP_WAVE;
   int *sc = reinterpret_cast<int *> (bgs_lds) + wv * BGS_CAP;
   VT *sv = reinterpret_cast<VT *> (bgs_lds + (size_t) BT_WAVES * BGS_CAP * sizeof (int)) + wv * BGS_CAP;
   const int blk = __builtin_amdgcn_readfirstlane ((int) ((blockIdx.x * BT_THREADS + threadIdx.x) / NKP_WAVE)) + b_first;
   const bool act = blk < b_end;
   const int lane = threadIdx.x & (NKP_WAVE - 1);
   int4 d4 = make_int4 (0, 0, 0, 0);
   if (act) {
      if (desc) d4 = desc[blk];
      else {
         d4.x = blk_start[blk];
         d4.y = blk_start[blk + 1] - d4.x;
         d4.z = d4.y > 0 ? rowptr[d4.x] : 0;
         d4.w = d4.y > 0 ? rowptr[d4.x + d4.y] - d4.z : 0;
      }
   }
   const int r0 = d4.x, len = d4.y;
   double y[RPL][K], xold[RPL][K], invd[RPL], L[RPL][P], U[RPL][P];
   int e0[RPL], rl[RPL];
   const int e_begin = d4.z, e_total = d4.w;
   const bool staged = e_total <= BGS_CAP;
   if (staged) {
      for (int k0 = 0; k0 < e_total; k0 += NKP_WAVE * 8) {
         int tc[8];
         VT tv[8];
#pragma unroll
         for (int u = 0; u < 8; u++) {
            const int k = k0 + u * NKP_WAVE + lane;
            tc[u] = k < e_total ? colind[e_begin + k] : 0;
            tv[u] = k < e_total ? val[e_begin + k] : (VT) 0;
         }
#pragma unroll
         for (int u = 0; u < 8; u++) {
            const int k = k0 + u * NKP_WAVE + lane;
            if (k < e_total) { sc[k] = tc[u]; sv[k] = tv[u]; }
         }
      }
   }
   wave_load_factors<P, RPL, R32> (n, r0, len, lane, fac, invd, L, U);
#pragma unroll
   for (int s = 0; s < RPL; s++) {
      const int li = s * NKP_WAVE + lane;
      e0[s] = 0; rl[s] = 0;
#pragma unroll
      for (int q = 0; q < K; q++) { y[s][q] = 0.0; xold[s][q] = 0.0; }
      if (li < len) {
         const int64_t r = r0 + li;
         e0[s] = rowptr[r];
         rl[s] = rowptr[r + 1] - e0[s];
         const double *xo = (r < split) ? xa : xb;
#pragma unroll
         for (int q = 0; q < K; q++) { y[s][q] = b[r * K + q]; xold[s][q] = xo[r * K + q]; }
      }
   }
   __syncthreads ();
#pragma unroll
   for (int s = 0; s < RPL; s++) {
      double acc[K];
#pragma unroll
      for (int q = 0; q < K; q++) acc[q] = 0.0;
      for (int k0 = 0; __any (k0 < rl[s]); k0 += BGS_UNROLL) {
         int cc[BGS_UNROLL];
         VT vv[BGS_UNROLL];
         if (staged) {
            const int off = e0[s] - e_begin + k0;
#pragma unroll
            for (int u = 0; u < BGS_UNROLL; u++) {
               const bool ok = k0 + u < rl[s];
               cc[u] = ok ? sc[off + u] : 0;
               vv[u] = ok ? sv[off + u] : (VT) 0;
            }
         } else {
#pragma unroll
            for (int u = 0; u < BGS_UNROLL; u++) {
               const bool ok = k0 + u < rl[s];
               cc[u] = ok ? colind[e0[s] + k0 + u] : 0;
               vv[u] = ok ? val[e0[s] + k0 + u] : (VT) 0;
            }
         }
         double2 xg[K / 2][BGS_UNROLL];
#pragma unroll
         for (int u = 0; u < BGS_UNROLL; u++) {
            const double *xs = ((cc[u] < split) ? xa : xb) + (int64_t) cc[u] * K;
#pragma unroll
            for (int h = 0; h < K / 2; h++) xg[h][u] = *reinterpret_cast<const double2 *> (xs + 2 * h);
         }
#pragma unroll
         for (int u = 0; u < BGS_UNROLL; u++)
            if (k0 + u < rl[s]) {
#pragma unroll
               for (int h = 0; h < K / 2; h++) { acc[2 * h] += (double) vv[u] * xg[h][u].x; acc[2 * h + 1] += (double) vv[u] * xg[h][u].y; }
            }
      }
      if (s * NKP_WAVE + lane < len) {
#pragma unroll
         for (int q = 0; q < K; q++) y[s][q] -= acc[q];
      }
   }
   wave_band_solve<P, RPL, K> (len, lane, y, invd, L, U);
#pragma unroll
   for (int s = 0; s < RPL; s++) {
      const int li = s * NKP_WAVE + lane;
      if (li < len) {
#pragma unroll
         for (int q = 0; q < K; q++) xout[((int64_t) r0 + li) * K + q] = xold[s][q] + y[s][q];
      }
   }
}

static inline dim3 bt_wave_grid (int nblk) { return dim3 ((nblk + BT_WAVES - 1) / BT_WAVES); }

void launch_colblock_apply_wave_batch (int K, const ColBlocksDev &B, int b0, int b1, const double *r, double *z, int accumulate, int r32, hipStream_t st)
{
   if (b1 <= b0) return;
   with_band_rows (B, [&] (auto p, auto rpl) {
      with_bool (r32, [&] (auto r32_) {
         with_k (K, [&] (auto k) {
            hipLaunchKernelGGL ((colblock_apply_wave_batch_kernel<decltype (p)::value, decltype (rpl)::value, decltype (r32_)::value, decltype (k)::value>),
                                bt_wave_grid (b1 - b0), dim3 (BT_THREADS), 0, st, B.blk_start, b0, b1, B.n, B.fac, r, z, accumulate);
         });
      });
   });
}

void launch_gs_wave_batch (int K, const CsrDev &L, const ColBlocksDev &B, int b0, int b1, const double *xa, const double *xb, int split, const double *b, double *xout,
                           int r32, hipStream_t st)
{
   if (b1 <= b0) return;
   with_band_rows (B, [&] (auto p, auto rpl) {
      with_storage (L.valf, L.val, [&] (auto val) {
         with_bool (r32, [&] (auto r32_) {
            with_k (K, [&] (auto k) {
               const auto kernel = gs_wave_batch_kernel<decltype (p)::value, decltype (rpl)::value, elem_t<decltype (val)>, decltype (r32_)::value, decltype (k)::value>;
               const size_t lds = (size_t) BT_WAVES * BGS_CAP * (sizeof (int) + sizeof (*val));
               // more than 48 KB of dynamic LDS needs an opt-in: once per instantiation (this lambda's body is one), before its first launch
               static bool opted = false;
               if (lds > 48 * 1024 && !opted) { (void) hipFuncSetAttribute ((const void *) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds); opted = true; }
               hipLaunchKernelGGL (kernel, bt_wave_grid (b1 - b0), dim3 (BT_THREADS), lds, st,
                                   L.rowptr, L.colind, val, B.blk_start, b0, b1, B.n, B.fac, xa, xb, split, b, xout, reinterpret_cast<const int4 *> (B.wave_desc));
            });
         });
      });
   });
}
