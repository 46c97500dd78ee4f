// Residual, norms and componentwise backward error of K given solutions in ONE pass over A (nkp_residual_batch):
//    t_c[i] = sum over the stored entries e of row i, in stored order, of val[e] * x_c[colind[e]]            (the bits of SpMV mode 0)
//    d_c[i] = the same sum of fabs (val[e] * x_c[colind[e]])                                                  (the bits of SpMV mode 2 before |b|)
//    r_c[i] = b_c[i] - t_c[i]      den_c[i] = d_c[i] + fabs (b_c[i])      q_c[i] = fabs (r_c[i]) / den_c[i] by the rule of berr_kernel (blas1.hip)
// and per column  sum_i r_c[i]^2,  sum_i b_c[i]^2,  max_or_nan_i q_c[i].  Every product and every sum is rounded on its own (no
// contraction); both sums start at +0.0.  A row that sits alone in its row block because it exceeds the LDS budget is summed in the
// SpMV's tree for such rows, t and d alike: lane-strided partial sums, the wave shuffle tree, then the waves in order.
//
// The scheme of values_product_kernel (valprod.hip): a workgroup per CSR-stream row block of A, numbered XCD-contiguously, stages the
// block's (value, column) stream in LDS with coalesced loads; every row's lane walks its own segment, gathers the K-wide rows of x
// and keeps its 2 K sums in registers.  K = 1 reads x in place; K >= 2 reads a K-interleaved copy (X[i * K + c]).  The epilogue reads
// b_c[i], writes r_c[i] straight into the caller's column-major R when asked (consecutive lanes write consecutive rows of one column;
// a lane reads its b before it writes its r, so R may be B), and the workgroup reduces r^2, b^2 (one rounded product each) and q in
// its fixed tree -- the wave shuffle tree, then the waves in order; a lane without a row holds +0.0 -- into partial[row block][3][K].
// residual_finish_kernel then reduces the partials per column in a fixed order: lane-strided over the row blocks, then the shuffle
// tree.  No atomics, no waiting between workgroups; the order of every sum depends on the row blocks of A alone, not on K, nk, the
// grid or the column's position.  Columns c >= nk of a width-K buffer take no part.  A row block without entries still gives r = b.
// Compulsory bytes: 12 nnz + 4 (n + 1) + 16 K n, plus 8 K n when R is written.
#include "nkp_dev.h"

#define RB_THREADS 256
#define RB_WAVES (RB_THREADS / NKP_WAVE)

// max_or_nan and the quotient of berr_kernel (blas1.hip): a NaN on either side wins; a / d keeps a NaN of either and makes one of
// Inf / Inf; d == 0 (an empty row with b_i = 0) follows the old rule
__device__ __forceinline__ double rb_max_or_nan (double q, double m) { return (q > m || q != q) ? q : m; }
__device__ __forceinline__ double rb_quotient (double r, double d)
{
   const double a = fabs (r);
   return (d > 0.0 || d != d) ? a / d : (a != a ? a : a > 0.0 ? 1.0e300 : 0.0);
}

template <int K>
__global__ __launch_bounds__ (RB_THREADS)
void residual_batch_kernel (const int *__restrict__ rowblk, int nrowblk, int per_xcd, const int *__restrict__ rowptr, const int *__restrict__ colind,
                            const double *__restrict__ val, const double *__restrict__ x, int nk, const double *B, int64_t ldb, double *R, int64_t ldr,
                            double *__restrict__ partial)
{
   __shared__ double sv[NKP_SPMV_LDS_NNZ];
   __shared__ int sc[NKP_SPMV_LDS_NNZ];
   __shared__ double wred[3][K][RB_WAVES];
   constexpr int SLOTS = NKP_SPMV_LDS_NNZ / RB_THREADS, GU = K == 1 ? 8 : 16 / K;
   const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
   const int lb = xcd * per_xcd + idx;
   if (idx >= per_xcd || lb >= nrowblk) return;
   const int tid = threadIdx.x, lane = tid & (NKP_WAVE - 1), wave = tid / NKP_WAVE;
   const int r0 = rowblk[lb], r1 = rowblk[lb + 1];
   const int e0 = rowptr[r0], e1 = rowptr[r1];
   const int cnt = e1 - e0;
   double *part = partial + (int64_t) lb * (3 * K);
   double t[K], d[K];
#pragma unroll
   for (int c = 0; c < K; c++) t[c] = d[c] = 0.0;
   if (cnt > NKP_SPMV_LDS_NNZ) {
      // a single long row, all K columns in one walk: per column the strided sums and the reduction of the SpMV kernels
      for (int e = e0 + tid; e < e1; e += RB_THREADS) {
         const double v = val[e];
         const double *xr = x + (int64_t) colind[e] * K;
         double xv[K];
         if constexpr (K == 1) xv[0] = xr[0];
         else {
#pragma unroll
            for (int g = 0; g < K / 2; g++) {
               const double2 q = *reinterpret_cast<const double2 *> (xr + 2 * g);
               xv[2 * g] = q.x; xv[2 * g + 1] = q.y;
            }
         }
#pragma unroll
         for (int c = 0; c < K; c++) {
            const double p = __dmul_rn (v, xv[c]);
            t[c] = __dadd_rn (t[c], p);
            d[c] = __dadd_rn (d[c], fabs (p));
         }
      }
#pragma unroll
      for (int c = 0; c < K; c++) {
         for (int off = NKP_WAVE / 2; off > 0; off >>= 1) {
            t[c] = __dadd_rn (t[c], __shfl_down (t[c], off));
            d[c] = __dadd_rn (d[c], __shfl_down (d[c], off));
         }
         if (lane == 0) { wred[0][c][wave] = t[c]; wred[1][c][wave] = d[c]; }
      }
      __syncthreads ();
      if (tid < K && tid < nk) {
         double ts = 0.0, ds = 0.0;
         for (int w = 0; w < RB_WAVES; w++) { ts = __dadd_rn (ts, wred[0][tid][w]); ds = __dadd_rn (ds, wred[1][tid][w]); }
         const double b = B[(int64_t) tid * ldb + r0];
         const double r = __dsub_rn (b, ts);
         const double q = rb_quotient (r, __dadd_rn (ds, fabs (b)));
         if (R) R[(int64_t) tid * ldr + r0] = r;
         // the block's tree over one row and 255 lanes of +0.0
         part[tid] = __dmul_rn (r, r);
         part[K + tid] = __dmul_rn (b, b);
         part[2 * K + tid] = rb_max_or_nan (q, 0.0);
      }
      return;
   }
   const int r = r0 + tid;
   const bool live = r < r1;
   int s0 = 0, s1 = 0;
   if (live) { s0 = rowptr[r] - e0; s1 = rowptr[r + 1] - e0; }
   {
      double v[SLOTS];
      int c[SLOTS];
#pragma unroll
      for (int u = 0; u < SLOTS; u++) {
         const int k = tid + u * RB_THREADS;
         v[u] = k < cnt ? val[e0 + k] : 0.0;
         c[u] = k < cnt ? colind[e0 + k] : 0;
      }
#pragma unroll
      for (int u = 0; u < SLOTS; u++) {
         const int k = tid + u * RB_THREADS;
         if (k < cnt) { sv[k] = v[u]; sc[k] = c[u]; }
      }
   }
   // b of this lane's row, requested before the walk
   double b[K];
#pragma unroll
   for (int c = 0; c < K; c++) b[c] = (live && c < nk) ? B[(int64_t) c * ldb + r] : 0.0;
   __syncthreads ();
   for (int k = s0; k < s1; k += GU) {
      double vv[GU], xv[GU][K];
#pragma unroll
      for (int u = 0; u < GU; u++) {
         const int kk = k + u < s1 ? k + u : s1 - 1;
         vv[u] = sv[kk];
         const double *xr = x + (int64_t) sc[kk] * K;
         if constexpr (K == 1) xv[u][0] = xr[0];
         else {
#pragma unroll
            for (int g = 0; g < K / 2; g++) {
               const double2 q = *reinterpret_cast<const double2 *> (xr + 2 * g);
               xv[u][2 * g] = q.x; xv[u][2 * g + 1] = q.y;
            }
         }
      }
#pragma unroll
      for (int u = 0; u < GU; u++)
         if (k + u < s1) {
#pragma unroll
            for (int c = 0; c < K; c++) {
               const double p = __dmul_rn (vv[u], xv[u][c]);
               t[c] = __dadd_rn (t[c], p);
               d[c] = __dadd_rn (d[c], fabs (p));
            }
         }
   }
   // epilogue of the row, then the block's tree; a lane without a row holds +0.0 in all three
#pragma unroll
   for (int c = 0; c < K; c++)
      if (c < nk) {
         double rr = 0.0, bb = 0.0, q = 0.0;
         if (live) {
            const double res = __dsub_rn (b[c], t[c]);
            q = rb_max_or_nan (rb_quotient (res, __dadd_rn (d[c], fabs (b[c]))), 0.0);
            if (R) R[(int64_t) c * ldr + r] = res;
            rr = __dmul_rn (res, res);
            bb = __dmul_rn (b[c], b[c]);
         }
         for (int off = NKP_WAVE / 2; off > 0; off >>= 1) {
            rr = __dadd_rn (rr, __shfl_down (rr, off));
            bb = __dadd_rn (bb, __shfl_down (bb, off));
            q = rb_max_or_nan (__shfl_down (q, off), q);
         }
         if (lane == 0) { wred[0][c][wave] = rr; wred[1][c][wave] = bb; wred[2][c][wave] = q; }
      }
   __syncthreads ();
   if (tid < 3 * K) {
      const int j = tid / K, c = tid % K;
      if (c < nk) {
         double v = wred[j][c][0];
         for (int w = 1; w < RB_WAVES; w++) v = j == 2 ? rb_max_or_nan (wred[j][c][w], v) : __dadd_rn (v, wred[j][c][w]);
         part[j * K + c] = v;
      }
   }
}

// out[j * K + c], j = 0: sum r^2, 1: sum b^2, 2: max_or_nan q of column c over the row blocks: one wave per (j, c), lane-strided over
// the row blocks in ascending order from +0.0, then the shuffle tree.  Columns c >= nk get +0.0 (the message of a row-distributed
// solver is 3 K doubles whatever nk is)
__global__ __launch_bounds__ (NKP_WAVE)
void residual_finish_kernel (const double *__restrict__ partial, int nrowblk, int K, int nk, double *__restrict__ out)
{
   constexpr int U = 32;      // loads in flight per lane: the wave is alone with the memory latency; the order of the sum is unchanged
   const int j = blockIdx.x / K, c = blockIdx.x % K;
   double v = 0.0;
   if (c < nk)
      for (int b0 = threadIdx.x; b0 < nrowblk; b0 += NKP_WAVE * U) {
         double p[U];
#pragma unroll
         for (int u = 0; u < U; u++) {
            const int b = b0 + u * NKP_WAVE;
            p[u] = b < nrowblk ? partial[(int64_t) b * (3 * K) + j * K + c] : 0.0;
         }
#pragma unroll
         for (int u = 0; u < U; u++)
            if (b0 + u * NKP_WAVE < nrowblk) v = j == 2 ? rb_max_or_nan (p[u], v) : __dadd_rn (v, p[u]);
      }
   for (int off = NKP_WAVE / 2; off > 0; off >>= 1) {
      const double o = __shfl_down (v, off);
      v = j == 2 ? rb_max_or_nan (o, v) : __dadd_rn (v, o);
   }
   if (threadIdx.x == 0) out[j * K + c] = v;
}

// r_c = b_c - A x_c for c < nk into R (column-major, vector c at c * ldr; NULL: not stored), and out[0 .. K) = sum r_c^2,
// out[K .. 2 K) = sum b_c^2, out[2 K .. 3 K) = max_or_nan of the rows' backward-error quotients.  K in {1, 2, 4, 8} is the interleave
// width of x (1: a plain vector), nk <= K; x is indexed by A's columns (row-distributed: [own | halo] like the SpMV's input); B is
// column-major, vector c at c * ldb.  partial: 3 K doubles per row block of A.  R may be B (with ldr == ldb), never x.
void launch_residual_batch (int K, int nk, const CsrDev &A, const double *x, const double *B, int64_t ldb, double *R, int64_t ldr, double *partial, double *out,
                            hipStream_t st)
{
   if (nk > K) nk = K;
   if (A.nrowblk > 0) {
      const int per_xcd = (A.nrowblk + 7) / 8;
      with_int<1, 2, 4, 8> (K, [&] (auto k) {
         hipLaunchKernelGGL ((residual_batch_kernel<decltype (k)::value>), dim3 (per_xcd * 8), dim3 (RB_THREADS), 0, st, A.rowblk, A.nrowblk, per_xcd, A.rowptr, A.colind,
                             A.val, x, nk, B, ldb, R, ldr, partial);
      });
   }
   hipLaunchKernelGGL (residual_finish_kernel, dim3 (3 * K), dim3 (NKP_WAVE), 0, st, partial, A.nrowblk > 0 ? A.nrowblk : 0, K, nk, out);
}
