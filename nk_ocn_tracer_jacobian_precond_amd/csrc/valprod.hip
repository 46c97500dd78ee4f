// A product with caller-supplied values on the solver's CSR pattern, K vectors wide (nkp_values_product):
//    t_c[i] = sum over the stored entries e of row i, in stored order, of val[e] * x_c[colind[e]]      y_c[i] = (y_c[i] +) alpha * t_c[i]
// every product and every sum rounded on its own (no contraction).  t_c has the bits the SpMV kernels (spmv.hip, batch.hip) give
// for x_c on a matrix that stores val: the sum starts at +0.0 and takes the products in stored order; a row that sits alone in its
// row block because it exceeds the LDS budget is summed in their tree -- lane-strided partial sums, the wave shuffle tree, then
// the waves in order.
//
// One pass over the pattern for any K: the scheme of csr_spmv_batch_rows_kernel (batch.hip).  A workgroup owns one CSR-stream
// row block (at most 256 rows and 2048 entries), stages the block's (value, column) stream in LDS with coalesced loads, then
// every row's lane walks its own segment, gathers the K-wide rows of x (GU entries in flight) and keeps its K sums in registers.
// The epilogue writes (y +) alpha * t straight into the caller's column-major y (vector c at c * ldy; consecutive lanes write
// consecutive rows of one vector): no temporary product, no scale-and-add pass, no de-interleave pass.
// K = 1 reads x in place; K >= 2 reads a K-interleaved copy (X[i * K + c]), a row of which comes with K / 2 16-byte loads.
// Columns c >= nk of a width-K buffer take no part: nothing of them is summed and y has no such column, so a width serves fewer
// vectors (3 in 4, 5 .. 7 in 8) with unchanged bits.  No atomics, no waiting between workgroups; a row block without entries
// still writes alpha * (+0.0) to its rows.
//
// The same kernel text serves nkp_values_product_trans (GATHER): the pattern is then the transposed index the solver keeps
// (rowptrT, colindT, its row blocks) and the value of entry p is val[src[p]], the caller's values staying in A's order.  The
// staging step issues all its src loads (coalesced), then the val gathers that depend on them, then writes LDS; the long-row
// walk gathers the same way.  Without GATHER src is not read and the instantiations are what they were.
//
// And nkp_values_product_trans_dist (GATHER and RECV): the pattern is the row block of A^T a rank assembled from its own entries and
// the products its peers shipped.  src[p] >= 0 is an own entry as above; src[p] < 0 is a received product, which sits in x at the
// row colind[p] (behind the own rows) and takes the value 1.0 -- 1.0 * p is p exactly, signed zeros and non-finite values included,
// so it enters the sum through the same rounded multiply and add as an own product.  Without RECV the sign of src is not looked at.
#include "nkp_dev.h"

#define VP_THREADS 256
#define VP_WAVES (VP_THREADS / NKP_WAVE)

template <int K, bool GATHER, bool RECV = false>
__global__ __launch_bounds__ (VP_THREADS)
void values_product_kernel (const int *__restrict__ rowblk, int nrowblk, int per_xcd, const int *__restrict__ rowptr, const int *__restrict__ colind,
                            const int *__restrict__ src, const double *__restrict__ val, const double *__restrict__ x, int nk, double alpha, int accumulate,
                            double *y, int64_t ldy)
{
   __shared__ double sv[NKP_SPMV_LDS_NNZ];
   __shared__ int sc[NKP_SPMV_LDS_NNZ];
   __shared__ double wsum[K][VP_WAVES];
   constexpr int SLOTS = NKP_SPMV_LDS_NNZ / VP_THREADS, GU = K == 1 ? 8 : 16 / K;
   const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
   const int lb = xcd * per_xcd + idx;
   if (idx >= per_xcd || lb >= nrowblk) return;
   const int tid = threadIdx.x;
   const int r0 = rowblk[lb], r1 = rowblk[lb + 1];
   const int e0 = rowptr[r0], e1 = rowptr[r1];
   const int cnt = e1 - e0;
   double acc[K];
#pragma unroll
   for (int c = 0; c < K; c++) acc[c] = 0.0;
   if (cnt > NKP_SPMV_LDS_NNZ) {
      // a single long row, all K columns in one walk: per column the strided sums and the reduction of the SpMV kernels
      for (int e = e0 + tid; e < e1; e += VP_THREADS) {
         double v;
         if constexpr (RECV) {
            const int o = src[e];
            v = o >= 0 ? val[o] : 1.0;
         } else
            v = val[GATHER ? src[e] : e];
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
         for (int c = 0; c < K; c++) acc[c] = __dadd_rn (acc[c], __dmul_rn (v, xv[c]));
      }
#pragma unroll
      for (int c = 0; c < K; c++) {
         for (int off = NKP_WAVE / 2; off > 0; off >>= 1) acc[c] = __dadd_rn (acc[c], __shfl_down (acc[c], off));
         if ((tid & (NKP_WAVE - 1)) == 0) wsum[c][tid / NKP_WAVE] = acc[c];
      }
      __syncthreads ();
      if (tid < K && tid < nk) {
         double s = 0.0;
         for (int w = 0; w < VP_WAVES; w++) s = __dadd_rn (s, wsum[tid][w]);
         double *yp = y + (int64_t) tid * ldy + r0;
         double v = __dmul_rn (alpha, s);
         if (accumulate) v = __dadd_rn (*yp, v);
         *yp = v;
      }
      return;
   }
   const int r = r0 + tid;
   int s0 = 0, s1 = 0;
   if (r < r1) { s0 = rowptr[r] - e0; s1 = rowptr[r + 1] - e0; }
   {
      double v[SLOTS];
      int c[SLOTS], from[SLOTS];
#pragma unroll
      for (int u = 0; u < SLOTS; u++) {
         const int k = tid + u * VP_THREADS;
         from[u] = e0 + k;
         if constexpr (GATHER) from[u] = k < cnt ? src[e0 + k] : 0;      // RECV: a padded slot reads val[0] like an own entry and stores nothing
      }
#pragma unroll
      for (int u = 0; u < SLOTS; u++) {
         const int k = tid + u * VP_THREADS;
         if constexpr (RECV) v[u] = k < cnt ? (from[u] >= 0 ? val[from[u]] : 1.0) : 0.0;
         else v[u] = k < cnt ? val[from[u]] : 0.0;
         c[u] = k < cnt ? colind[e0 + k] : 0;
      }
#pragma unroll
      for (int u = 0; u < SLOTS; u++) {
         const int k = tid + u * VP_THREADS;
         if (k < cnt) { sv[k] = v[u]; sc[k] = c[u]; }
      }
   }
   // the old y of this lane's row, requested before the walk
   double yo[K];
#pragma unroll
   for (int c = 0; c < K; c++) yo[c] = (accumulate && r < r1 && c < nk) ? y[(int64_t) c * ldy + r] : 0.0;
   __syncthreads ();
   if (r >= r1) return;
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
            for (int c = 0; c < K; c++) acc[c] = __dadd_rn (acc[c], __dmul_rn (vv[u], xv[u][c]));
         }
   }
#pragma unroll
   for (int c = 0; c < K; c++)
      if (c < nk) {
         double v = __dmul_rn (alpha, acc[c]);
         if (accumulate) v = __dadd_rn (yo[c], v);
         y[(int64_t) c * ldy + r] = v;
      }
}

// one launch for both products: a workgroup per row block of A, numbered XCD-contiguously
template <bool GATHER, bool RECV = false>
static void launch_product (int K, int nk, const CsrDev &A, const int *src, const double *val, const double *x, double alpha, int accumulate, double *y, int64_t ldy,
                            hipStream_t st)
{
   if (A.nrowblk <= 0) return;
   const int per_xcd = (A.nrowblk + 7) / 8;
   with_int<1, 2, 4, 8> (K, [&] (auto k) {
      hipLaunchKernelGGL ((values_product_kernel<decltype (k)::value, GATHER, RECV>), dim3 (per_xcd * 8), dim3 (VP_THREADS), 0, st, A.rowblk, A.nrowblk, per_xcd, A.rowptr,
                          A.colind, src, val, x, nk < K ? nk : K, alpha, accumulate, y, ldy);
   });
}

// y_c (+)= alpha * (pattern of A with the values val) x_c for c < nk, y column-major (vector c at c * ldy).  K in {1, 2, 4, 8} is
// the interleave width of x (1: a plain vector), nk <= K.  x is indexed by A's columns (row-distributed: [own | halo] like the
// SpMV's input).  Every row of A is written, also when A has no entries.
void launch_values_product (int K, int nk, const CsrDev &A, const double *val, const double *x, double alpha, int accumulate, double *y, int64_t ldy, hipStream_t st)
{
   launch_product<false> (K, nk, A, nullptr, val, x, alpha, accumulate, y, ldy, st);
}

// The same with the value of entry p of T taken from val[src[p]]: T holds the pattern of A^T (rowptr, colind, rowblk, nrowblk; no
// values), val the caller's values in A's order, x is indexed by A's rows and y by A's columns
void launch_values_product_trans (int K, int nk, const CsrDev &T, const int *src, const double *val, const double *x, double alpha, int accumulate, double *y,
                                  int64_t ldy, hipStream_t st)
{
   launch_product<true> (K, nk, T, src, val, x, alpha, accumulate, y, ldy, st);
}

// The same on the row block of A^T a rank of a row-distributed solver assembled (nkp_values_product_trans_dist): src[p] >= 0 a
// position in val, src[p] < 0 a product a peer shipped, found in x at row T.colind[p] and multiplied by 1.0
void launch_values_product_trans_recv (int K, int nk, const CsrDev &T, const int *src, const double *val, const double *x, double alpha, int accumulate, double *y,
                                       int64_t ldy, hipStream_t st)
{
   launch_product<true, true> (K, nk, T, src, val, x, alpha, accumulate, y, ldy, st);
}
