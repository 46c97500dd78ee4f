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

// ---------------------------------------------------------------- per-system vectors <-> the interleaved layout
// the K per-system vectors of a launch; a system without one (NULL) reads as zeros / is not written
template <class T>
struct BatchVecs {
   T *p[NKP_BATCH_MAX] = {};
   BatchVecs () = default;
   BatchVecs (int K, T *const *v) { for (int k = 0; k < K; k++) p[k] = v[k]; }
};
using BatchPtrs = BatchVecs<const double>;
using BatchOutPtrs = BatchVecs<double>;

// the launch line of the K-wide glue kernels: kernel_of (k tag) names the kernel, one thread per unit of work; no work, no launch
template <class F, class... Args>
static void bt_launch (int K, int64_t work, hipStream_t st, F &&kernel_of, Args... args)
{
   if (work > 0) with_k (K, [&] (auto k) { hipLaunchKernelGGL (kernel_of (k), dim3 (bt_grid (work)), dim3 (BT_THREADS), 0, st, args...); });
}

// GATHER, rows -> K wide: out[i * K + k] = src_k[row (i)] (* scale[row (i)]), zeros for a system without a vector.
//   INDEXED  row (i) = idx[i] (a permutation, or the rows of a message), else i
//   SCALED   row-weighted iteration: the value times scale[row], the product rounded like launch_vmul rounds it
//   OVERLAP  row-distributed flavour, extended rows [own | overlap]: a row >= n_own is read from the K-interleaved rows that have
//            just arrived -- OV_SEL: the halo, at position sel[row - n_own]; OV_BLOCK: row - n_own of a receive block that holds the
//            overlap rows alone, in the hierarchy's order (two or more rings)
// One message row carries the K systems' values of one matrix row (8 K bytes, consecutive lanes write consecutive rows:
// coalesced 16- / 32- / 64-byte stores), so that ONE alltoallv with K times the plan's counts serves the whole group and
// the receiver's halo part is K-interleaved as it arrives.
enum { OV_NONE, OV_SEL, OV_BLOCK };
template <int K, bool INDEXED, bool SCALED, int OVERLAP>
__global__ __launch_bounds__ (BT_THREADS)
void gather_rows_kernel (const int *__restrict__ idx, BatchPtrs src, const double *__restrict__ scale, const double *__restrict__ ext,
                         const int *__restrict__ sel, int64_t n_own, double *__restrict__ out, int64_t n)
{
   const int64_t stride = (int64_t) gridDim.x * BT_THREADS;
   for (int64_t i = (int64_t) blockIdx.x * BT_THREADS + threadIdx.x; i < n; i += stride) {
      const int64_t r = INDEXED ? (int64_t) idx[i] : i;
      if (OVERLAP != OV_NONE && r >= n_own) {
         const double *h = ext + (OVERLAP == OV_SEL ? (int64_t) sel[r - n_own] : r - n_own) * K;
#pragma unroll
         for (int k = 0; k < K; k++) out[i * K + k] = src.p[k] ? h[k] : 0.0;
      } else if (SCALED) {
         const double sc = scale[r];
#pragma unroll
         for (int k = 0; k < K; k++) out[i * K + k] = src.p[k] ? __dmul_rn (src.p[k][r], sc) : 0.0;
      } else {
#pragma unroll
         for (int k = 0; k < K; k++) out[i * K + k] = src.p[k] ? src.p[k][r] : 0.0;
      }
   }
}

// SCATTER, K wide -> rows: dst_k[row (i)] = in[i * K + k] for the systems that want their vector (dst_k != NULL).
//   INDEXED  row (i) = perm[i], else i
//   WIDE     the exit of a batched cycle: z[row (i) * K + k] = in[i * K + k] as well, for every k
//   OWN      row-distributed flavour: rows < n_own only (the correction on the overlap rows belongs to their owners)
template <int K, bool INDEXED, bool WIDE, bool OWN>
__global__ __launch_bounds__ (BT_THREADS)
void scatter_rows_kernel (const int *__restrict__ perm, const double *__restrict__ in, double *__restrict__ z, BatchOutPtrs dst, int64_t n_own, int64_t n)
{
   const int64_t stride = (int64_t) gridDim.x * BT_THREADS;
   for (int64_t i = (int64_t) blockIdx.x * BT_THREADS + threadIdx.x; i < n; i += stride) {
      const int64_t r = INDEXED ? (int64_t) perm[i] : i;
      if (OWN && r >= n_own) continue;
#pragma unroll
      for (int k = 0; k < K; k++) {
         if (!WIDE && !dst.p[k]) continue;
         const double v = in[i * K + k];
         if (WIDE) z[r * K + k] = v;
         if (dst.p[k]) dst.p[k][r] = v;
      }
   }
}

// ADD, z_k += p_k between two chained cycles, on the interleaved z that feeds the operator and on the systems' own vectors at once:
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

// X[i * K + k] = src_k[i].  This one and launch_deinterleave have always launched for n = 0 too (one block that finds nothing to
// do), so they ask for one unit of work at least
void launch_interleave (int K, const double *const *src, double *X, int64_t n, hipStream_t st, const double *scale)
{
   with_bool (scale != nullptr, [&] (auto scaled) {
      bt_launch (K, n > 0 ? n : 1, st, [] (auto k) { return gather_rows_kernel<decltype (k)::value, false, decltype (scaled)::value, OV_NONE>; },
                 nullptr, BatchPtrs (K, src), scale, nullptr, nullptr, 0, X, n);
   });
}
// out[i * K + k] = src_k[idx[i]]: the entry of a batched cycle (idx = the hierarchy's permutation), a K-wide message (idx = its rows)
void launch_gather_interleave (int K, const int *idx, const double *const *src, double *out, int64_t n, hipStream_t st, const double *scale)
{
   with_bool (scale != nullptr, [&] (auto scaled) {
      bt_launch (K, n, st, [] (auto k) { return gather_rows_kernel<decltype (k)::value, true, decltype (scaled)::value, OV_NONE>; },
                 idx, BatchPtrs (K, src), scale, nullptr, nullptr, 0, out, n);
   });
}
// the entry on the extended rows of a rank: rows perm[i] >= n_own from ext, through sel or (sel NULL) as a block of their own
void launch_gather_interleave_ext (int K, const int *perm, const double *const *src, const double *ext, const int *sel, int64_t n_own, double *out, int64_t n,
                                   hipStream_t st)
{
   with_int<OV_SEL, OV_BLOCK> (sel ? OV_SEL : OV_BLOCK, [&] (auto ov) {
      bt_launch (K, n, st, [] (auto k) { return gather_rows_kernel<decltype (k)::value, true, false, decltype (ov)::value>; },
                 perm, BatchPtrs (K, src), nullptr, ext, sel, n_own, out, n);
   });
}
void launch_deinterleave (int K, const double *X, double *const *dst, int64_t n, hipStream_t st)
{
   bt_launch (K, n > 0 ? n : 1, st, [] (auto k) { return scatter_rows_kernel<decltype (k)::value, false, false, false>; }, nullptr, X, nullptr, BatchOutPtrs (K, dst), 0, n);
}
// the exit of a batched cycle: z[perm[i] * K + k] = dst_k[perm[i]] = in[i * K + k]; _own: on the extended rows of a rank
void launch_scatter_split (int K, const int *perm, const double *in, double *z, double *const *dst, int64_t n, hipStream_t st)
{
   bt_launch (K, n, st, [] (auto k) { return scatter_rows_kernel<decltype (k)::value, true, true, false>; }, perm, in, z, BatchOutPtrs (K, dst), 0, n);
}
void launch_scatter_split_own (int K, const int *perm, const double *in, double *z, double *const *dst, int64_t n_own, int64_t n, hipStream_t st)
{
   bt_launch (K, n, st, [] (auto k) { return scatter_rows_kernel<decltype (k)::value, true, true, true>; }, perm, in, z, BatchOutPtrs (K, dst), n_own, n);
}
void launch_add_split (int K, const double *p, double *z, double *const *dst, int64_t n, hipStream_t st)
{
   bt_launch (K, n, st, [] (auto k) { return add_split_kernel<decltype (k)::value>; }, p, z, BatchOutPtrs (K, dst), n);
}

// ---------------------------------------------------------------- CSR SpMV, K columns
// A row block that is a single long row (more than NKP_SPMV_LDS_NNZ entries): the sums of the systems 2g, 2g + 1, accumulated
// strided and reduced over the workgroup in the order of the single-vector kernel -- wave shuffles, then wsum in fixed order.
// Thread 0 returns the pair; the caller puts a barrier behind its use of it, before wsum is written again.
template <class VT, int K>
__device__ __forceinline__ double2 long_row_pair (int e0, int e1, int tid, int g, const int *__restrict__ colind, const VT *__restrict__ val,
                                                  const double *__restrict__ x, double2 *wsum)
{
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
   double2 s = make_double2 (0.0, 0.0);
   if (tid == 0)
      for (int w = 0; w < BT_WAVES; w++) { s.x += wsum[w].x; s.y += wsum[w].y; }
   return s;
}

// The end of row r for the systems 2g, 2g + 1, the same text behind every sum of both kernels below.
// MODE 0: y = A x   1: y = b - A x
// SPLIT: the results go to the systems' own vectors (split.p[k][r]; NULL = dropped) instead of the interleaved y, and with MODE 1
// the right-hand side comes from per-system vectors too (bsplit.p[k][r]; NULL = zero).
// SCALED (row-weighted iteration): MODE 0 multiplies the finished sum by scale[r]; MODE 1 + SPLIT multiplies the right-hand side
// it reads by scale[r].  Either is ONE rounded multiplication of a finished value, which is what launch_vmul does.
// pair_rhs is the right-hand side finish_pair subtracts from (MODE 1; zero otherwise), read apart from it because the rows kernel
// requests it ahead of its gathers.
template <int MODE, bool SPLIT, bool SCALED, int K>
__device__ __forceinline__ double2 pair_rhs (int64_t r, int g, const double *__restrict__ b, BatchPtrs bsplit, const double *__restrict__ scale)
{
   double2 bv = make_double2 (0.0, 0.0);
   if (MODE == 1 && SPLIT) {
      if (bsplit.p[2 * g]) bv.x = bsplit.p[2 * g][r];
      if (bsplit.p[2 * g + 1]) bv.y = bsplit.p[2 * g + 1][r];
      if (SCALED) { const double sc = scale[r]; bv.x = __dmul_rn (bv.x, sc); bv.y = __dmul_rn (bv.y, sc); }
   } else if (MODE == 1) bv = *reinterpret_cast<const double2 *> (b + r * K + 2 * g);
   return bv;
}
template <int MODE, bool SPLIT, bool SCALED, int K>
__device__ __forceinline__ void finish_pair (double2 s, double2 bv /* pair_rhs */, int64_t r, int g, const double *__restrict__ scale, double *__restrict__ y,
                                             BatchOutPtrs split)
{
   static_assert (!(MODE == 1 && SCALED && !SPLIT), "b - A x is scaled through its right-hand side, which only the split form reads scaled");
   if (MODE == 1) { s.x = bv.x - s.x; s.y = bv.y - s.y; }
   else if (SCALED) { const double sc = scale[r]; s.x = __dmul_rn (s.x, sc); s.y = __dmul_rn (s.y, sc); }
   if (SPLIT) { if (split.p[2 * g]) split.p[2 * g][r] = s.x; if (split.p[2 * g + 1]) split.p[2 * g + 1][r] = s.y; }
   else *reinterpret_cast<double2 *> (y + r * K + 2 * g) = s;
}

// csr_spmv_stream_kernel (spmv.hip) with the (value, column) stream of a row block read ONCE into registers and K / 2 passes
// over it: a pass gathers the 16-byte pair (x[c][2g], x[c][2g + 1]), parks both products in LDS and sums every row's segment
// in stored order.  MODE and SCALED (MODE 0 only) as in finish_pair; vectors interleaved on both sides.
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
      for (int g = 0; g < K / 2; g++) {
         const double2 s = long_row_pair<VT, K> (e0, e1, tid, g, colind, val, x, wsum);
         if (tid == 0) finish_pair<MODE, false, SCALED, K> (s, pair_rhs<MODE, false, SCALED, K> (r0, g, b, BatchPtrs (), scale), r0, g, scale, y, BatchOutPtrs ());
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
         finish_pair<MODE, false, SCALED, K> (acc, pair_rhs<MODE, false, SCALED, K> (r, g, b, BatchPtrs (), scale), r, g, scale, y, BatchOutPtrs ());
      }
      if (g + 1 < K / 2) __syncthreads ();
   }
}

// The other way round: the workgroup stages the row block's (value, column) stream in LDS with coalesced loads (8 bytes per
// entry instead of 16 K of products: 16 KB per workgroup, twice the workgroups per CU), then every row's lane walks its own
// segment, gathers the K-wide rows of x itself (GU entries in flight) and accumulates its K sums in registers -- same
// products, same stored order, one pass for any K.
// SPLIT (finish_pair): the operator product at the end of an Arnoldi step writes every system's w directly; with MODE 1, the
// residual between two chained cycles, p1_k = v_k - A z_k, from and to per-system vectors.
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
         const double2 s = long_row_pair<VT, K> (e0, e1, tid, g, colind, val, x, wsum);
         if (tid == 0) finish_pair<MODE, SPLIT, SCALED, K> (s, pair_rhs<MODE, SPLIT, SCALED, K> (r0, g, b, bsplit, scale), r0, g, scale, y, split);
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
      if (MODE == 1 && r < r1) bv[g] = pair_rhs<MODE, SPLIT, SCALED, K> (r, g, b, bsplit, scale);       // requested ahead of the gathers
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
   for (int g = 0; g < K / 2; g++) finish_pair<MODE, SPLIT, SCALED, K> (acc[g], bv[g], r, g, scale, y, split);
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
   const BatchOutPtrs P (K, dst);
   if (scale) launch_batch_rows<0, true, true> (K, A, rb0, rb1 - rb0, x, nullptr, nullptr, P, BatchPtrs (), scale, st);
   else launch_batch_rows<0, true, false> (K, A, rb0, rb1 - rb0, x, nullptr, nullptr, P, BatchPtrs (), nullptr, st);
}

// dst_k = b_k - A x_k (b_k, times bscale when given, and dst_k per system; NULL: system takes no part), row blocks [rb0, rb1)
void launch_csr_residual_batch_split_range (int K, const CsrDev &A, int rb0, int rb1, const double *x, const double *const *b, const double *bscale,
                                            double *const *dst, hipStream_t st)
{
   if (rb1 <= rb0) return;
   const BatchOutPtrs P (K, dst);
   const BatchPtrs Q (K, b);
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
   bt_launch (K, nc * K, st, [] (auto k) { return restrict_sum_batch_kernel<decltype (k)::value>; }, rptr, ridx, fine, coarse, nc);
}
void launch_prolong_add_batch (int K, const int *cmap, const double *coarse, double *fine, int64_t nf, double omega, hipStream_t st)
{
   bt_launch (K, nf * K, st, [] (auto k) { return prolong_add_batch_kernel<decltype (k)::value>; }, cmap, coarse, fine, nf, omega);
}
void launch_gather_batch (int K, const int *perm, const double *in, double *out, int64_t n, hipStream_t st)
{
   bt_launch (K, n * K, st, [] (auto k) { return gather_batch_kernel<decltype (k)::value>; }, perm, in, out, n);
}
void launch_dense_matvec_batch (int K, const double *Minv, const double *x, double *y, int n, hipStream_t st)
{
   // a wave per row and no stride in the kernel: the grid is not clamped like bt_launch's
   if (n > 0) with_k (K, [&] (auto k) { hipLaunchKernelGGL (dense_matvec_batch_kernel<decltype (k)::value>, dim3 ((n + BT_WAVES - 1) / BT_WAVES), dim3 (BT_THREADS), 0, st, Minv, x, y, n); });
}

// ---------------------------------------------------------------- water columns, one per wave, K columns of right-hand sides
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
            for (int q = 0; q < K; q++) yk[q] = readlane_f64 (y[s][q], kl);
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
               xk[q] = readlane_f64 (y[s][q], kl);
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

// the factors of the rows a lane holds, as the band solve takes them (colblock_apply_kernel and gs_wave_kernel load theirs in the
// loop that loads their one right-hand side; taking this function there changes their code)
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
