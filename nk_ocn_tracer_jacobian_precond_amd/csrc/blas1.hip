// Vector kernels of the Krylov drivers (gfx950).  All are HBM-bound streams: 16-byte loads
// per lane, grid-stride, 64-lane __shfl_down wave reductions, and a FIXED number of partial
// sums that a second tiny kernel adds in a fixed order -- so every inner product is bitwise
// reproducible (no float atomics) and, in the multi-GPU build, is the local contribution fed
// to one RCCL allreduce per Gram-Schmidt sweep.
//
// Stand in for the norm / update bookkeeping of pdgsrfs_ABXglobal (reference
// src/SuperLU_brief_tree.txt:20).  The fused multi-dot reads w once per chunk of 8 basis
// vectors and every basis vector exactly once.
#include "nkp_dev.h"

#include <stdint.h>

#define B1_THREADS 256

__device__ __forceinline__ double wave_sum (double v)
{
#pragma unroll
   for (int off = NKP_WAVE / 2; off > 0; off >>= 1) v += __shfl_down (v, off);
   return v;
}

// block-wide sum, result valid in thread 0
__device__ __forceinline__ double block_sum (double v, double *sh /* [B1_THREADS/64] */)
{
   v = wave_sum (v);
   const int lane = threadIdx.x & (NKP_WAVE - 1), wv = threadIdx.x / NKP_WAVE;
   __syncthreads ();
   if (lane == 0) sh[wv] = v;
   __syncthreads ();
   double s = 0.0;
   if (threadIdx.x == 0) {
#pragma unroll
      for (int w = 0; w < B1_THREADS / NKP_WAVE; w++) s += sh[w];
   }
   return s;
}

static inline int red_grid (int64_t n)
{
   int64_t g = (n + 2 * B1_THREADS - 1) / (2 * B1_THREADS);
   if (g < 1) g = 1;
   if (g > NKP_RED_BLOCKS) g = NKP_RED_BLOCKS;
   return (int) g;
}

// ---------------------------------------------------------------- multi-dot
// grid (nblk, nchunk).  partial[(chunk*nblk + blk)*(CHUNK+1) + c]; slot CHUNK of chunk 0 = w.w
template <class VT, class VT2>
__device__ __forceinline__ void multi_dot_body (const VT *__restrict__ V, int64_t ld, int k, const double *__restrict__ w,
                                                int64_t n, double *__restrict__ partial, double *sh)
{
   const int chunk = blockIdx.y;
   const int j0 = chunk * NKP_DOT_CHUNK;
   const int kc = (k - j0) < NKP_DOT_CHUNK ? (k - j0) : NKP_DOT_CHUNK;
   const VT *Vc = V + (int64_t) j0 * ld;
   double acc[NKP_DOT_CHUNK];
#pragma unroll
   for (int c = 0; c < NKP_DOT_CHUNK; c++) acc[c] = 0.0;
   double accw = 0.0;
   const int64_t stride = (int64_t) gridDim.x * B1_THREADS * 2;
   for (int64_t i = ((int64_t) blockIdx.x * B1_THREADS + threadIdx.x) * 2; i < n; i += stride) {
      if (i + 1 < n) {
         const double2 w2 = *reinterpret_cast<const double2 *> (w + i);
         accw += w2.x * w2.x + w2.y * w2.y;
#pragma unroll
         for (int c = 0; c < NKP_DOT_CHUNK; c++)
            if (c < kc) {
               const VT2 v2 = *reinterpret_cast<const VT2 *> (Vc + (int64_t) c * ld + i);
               acc[c] += (double) v2.x * w2.x + (double) v2.y * w2.y;
            }
      } else {
         const double w1 = w[i];
         accw += w1 * w1;
#pragma unroll
         for (int c = 0; c < NKP_DOT_CHUNK; c++)
            if (c < kc) acc[c] += (double) Vc[(int64_t) c * ld + i] * w1;
      }
   }
   double *out = partial + ((int64_t) chunk * gridDim.x + blockIdx.x) * (NKP_DOT_CHUNK + 1);
#pragma unroll
   for (int c = 0; c < NKP_DOT_CHUNK; c++) {
      const double s = block_sum (acc[c], sh);
      if (threadIdx.x == 0) out[c] = s;
   }
   const double sw = block_sum (accw, sh);
   if (threadIdx.x == 0) out[NKP_DOT_CHUNK] = sw;
}

template <class VT, class VT2>
__global__ __launch_bounds__ (B1_THREADS)
void multi_dot_kernel (const VT *__restrict__ V, int64_t ld, int k, const double *__restrict__ w,
                       int64_t n, double *__restrict__ partial)
{
   __shared__ double sh[B1_THREADS / NKP_WAVE];
   multi_dot_body<VT, VT2> (V, ld, k, w, n, partial, sh);
}

// the same for system blockIdx.z of a group
__global__ __launch_bounds__ (B1_THREADS)
void multi_dot_group_kernel (GsGroup G, int64_t ld, int k, int64_t n)
{
   __shared__ double sh[B1_THREADS / NKP_WAVE];
   const int r = blockIdx.z;
   multi_dot_body<double, double2> (G.V[r], ld, k, G.w[r], n, G.partial[r], sh);
}

// one wave per output: out[j] = sum_blk partial[...], fixed order.  out[k] = w.w (chunk 0)
__device__ __forceinline__ void multi_dot_finish_body (const double *__restrict__ partial, int nblk, int k, double *__restrict__ out)
{
   const int j = blockIdx.x;                   // 0..k  (k = the w.w slot)
   const int chunk = (j < k) ? j / NKP_DOT_CHUNK : 0;
   const int c = (j < k) ? j % NKP_DOT_CHUNK : NKP_DOT_CHUNK;
   const double *p = partial + (int64_t) chunk * nblk * (NKP_DOT_CHUNK + 1) + c;
   double s = 0.0;
   for (int b = threadIdx.x; b < nblk; b += NKP_WAVE) s += p[(int64_t) b * (NKP_DOT_CHUNK + 1)];
   s = wave_sum (s);
   if (threadIdx.x == 0) out[j] = s;
}

__global__ __launch_bounds__ (NKP_WAVE)
void multi_dot_finish_kernel (const double *__restrict__ partial, int nblk, int k, double *__restrict__ out)
{
   multi_dot_finish_body (partial, nblk, k, out);
}

__global__ __launch_bounds__ (NKP_WAVE)
void multi_dot_finish_group_kernel (GsGroup G, int nblk, int k, double *__restrict__ msg)
{
   multi_dot_finish_body (G.partial[blockIdx.y], nblk, k, msg + (int64_t) blockIdx.y * (k + 1));
}

void launch_multi_dot (const void *V, int v_f32, int64_t ld, int k, const double *w, int64_t n, double *partial, double *out, hipStream_t st)
{
   const int g = red_grid (n);
   const int nchunk = k > 0 ? (k + NKP_DOT_CHUNK - 1) / NKP_DOT_CHUNK : 1;
   if (v_f32) hipLaunchKernelGGL ((multi_dot_kernel<float, float2>), dim3 (g, nchunk), dim3 (B1_THREADS), 0, st, (const float *) V, ld, k, w, n, partial);
   else hipLaunchKernelGGL ((multi_dot_kernel<double, double2>), dim3 (g, nchunk), dim3 (B1_THREADS), 0, st, (const double *) V, ld, k, w, n, partial);
   hipLaunchKernelGGL (multi_dot_finish_kernel, dim3 (k + 1), dim3 (NKP_WAVE), 0, st, partial, g, k, out);
}

void launch_multi_dot_group (int R, const GsGroup &G, int64_t ld, int k, int64_t n, double *msg, hipStream_t st)
{
   if (R <= 0) return;
   const int g = red_grid (n);
   const int nchunk = k > 0 ? (k + NKP_DOT_CHUNK - 1) / NKP_DOT_CHUNK : 1;
   hipLaunchKernelGGL (multi_dot_group_kernel, dim3 (g, nchunk, R), dim3 (B1_THREADS), 0, st, G, ld, k, n);
   hipLaunchKernelGGL (multi_dot_finish_group_kernel, dim3 (k + 1, R), dim3 (NKP_WAVE), 0, st, G, g, k, msg);
}

// ---------------------------------------------------------------- w -= V h, with ||w||^2
#define B1_MAX_K NKP_MAX_K
template <class VT, class VT2>
__device__ __forceinline__ void update_w_body (const VT *__restrict__ V, int64_t ld, int k, const double *__restrict__ h,
                                               double *__restrict__ w, int64_t n, double *__restrict__ partial, double sign, double *hs, double *sh)
{
   for (int j = threadIdx.x; j < k; j += B1_THREADS) hs[j] = sign * h[j];
   __syncthreads ();
   double nrm = 0.0;
   const int64_t stride = (int64_t) gridDim.x * B1_THREADS * 2;
   for (int64_t i = ((int64_t) blockIdx.x * B1_THREADS + threadIdx.x) * 2; i < n; i += stride) {
      if (i + 1 < n) {
         double2 a = *reinterpret_cast<const double2 *> (w + i);
         int j = 0;
         for (; j + 4 <= k; j += 4) {
            const VT2 v0 = *reinterpret_cast<const VT2 *> (V + (int64_t) (j + 0) * ld + i);
            const VT2 v1 = *reinterpret_cast<const VT2 *> (V + (int64_t) (j + 1) * ld + i);
            const VT2 v2 = *reinterpret_cast<const VT2 *> (V + (int64_t) (j + 2) * ld + i);
            const VT2 v3 = *reinterpret_cast<const VT2 *> (V + (int64_t) (j + 3) * ld + i);
            a.x += hs[j] * v0.x; a.y += hs[j] * v0.y;
            a.x += hs[j + 1] * v1.x; a.y += hs[j + 1] * v1.y;
            a.x += hs[j + 2] * v2.x; a.y += hs[j + 2] * v2.y;
            a.x += hs[j + 3] * v3.x; a.y += hs[j + 3] * v3.y;
         }
         for (; j < k; j++) {
            const VT2 v0 = *reinterpret_cast<const VT2 *> (V + (int64_t) j * ld + i);
            a.x += hs[j] * v0.x; a.y += hs[j] * v0.y;
         }
         *reinterpret_cast<double2 *> (w + i) = a;
         nrm += a.x * a.x + a.y * a.y;
      } else {
         double a = w[i];
         for (int j = 0; j < k; j++) a += hs[j] * V[(int64_t) j * ld + i];
         w[i] = a;
         nrm += a * a;
      }
   }
   if (partial) {
      const double s = block_sum (nrm, sh);
      if (threadIdx.x == 0) partial[blockIdx.x] = s;
   }
}

template <class VT, class VT2>
__global__ __launch_bounds__ (B1_THREADS)
void update_w_kernel (const VT *__restrict__ V, int64_t ld, int k, const double *__restrict__ h,
                      double *__restrict__ w, int64_t n, double *__restrict__ partial, double sign)
{
   __shared__ double hs[B1_MAX_K];
   __shared__ double sh[B1_THREADS / NKP_WAVE];
   update_w_body<VT, VT2> (V, ld, k, h, w, n, partial, sign, hs, sh);
}

__global__ __launch_bounds__ (B1_THREADS)
void update_w_group_kernel (GsGroup G, int64_t ld, int k, const double *__restrict__ msg, int64_t n)
{
   __shared__ double hs[B1_MAX_K];
   __shared__ double sh[B1_THREADS / NKP_WAVE];
   const int r = blockIdx.y;
   update_w_body<double, double2> (G.V[r], ld, k, msg + (int64_t) r * (k + 1), G.w[r], n, G.partial[r], -1.0, hs, sh);
}

__device__ __forceinline__ void sum_partials_body (const double *__restrict__ partial, int nblk, double *__restrict__ out)
{
   double s = 0.0;
   for (int b = threadIdx.x; b < nblk; b += NKP_WAVE) s += partial[b];
   s = wave_sum (s);
   if (threadIdx.x == 0) out[0] = s;
}

__global__ __launch_bounds__ (NKP_WAVE)
void sum_partials_kernel (const double *__restrict__ partial, int nblk, double *__restrict__ out)
{
   sum_partials_body (partial, nblk, out);
}

__global__ __launch_bounds__ (NKP_WAVE)
void sum_partials_group_kernel (GsGroup G, int nblk, double *__restrict__ out)
{
   sum_partials_body (G.partial[blockIdx.x], nblk, out + blockIdx.x);
}

void launch_update_w (const void *V, int v_f32, int64_t ld, int k, const double *h, double *w, int64_t n, double *partial, double *out_nrm2, hipStream_t st)
{
   const int g = red_grid (n);
   if (v_f32) hipLaunchKernelGGL ((update_w_kernel<float, float2>), dim3 (g), dim3 (B1_THREADS), 0, st, (const float *) V, ld, k, h, w, n, partial, -1.0);
   else hipLaunchKernelGGL ((update_w_kernel<double, double2>), dim3 (g), dim3 (B1_THREADS), 0, st, (const double *) V, ld, k, h, w, n, partial, -1.0);
   if (out_nrm2) hipLaunchKernelGGL (sum_partials_kernel, dim3 (1), dim3 (NKP_WAVE), 0, st, partial, g, out_nrm2);      // NULL: launch_finish_column_host adds them up
}

void launch_update_w_group (int R, const GsGroup &G, int64_t ld, int k, const double *msg, int64_t n, double *nrm2, hipStream_t st)
{
   if (R <= 0) return;
   const int g = red_grid (n);
   hipLaunchKernelGGL (update_w_group_kernel, dim3 (g, R), dim3 (B1_THREADS), 0, st, G, ld, k, msg, n);
   hipLaunchKernelGGL (sum_partials_group_kernel, dim3 (R), dim3 (NKP_WAVE), 0, st, G, g, nrm2);
}

void launch_axpy_multi (const double *Z, int64_t ld, int k, const double *c, double *x, int64_t n, hipStream_t st)
{
   const int g = red_grid (n);
   hipLaunchKernelGGL ((update_w_kernel<double, double2>), dim3 (g), dim3 (B1_THREADS), 0, st, Z, ld, k, c, x, n, (double *) nullptr, 1.0);
}

// ---------------------------------------------------------------- simple streams
// y = alpha x ; optionally also yf = (float) (alpha x)  (f32 copy of a Krylov basis vector)
__device__ __forceinline__ void scale_to_body (const double *__restrict__ x, const double *__restrict__ alpha, double *__restrict__ y, float *__restrict__ yf, int64_t n)
{
   const double a = alpha[0];
   const int64_t stride = (int64_t) gridDim.x * B1_THREADS * 2;
   for (int64_t i = ((int64_t) blockIdx.x * B1_THREADS + threadIdx.x) * 2; i < n; i += stride) {
      if (i + 1 < n) {
         double2 v = *reinterpret_cast<const double2 *> (x + i);
         v.x *= a; v.y *= a;
         *reinterpret_cast<double2 *> (y + i) = v;
         if (yf) *reinterpret_cast<float2 *> (yf + i) = make_float2 ((float) v.x, (float) v.y);
      } else {
         y[i] = a * x[i];
         if (yf) yf[i] = (float) (a * x[i]);
      }
   }
}

__global__ __launch_bounds__ (B1_THREADS)
void scale_to_kernel (const double *__restrict__ x, const double *__restrict__ alpha, double *__restrict__ y, float *__restrict__ yf, int64_t n)
{
   scale_to_body (x, alpha, y, yf, n);
}

__global__ __launch_bounds__ (B1_THREADS)
void scale_to_group_kernel (GsGroup G, const double *__restrict__ inv, int64_t n)
{
   const int r = blockIdx.y;
   scale_to_body (G.w[r], inv + r, G.vnext[r], nullptr, n);
}

void launch_scale_to (const double *x, const double *alpha_dev, double *y, float *yf, int64_t n, hipStream_t st)
{
   hipLaunchKernelGGL (scale_to_kernel, dim3 (red_grid (n)), dim3 (B1_THREADS), 0, st, x, alpha_dev, y, yf, n);
}

void launch_scale_to_group (int R, const GsGroup &G, const double *inv, int64_t n, hipStream_t st)
{
   if (R > 0) hipLaunchKernelGGL (scale_to_group_kernel, dim3 (red_grid (n), R), dim3 (B1_THREADS), 0, st, G, inv, n);
}

__global__ __launch_bounds__ (B1_THREADS)
void axpby_kernel (double a, const double *__restrict__ x, double b, double *__restrict__ y, int64_t n)
{
   const int64_t stride = (int64_t) gridDim.x * B1_THREADS;
   for (int64_t i = (int64_t) blockIdx.x * B1_THREADS + threadIdx.x; i < n; i += stride)
      y[i] = (b == 0.0 ? 0.0 : b * y[i]) + (x ? a * x[i] : a);
}

void launch_axpby (double a, const double *x, double b, double *y, int64_t n, hipStream_t st)
{
   hipLaunchKernelGGL (axpby_kernel, dim3 (red_grid (n) * 2), dim3 (B1_THREADS), 0, st, a, x, b, y, n);
}

__global__ __launch_bounds__ (B1_THREADS)
void vmul_kernel (const double *x, const double *__restrict__ w, double *y, int64_t n)
{
   const int64_t stride = (int64_t) gridDim.x * B1_THREADS;
   for (int64_t i = (int64_t) blockIdx.x * B1_THREADS + threadIdx.x; i < n; i += stride) y[i] = x[i] * w[i];
}

void launch_vmul (const double *x, const double *w, double *y, int64_t n, hipStream_t st)
{
   hipLaunchKernelGGL (vmul_kernel, dim3 (red_grid (n) * 2), dim3 (B1_THREADS), 0, st, x, w, y, n);
}

void launch_copy (const double *x, double *y, int64_t n, hipStream_t st)
{
   (void) hipMemcpyAsync (y, x, (size_t) n * sizeof (double), hipMemcpyDeviceToDevice, st);
}

// zero fill in ONE launch: hipMemsetAsync splits a buffer whose size is not a multiple of its block into two kernels (an aligned
// body and a 256-thread remainder), ~10 us of launch floors per level of the cycle instead of ~5
__global__ __launch_bounds__ (B1_THREADS)
void zero_kernel (double *__restrict__ y, int64_t n)
{
   const int64_t stride = (int64_t) gridDim.x * B1_THREADS * 2;
   for (int64_t i = ((int64_t) blockIdx.x * B1_THREADS + threadIdx.x) * 2; i < n; i += stride) {
      if (i + 1 < n) *reinterpret_cast<double2 *> (y + i) = make_double2 (0.0, 0.0);       // vectors are 16-byte aligned (hipMalloc, even offsets)
      else y[i] = 0.0;
   }
}

void launch_fill (double *y, double v, int64_t n, hipStream_t st)
{
   if (n <= 0) return;
   if (v == 0.0) {
      if ((reinterpret_cast<uintptr_t> (y) & 15) == 0) hipLaunchKernelGGL (zero_kernel, dim3 (red_grid (n) * 2), dim3 (B1_THREADS), 0, st, y, n);
      else (void) hipMemsetAsync (y, 0, (size_t) n * sizeof (double), st);
   } else
      launch_axpby (v, nullptr, 0.0, y, n, st);
}

// ---------------------------------------------------------------- dot, berr
__global__ __launch_bounds__ (B1_THREADS)
void dot_kernel (const double *__restrict__ x, const double *__restrict__ y, int64_t n, double *__restrict__ partial)
{
   __shared__ double sh[B1_THREADS / NKP_WAVE];
   double acc = 0.0;
   const int64_t stride = (int64_t) gridDim.x * B1_THREADS * 2;
   for (int64_t i = ((int64_t) blockIdx.x * B1_THREADS + threadIdx.x) * 2; i < n; i += stride) {
      if (i + 1 < n) {
         const double2 a = *reinterpret_cast<const double2 *> (x + i);
         const double2 b = *reinterpret_cast<const double2 *> (y + i);
         acc += a.x * b.x + a.y * b.y;
      } else
         acc += x[i] * y[i];
   }
   const double s = block_sum (acc, sh);
   if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

void launch_dot (const double *x, const double *y, int64_t n, double *partial, double *out, hipStream_t st)
{
   const int g = red_grid (n);
   hipLaunchKernelGGL (dot_kernel, dim3 (g), dim3 (B1_THREADS), 0, st, x, y, n, partial);
   hipLaunchKernelGGL (sum_partials_kernel, dim3 (1), dim3 (NKP_WAVE), 0, st, partial, g, out);
}

// The larger of two quotients, NaN sticky: a NaN on either side wins (a plain q > m ? q : m drops it), so that a residual or a
// denominator that is not a number gives a backward error that is not one either, through every stage of the reduction.
__device__ __forceinline__ double max_or_nan (double q, double m)
{
   return (q > m || q != q) ? q : m;
}

__global__ __launch_bounds__ (B1_THREADS)
void berr_kernel (const double *__restrict__ r, const double *__restrict__ den, int64_t n, double *__restrict__ partial)
{
   __shared__ double sh[B1_THREADS / NKP_WAVE];
   double m = 0.0;
   const int64_t stride = (int64_t) gridDim.x * B1_THREADS;
   for (int64_t i = (int64_t) blockIdx.x * B1_THREADS + threadIdx.x; i < n; i += stride) {
      const double a = fabs (r[i]), d = den[i];
      // a / d keeps a NaN of either and makes one of Inf / Inf; d == 0 (an empty row with b_i = 0) follows the old rule
      const double q = (d > 0.0 || d != d) ? a / d : (a != a ? a : a > 0.0 ? 1.0e300 : 0.0);
      m = max_or_nan (q, m);
   }
   for (int off = NKP_WAVE / 2; off > 0; off >>= 1) m = max_or_nan (__shfl_down (m, off), m);
   const int lane = threadIdx.x & (NKP_WAVE - 1), wv = threadIdx.x / NKP_WAVE;
   if (lane == 0) sh[wv] = m;
   __syncthreads ();
   if (threadIdx.x == 0) {
      for (int w = 1; w < B1_THREADS / NKP_WAVE; w++) m = max_or_nan (sh[w], m);
      partial[blockIdx.x] = m;
   }
}

__global__ __launch_bounds__ (NKP_WAVE)
void max_partials_kernel (const double *__restrict__ partial, int nblk, double *__restrict__ out)
{
   double m = 0.0;
   for (int b = threadIdx.x; b < nblk; b += NKP_WAVE) m = max_or_nan (partial[b], m);
   for (int off = NKP_WAVE / 2; off > 0; off >>= 1) m = max_or_nan (__shfl_down (m, off), m);
   if (threadIdx.x == 0) out[0] = m;
}

void launch_berr (const double *r, const double *den, int64_t n, double *partial, double *out, hipStream_t st)
{
   const int g = red_grid (n);
   hipLaunchKernelGGL (berr_kernel, dim3 (g), dim3 (B1_THREADS), 0, st, r, den, n, partial);
   hipLaunchKernelGGL (max_partials_kernel, dim3 (1), dim3 (NKP_WAVE), 0, st, partial, g, out);
}

// out[0] = entries of x that are NaN or Inf, out[1] = entries that are not zero (those included), as doubles: exact below 2^53,
// and a row-distributed solver adds them across ranks like any other sum.  Only for a right-hand side whose norm has left the
// range in which it decides alone (krylov.hip, classify_rhs).  partial: 2 * NKP_RED_BLOCKS doubles.
__global__ __launch_bounds__ (B1_THREADS)
void count_entries_kernel (const double *__restrict__ x, int64_t n, double *__restrict__ partial)
{
   __shared__ double sh[B1_THREADS / NKP_WAVE];
   double bad = 0.0, set = 0.0;
   const int64_t stride = (int64_t) gridDim.x * B1_THREADS;
   for (int64_t i = (int64_t) blockIdx.x * B1_THREADS + threadIdx.x; i < n; i += stride) {
      const double v = x[i];
      bad += (v - v == 0.0) ? 0.0 : 1.0;
      set += (v == 0.0) ? 0.0 : 1.0;
   }
   const double sb = block_sum (bad, sh);
   if (threadIdx.x == 0) partial[blockIdx.x] = sb;
   const double ss = block_sum (set, sh);
   if (threadIdx.x == 0) partial[NKP_RED_BLOCKS + blockIdx.x] = ss;
}

void launch_count_entries (const double *x, int64_t n, double *partial, double *out, hipStream_t st)
{
   const int g = red_grid (n);
   hipLaunchKernelGGL (count_entries_kernel, dim3 (g), dim3 (B1_THREADS), 0, st, x, n, partial);
   hipLaunchKernelGGL (sum_partials_kernel, dim3 (1), dim3 (NKP_WAVE), 0, st, partial, g, out);
   hipLaunchKernelGGL (sum_partials_kernel, dim3 (1), dim3 (NKP_WAVE), 0, st, partial + NKP_RED_BLOCKS, g, out + 1);
}

// ---------------------------------------------------------------- Hessenberg column epilogue
__device__ __forceinline__ void finish_column_body (double *__restrict__ h, const double *__restrict__ h2, int k,
                                                    const double *__restrict__ nrm2, double *__restrict__ inv)
{
   if (h2)
      for (int j = threadIdx.x; j < k; j += NKP_WAVE) h[j] += h2[j];
   if (threadIdx.x == 0) {
      const double t = sqrt (nrm2[0]);
      h[k] = t;
      inv[0] = (t > 0.0) ? 1.0 / t : 0.0;
   }
}

__global__ __launch_bounds__ (NKP_WAVE)
void finish_column_kernel (double *__restrict__ h, const double *__restrict__ h2, int k,
                           const double *__restrict__ nrm2, double *__restrict__ inv)
{
   finish_column_body (h, h2, k, nrm2, inv);
}

// distributed flavour: ||w - V h||^2 = w.w - sum h_i^2 from the ALREADY reduced multi-dot message (h[0..k-1], h[k] = w.w), so
// that an Arnoldi step needs one allreduce instead of two.  The difference loses log10 (w.w / result) digits; below 1e-8 of
// w.w (the new direction is numerically inside the old space) h[k] is returned NEGATIVE: the host takes its magnitude and ends
// the restart cycle there, and the true residual of the restart decides.  One wave, fixed order.
__device__ __forceinline__ void finish_column_pythagoras_body (double *__restrict__ h, int k, double *__restrict__ inv)
{
   double s = 0.0;
   for (int j = threadIdx.x; j < k; j += NKP_WAVE) s += h[j] * h[j];
   for (int off = NKP_WAVE / 2; off > 0; off >>= 1) s += __shfl_down (s, off);
   if (threadIdx.x == 0) {
      const double ww = h[k];
      double t2 = ww - s;
      const bool weak = !(t2 >= 1e-8 * ww);
      if (!(t2 > 0.0)) t2 = 0.0;
      const double t = sqrt (t2);
      h[k] = weak ? -t : t;
      inv[0] = (t > 0.0) ? 1.0 / t : 0.0;
   }
}

__global__ __launch_bounds__ (NKP_WAVE)
void finish_column_pythagoras_kernel (double *__restrict__ h, int k, double *__restrict__ inv)
{
   finish_column_pythagoras_body (h, k, inv);
}

// row blockIdx.x of a group's message
__global__ __launch_bounds__ (NKP_WAVE)
void finish_column_group_kernel (double *__restrict__ msg, const double *__restrict__ msg2, int k, const double *__restrict__ nrm2, double *__restrict__ inv)
{
   const int64_t r = blockIdx.x;
   if (nrm2) finish_column_body (msg + r * (k + 1), msg2 ? msg2 + r * (k + 1) : nullptr, k, nrm2 + r, inv + r);
   else finish_column_pythagoras_body (msg + r * (k + 1), k, inv + r);
}

void launch_finish_column_group (int R, double *msg, const double *msg2, int k, const double *nrm2, double *inv, hipStream_t st)
{
   if (R > 0) hipLaunchKernelGGL (finish_column_group_kernel, dim3 (R), dim3 (NKP_WAVE), 0, st, msg, msg2, k, nrm2, inv);
}

void launch_finish_column_pythagoras (double *h, int k, double *inv, hipStream_t st)
{
   hipLaunchKernelGGL (finish_column_pythagoras_kernel, dim3 (1), dim3 (NKP_WAVE), 0, st, h, k, inv);
}

// The same for the step that hands its column over early (tuning step_glue bit 8), one launch and one copy command fewer: ||w||^2 is summed here from
// the partial sums of update_w_kernel, in the order of sum_partials_kernel (and still stored to nrm2_out), and the finished column
// h[0 .. k] also goes to host_col: pinned host memory the device can address, which the host reads after an event behind this
// kernel -- no copy command between this kernel and the next.
__global__ __launch_bounds__ (NKP_WAVE)
void finish_column_host_kernel (double *__restrict__ h, const double *__restrict__ h2, int k, const double *__restrict__ partial, int nblk,
                                double *__restrict__ nrm2_out, double *__restrict__ inv, double *__restrict__ host_col)
{
   double s = 0.0;
   for (int b = threadIdx.x; b < nblk; b += NKP_WAVE) s += partial[b];
   s = wave_sum (s);
   if (h2)
      for (int j = threadIdx.x; j < k; j += NKP_WAVE) h[j] += h2[j];
   if (threadIdx.x == 0) {
      nrm2_out[0] = s;
      const double t = sqrt (s);
      h[k] = t;
      inv[0] = (t > 0.0) ? 1.0 / t : 0.0;
   }
   __syncthreads ();
   for (int j = threadIdx.x; j <= k; j += NKP_WAVE) host_col[j] = h[j];
   __threadfence_system ();
}

// partial: the n-vector's block sums as launch_update_w_only left them
void launch_finish_column_host (double *h, const double *h2, int k, const double *partial, int64_t n, double *nrm2_out, double *inv, double *host_col, hipStream_t st)
{
   hipLaunchKernelGGL (finish_column_host_kernel, dim3 (1), dim3 (NKP_WAVE), 0, st, h, h2, k, partial, red_grid (n), nrm2_out, inv, host_col);
}

void launch_finish_column (double *h, const double *h2, int k, const double *nrm2, double *inv, hipStream_t st)
{
   hipLaunchKernelGGL (finish_column_kernel, dim3 (1), dim3 (NKP_WAVE), 0, st, h, h2, k, nrm2, inv);
}

// ---------------------------------------------------------------- grid transfer / permutation
__global__ __launch_bounds__ (B1_THREADS)
void restrict_sum_kernel (const int *__restrict__ rptr, const int *__restrict__ ridx, const double *__restrict__ fine,
                          double *__restrict__ coarse, int64_t nc)
{
   const int64_t stride = (int64_t) gridDim.x * B1_THREADS;
   for (int64_t I = (int64_t) blockIdx.x * B1_THREADS + threadIdx.x; I < nc; I += stride) {
      double acc = 0.0;
      for (int q = rptr[I]; q < rptr[I + 1]; q++) acc += fine[ridx[q]];
      coarse[I] = acc;
   }
}

// Tuning step_glue bit 4: the same sums, and coarse_x = 0 (the fill the coarse level's cycle would start with) in the same pass.
// A coarse row's indices are requested eight at a time, then their fine values, and only then added -- in q order, from +0.0,
// as above: same bits, the loads no longer wait for each other.
__global__ __launch_bounds__ (B1_THREADS)
void restrict_sum_fill_kernel (const int *__restrict__ rptr, const int *__restrict__ ridx, const double *__restrict__ fine,
                               double *__restrict__ coarse, double *__restrict__ coarse_x, int64_t nc)
{
   const int64_t stride = (int64_t) gridDim.x * B1_THREADS;
   for (int64_t I = (int64_t) blockIdx.x * B1_THREADS + threadIdx.x; I < nc; I += stride) {
      const int q1 = rptr[I + 1];
      double acc = 0.0;
      for (int q0 = rptr[I]; q0 < q1; q0 += 8) {
         int id[8];
         double v[8];
#pragma unroll
         for (int t = 0; t < 8; t++) id[t] = (q0 + t < q1) ? ridx[q0 + t] : -1;
#pragma unroll
         for (int t = 0; t < 8; t++) v[t] = (id[t] >= 0) ? fine[id[t]] : 0.0;
#pragma unroll
         for (int t = 0; t < 8; t++)
            if (q0 + t < q1) acc += v[t];
      }
      coarse[I] = acc;
      coarse_x[I] = 0.0;
   }
}

void launch_restrict_sum (const int *rptr, const int *ridx, const double *fine, double *coarse, int64_t nc, hipStream_t st, double *coarse_x)
{
   if (nc <= 0) return;
   if (coarse_x) {
      hipLaunchKernelGGL (restrict_sum_fill_kernel, dim3 (red_grid (nc) * 2), dim3 (B1_THREADS), 0, st, rptr, ridx, fine, coarse, coarse_x, nc);
      return;
   }
   hipLaunchKernelGGL (restrict_sum_kernel, dim3 (red_grid (nc) * 2), dim3 (B1_THREADS), 0, st, rptr, ridx, fine, coarse, nc);
}

__global__ __launch_bounds__ (B1_THREADS)
void prolong_add_kernel (const int *__restrict__ cmap, const double *__restrict__ coarse, double *__restrict__ fine, int64_t nf, double omega)
{
   const int64_t stride = (int64_t) gridDim.x * B1_THREADS;
   for (int64_t i = (int64_t) blockIdx.x * B1_THREADS + threadIdx.x; i < nf; i += stride) fine[i] += omega * coarse[cmap[i]];
}

// fine += omega * P coarse (omega = 1: the plain piecewise-constant prolongation; x * 1.0 is exact)
void launch_prolong_add (const int *cmap, const double *coarse, double *fine, int64_t nf, double omega, hipStream_t st)
{
   if (nf <= 0) return;
   hipLaunchKernelGGL (prolong_add_kernel, dim3 (red_grid (nf) * 2), dim3 (B1_THREADS), 0, st, cmap, coarse, fine, nf, omega);
}

__global__ __launch_bounds__ (B1_THREADS)
void gather_kernel (const int *__restrict__ perm, const double *__restrict__ in, double *__restrict__ out, int64_t n, int scatter)
{
   const int64_t stride = (int64_t) gridDim.x * B1_THREADS;
   for (int64_t i = (int64_t) blockIdx.x * B1_THREADS + threadIdx.x; i < n; i += stride) {
      if (scatter) out[perm[i]] = in[i];
      else out[i] = in[perm[i]];
   }
}

void launch_gather (const int *perm, const double *in, double *out, int64_t n, hipStream_t st)
{
   if (n <= 0) return;
   hipLaunchKernelGGL (gather_kernel, dim3 (red_grid (n) * 2), dim3 (B1_THREADS), 0, st, perm, in, out, n, 0);
}

void launch_scatter (const int *perm, const double *in, double *out, int64_t n, hipStream_t st)
{
   if (n <= 0) return;
   hipLaunchKernelGGL (gather_kernel, dim3 (red_grid (n) * 2), dim3 (B1_THREADS), 0, st, perm, in, out, n, 1);
}

// Tuning step_glue bit 8: what scale_to_kernel (w -> v), gather_kernel (v -> level 0's b) and zero_kernel (level 0's x) do in
// three launches.  v = w * inv is the product scale_to_kernel forms, formed once per element.
__global__ __launch_bounds__ (B1_THREADS)
void cycle_entry_kernel (const int *__restrict__ perm, const double *__restrict__ w, const double *__restrict__ inv,
                         double *__restrict__ vnext, double *__restrict__ b0, double *__restrict__ x0, int64_t n)
{
   const double a = inv[0];
   const int64_t stride = (int64_t) gridDim.x * B1_THREADS;
   for (int64_t i = (int64_t) blockIdx.x * B1_THREADS + threadIdx.x; i < n; i += stride) {
      const int p = perm[i];
      const double v = w[p] * a;
      vnext[p] = v;
      b0[i] = v;
      x0[i] = 0.0;
   }
}

void launch_cycle_entry (const int *perm, const double *w, const double *inv, double *vnext, double *b0, double *x0, int64_t n, hipStream_t st)
{
   if (n <= 0) return;
   hipLaunchKernelGGL (cycle_entry_kernel, dim3 (red_grid (n) * 2), dim3 (B1_THREADS), 0, st, perm, w, inv, vnext, b0, x0, n);
}

// one wave per output row; the coarsest level is at most a few thousand unknowns
__global__ __launch_bounds__ (B1_THREADS)
void dense_matvec_kernel (const double *__restrict__ M, const double *__restrict__ x, double *__restrict__ y, int n)
{
   const int row = (int) ((blockIdx.x * B1_THREADS + threadIdx.x) / NKP_WAVE);
   const int lane = threadIdx.x & (NKP_WAVE - 1);
   if (row >= n) return;
   const double *m = M + (int64_t) row * n;
   double acc = 0.0;
   for (int c = lane; c < n; c += NKP_WAVE) acc += m[c] * x[c];
   acc = wave_sum (acc);
   if (lane == 0) y[row] = acc;
}

void launch_dense_matvec (const double *Minv, const double *x, double *y, int n, hipStream_t st)
{
   if (n <= 0) return;
   const int waves_per_block = B1_THREADS / NKP_WAVE;
   hipLaunchKernelGGL (dense_matvec_kernel, dim3 ((n + waves_per_block - 1) / waves_per_block), dim3 (B1_THREADS), 0, st, Minv, x, y, n);
}
