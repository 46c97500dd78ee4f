// ================================================================ lane-per-column apply
// The wave-per-column substitution (colblock.hip) is VALU-issue bound: 2*len dependent steps of
// readlane + predicated FMA per column (rocprof: 137 us per half sweep at 1 degree against ~25 us
// of HBM time).  Here one LANE owns one column: a wave stages the right-hand side of 64
// consecutive columns (a contiguous row range) into LDS with coalesced loads, every lane then
// runs its own short recurrence with the factors stored [diagonal][step k][lane] so that each
// step is one coalesced 512-byte load per diagonal, and the result goes back coalesced.
// 64x fewer wave-instructions per column; same operation order as the sequential kernel and
// the CPU restatement used by the tests, so results are bit-identical.
#include "colblock_impl.h"

// WPE is the least number of waves per SIMD the register allocation has to leave room for; 1 asks for nothing.  Only the
// 80-level instantiations (65-80 rows per column) are launched with 3, as <*, 80, *, 3>: left alone the compiler spends all
// 256 VGPRs on hoisted factor reads and ONE wave per SIMD remains -- 0.25 degree x 80: 1120 us per colour of the fine level
// (1 TB/s); capped it spills 56 registers of a kernel in which 8 lanes compute and runs three waves per SIMD: 619 us, whole
// cycle 32.8 -> 24.9 ms, same bits.  The cap HURTS the 64-level kernel (3 degree: 16.1 -> 25.5 us) and the streamed kernel
// (26 -> 94 us), so no other instantiation gets it.  The attribute takes the template parameter, so the text exists once and
// <*, *, *, 1> compiles to what the kernel without the attribute does.
template <int P, int MAXL, class FT, int WPE = 1>
__global__ __launch_bounds__ (NKP_WAVE) __attribute__ ((amdgpu_waves_per_eu (WPE)))
void colblock_apply_lanes_kernel (const int *__restrict__ blk_start, const int *__restrict__ grp_b0, const int *__restrict__ grp_nb,
                                  const int *__restrict__ grp_maxlen, const long long *__restrict__ grp_base, int g_first,
                                  const FT *__restrict__ fac_t, const double *__restrict__ rhs, double *__restrict__ z, int accumulate,
                                  int gw, int rhs_slots, const int *__restrict__ grp_row0, const int *__restrict__ col_slot, int ngrp)
{
   extern __shared__ double lds[];            // [rhs_slots] staged right-hand side | [(2P+1)*ml*gw] the group's factors
   const int g = blockIdx.x + g_first;
   const int lane = threadIdx.x;
   // every index this wave needs depends on g alone: one round trip, not a chain through blk_start
   const int nb = grp_nb[g], ml = grp_maxlen[g];
   const int R0 = grp_row0[g], nrows = grp_row0[ngrp + g];
   int s_pre = 0, len_pre = 0;
   if (lane < gw) { s_pre = col_slot[g * gw + lane]; len_pre = col_slot[(ngrp + g) * gw + lane]; }
   FT *fl = reinterpret_cast<FT *> (lds + rhs_slots);
   // the accumulate target is requested together with the right-hand side
   double tz[8];
#pragma unroll
   for (int u = 0; u < 8; u++) {
      const int i = lane + u * NKP_WAVE;
      tz[u] = (accumulate && i < nrows) ? z[(int64_t) R0 + i] : 0.0;
   }
   // bulk, fully coalesced staging: every load is independent, so the whole group is in flight at once
   {
      // 16-byte units of the group's factor block (ml*gw is a multiple of 64, so this is exact for f32 too)
      const double2 *src = reinterpret_cast<const double2 *> (fac_t + grp_base[g]);
      double2 *dst = reinterpret_cast<double2 *> (fl);
      const int cnt2 = (int) (((size_t) (2 * P + 1) * ml * gw * sizeof (FT)) >> 4);
      // the right-hand side and a batch of 20 factor loads per lane are all in flight before the first LDS
      // store waits on them (a group of 8 columns x 64 levels x 5 diagonals is exactly one batch)
      double tr[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
         const int i = lane + u * NKP_WAVE;
         tr[u] = (i < nrows) ? rhs[(int64_t) R0 + i] : 0.0;
      }
      constexpr int BATCH = sizeof (FT) == 4 ? 10 : 20;      // 16-byte loads per lane: one batch covers 8 x 64 x 5 factors
      for (int i0 = lane; i0 < cnt2; i0 += BATCH * NKP_WAVE) {
         double2 t[BATCH];
#pragma unroll
         for (int u = 0; u < BATCH; u++) {
            const int i = i0 + u * NKP_WAVE;
            t[u] = (i < cnt2) ? src[i] : make_double2 (0.0, 0.0);
         }
#pragma unroll
         for (int u = 0; u < BATCH; u++) {
            const int i = i0 + u * NKP_WAVE;
            if (i < cnt2) dst[i] = t[u];
         }
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
         const int i = lane + u * NKP_WAVE;
         if (i < nrows) lds[LDS_PAD (i)] = tr[u];
      }
   }
   for (int i = lane + 8 * NKP_WAVE; i < nrows; i += NKP_WAVE) lds[LDS_PAD (i)] = rhs[(int64_t) R0 + i];
   __syncthreads ();

   if (lane < nb) {
      const int s = s_pre;
      const int len = len_pre;
      const FT *ft = fl + lane;
      const int dstride = ml * gw;
      // the whole column lives in registers: no LDS write sits between two LDS reads, so the compiler
      // can keep the (read-only) factor reads in flight ahead of the dependent arithmetic
      double v[MAXL];
#pragma unroll
      for (int k = 0; k < MAXL; k++) v[k] = (k < len) ? lds[LDS_PAD (s + k)] : 0.0;
      // forward: y_k = ((r_k - l(k,k-P) y_{k-P}) ... - l(k,k-1) y_{k-1})   (far diagonal first, like the column sweep)
      // steps k >= len need no predicate: their factors are zero-padded, so they compute 0 - 0*x = 0;
      // the only branch left is wave-uniform (k < ml), which keeps the LDS reads hoistable
      // ml is a multiple of 8 (layout builder), so the only branch is one wave-uniform test per 8 steps and
      // the 8*P factor reads of a chunk are issued together, ahead of the dependent arithmetic
#pragma unroll
      for (int k0 = 0; k0 < MAXL; k0 += 8) {
         if (k0 < ml) {
#pragma unroll
            for (int k = k0; k < k0 + 8; k++) {
               double y = v[k];
#pragma unroll
               for (int q = P; q >= 1; q--)
                  if (k - q >= 0) y -= (double) ft[(P - q) * dstride + k * gw] * v[k - q];
               v[k] = y;
            }
         }
      }
      // backward: x_k = (((y_k - u(k,k+P) x_{k+P}) ... - u(k,k+1) x_{k+1}) * (1/u_kk)
#pragma unroll
      for (int k0 = MAXL - 8; k0 >= 0; k0 -= 8) {
         if (k0 < ml) {
#pragma unroll
            for (int k = k0 + 7; k >= k0; k--) {
               double x = v[k];
#pragma unroll
               for (int q = P; q >= 1; q--)
                  if (k + q < MAXL) x -= (double) ft[(P + q) * dstride + k * gw] * v[k + q];
               x *= (double) ft[P * dstride + k * gw];
               v[k] = x;
            }
         }
      }
#pragma unroll
      for (int k = 0; k < MAXL; k++)
         if (k < len) lds[LDS_PAD (s + k)] = v[k];
   }
   __syncthreads ();
   if (accumulate) {
#pragma unroll
      for (int u = 0; u < 8; u++) {
         const int i = lane + u * NKP_WAVE;
         if (i < nrows) z[(int64_t) R0 + i] = tz[u] + lds[LDS_PAD (i)];
      }
      for (int i = lane + 8 * NKP_WAVE; i < nrows; i += NKP_WAVE) z[(int64_t) R0 + i] += lds[LDS_PAD (i)];
   } else
      for (int i = lane; i < nrows; i += NKP_WAVE) z[(int64_t) R0 + i] = lds[LDS_PAD (i)];
}

// ================================================================ lane-per-column apply, 64 columns per wave, factors streamed
// The 8-columns-per-wave kernel above keeps 56 of 64 lanes idle during the substitution and stages the factors through
// LDS, which caps a CU at 11 waves; all of them load, then all of them compute, and HBM idles during the compute phase
// (1 degree fine level: 44 us per colour for 93 MB = 2.1 TB/s).  Here a wave owns GW = 32 (or 64) columns: only the
// right-hand side goes through LDS (coalesced staging of the group's contiguous rows), every lane below GW runs its own
// substitution, and each step reads its factors straight from HBM/L2 as ONE coalesced 128- or 256-byte load per diagonal
// ([diag][k][lane] layout) that the unrolled code requests many steps ahead (244 VGPRs: two waves per SIMD, all waves of
// a colour resident at once).  Same operations in the same order => same bits as the other kernels.
template <int P, int MAXL, class FT, int GW>
__global__ __launch_bounds__ (NKP_WAVE)
void colblock_apply_stream_kernel (const int *__restrict__ grp_nb, const int *__restrict__ grp_maxlen, const long long *__restrict__ grp_base, int g_first,
                                   const FT *__restrict__ fac_t, const double *__restrict__ rhs, double *__restrict__ z, int accumulate,
                                   const int *__restrict__ grp_row0, const int *__restrict__ col_slot, int ngrp)
{
   extern __shared__ double lds[];            // the group's right-hand side, then its solution
   constexpr int gw = GW;
   const int g = blockIdx.x + g_first;
   const int lane = threadIdx.x;
   const int nb = grp_nb[g], ml = grp_maxlen[g];
   const int R0 = grp_row0[g], nrows = grp_row0[ngrp + g];
   int s = 0, len = 0;
   if (lane < gw) { s = col_slot[g * gw + lane]; len = col_slot[(ngrp + g) * gw + lane]; }
   const FT *ft = fac_t + grp_base[g] + lane;
   const int dstride = ml * gw;
   for (int i0 = lane; i0 < nrows; i0 += 8 * NKP_WAVE) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; u++) t[u] = (i0 + u * NKP_WAVE < nrows) ? rhs[(int64_t) R0 + i0 + u * NKP_WAVE] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; u++)
         if (i0 + u * NKP_WAVE < nrows) lds[LDS_PAD (i0 + u * NKP_WAVE)] = t[u];
   }
   __syncthreads ();
   if (lane < nb) {
      double v[MAXL];
#pragma unroll
      for (int k = 0; k < MAXL; k++) v[k] = (k < len) ? lds[LDS_PAD (s + k)] : 0.0;
#pragma unroll
      for (int k0 = 0; k0 < MAXL; k0 += 8) {
         if (k0 < ml) {
#pragma unroll
            for (int k = k0; k < k0 + 8; k++) {
               double y = v[k];
#pragma unroll
               for (int q = P; q >= 1; q--)
                  if (k - q >= 0) y -= (double) ft[(P - q) * dstride + k * gw] * v[k - q];
               v[k] = y;
            }
         }
      }
#pragma unroll
      for (int k0 = MAXL - 8; k0 >= 0; k0 -= 8) {
         if (k0 < ml) {
#pragma unroll
            for (int k = k0 + 7; k >= k0; k--) {
               double x = v[k];
#pragma unroll
               for (int q = P; q >= 1; q--)
                  if (k + q < MAXL) x -= (double) ft[(P + q) * dstride + k * gw] * v[k + q];
               x *= (double) ft[P * dstride + k * gw];
               v[k] = x;
            }
         }
      }
#pragma unroll
      for (int k = 0; k < MAXL; k++)
         if (k < len) lds[LDS_PAD (s + k)] = v[k];
   }
   __syncthreads ();
   if (accumulate)
      for (int i = lane; i < nrows; i += NKP_WAVE) z[(int64_t) R0 + i] += lds[LDS_PAD (i)];
   else
      for (int i = lane; i < nrows; i += NKP_WAVE) z[(int64_t) R0 + i] = lds[LDS_PAD (i)];
}


// ================================================================ lane-per-column apply, 32 columns per wave, column resident in LDS
// The streamed kernel above keeps the whole column in registers (2 VGPRs per level): at 80 levels nothing is left for
// loads in flight and it loses to the small-group kernel, which in turn runs at a fifth of the HBM peak there.  Here the
// column stays in LDS, where the right-hand side is staged anyway: a substitution step reads its right-hand side from LDS
// and writes its result back, the registers hold only the P previous values and TWO chunks of CH steps' factors -- the
// chunk being consumed and the next one, requested before the current one is used -- so the register count does not
// depend on the column length.  Same operations in the same order as the other kernels => same bits.
template <int P, int CH, class FT>
struct FacChunk { FT f[P + 1][CH]; };

template <int P, int CH, class FT>
__device__ __forceinline__ void load_fwd (FacChunk<P, CH, FT> &c, const FT *__restrict__ ft, int dstride, int k0, int gw)
{
#pragma unroll
   for (int q = 1; q <= P; q++)
#pragma unroll
      for (int j = 0; j < CH; j++) c.f[q - 1][j] = ft[(P - q) * dstride + (k0 + j) * gw];
}

template <int P, int CH, class FT>
__device__ __forceinline__ void load_bwd (FacChunk<P, CH, FT> &c, const FT *__restrict__ ft, int dstride, int k0, int gw)
{
#pragma unroll
   for (int q = 0; q <= P; q++)
#pragma unroll
      for (int j = 0; j < CH; j++) c.f[q][j] = ft[(P + q) * dstride + (k0 + j) * gw];
}

// steps k0 .. k0 + CH - 1 of the forward substitution; w[q - 1] = y_{k - q} on entry and on exit
template <int P, int CH, class FT>
__device__ __forceinline__ void step_fwd (const FacChunk<P, CH, FT> &c, double *lds, int s, int len, int k0, double (&w)[P])
{
   double b[CH];
#pragma unroll
   for (int j = 0; j < CH; j++) b[j] = (k0 + j < len) ? lds[LDS_PAD (s + k0 + j)] : 0.0;
#pragma unroll
   for (int j = 0; j < CH; j++) {
      double y = b[j];
#pragma unroll
      for (int q = P; q >= 1; q--)
         if (k0 + j - q >= 0) y -= (double) c.f[q - 1][j] * w[q - 1];
#pragma unroll
      for (int q = P - 1; q >= 1; q--) w[q] = w[q - 1];
      w[0] = y;
      if (k0 + j < len) lds[LDS_PAD (s + k0 + j)] = y;
   }
}

// steps k0 + CH - 1 .. k0 of the back substitution; u[q - 1] = x_{k + q}
template <int P, int CH, class FT>
__device__ __forceinline__ void step_bwd (const FacChunk<P, CH, FT> &c, double *lds, int s, int len, int k0, double (&u)[P])
{
   double y[CH];
#pragma unroll
   for (int j = 0; j < CH; j++) y[j] = (k0 + j < len) ? lds[LDS_PAD (s + k0 + j)] : 0.0;
#pragma unroll
   for (int j = CH - 1; j >= 0; j--) {
      double x = y[j];
#pragma unroll
      for (int q = P; q >= 1; q--) x -= (double) c.f[q][j] * u[q - 1];
      x *= (double) c.f[0][j];
#pragma unroll
      for (int q = P - 1; q >= 1; q--) u[q] = u[q - 1];
      u[0] = x;
      if (k0 + j < len) lds[LDS_PAD (s + k0 + j)] = x;
   }
}

template <int P, class FT, int CH, bool EARLY>
__global__ __launch_bounds__ (NKP_WAVE)
void colblock_apply_ldsres_kernel (const int *__restrict__ grp_nb, const int *__restrict__ grp_maxlen, const long long *__restrict__ grp_base, int g_first,
                                   const FT *__restrict__ fac_t, const double *__restrict__ rhs, double *__restrict__ z, int accumulate,
                                   const int *__restrict__ grp_row0, const int *__restrict__ col_slot, int ngrp)
{
   extern __shared__ double lds[];            // the group's right-hand side, then its solution
   constexpr int gw = 32;
   const int g = blockIdx.x + g_first;
   const int lane = threadIdx.x;
   const int nb = grp_nb[g], ml = grp_maxlen[g];            // ml is a multiple of CH (layout built for this kernel)
   const int R0 = grp_row0[g], nrows = grp_row0[ngrp + g];
   int s = 0, len = 0;
   if (lane < gw) { s = col_slot[g * gw + lane]; len = col_slot[(ngrp + g) * gw + lane]; }
   const FT *ft = fac_t + grp_base[g] + lane;
   const int dstride = ml * gw;
   FacChunk<P, CH, FT> A, B, C;
   // EARLY: the first factor chunk of either sweep is requested before the right-hand side is staged, so the two round trips
   // overlap instead of following each other (the lanes of columns that do not exist read zero-padded factors)
   if (EARLY && lane < gw) {
      load_fwd<P, CH, FT> (A, ft, dstride, 0, gw);
      load_bwd<P, CH, FT> (C, ft, dstride, ml - CH, gw);
   }
   double tz[8];
   if (EARLY && accumulate) {
#pragma unroll
      for (int u = 0; u < 8; u++) tz[u] = (lane + u * NKP_WAVE < nrows) ? z[(int64_t) R0 + lane + u * NKP_WAVE] : 0.0;
   }
   for (int i0 = lane; i0 < nrows; i0 += 8 * NKP_WAVE) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; u++) t[u] = (i0 + u * NKP_WAVE < nrows) ? rhs[(int64_t) R0 + i0 + u * NKP_WAVE] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; u++)
         if (i0 + u * NKP_WAVE < nrows) lds[LDS_PAD (i0 + u * NKP_WAVE)] = t[u];
   }
   __syncthreads ();
   if (lane < nb) {
      double w[P];
#pragma unroll
      for (int q = 0; q < P; q++) w[q] = 0.0;
      if (!EARLY) load_fwd<P, CH, FT> (A, ft, dstride, 0, gw);
      for (int k0 = 0; k0 < ml; k0 += 2 * CH) {
         const bool more = k0 + CH < ml;
         if (more) load_fwd<P, CH, FT> (B, ft, dstride, k0 + CH, gw);
         step_fwd<P, CH, FT> (A, lds, s, len, k0, w);
         if (more) {
            if (k0 + 2 * CH < ml) load_fwd<P, CH, FT> (A, ft, dstride, k0 + 2 * CH, gw);
            step_fwd<P, CH, FT> (B, lds, s, len, k0 + CH, w);
         }
      }
#pragma unroll
      for (int q = 0; q < P; q++) w[q] = 0.0;
      if (!EARLY) load_bwd<P, CH, FT> (C, ft, dstride, ml - CH, gw);
      // the back substitution walks the chunks C, then B / A alternately
      int k0 = ml - CH;
      if (k0 - CH >= 0) load_bwd<P, CH, FT> (B, ft, dstride, k0 - CH, gw);
      step_bwd<P, CH, FT> (C, lds, s, len, k0, w);
      for (k0 -= CH; k0 >= 0; k0 -= 2 * CH) {
         const bool more = k0 - CH >= 0;
         if (more) load_bwd<P, CH, FT> (A, ft, dstride, k0 - CH, gw);
         step_bwd<P, CH, FT> (B, lds, s, len, k0, w);
         if (more) {
            if (k0 - 2 * CH >= 0) load_bwd<P, CH, FT> (B, ft, dstride, k0 - 2 * CH, gw);
            step_bwd<P, CH, FT> (A, lds, s, len, k0 - CH, w);
         }
      }
   }
   __syncthreads ();
   if (accumulate) {
      if (EARLY) {
#pragma unroll
         for (int u = 0; u < 8; u++) {
            const int i = lane + u * NKP_WAVE;
            if (i < nrows) z[(int64_t) R0 + i] = tz[u] + lds[LDS_PAD (i)];
         }
         for (int i = lane + 8 * NKP_WAVE; i < nrows; i += NKP_WAVE) z[(int64_t) R0 + i] += lds[LDS_PAD (i)];
      } else
         for (int i = lane; i < nrows; i += NKP_WAVE) z[(int64_t) R0 + i] += lds[LDS_PAD (i)];
   } else
      for (int i = lane; i < nrows; i += NKP_WAVE) z[(int64_t) R0 + i] = lds[LDS_PAD (i)];
}

// Software-pipelined variant for the common shape (f32 factors, columns of at most 64 levels, 8 columns per wave,
// half bandwidth <= 2).  SQ counters on colblock_apply_lanes_kernel: a wave lives ~14 us, 46 % of it parked on
// the staging loads, and LDS (14.5 KB per wave) caps a CU at 11 waves.  Here a persistent wave walks groups g,
// g + gridDim.x, ...: it commits the prefetched registers of group i to LDS, requests group i+1 (index words, then
// right-hand side, accumulate target and the factor block: 26 registers of loads in flight) and only then runs group
// i's recurrence, so the HBM latency hides under arithmetic.  Same arithmetic in the same order => same bits.
#define LANES_PIPE_BATCH 10
template <int P>
__global__ __launch_bounds__ (NKP_WAVE)
void colblock_apply_lanes_pipe_kernel (const int *__restrict__ grp_nb, const int *__restrict__ grp_maxlen, const long long *__restrict__ grp_base,
                                       int g_first, int g_end, const float *__restrict__ fac_t, const double *__restrict__ rhs,
                                       double *__restrict__ z, int accumulate, int rhs_slots, const int *__restrict__ grp_row0,
                                       const int *__restrict__ col_slot, int ngrp)
{
   extern __shared__ double lds[];
   constexpr int gw = 8, MAXL = 64;
   float *fl = reinterpret_cast<float *> (lds + rhs_slots);
   const int lane = threadIdx.x;
   int g = g_first + (int) blockIdx.x;
   if (g >= g_end) return;

   int n_nb, n_ml, n_R0, n_nrows, n_s, n_len;
   double n_tz[8], n_tr[8];
   double2 n_t[LANES_PIPE_BATCH];
#define LANES_PREFETCH(GG)                                                                            \
   do {                                                                                               \
      n_nb = grp_nb[GG];                                                                              \
      n_ml = grp_maxlen[GG];                                                                          \
      n_R0 = grp_row0[GG];                                                                            \
      n_nrows = grp_row0[ngrp + (GG)];                                                                \
      n_s = n_len = 0;                                                                                \
      if (lane < gw) { n_s = col_slot[(GG) * gw + lane]; n_len = col_slot[(ngrp + (GG)) * gw + lane]; } \
      _Pragma ("unroll")                                                                              \
      for (int u = 0; u < 8; u++) {                                                                   \
         const int i = lane + u * NKP_WAVE;                                                           \
         n_tz[u] = (accumulate && i < n_nrows) ? z[(int64_t) n_R0 + i] : 0.0;                         \
         n_tr[u] = (i < n_nrows) ? rhs[(int64_t) n_R0 + i] : 0.0;                                     \
      }                                                                                               \
      {                                                                                               \
         const double2 *src_ = reinterpret_cast<const double2 *> (fac_t + grp_base[GG]);              \
         const int cnt2_ = (int) (((size_t) (2 * P + 1) * n_ml * gw * sizeof (float)) >> 4);          \
         _Pragma ("unroll")                                                                           \
         for (int u = 0; u < LANES_PIPE_BATCH; u++) {                                                 \
            const int i = lane + u * NKP_WAVE;                                                        \
            n_t[u] = (i < cnt2_) ? src_[i] : make_double2 (0.0, 0.0);                                 \
         }                                                                                            \
      }                                                                                               \
   } while (0)

   LANES_PREFETCH (g);
   for (;;) {
      // commit the prefetched group to LDS; it becomes the current one
      const int nb = n_nb, ml = n_ml, R0 = n_R0, nrows = n_nrows, s = n_s, len = n_len;
      double tz[8];
      {
         double2 *dst = reinterpret_cast<double2 *> (fl);
         const int cnt2 = (int) (((size_t) (2 * P + 1) * ml * gw * sizeof (float)) >> 4);
#pragma unroll
         for (int u = 0; u < LANES_PIPE_BATCH; u++) {
            const int i = lane + u * NKP_WAVE;
            if (i < cnt2) dst[i] = n_t[u];
         }
#pragma unroll
         for (int u = 0; u < 8; u++) {
            const int i = lane + u * NKP_WAVE;
            tz[u] = n_tz[u];
            if (i < nrows) lds[LDS_PAD (i)] = n_tr[u];
         }
      }
      __syncthreads ();
      const int gn = g + (int) gridDim.x;
      const bool have_next = gn < g_end;
      if (have_next) LANES_PREFETCH (gn);

      if (lane < nb) {
         const float *ft = fl + lane;
         const int dstride = ml * gw;
         double v[MAXL];
#pragma unroll
         for (int k = 0; k < MAXL; k++) v[k] = (k < len) ? lds[LDS_PAD (s + k)] : 0.0;
#pragma unroll
         for (int k0 = 0; k0 < MAXL; k0 += 8) {
            if (k0 < ml) {
#pragma unroll
               for (int k = k0; k < k0 + 8; k++) {
                  double y = v[k];
#pragma unroll
                  for (int q = P; q >= 1; q--)
                     if (k - q >= 0) y -= (double) ft[(P - q) * dstride + k * gw] * v[k - q];
                  v[k] = y;
               }
            }
         }
#pragma unroll
         for (int k0 = MAXL - 8; k0 >= 0; k0 -= 8) {
            if (k0 < ml) {
#pragma unroll
               for (int k = k0 + 7; k >= k0; k--) {
                  double x = v[k];
#pragma unroll
                  for (int q = P; q >= 1; q--)
                     if (k + q < MAXL) x -= (double) ft[(P + q) * dstride + k * gw] * v[k + q];
                  x *= (double) ft[P * dstride + k * gw];
                  v[k] = x;
               }
            }
         }
#pragma unroll
         for (int k = 0; k < MAXL; k++)
            if (k < len) lds[LDS_PAD (s + k)] = v[k];
      }
      __syncthreads ();
#pragma unroll
      for (int u = 0; u < 8; u++) {
         const int i = lane + u * NKP_WAVE;
         if (i < nrows) z[(int64_t) R0 + i] = accumulate ? tz[u] + lds[LDS_PAD (i)] : lds[LDS_PAD (i)];
      }
      __syncthreads ();          // the LDS image is free again
      if (!have_next) break;
      g = gn;
   }
#undef LANES_PREFETCH
}

// ================================================================ selection, opt-in, launch
// with_<family>_kernel: f (kernel, (const FT *) nullptr) for the instantiation the arguments name, FT its factor storage.  The
// launcher passes the level's values (B.kern: col_plan.cpp chose them), the family's opt-in routine walks the same lists.
template <class F>
static void with_lanes_kernel (int P, int maxl, int wpe, bool f32, F &&f)
{
   with_band (P, [&] (auto p) {
      with_int<64, 80, 128> (maxl, [&] (auto ml) {
         with_int<1, 3> (wpe, [&] (auto w) {
            with_bool (f32, [&] (auto s) {
               using FT = std::conditional_t<decltype (s)::value, float, double>;
               constexpr int ML = decltype (ml)::value, WPE = decltype (w)::value;
               if constexpr ((ML == 80) == (WPE == 3)) f (colblock_apply_lanes_kernel<decltype (p)::value, ML, FT, WPE>, (const FT *) nullptr);
            });
         });
      });
   });
}

template <class F>
static void with_stream_kernel (int P, int gw, bool f32, F &&f)
{
   with_band (P, [&] (auto p) {
      with_int<32, 64> (gw, [&] (auto g) {
         with_bool (f32, [&] (auto s) {
            using FT = std::conditional_t<decltype (s)::value, float, double>;
            f (colblock_apply_stream_kernel<decltype (p)::value, 64, FT, decltype (g)::value>, (const FT *) nullptr);
         });
      });
   });
}

template <class F>
static void with_ldsres_kernel (int P, bool early, bool f32, F &&f)
{
   with_band (P, [&] (auto p) {
      with_bool (early, [&] (auto e) {
         with_bool (f32, [&] (auto s) {
            using FT = std::conditional_t<decltype (s)::value, float, double>;
            f (colblock_apply_ldsres_kernel<decltype (p)::value, FT, NKP_LDSRES_CH, decltype (e)::value>, (const FT *) nullptr);
         });
      });
   });
}

void colblock_lanes_opt_in (int lds_bytes)
{
   const auto opt_in = [&] (auto kernel, auto) { colblock_opt_in ((const void *) kernel, lds_bytes); };
   static const int shapes[3][2] = { { 64, 1 }, { 80, 3 }, { 128, 1 } };      // MAXL, WPE
   for (int P : { 1, 2, 4 })
      for (const auto &mw : shapes)
         for (bool f32 : { false, true }) with_lanes_kernel (P, mw[0], mw[1], f32, opt_in);
}

void colblock_stream_opt_in (int lds_bytes)
{
   const auto opt_in = [&] (auto kernel, auto) { colblock_opt_in ((const void *) kernel, lds_bytes); };
   for (int P : { 1, 2, 4 })
      for (int gw : { 32, 64 })
         for (bool f32 : { false, true }) with_stream_kernel (P, gw, f32, opt_in);
}

void colblock_ldsres_opt_in (int lds_bytes)
{
   const auto opt_in = [&] (auto kernel, auto) { colblock_opt_in ((const void *) kernel, lds_bytes); };
   for (int P : { 1, 2, 4 })
      for (bool early : { false, true })
         for (bool f32 : { false, true }) with_ldsres_kernel (P, early, f32, opt_in);
}

static inline const float *factors (const ColBlocksDev &B, const float *) { return B.fac_tf; }
static inline const double *factors (const ColBlocksDev &B, const double *) { return B.fac_t; }

void launch_colblock_apply_lanes (const ColBlocksDev &B, int g0, int g1, const double *r, double *z, int accumulate, hipStream_t st)
{
   if (g1 <= g0) return;
   const size_t lds = (size_t) B.lds_doubles * sizeof (double);
   const bool f32 = B.fac_tf != nullptr;
   // the kernels that keep the factors out of LDS take one argument list
   const auto streamed = [&] (auto kernel, auto ft) {
      hipLaunchKernelGGL (kernel, dim3 (g1 - g0), dim3 (NKP_WAVE), lds, st, B.grp_nb, B.grp_maxlen, B.grp_base, g0, factors (B, ft), r, z, accumulate, B.grp_row0, B.col_slot, B.ngrp);
   };
   switch (B.kern.family) {
   case COL_LDSPACK: launch_colblock_apply_ldspack (B, g0, g1, r, z, accumulate, st); break;
   case COL_LDSRES: with_ldsres_kernel (B.P, B.kern.early, f32, streamed); break;
   case COL_STREAM: with_stream_kernel (B.P, B.gw, f32, streamed); break;
   default:
      if (B.kern.pipe_min > 0 && g1 - g0 >= B.kern.pipe_min) {
         int waves = 256 * 8;                         // two waves per SIMD fit the ~230 registers
         if (waves > (g1 - g0 + 1) / 2) waves = (g1 - g0 + 1) / 2;
         with_int<1, 2> (B.P, [&] (auto p) {
            hipLaunchKernelGGL ((colblock_apply_lanes_pipe_kernel<decltype (p)::value>), dim3 (waves), dim3 (NKP_WAVE), lds, st, B.grp_nb, B.grp_maxlen, B.grp_base, g0, g1,
                                B.fac_tf, r, z, accumulate, B.rhs_slots, B.grp_row0, B.col_slot, B.ngrp);
         });
      } else
         with_lanes_kernel (B.P, B.kern.maxl, B.kern.wpe, f32, [&] (auto kernel, auto ft) {
            hipLaunchKernelGGL (kernel, dim3 (g1 - g0), dim3 (NKP_WAVE), lds, st, B.blk_start, B.grp_b0, B.grp_nb, B.grp_maxlen, B.grp_base, g0, factors (B, ft), r, z,
                                accumulate, B.gw, B.rhs_slots, B.grp_row0, B.col_slot, B.ngrp);
         });
   }
}
