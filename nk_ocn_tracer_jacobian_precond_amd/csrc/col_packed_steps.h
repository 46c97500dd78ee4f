// The packed factor chunks of the lane-per-column band solves (COL_LDSPACK: [diag][k / 4][lane][4], f32) and the substitution
// steps on a column's LDS slot: shared by the kernels of col_packed.hip, which keep the chunks in registers on a static
// schedule, and gs_lanes_diag_kernel (col_gs_lanes.hip), which reads them from an LDS copy of the group's block.
#pragma once
#include "colblock_impl.h"

// a chunk of 16 steps as it comes off the loads: one float4 per diagonal and 4 steps
template <int P>
struct PackChunk { float4 q[P + 1][4]; };

// keeps a loaded float4 as it is until this point of the program: without it the compiler converts every factor to f64
// right behind its load (twice the registers, and a wait for the load where it was meant to stay in flight)
__device__ __forceinline__ void ldsp_pin (float4 &v) { asm volatile ("" : "+v" (v.x), "+v" (v.y), "+v" (v.z), "+v" (v.w)); }

template <int P>
__device__ __forceinline__ void ldsp_load_fwd (PackChunk<P> &c, const float4 *__restrict__ f4, int mlq, int k0, int gw)
{
#pragma unroll
   for (int q = 1; q <= P; q++)
#pragma unroll
      for (int j4 = 0; j4 < 4; j4++) c.q[q - 1][j4] = f4[((int64_t) (P - q) * mlq + (k0 >> 2) + j4) * gw];
}

template <int P>
__device__ __forceinline__ void ldsp_load_bwd (PackChunk<P> &c, const float4 *__restrict__ f4, int mlq, int k0, int gw)
{
#pragma unroll
   for (int q = 0; q <= P; q++)
#pragma unroll
      for (int j4 = 0; j4 < 4; j4++) c.q[q][j4] = f4[((int64_t) (P + q) * mlq + (k0 >> 2) + j4) * gw];
}

__device__ __forceinline__ float ldsp_elem (const float4 &v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

// steps k0 .. k0 + 15 of the forward substitution; the column sits at col[0 .. ml) in LDS (zero beyond its length)
template <int P>
__device__ __forceinline__ void ldsp_step_fwd (PackChunk<P> &c, double *col, int k0, double (&w)[P])
{
   double b[16];
#pragma unroll
   for (int j = 0; j < 16; j++) b[j] = col[k0 + j];
#pragma unroll
   for (int j4 = 0; j4 < 4; j4++) {
#pragma unroll
      for (int q = 0; q < P; q++) ldsp_pin (c.q[q][j4]);
#pragma unroll
      for (int i = 0; i < 4; i++) {
         const int j = 4 * j4 + i;
         double y = b[j];
#pragma unroll
         for (int q = P; q >= 1; q--) y -= (double) ldsp_elem (c.q[q - 1][j4], i) * w[q - 1];     // steps before the column's first: w = 0
#pragma unroll
         for (int q = P - 1; q >= 1; q--) w[q] = w[q - 1];
         w[0] = y;
         col[k0 + j] = y;
      }
   }
}

// steps k0 + 15 .. k0 of the back substitution
template <int P>
__device__ __forceinline__ void ldsp_step_bwd (PackChunk<P> &c, double *col, int k0, double (&u)[P])
{
   double y[16];
#pragma unroll
   for (int j = 0; j < 16; j++) y[j] = col[k0 + j];
#pragma unroll
   for (int j4 = 3; j4 >= 0; j4--) {
#pragma unroll
      for (int q = 0; q <= P; q++) ldsp_pin (c.q[q][j4]);
#pragma unroll
      for (int i = 3; i >= 0; i--) {
         const int j = 4 * j4 + i;
         double x = y[j];
#pragma unroll
         for (int q = P; q >= 1; q--) x -= (double) ldsp_elem (c.q[q][j4], i) * u[q - 1];
         x *= (double) ldsp_elem (c.q[0][j4], i);
#pragma unroll
         for (int q = P - 1; q >= 1; q--) u[q] = u[q - 1];
         u[0] = x;
         col[k0 + j] = x;
      }
   }
}
