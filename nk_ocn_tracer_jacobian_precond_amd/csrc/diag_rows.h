// (L x) of one row per lane on an operator's per-column diagonals (CsrDev::dg_*, nkp_dev.h): the text that diag_residual_kernel,
// gs_wave_diag_kernel (diagop.hip) and gs_lanes_diag_kernel (col_gs_lanes.hip) share.  diagop.hip says what the groups are and
// why the loads are shaped like this.
#pragma once
#include "nkp_dev.h"

#define DG_GROUPS 3              // groups whose loads are in flight together (f64 values: 2 and 4 measured the same)

__device__ __forceinline__ double dg_lane_up (double w)
{
   // v_mov_b32_dpp wave_shl:1 -- lane i takes lane i + 1's, lane 63 keeps its own (bound_ctrl off); __shfl_down (w, 1), two
   // ds_bpermute_b32, measured no faster
   int lo = __double2loint (w), hi = __double2hiint (w);
   lo = __builtin_amdgcn_update_dpp (lo, lo, 0x130, 0xf, 0xf, false);
   hi = __builtin_amdgcn_update_dpp (hi, hi, 0x130, 0xf, 0xf, false);
   return __hiloint2double (hi, lo);
}

template <int U, class VT>
__device__ __forceinline__ void dg_vals (const VT *__restrict__ p, int len, int m, VT (&v)[DG_RUN_MAX])
{
   v[U] = p[(size_t) U * len];
   if constexpr (U + 1 < DG_RUN_MAX)
      if (m > U + 1) dg_vals<U + 1> (p, len, m, v);
}

template <int U, class VT>
__device__ __forceinline__ void dg_sums (const VT (&v)[DG_RUN_MAX], int m, double w, double &acc)
{
   acc += (double) v[U] * w;
   if constexpr (U + 1 < DG_RUN_MAX)
      if (m > U + 1) dg_sums<U + 1> (v, m, dg_lane_up (w), acc);
}

// TWO: the window of x comes from two buffers, position idx < split from x and the others from xb, chosen per lane by the
// clamped index (the fused half sweeps, which must not see their own colour's new values).
template <int G, class VT, bool TWO>
__device__ __forceinline__ void dg_step (const DgGroup *__restrict__ grp, const VT *__restrict__ val, const double *__restrict__ x, int len, int kl,
                                         int base, int n, double &acc, const double *__restrict__ xb, int split)
{
   VT v[G][DG_RUN_MAX];
   double w[G];
   int m[G];
   DgGroup R[G];
#pragma unroll
   for (int g = 0; g < G; g++) R[g] = grp[g];
#pragma unroll
   for (int g = 0; g < G; g++) {
      m[g] = R[g].slots >> 16;
      const int idx = min (max (R[g].key0 + base, 0), n - 1);
      if constexpr (TWO) w[g] = idx < split ? x[idx] : xb[idx];
      else w[g] = x[idx];
      dg_vals<0> (val + (size_t) (R[g].slots & 0xffff) * len + kl, len, m[g], v[g]);
   }
#pragma unroll
   for (int g = 0; g < G; g++) dg_sums<0> (v[g], m[g], w[g], acc);
}

// (L x) of the row a lane owns in tile T (lr = its row inside the tile, clamped to the tile's last row): all groups of the column
template <class VT, bool TWO>
__device__ __forceinline__ double dg_row_sum (const DgTile &T, const DgGroup *__restrict__ dg_grp, const VT *__restrict__ dg_val, int lane, int lr,
                                              const double *__restrict__ x, int n, const double *__restrict__ xb = nullptr, int split = 0)
{
   const int kl = T.kl0 + lr;
   const int base = T.kl0 + lane;
   const DgGroup *__restrict__ grp = dg_grp + T.g0;
   const VT *__restrict__ val = dg_val + T.voff;
   double acc = 0.0;
   int g = 0;
   for (; g + DG_GROUPS <= T.ng; g += DG_GROUPS) dg_step<DG_GROUPS, VT, TWO> (grp + g, val, x, T.len, kl, base, n, acc, xb, split);
   static_assert (DG_GROUPS == 3, "one case per length of the last step");
   switch (T.ng - g) {
      case 1: dg_step<1, VT, TWO> (grp + g, val, x, T.len, kl, base, n, acc, xb, split); break;
      case 2: dg_step<2, VT, TWO> (grp + g, val, x, T.len, kl, base, n, acc, xb, split); break;
      default: break;
   }
   return acc;
}
