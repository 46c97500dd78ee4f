// The lane-per-column layout of the factored column blocks: col_plan (col_plan.cpp) decides the kernel family and forms the
// groups on the host; here its tables go to the device, the factors are transposed into [diagonal][step k][lane] per group, and
// the family's kernels are opted in to the LDS they need.  nkp_refactor repacks new factors into the same layout.
#include "colblock_impl.h"

#include <algorithm>
#include <vector>

__global__ __launch_bounds__ (NKP_WAVE)
void colblock_transpose_kernel (const int *__restrict__ blk_start, const int *__restrict__ grp_b0, const int *__restrict__ grp_nb,
                                const int *__restrict__ grp_maxlen, const long long *__restrict__ grp_base, int ndiag, int64_t n,
                                const double *__restrict__ fac, double *__restrict__ fac_t, int gw, float *__restrict__ fac_tf, int pack,
                                const int *__restrict__ grp_cols /* NULL: the group is the nb consecutive columns from b0 */)
{
   const int g = blockIdx.x;
   const int lane = threadIdx.x;
   const int b0 = grp_b0[g], nb = grp_nb[g], ml = grp_maxlen[g];
   const long long base = grp_base[g];
   int r0 = 0, len = 0;
   if (lane < nb) {
      const int col = grp_cols ? grp_cols[g * gw + lane] : b0 + lane;
      r0 = blk_start[col];
      len = blk_start[col + 1] - r0;
   }
   if (lane >= gw) return;
   for (int d = 0; d < ndiag; d++)
      for (int k = 0; k < ml; k++)
      {
         const double v = (k < len) ? fac[(int64_t) d * n + r0 + k] : 0.0;
         // pack > 1 (colblock_apply_ldspack_kernel): `pack` consecutive steps of one column side by side, one 16-byte load
         const int64_t at = pack > 1 ? base + (((int64_t) d * (ml / pack) + k / pack) * gw + lane) * pack + (k % pack) : base + ((int64_t) d * ml + k) * gw + lane;
         if (fac_tf) fac_tf[at] = (float) v;
         else fac_t[at] = v;
      }
}

template <class T>
static int up (T **dst, const std::vector<T> &src, size_t *bytes)
{
   void *q = nullptr;
   const size_t b = (src.size () ? src.size () : 1) * sizeof (T);
   hipError_t e = hipMalloc (&q, b);
   if (e != hipSuccess) return (int) e;
   if (!src.empty ()) {
      e = hipMemcpy (q, src.data (), src.size () * sizeof (T), hipMemcpyHostToDevice);
      if (e != hipSuccess) { (void) hipFree (q); return (int) e; }
   }
   *dst = (T *) q;
   *bytes += b;
   return 0;
}

static const int PACK_STEPS = 4;      // COL_LDSPACK: consecutive steps of a column side by side in the factor array

static void transpose_factors (const ColBlocksDev &B, const int *d_gcols, hipStream_t st)
{
   hipLaunchKernelGGL (colblock_transpose_kernel, dim3 (B.ngrp), dim3 (NKP_WAVE), 0, st, B.blk_start, B.grp_b0, B.grp_nb, B.grp_maxlen,
                       B.grp_base, 2 * B.P + 1, B.n, B.fac, B.fac_t, B.gw, B.fac_tf, B.kern.family == COL_LDSPACK ? PACK_STEPS : 1, d_gcols);
}

int colblock_build_lane_layout (ColBlocksDev &B, const int *h_blk_start, const int *ranges, int nranges,
                                int *grp_first, size_t *device_bytes, hipStream_t st, int f32, const int *h_rowptr)
{
   ColPlanInput in;
   in.P = B.P; in.max_len = B.max_len; in.dropped = B.dropped; in.f32 = f32;
   in.h_blk_start = h_blk_start; in.ranges = ranges; in.nranges = nranges; in.h_rowptr = h_rowptr;
   in.ncol = B.ml_level ? B.nblk : -1;
   ColPlan pl;
   if (col_plan (in, B.tune ? *B.tune : nkp_builtin_tuning (), pl)) return (int) hipErrorInvalidValue;
   std::copy (pl.grp_first.begin (), pl.grp_first.end (), grp_first);
   B.kern = pl.kern;
   B.gw = pl.gw; B.stream = pl.stream; B.ldsres = pl.ldsres; B.ngrp = pl.ngrp;
   B.rhs_slots = pl.rhs_slots; B.lds_doubles = pl.lds_doubles; B.gs_ok = pl.gs_ok; B.gs_lds_bytes = pl.gs_lds_bytes;
   int rc;
   if (!pl.gs_rb_ptr.empty () && ((rc = up (&B.gs_rb_ptr, pl.gs_rb_ptr, device_bytes)) || (rc = up (&B.gs_rb, pl.gs_rb, device_bytes)))) return rc;
   if ((rc = up (&B.grp_b0, pl.grp_b0, device_bytes)) || (rc = up (&B.grp_nb, pl.grp_nb, device_bytes)) || (rc = up (&B.grp_maxlen, pl.grp_maxlen, device_bytes)) ||
       (rc = up (&B.grp_base, pl.grp_base, device_bytes)) || (rc = up (&B.grp_row0, pl.grp_row0, device_bytes)) || (rc = up (&B.col_slot, pl.col_slot, device_bytes)))
      return rc;
   if (pl.kern.lane_fused && (rc = up (&B.grp_tile, pl.grp_tile, device_bytes))) return rc;
   B.grp_tile_cnt = pl.ntile;
   void *q = nullptr;
   const size_t fsz = f32 ? sizeof (float) : sizeof (double);
   hipError_t e = hipMalloc (&q, (size_t) (pl.fac_total ? pl.fac_total : 1) * fsz);
   if (e != hipSuccess) return (int) e;
   if (f32) B.fac_tf = (float *) q;
   else B.fac_t = (double *) q;
   *device_bytes += (size_t) pl.fac_total * fsz;
   // sorted groups: the transpose reads the lanes' columns from a temporary device copy; the host keeps the list for nkp_refactor
   int *d_gcols = nullptr;
   if (pl.sorted && (rc = up (&d_gcols, pl.grp_cols, device_bytes))) return rc;
   if (B.ngrp) transpose_factors (B, d_gcols, st);
   if (d_gcols) {
      (void) hipStreamSynchronize (st);
      (void) hipFree (d_gcols);
      *device_bytes -= pl.grp_cols.size () * sizeof (int);
   }
   if (pl.sorted) B.grp_cols = new std::vector<int> (std::move (pl.grp_cols));
   const int lds_bytes = B.lds_doubles * (int) sizeof (double);
   if (lds_bytes > COL_LDS_DEFAULT_BYTES) {
      colblock_lanes_opt_in (lds_bytes);
      colblock_stream_opt_in (lds_bytes);
      colblock_ldsres_opt_in (lds_bytes);
      colblock_ldspack_opt_in (lds_bytes);
   }
   return (int) hipStreamSynchronize (st);
}

int colblock_repack_lane_layout (const ColBlocksDev &B, const int *d_gcols, hipStream_t st)
{
   if (B.ngrp == 0 || !(B.fac_t || B.fac_tf)) return 0;
   transpose_factors (B, d_gcols, st);
   return (int) hipGetLastError ();
}
