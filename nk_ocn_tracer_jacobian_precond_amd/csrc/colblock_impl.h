// What crosses the units of the lane-per-column band solves: col_layout.hip (layout), col_lanes.hip (lanes, pipelined, streamed
// and LDS-resident kernels; launch_colblock_apply_lanes), col_packed.hip (packed kernels), col_gs_fused.hip, col_gs_lanes.hip.  Private to them.
#pragma once
#include "nkp_dev.h"

// Dynamic LDS above COL_LDS_DEFAULT_BYTES needs an explicit opt-in: one routine per family, which walks the selector lists of
// the family's launcher, so that every instantiation the launcher can name is opted in for lds_bytes.
void colblock_lanes_opt_in (int lds_bytes);
void colblock_stream_opt_in (int lds_bytes);
void colblock_ldsres_opt_in (int lds_bytes);
void colblock_ldspack_opt_in (int lds_bytes);

// groups [g0, g1) of a level with the packed layout (B.kern.family == COL_LDSPACK), one right-hand side: the case of
// launch_colblock_apply_lanes that col_packed.hip serves
void launch_colblock_apply_ldspack (const ColBlocksDev &B, int g0, int g1, const double *r, double *z, int accumulate, hipStream_t st);

inline void colblock_opt_in (const void *kernel, int lds_bytes)
{
   (void) hipFuncSetAttribute (kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
}
