// ================================================================ one Gauss-Seidel half sweep of a lane-per-column level, one launch
// The levels between the wave-per-column end of the cycle and the bandwidth-bound fine level (1 degree: level 1, 24 k columns)
// ran every half sweep as two launches, each at its own latency floor: diag_residual_kernel (r = b - L x of the colour's rows)
// and colblock_apply_ldspack_kernel (x += M^-1 r).  Here a workgroup owns one packed group of 32 columns (COL_LDSPACK, col_plan.h)
// and does both: its GL_WAVES waves share the group's columns and compute their residual rows on L's per-column diagonals, one
// wave per column and one lane per row (dg_row_sum, diag_rows.h -- the text of gs_wave_diag_kernel), straight into the LDS image of
// the packed kernel (column l at l * (NCH * 16 + 1) doubles, zeros behind its end); lanes 0-31 of the first wave then run the
// band substitutions on that image (ldsp_step_fwd / ldsp_step_bwd, col_packed_steps.h), and every wave writes its columns' rows
// of x.  r never goes to memory, and there is one launch ramp and one descriptor chain per half sweep.
//
// Factors: the group's block [diag][k / 4][lane][4] (f32) is contiguous, at most 40 KB at P = 2.  All threads request it at
// kernel entry, park it in registers under the residual phase and commit it to LDS behind it; the sweeps read float4s from there
// (lane stride 16 bytes: no bank conflict).  The alternative, the register schedule of the packed kernel in the substitution wave,
// needs that kernel's 200-register budget in every wave of the workgroup; the LDS copy needs FB float4s per thread, the loads
// are spread over all waves, and the sweeps wait for LDS, not for memory.
// LDS: 16.6 KB image + (2P + 1) * 8 KB factors = 57.6 KB at P = 2, so two workgroups fit a CU (160 KB) and a colour of the
// 1 degree level 1 (373 groups on 256 CUs) is resident in one round; col_plan keeps P = 4 (90 KB) on the two-kernel path.
//
// x comes from two buffers like the other fused half sweeps (col_gs_fused.hip says why): rows < split from xa, the others from
// xb, the colour's new values to xout; the caller ping-pongs.  Same products in the same order, the same substitution text, and
// xout = old x + solution with the operands in the order of ldsp_write_back: the bits of the two-kernel path.
#include "col_packed_steps.h"
#include "diag_rows.h"

#define GL_WAVES 8               // 4 columns per wave; 4 waves (8 columns each, one behind the other) measured slower, see DESIGN.md section 4
#define GL_THREADS (GL_WAVES * NKP_WAVE)

// grp_tile: per group slot the tile of L's diagonals that is the slot's column (a column of at most 64 rows is one tile), -1 = no
// column (behind the last column of a colour's last group, or a column without rows)
template <int P, int NCH>
__global__ __launch_bounds__ (GL_THREADS, 2 * GL_WAVES / 4)
void gs_lanes_diag_kernel (const int *__restrict__ grp_maxlen, const long long *__restrict__ grp_base, int g_first, const float *__restrict__ fac_t,
                           const int *__restrict__ grp_tile, const DgTile *__restrict__ tile, const DgGroup *__restrict__ dg_grp,
                           const float *__restrict__ dg_val, int n, const double *__restrict__ xa, const double *__restrict__ xb, int split,
                           const double *__restrict__ b, double *__restrict__ xout)
{
   extern __shared__ double lds[];            // the columns' image | the group's factors
   constexpr int gw = 32, CH = 16, STRIDE = NCH * CH + 1, CPW = gw / GL_WAVES;
   constexpr int FB = ((2 * P + 1) * NCH * 4 * gw + GL_THREADS - 1) / GL_THREADS;      // float4s of the largest block per thread
   static_assert (gw % GL_WAVES == 0 && (gw * STRIDE) % 2 == 0, "columns per wave; the factor area is 16-byte aligned");
   float4 *fl = reinterpret_cast<float4 *> (lds + gw * STRIDE);
   const int g = blockIdx.x + g_first;
   const int tid = threadIdx.x, lane = tid & (NKP_WAVE - 1);
   const int wave = __builtin_amdgcn_readfirstlane (tid >> 6);
   const int ml = grp_maxlen[g];              // a multiple of 16, at most NCH * 16
   const int nch = ml / CH, mlq = ml >> 2;
   // the factor block: requested now, committed to LDS behind the residual phase (a thread behind its end repeats the first float4)
   const float4 *fsrc = reinterpret_cast<const float4 *> (fac_t + grp_base[g]);
   const int cnt4 = (2 * P + 1) * mlq * gw;
   float4 fr[FB];
#pragma unroll
   for (int u = 0; u < FB; u++) {
      const int i = tid + u * GL_THREADS;
      fr[u] = fsrc[i < cnt4 ? i : 0];
   }
   // residual phase: this wave's columns, lane = row.  All tiles first (scalar), then b and the old x of all columns in one burst;
   // an absent column reads tile 0 and row 0 and takes zeros
   int tix[CPW];
   DgTile T[CPW];
   double bv[CPW], xold[CPW];
#pragma unroll
   for (int j = 0; j < CPW; j++) tix[j] = grp_tile[(int64_t) g * gw + wave * CPW + j];
#pragma unroll
   for (int j = 0; j < CPW; j++) T[j] = tile[tix[j] >= 0 ? tix[j] : 0];
#pragma unroll
   for (int j = 0; j < CPW; j++) {
      const int64_t r = T[j].row0 + min (lane, T[j].rows - 1);
      bv[j] = b[r];
      xold[j] = r < split ? xa[r] : xb[r];
   }
#pragma unroll
   for (int j = 0; j < CPW; j++) {
      double res = 0.0;
      if (tix[j] >= 0) {
         const double acc = dg_row_sum<float, true> (T[j], dg_grp, dg_val, lane, min (lane, T[j].rows - 1), xa, n, xb, split);
         res = lane < T[j].rows ? bv[j] - acc : 0.0;
      }
      lds[(wave * CPW + j) * STRIDE + lane] = res;
   }
#pragma unroll
   for (int u = 0; u < FB; u++) {
      const int i = tid + u * GL_THREADS;
      if (i < cnt4) fl[i] = fr[u];
   }
   __syncthreads ();
   // the sweeps of colblock_apply_ldspack_kernel, chunk by chunk from the LDS copy
   if (tid < gw) {
      double *col = lds + tid * STRIDE;
      const float4 *f4 = fl + tid;
      double w[P];
#pragma unroll
      for (int q = 0; q < P; q++) w[q] = 0.0;
#pragma unroll
      for (int c = 0; c < NCH; c++)
         if (c < nch) {
            PackChunk<P> F;
            ldsp_load_fwd<P> (F, f4, mlq, c * CH, gw);
            ldsp_step_fwd<P> (F, col, c * CH, w);
         }
#pragma unroll
      for (int q = 0; q < P; q++) w[q] = 0.0;
#pragma unroll
      for (int j = 0; j < NCH; j++)
         if (j < nch) {
            PackChunk<P> Bq;
            ldsp_load_bwd<P> (Bq, f4, mlq, (nch - 1 - j) * CH, gw);
            ldsp_step_bwd<P> (Bq, col, (nch - 1 - j) * CH, w);
         }
   }
   __syncthreads ();
   // old x + solution, the operands in this order (ldsp_write_back, gs_wave_diag_kernel)
#pragma unroll
   for (int j = 0; j < CPW; j++)
      if (tix[j] >= 0 && lane < T[j].rows) xout[(int64_t) T[j].row0 + lane] = xold[j] + lds[(wave * CPW + j) * STRIDE + lane];
}

// groups [g0, g1) of one colour of a level that ml_setup marked lane_diag: packed layout with its tile map, f32 factors, columns of
// at most 64 rows, L on its diagonals
void launch_gs_lanes_diag (const CsrDev &L, const ColBlocksDev &B, int g0, int g1, const double *xa, const double *xb, int split, const double *b,
                           double *xout, hipStream_t st)
{
   if (g1 <= g0) return;
   constexpr int NCH = 4;
   const auto lds_bytes = [] (int P) { return (int) (32 * (NCH * NKP_LDSRES_CH + 1) * sizeof (double) + (size_t) (2 * P + 1) * NCH * NKP_LDSRES_CH * 32 * sizeof (float)); };
   static bool opted = false;
   if (!opted) {
      opted = true;
      for (int P : { 1, 2 })
         with_int<1, 2> (P, [&] (auto p) { colblock_opt_in ((const void *) gs_lanes_diag_kernel<decltype (p)::value, NCH>, lds_bytes (decltype (p)::value)); });
   }
   with_int<1, 2> (B.P, [&] (auto p) {
      constexpr int P = decltype (p)::value;
      hipLaunchKernelGGL ((gs_lanes_diag_kernel<P, NCH>), dim3 (g1 - g0), dim3 (GL_THREADS), (size_t) lds_bytes (P), st, B.grp_maxlen, B.grp_base, g0,
                          (const float *) B.fac_tf, B.grp_tile, (const DgTile *) L.dg_tile, (const DgGroup *) L.dg_grp, (const float *) L.dg_val, (int) L.n, xa,
                          xb, split, b, xout);
   });
}
