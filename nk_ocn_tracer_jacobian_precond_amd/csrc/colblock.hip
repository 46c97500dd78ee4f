// Water-column block preconditioner for gfx950: ONE WATER COLUMN PER WAVEFRONT.
//
// The flat state vector enumerates j outer, i middle, k inner (reference src/matrix.c:239-251),
// so the levels k = 0..KMT-1 of one column are contiguous rows and the within-column coupling
// (k+-1 from vertical mixing/advection src/matrix.c:808-819, k+-2 with upwind3 :843-854) is a
// narrow band.  Lane l of a wave owns level l of the column (two levels per lane when a block
// is longer than 64, e.g. km = 80), the band lives in registers, and the sequential
// elimination/substitution over k broadcasts one value per step with v_readlane (the step
// index is wave-uniform, so no LDS round trip and no bpermute).
//
// Exact LU of the band == ILU(0) of the column block (no fill leaves the band), so this one
// kernel pair is both the "block-Jacobi" and the "column-ILU(0)" preconditioner; it stands in
// for SuperLU's pdgstrf + pdgstrs_Bglobal (reference src/SuperLU_brief_tree.txt:8-17).
//
// Roofline: HBM-bound.  Apply traffic = (2P+1)*8*n factor bytes + 16*n vector bytes.
//
// This unit: measure, factor, the wave-per-column apply and fused half sweep, their launchers.  The lane-per-column kernels that
// serve the large levels are col_lanes.hip, col_packed.hip and col_gs_fused.hip, on the layout of col_layout.hip.
#include "nkp_dev.h"

#define CB_THREADS 256
#define CB_WAVES (CB_THREADS / NKP_WAVE)

__device__ __forceinline__ int wave_block_id ()
{
   // wave-uniform by construction; readfirstlane tells the compiler so (scalar loads, SGPR loop bounds)
   return __builtin_amdgcn_readfirstlane ((int) ((blockIdx.x * CB_THREADS + threadIdx.x) / NKP_WAVE));
}

// ---------------------------------------------------------------- measure
// out[0] = max in-block |col - row| ; out[1] = rows whose diagonal entry is missing or zero ;
// out[2] = longest block
__global__ __launch_bounds__ (CB_THREADS)
void colblock_measure_kernel (const int *__restrict__ rowptr, const int *__restrict__ colind,
                              const double *__restrict__ val, const int *__restrict__ blk_start, int nblk, int *out)
{
   const int b = wave_block_id ();
   if (b >= nblk) return;
   const int lane = threadIdx.x & (NKP_WAVE - 1);
   const int r0 = blk_start[b], r1 = blk_start[b + 1];
   int bw = 0, nodiag = 0;
   for (int r = r0 + lane; r < r1; r += NKP_WAVE) {
      double diag = 0.0;                  // repeated entries add up (check_rows of create.hip sums them in this order)
      for (int e = rowptr[r]; e < rowptr[r + 1]; e++) {
         const int c = colind[e];
         if (c >= r0 && c < r1) {
            const int d = c > r ? c - r : r - c;
            bw = d > bw ? d : bw;
            if (c == r) diag += val[e];
         }
      }
      nodiag += diag != 0.0 ? 0 : 1;
   }
   for (int off = NKP_WAVE / 2; off > 0; off >>= 1) {
      const int o = __shfl_down (bw, off);
      bw = o > bw ? o : bw;
      nodiag += __shfl_down (nodiag, off);
   }
   if (lane == 0) {
      atomicMax (&out[0], bw);
      if (nodiag) atomicAdd (&out[1], nodiag);
      atomicMax (&out[2], r1 - r0);
   }
}

// ---------------------------------------------------------------- extract + factor
template <int P, int RPL>
__global__ __launch_bounds__ (CB_THREADS)
void colblock_factor_kernel (const int *__restrict__ rowptr, const int *__restrict__ colind,
                             const double *__restrict__ val, const int *__restrict__ blk_start, int nblk,
                             int64_t n, double *__restrict__ fac, int *status, int *dropped)
{
   const int b = wave_block_id ();
   if (b >= nblk) return;
   const int lane = threadIdx.x & (NKP_WAVE - 1);
   const int r0 = blk_start[b];
   const int len = blk_start[b + 1] - r0;

   double a[RPL][2 * P + 1];
   int drop = 0;
#pragma unroll
   for (int s = 0; s < RPL; s++) {
#pragma unroll
      for (int d = 0; d <= 2 * P; d++) a[s][d] = 0.0;
      const int li = s * NKP_WAVE + lane;
      if (li < len) {
         const int r = r0 + li;
         for (int e = rowptr[r]; e < rowptr[r + 1]; e++) {
            const int c = colind[e];
            if (c < r0 || c >= r0 + len) continue;
            const int d = c - r;
            const double v = val[e];
            if (d < -P || d > P) { drop = 1; continue; }
            // repeated entries add up, in stored order; a single one is added to +0.0, which leaves its bits
#pragma unroll
            for (int dd = -P; dd <= P; dd++)
               if (d == dd) a[s][dd + P] += v;
         }
      }
   }

   // right-looking banded LU without pivoting; step k is wave-uniform
   int bad = 0;
   for (int k = 0; k < len; k++) {
      const int ks = k >> 6, kl = k & (NKP_WAVE - 1);
      double u[P + 1];
#pragma unroll
      for (int s = 0; s < RPL; s++)
         if (ks == s) {
#pragma unroll
            for (int q = 0; q <= P; q++) u[q] = readlane_f64 (a[s][P + q], kl);
         }
      if (!(fabs (u[0]) > 1.0e-300) && bad == 0) bad = r0 + k + 1;
      const double inv = 1.0 / u[0];
#pragma unroll
      for (int dist = 1; dist <= P; dist++) {
         const int kr = k + dist;
         if (kr < len) {
            const int ts = kr >> 6, tl = kr & (NKP_WAVE - 1);
#pragma unroll
            for (int s = 0; s < RPL; s++)
               if (ts == s && lane == tl) {
                  const double l = a[s][P - dist] * inv;
                  a[s][P - dist] = l;
#pragma unroll
                  for (int q = 1; q <= P; q++)
                     if (P - dist + q <= 2 * P) a[s][P - dist + q] -= l * u[q];
               }
         }
      }
   }

#pragma unroll
   for (int s = 0; s < RPL; s++) {
      const int li = s * NKP_WAVE + lane;
      if (li < len) {
         const int64_t r = r0 + li;
         a[s][P] = 1.0 / a[s][P];
#pragma unroll
         for (int d = 0; d <= 2 * P; d++) fac[(int64_t) d * n + r] = a[s][d];
      }
   }
   if (lane == 0 && bad) atomicCAS (status, 0, bad);
   if (drop) *dropped = 1;
}

// ---------------------------------------------------------------- apply  z = (LU)^-1 r
// R32: the factors are rounded to f32 on the way in, which gives exactly the values the f32 lane layouts store, so the
// result is the one of the lane-per-column kernels in the f32-storage mode of the multilevel cycle
template <int P, int RPL, bool R32 = false>
__global__ __launch_bounds__ (CB_THREADS)
void colblock_apply_kernel (const int *__restrict__ blk_start, int b_first, int nblk, int64_t n,
                            const double *__restrict__ fac, const double *__restrict__ rhs, double *__restrict__ z, int accumulate)
{
   const int b = wave_block_id () + b_first;
   if (b >= nblk) return;
   const int lane = threadIdx.x & (NKP_WAVE - 1);
   const int r0 = blk_start[b];
   const int len = blk_start[b + 1] - r0;

   double y[RPL][1], invd[RPL], L[RPL][P], U[RPL][P];
#pragma unroll
   for (int s = 0; s < RPL; s++) {
      const int li = s * NKP_WAVE + lane;
      y[s][0] = 0.0;
      invd[s] = 0.0;
#pragma unroll
      for (int q = 0; q < P; q++) { L[s][q] = 0.0; U[s][q] = 0.0; }
      if (li < len) {
         const int64_t r = r0 + li;
         y[s][0] = rhs[r];
         invd[s] = fac[(int64_t) P * n + r];
         if (R32) invd[s] = (double) (float) invd[s];
#pragma unroll
         for (int q = 1; q <= P; q++) {
            L[s][q - 1] = fac[(int64_t) (P - q) * n + r];     // l(r, r-q)
            U[s][q - 1] = fac[(int64_t) (P + q) * n + r];     // u(r, r+q)
            if (R32) { L[s][q - 1] = (double) (float) L[s][q - 1]; U[s][q - 1] = (double) (float) U[s][q - 1]; }
         }
      }
   }

   wave_band_sweeps<P, RPL, 1> (len, lane, y, invd, L, U);
#pragma unroll
   for (int s = 0; s < RPL; s++) {
      const int li = s * NKP_WAVE + lane;
      if (li < len) {
         if (accumulate) z[(int64_t) r0 + li] += y[s][0];
         else z[(int64_t) r0 + li] = y[s][0];
      }
   }
}

// ---------------------------------------------------------------- fused half sweep, one water column per wave
// Small levels of the multilevel cycle (a few thousand columns) run at the latency floor of their launches: a residual SpMV
// over the colour's rows (~7 us) followed by the wave-per-column solve above (~11 us), both far below one wave per SIMD.
// Here ONE launch does both for one colour: lane l of the wave that owns a column computes the residual of ITS row straight
// from the CSR arrays (row-per-lane: a level of this size sits in L2 / MALL, so the uncoalesced row reads cost latency, not
// bandwidth, and the loads of 8 entries are in flight together), then the wave runs the band substitution on the
// residual it holds in registers, and x_new = x_old + z goes out.  r never touches memory and half of the launches go.
// x comes from TWO buffers like gs_fused_kernel's (rows < split from xa, the others from xb; new values to xout): columns
// of one colour are coupled, so the sweep must not see its own updates (mlcycle.hip ping-pongs the buffers).
// Same products, same per-row summation order, same substitution as the two-kernel path => identical bits.
#define GSW_UNROLL 24
#define GSW_CAP 1536          // entries of one water column staged per wave (LDS: 4 waves x 1536 x 8 bytes = 48 KB with f32 values)
#define GSW_STAGE 8
template <int P, int RPL, class VT, bool R32>
__global__ __launch_bounds__ (CB_THREADS)
void gs_wave_kernel (const int *__restrict__ rowptr, const int *__restrict__ colind, const VT *__restrict__ val,
                     const int *__restrict__ blk_start, int b_first, int b_end, int64_t n, const double *__restrict__ fac,
                     const double *__restrict__ xa, const double *__restrict__ xb, int split, const double *__restrict__ b, double *__restrict__ xout,
                     const int4 *__restrict__ desc)
{
   // the (column, value) entries of the wave's water column -- one contiguous stretch of the CSR arrays -- are staged through LDS with
   // coalesced loads; the row-per-lane reads they replace asked the L1 for every 128-byte line about 24 times (lanes 54 bytes
   // apart, one instruction per entry of the row) and bounded the launch: 26 us per half sweep of the 1 degree level 2 (3416 waves)
   extern __shared__ unsigned char gsw_lds[];
   const int wv = threadIdx.x / NKP_WAVE;
   int *sc = reinterpret_cast<int *> (gsw_lds) + wv * GSW_CAP;
   VT *sv = reinterpret_cast<VT *> (gsw_lds + (size_t) CB_WAVES * GSW_CAP * sizeof (int)) + wv * GSW_CAP;
   const int blk = wave_block_id () + b_first;
   if (blk >= b_end) return;                        // a wave stages and reads its own LDS region only: no workgroup barrier below
   const int lane = threadIdx.x & (NKP_WAVE - 1);
   // {first row, rows, first entry, entries} of the column in one 16-byte load (desc: built at setup), else through blk_start and rowptr
   int4 d4;
   if (desc) d4 = desc[blk];
   else {
      d4.x = blk_start[blk];
      d4.y = blk_start[blk + 1] - d4.x;
      d4.z = d4.y > 0 ? rowptr[d4.x] : 0;
      d4.w = d4.y > 0 ? rowptr[d4.x + d4.y] - d4.z : 0;
   }
   const int r0 = d4.x, len = d4.y;

   double y[RPL][1], xold[RPL], invd[RPL], L[RPL][P], U[RPL][P];
   int e0[RPL], rl[RPL];
   const int e_begin = d4.z, e_total = d4.w;
   const bool staged = e_total <= GSW_CAP;
   if (staged) {
      for (int k0 = 0; k0 < e_total; k0 += NKP_WAVE * GSW_STAGE) {
         int tc[GSW_STAGE];
         VT tv[GSW_STAGE];
#pragma unroll
         for (int u = 0; u < GSW_STAGE; u++) {
            const int k = k0 + u * NKP_WAVE + lane;
            tc[u] = k < e_total ? colind[e_begin + k] : 0;
            tv[u] = k < e_total ? val[e_begin + k] : (VT) 0;
         }
#pragma unroll
         for (int u = 0; u < GSW_STAGE; u++) {
            const int k = k0 + u * NKP_WAVE + lane;
            if (k < e_total) { sc[k] = tc[u]; sv[k] = tv[u]; }
         }
      }
   }
#pragma unroll
   for (int s = 0; s < RPL; s++) {
      const int li = s * NKP_WAVE + lane;
      y[s][0] = 0.0; xold[s] = 0.0; invd[s] = 0.0; e0[s] = 0; rl[s] = 0;
#pragma unroll
      for (int q = 0; q < P; q++) { L[s][q] = 0.0; U[s][q] = 0.0; }
      if (li < len) {
         const int64_t r = r0 + li;
         e0[s] = rowptr[r];
         rl[s] = rowptr[r + 1] - e0[s];
         y[s][0] = b[r];
         xold[s] = (r < split) ? xa[r] : xb[r];
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
   // the staged entries are written and read by this wave alone, and a wave's LDS operations complete in order: all that is
   // needed is that the compiler keeps the writes above in front of the reads below
   __builtin_amdgcn_fence (__ATOMIC_ACQ_REL, "wavefront");
   __builtin_amdgcn_wave_barrier ();
   // residual of this lane's row(s): entries in stored order, GSW_UNROLL of them requested together (from LDS, or one round trip for the (column, value) pairs of a column too long to stage; then one for the gathered x)
#pragma unroll
   for (int s = 0; s < RPL; s++) {
      double acc = 0.0;
      for (int k0 = 0; __any (k0 < rl[s]); k0 += GSW_UNROLL) {
         int cc[GSW_UNROLL];
         VT vv[GSW_UNROLL];
         if (staged) {
            const int off = e0[s] - e_begin + k0;
#pragma unroll
            for (int u = 0; u < GSW_UNROLL; u++) {
               const bool ok = k0 + u < rl[s];
               cc[u] = ok ? sc[off + u] : 0;
               vv[u] = ok ? sv[off + u] : (VT) 0;
            }
         } else {
#pragma unroll
            for (int u = 0; u < GSW_UNROLL; u++) {
               const bool ok = k0 + u < rl[s];
               cc[u] = ok ? colind[e0[s] + k0 + u] : 0;
               vv[u] = ok ? val[e0[s] + k0 + u] : (VT) 0;
            }
         }
         double xv[GSW_UNROLL];
#pragma unroll
         for (int u = 0; u < GSW_UNROLL; u++) xv[u] = (cc[u] < split) ? xa[cc[u]] : xb[cc[u]];
#pragma unroll
         for (int u = 0; u < GSW_UNROLL; u++)
            if (k0 + u < rl[s]) acc += (double) vv[u] * xv[u];
      }
      if (s * NKP_WAVE + lane < len) y[s][0] -= acc;
   }
#if defined(NKP_ABLATION) && defined(NKP_ABLATE_GSW_SWEEPS)
   // TIMING-ONLY (wrong results by design; `make ablation ABLATE=-DNKP_ABLATE_GSW_SWEEPS`): the launch without its two sweeps;
   // the factor loads stay alive.  What this takes off a launch is the most any rewrite of the sweeps can gain
#pragma unroll
   for (int s = 0; s < RPL; s++) {
      double f = invd[s];
#pragma unroll
      for (int q = 0; q < P; q++) f += L[s][q] + U[s][q];
      if (f == 123.456) y[s][0] = f;
   }
#else
   wave_band_sweeps<P, RPL, 1> (len, lane, y, invd, L, U);
#endif
#pragma unroll
   for (int s = 0; s < RPL; s++) {
      const int li = s * NKP_WAVE + lane;
      if (li < len) xout[(int64_t) r0 + li] = xold[s] + y[s][0];
   }
}

// ---------------------------------------------------------------- launchers
static inline dim3 cb_grid (int nblk) { return dim3 ((nblk + CB_WAVES - 1) / CB_WAVES); }

void launch_colblock_measure (const CsrDev &A, const ColBlocksDev &B, int *d_out3, hipStream_t st)
{
   if (B.nblk == 0) return;
   hipLaunchKernelGGL (colblock_measure_kernel, cb_grid (B.nblk), dim3 (CB_THREADS), 0, st,
                       A.rowptr, A.colind, A.val, B.blk_start, B.nblk, d_out3);
}

void launch_colblock_factor (const CsrDev &A, ColBlocksDev &B, int *d_status, hipStream_t st)
{
   if (B.nblk == 0) return;
   int *d_dropped = d_status + 1;
   with_band_rows (B, [&] (auto p, auto rpl) {
      hipLaunchKernelGGL ((colblock_factor_kernel<decltype (p)::value, decltype (rpl)::value>), cb_grid (B.nblk), dim3 (CB_THREADS), 0, st,
                          A.rowptr, A.colind, A.val, B.blk_start, B.nblk, B.n, B.fac, d_status, d_dropped);
   });
}

// blocks [b0, b1) only; accumulate: z_blk += M_blk^-1 r_blk, else z_blk = M_blk^-1 r_blk; r32: the factors rounded to f32 on
// load (multilevel cycle with f32 storage)
static void colblock_apply_blocks (const ColBlocksDev &B, int b0, int b1, const double *r, double *z, int accumulate, bool r32, hipStream_t st)
{
   if (b1 <= b0) return;
   with_band_rows (B, [&] (auto p, auto rpl) {
      with_bool (r32, [&] (auto r32_) {
         hipLaunchKernelGGL ((colblock_apply_kernel<decltype (p)::value, decltype (rpl)::value, decltype (r32_)::value>), cb_grid (b1 - b0), dim3 (CB_THREADS), 0, st,
                             B.blk_start, b0, b1, B.n, B.fac, r, z, accumulate);
      });
   });
}

void launch_colblock_apply (const ColBlocksDev &B, const double *r, double *z, hipStream_t st)
{
   colblock_apply_blocks (B, 0, B.nblk, r, z, 0, false, st);
}

void launch_colblock_apply_range (const ColBlocksDev &B, int b0, int b1, const double *r, double *z, int accumulate, hipStream_t st)
{
   colblock_apply_blocks (B, b0, b1, r, z, accumulate, false, st);
}

void launch_colblock_apply_range_r32 (const ColBlocksDev &B, int b0, int b1, const double *r, double *z, int accumulate, hipStream_t st)
{
   colblock_apply_blocks (B, b0, b1, r, z, accumulate, true, st);
}

__global__ __launch_bounds__ (CB_THREADS)
void wave_desc_kernel (const int *__restrict__ rowptr, const int *__restrict__ blk_start, int nblk, int4 *__restrict__ desc)
{
   const int b = blockIdx.x * CB_THREADS + threadIdx.x;
   if (b >= nblk) return;
   const int r0 = blk_start[b], len = blk_start[b + 1] - r0;
   const int e0 = len > 0 ? rowptr[r0] : 0;
   desc[b] = make_int4 (r0, len, e0, len > 0 ? rowptr[r0 + len] - e0 : 0);
}

void launch_build_wave_desc (const CsrDev &L, ColBlocksDev &B, hipStream_t st)
{
   if (B.nblk > 0 && B.wave_desc)
      hipLaunchKernelGGL (wave_desc_kernel, dim3 ((B.nblk + CB_THREADS - 1) / CB_THREADS), dim3 (CB_THREADS), 0, st, L.rowptr, B.blk_start, B.nblk, reinterpret_cast<int4 *> (B.wave_desc));
}

// blocks [b0, b1) of one colour: xout_rows = x_rows + M^-1 (b - L x)_rows in one launch (gs_wave_kernel); r32: factors rounded
// to f32 on load (the f32 storage mode of the cycle).  The level operator is read through L.valf when it has an f32 copy.
void launch_gs_wave (const CsrDev &L, const ColBlocksDev &B, int b0, int b1, const double *xa, const double *xb, int split, const double *b, double *xout,
                     int r32, hipStream_t st)
{
   if (b1 <= b0) return;
   with_band_rows (B, [&] (auto p, auto rpl) {
      with_storage (L.valf, L.val, [&] (auto val) {
         with_bool (r32, [&] (auto r32_) {
            const auto kernel = gs_wave_kernel<decltype (p)::value, decltype (rpl)::value, elem_t<decltype (val)>, decltype (r32_)::value>;
            const size_t lds = (size_t) CB_WAVES * GSW_CAP * (sizeof (int) + sizeof (*val));
            // more than 48 KB of dynamic LDS needs an opt-in: once per instantiation (this lambda's body is one), before its first launch
            static bool opted = false;
            if (lds > 48 * 1024 && !opted) { (void) hipFuncSetAttribute ((const void *) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds); opted = true; }
            hipLaunchKernelGGL (kernel, cb_grid (b1 - b0), dim3 (CB_THREADS), lds, st, L.rowptr, L.colind, val,
                                B.blk_start, b0, b1, B.n, B.fac, xa, xb, split, b, xout, reinterpret_cast<const int4 *> (B.wave_desc));
         });
      });
   });
}
