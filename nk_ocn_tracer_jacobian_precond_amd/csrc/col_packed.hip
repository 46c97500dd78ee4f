// Lane-per-column band solves on the packed layout (col_plan.h: COL_LDSPACK): the single-vector kernel and its siblings for two
// and for four interleaved right-hand sides, which share the schedule and the substitution helpers below.
#include "colblock_impl.h"
#include "col_packed_steps.h"

// ================================================================ LDS-resident columns, factors packed along the column
// What held the kernel above at 0.43 of the HBM peak (1 degree fine level: 27 us for 93 MB): a colour is ONE round of
// waves (1468 groups of 32 columns on 256 CUs, 8 wave slots each), every wave walks its 2 x 4 factor chunks one behind
// the other with a single chunk of look-ahead, and a chunk is 32-48 load instructions of 128 bytes -- the 63 loads a
// wave may have in flight are 8 KB.  A latency-bound chain per wave with nothing to overlap it.
// Here the factors of 4 consecutive steps of a column sit side by side ([diag][k / 4][lane][4], f32), so one instruction
// moves 512 bytes and a chunk of 16 steps is 2-3 instructions per diagonal; and the schedule is static: the forward chunks
// are requested around the right-hand side's burst (the batch kernels: all before it), the backward chunks follow as the
// registers of consumed forward chunks come free (a compile-time budget of LDSP_BUDGET registers decides what is in flight when), so by the time the
// forward sweep is done the backward factors have landed.  Same operations in the same order => same bits.
#define LDSP_BUDGET 200

// RR: the registers of one double per column and 64 rows (the right-hand side on its way into LDS, the accumulate target on
// its way out), which the single-vector kernel holds in one burst beside the factor chunks; the factor schedule itself does
// not depend on it.  f_staged = forward chunks (of the f_upfront) requested before the right-hand side is written to LDS, the
// others follow the writes that free its registers; z_after = backward steps done when the accumulate target is requested:
// the first point at which it fits beside the backward chunks still in flight (+ 16: the request is made with nothing else
// of the wave waiting, and its addresses want registers too -- without them the P = 1 kernels spill).
template <int NCH, int FR, int BR, int RR = 0>
struct LdspSchedule {
   int f_upfront = 0, b_upfront = 0, f_staged = 0, z_after = NCH;
   int f_after[NCH] = {}, b_after_f[NCH] = {}, b_after_b[NCH] = {};     // chunks issued in total once fwd step c / bwd step j is done
   constexpr LdspSchedule ()
   {
      int fi = 0, bi = 0, fc = 0, bc = 0;
      while (fi < NCH && ((fi - fc) * FR + (bi - bc) * BR + FR <= LDSP_BUDGET || fi == fc)) fi++;
      while (bi < NCH && (fi - fc) * FR + (bi - bc) * BR + BR <= LDSP_BUDGET) bi++;
      f_upfront = fi;
      b_upfront = bi;
      while (f_staged < f_upfront && (RR + (f_staged + 1) * FR <= LDSP_BUDGET || f_staged == 0)) f_staged++;
      for (int c = 0; c < NCH; c++) {
         fc++;
         while (fi < NCH && ((fi - fc) * FR + (bi - bc) * BR + FR <= LDSP_BUDGET || fi == fc)) fi++;
         while (bi < NCH && ((fi - fc) * FR + (bi - bc) * BR + BR <= LDSP_BUDGET || (fc == NCH && bi == bc))) bi++;
         f_after[c] = fi;
         b_after_f[c] = bi;
      }
      if (bi * BR + RR + 16 <= LDSP_BUDGET) z_after = 0;
      for (int j = 0; j < NCH; j++) {
         bc++;
         while (bi < NCH && ((bi - bc) * BR + BR + (z_after <= j ? RR : 0) <= LDSP_BUDGET || bi == bc)) bi++;
         b_after_b[j] = bi;
         if (z_after == NCH && (bi - bc) * BR + RR + 16 <= LDSP_BUDGET) z_after = j + 1;
      }
   }
};

// one double per column of the group and 64 rows, as it travels between global memory and the LDS image: the right-hand side on
// the way in, the accumulate target on the way out (NCH = 5: rows 64-79 too, in v[32 ...])
template <int NCH>
struct PackRows { double v[NCH > 4 ? 64 : 32]; };

// Requests the rows of all 32 columns from x in ONE burst: no load of it is waited for before the last is issued.  A lane behind
// the end of its column reads the column's first row instead (an absent column of the last group: row R0), an address that is
// always valid, so these loads are unconditional like the factor loads -- a `lane < len` around each compiles to a branch and a
// full wait per column.  Whoever consumes the value discards it for those lanes.
template <int NCH>
__device__ __forceinline__ void ldsp_request_rows (PackRows<NCH> &t, const double *x, int R0, int s, int len, int lane)
{
#pragma unroll
   for (int c = 0; c < 32; c++) {
      const int sc = __builtin_amdgcn_readlane (s, c), lc = __builtin_amdgcn_readlane (len, c);
      t.v[c] = x[(int64_t) R0 + sc + (lane < lc ? lane : 0)];
      if (NCH > 4) t.v[32 + c] = x[(int64_t) R0 + sc + (lane + NKP_WAVE < lc ? lane + NKP_WAVE : 0)];
   }
}

// No access to memory moves across this point of the program, neither in the compiler's passes nor in its instruction scheduler;
// no instruction and no wait of its own.  p: the array whose loads are to stay where they are -- the compiler knows that an
// empty statement cannot reach a __restrict__ array it has not been handed, and moves such loads across it all the same.
__device__ __forceinline__ void ldsp_fence (const void *p)
{
   asm volatile ("" : : "v" (p) : "memory");
   __builtin_amdgcn_sched_barrier (0);
}

// The solution leaves the LDS image: z = (ACC ? target : 0.0) + solution, the operands in this order.  All LDS reads first, then
// the stores, one behind the other without a wait: with the read inside the `lane < len` of its store every column would pay an
// LDS round trip of its own.  t is read only where ACC says that it has been requested.
template <int NCH, bool ACC>
__device__ __forceinline__ void ldsp_write_back (const PackRows<NCH> &t, const double *lds, double *z, int R0, int s, int len, int lane)
{
   constexpr int STRIDE = NCH * 16 + 1;
   // h = 1: rows 64-79 of the columns (NCH = 5), the lane clamped into the column's slot
#pragma unroll
   for (int h = 0; h < (NCH > 4 ? 2 : 1); h++) {
      const int row = h ? (lane + NKP_WAVE < STRIDE - 1 ? lane + NKP_WAVE : STRIDE - 2) : lane;
      double x[32];
#pragma unroll
      for (int c = 0; c < 32; c++) x[c] = (ACC ? t.v[32 * h + c] : 0.0) + lds[c * STRIDE + row];
      ldsp_fence (z);
#pragma unroll
      for (int c = 0; c < 32; c++) {
         const int sc = __builtin_amdgcn_readlane (s, c), lc = __builtin_amdgcn_readlane (len, c);
         if (lane + h * NKP_WAVE < lc) z[(int64_t) R0 + sc + lane + h * NKP_WAVE] = x[c];
      }
   }
}

// The end of a wave's work: (ACC) the accumulate target of all 32 columns is requested by all 64 lanes, into registers that
// backward chunks have left; the backward steps from S.z_after on run over that round trip; the solution goes back out.
template <int P, int NCH, bool ACC, class SCHED>
__device__ __forceinline__ void ldsp_finish (PackChunk<P> (&Bq)[NCH], double (&w)[P], const float4 *f4, int mlq, int nch, double *lds, double *z, int R0,
                                             int s, int len, int lane)
{
   constexpr SCHED S;
   constexpr int gw = 32, CH = 16, STRIDE = NCH * CH + 1;
   double *col = lds + (lane & (gw - 1)) * STRIDE;
   PackRows<NCH> Z;
   if (ACC) {
      ldsp_fence (z);
      ldsp_request_rows<NCH> (Z, z, R0, s, len, lane);
      ldsp_fence (z);
   }
#pragma unroll
   for (int j = 0; j < NCH; j++) {
      if (j >= S.z_after) {
         if (lane < gw && j < nch) ldsp_step_bwd<P> (Bq[j], col, (nch - 1 - j) * CH, w);
#pragma unroll
         for (int t = 0; t < NCH; t++)
            if (t >= (j ? S.b_after_b[j - 1] : S.b_after_f[NCH - 1]) && t < S.b_after_b[j])
               ldsp_load_bwd<P> (Bq[t], f4, mlq, (nch - 1 - t > 0 ? nch - 1 - t : 0) * CH, gw);
      }
   }
   __syncthreads ();
   ldsp_write_back<NCH, ACC> (Z, lds, z, R0, s, len, lane);
}

// first step of the chunk a packed kernel (ldspack, ldspack2, ldspack4) keeps in F[t] and in Bq[t], from the kernel's nch and CH;
// undefined again behind the last of them
#define LDSP_FWD_K0(t) (((t) < nch ? (t) : nch - 1) * CH)
#define LDSP_BWD_K0(t) ((nch - 1 - (t) > 0 ? nch - 1 - (t) : 0) * CH)

// LDS image: column l of the group at [l * LDSP_STRIDE, ...), LDSP_STRIDE = NCH * 16 + 1 doubles.  Odd stride: the 32 lanes of
// a substitution step hit 32 different bank pairs; fixed stride: every LDS address of the sweeps is "lane base + constant",
// no address arithmetic and no predicate (SQ counters of the first version: 21 VALU instructions per step, most of them
// the padded index of the linear image, and 41 % of a wave's life spent issuing).  Rows beyond a column's length are zero
// (their factors are zero too), so the sweeps need no length test.
// A wave's dependent trips to memory, in the order of its requests (= the order of arrival):
//   1. the group's descriptors (scalar), 2. col_slot, with the first forward chunk requested beside it, 3. the right-hand side of
//   all 32 columns in one burst, the other forward chunks behind it -- the burst is waited for with counts that leave those in
//   flight, and the chunks that did not fit beside its registers follow the LDS writes, 4. the accumulate target of all 32
//   columns in one burst from inside the backward sweep (S.z_after: as soon as it fits beside the backward chunks still in
//   flight), so that it has landed when the sweep ends, 5. the stores, none of them waited for.
// Before, the staging was four batches of 8 columns, each drained with vmcnt(0) (the first behind the whole factor burst), and
// the write-back four batches of target loads, each drained, with a drain behind every store as well.
template <int P, int NCH>
__global__ __launch_bounds__ (NKP_WAVE, 2)
void colblock_apply_ldspack_kernel (const int *__restrict__ grp_nb, const int *__restrict__ grp_maxlen, const long long *__restrict__ grp_base, int g_first,
                                    const float *__restrict__ fac_t, const double *__restrict__ rhs, double *__restrict__ z, int accumulate,
                                    const int *__restrict__ grp_row0, const int *__restrict__ col_slot, int ngrp)
{
   extern __shared__ double lds[];
   constexpr int gw = 32, CH = 16, STRIDE = NCH * CH + 1;
   constexpr LdspSchedule<NCH, P * CH, (P + 1) * CH, 2 * (NCH > 4 ? 64 : 32)> S;
   const int g = blockIdx.x + g_first;
   const int lane = threadIdx.x;
   const int ml = grp_maxlen[g];                            // a multiple of 16, at most NCH * 16
   const int nch = ml / CH, mlq = ml >> 2;
   const int R0 = grp_row0[g];
   const int cl = lane & (gw - 1);
   // first row (within the group) and length of lane's column; lanes 32-63 mirror 0-31 (the staging loops broadcast from them)
   const int s = col_slot[g * gw + cl], len = col_slot[(ngrp + g) * gw + cl];
   const float4 *f4 = reinterpret_cast<const float4 *> (fac_t + grp_base[g]) + cl;
   // The factor loads are unconditional so that the kernel is one straight line the static schedule can be written into: a
   // group with fewer than NCH chunks requests its last chunk again (an L2 hit) and skips the steps.
   // F[c] = forward chunk min (c, nch - 1);  Bq[j] = backward chunk max (nch - 1 - j, 0)
   PackChunk<P> F[NCH], Bq[NCH];
   PackRows<NCH> T;
   // the fences keep the requests in this order: left alone, the compiler moves the factor loads to their first use (behind
   // the staging, inside the sweep) or ahead of the burst, and in-order return then delivers the burst behind all of them
   ldsp_load_fwd<P> (F[0], f4, mlq, LDSP_FWD_K0 (0), gw);
   ldsp_fence (f4);
   ldsp_request_rows<NCH> (T, rhs, R0, s, len, lane);
   ldsp_fence (f4);
#pragma unroll
   for (int t = 1; t < NCH; t++)
      if (t < S.f_staged) ldsp_load_fwd<P> (F[t], f4, mlq, LDSP_FWD_K0 (t), gw);
   ldsp_fence (f4);
   // staging: the 64 lanes hold up to 64 consecutive rows of each column (coalesced) and write them to its slot, zeros behind its end
#pragma unroll
   for (int c = 0; c < gw; c++) {
      const int lc = __builtin_amdgcn_readlane (len, c);
      lds[c * STRIDE + lane] = (lane < lc) ? T.v[c] : 0.0;
      if (NCH > 4 && lane < STRIDE - 1 - NKP_WAVE) lds[c * STRIDE + lane + NKP_WAVE] = (lane + NKP_WAVE < lc) ? T.v[32 + c] : 0.0;
   }
   ldsp_fence (f4);
#pragma unroll
   for (int t = 1; t < NCH; t++)
      if (t >= S.f_staged && t < S.f_upfront) ldsp_load_fwd<P> (F[t], f4, mlq, LDSP_FWD_K0 (t), gw);
#pragma unroll
   for (int t = 0; t < NCH; t++)
      if (t < S.b_upfront) ldsp_load_bwd<P> (Bq[t], f4, mlq, LDSP_BWD_K0 (t), gw);
   __syncthreads ();
   // The sweeps: lanes 0-31 run the steps, all 64 request the chunks (the upper half its mirror's, from the same addresses) --
   // a chunk requested under `lane < gw` and consumed under the next is a value the compiler keeps a second, undefined copy of
   // for the other lanes, and the register allocation that follows spills
   double *col = lds + cl * STRIDE;
   double w[P];
#pragma unroll
   for (int q = 0; q < P; q++) w[q] = 0.0;
#pragma unroll
   for (int c = 0; c < NCH; c++) {
      if (lane < gw && c < nch) ldsp_step_fwd<P> (F[c], col, c * CH, w);
#pragma unroll
      for (int t = 0; t < NCH; t++)
         if (t >= (c ? S.f_after[c - 1] : S.f_upfront) && t < S.f_after[c]) ldsp_load_fwd<P> (F[t], f4, mlq, LDSP_FWD_K0 (t), gw);
#pragma unroll
      for (int t = 0; t < NCH; t++)
         if (t >= (c ? S.b_after_f[c - 1] : S.b_upfront) && t < S.b_after_f[c]) ldsp_load_bwd<P> (Bq[t], f4, mlq, LDSP_BWD_K0 (t), gw);
   }
#pragma unroll
   for (int q = 0; q < P; q++) w[q] = 0.0;
#pragma unroll
   for (int j = 0; j < NCH; j++) {
      if (j < S.z_after) {
         if (lane < gw && j < nch) ldsp_step_bwd<P> (Bq[j], col, (nch - 1 - j) * CH, w);
#pragma unroll
         for (int t = 0; t < NCH; t++)
            if (t >= (j ? S.b_after_b[j - 1] : S.b_after_f[NCH - 1]) && t < S.b_after_b[j]) ldsp_load_bwd<P> (Bq[t], f4, mlq, LDSP_BWD_K0 (t), gw);
      }
   }
   // two copies of the rest, not one with `if (accumulate)` around the request: where the two paths meet again the compiler
   // waits for a chunk with the count that is right when nothing was requested behind it, and that drains the target
   if (accumulate) ldsp_finish<P, NCH, true, decltype (S)> (Bq, w, f4, mlq, nch, lds, z, R0, s, len, lane);
   else ldsp_finish<P, NCH, false, decltype (S)> (Bq, w, f4, mlq, nch, lds, z, R0, s, len, lane);
}

// The same kernel on TWO right-hand sides of a K-interleaved batch (batch.hip): lanes 0-31 run the columns on system k0, lanes
// 32-63 the same columns on system k0 + 1 -- the half of the wave that idles in the single-vector kernel (and already loads
// the same factors) does the second system, so the factor stream is read once per pair.  rhs / z are K-interleaved
// (element (row, k) at row * K + k); K = 4 takes two launches (k0 = 0, 2).  Same operations per column => same bits.
template <int P, int NCH>
__global__ __launch_bounds__ (NKP_WAVE, 2)
void colblock_apply_ldspack2_kernel (const int *__restrict__ grp_maxlen, const long long *__restrict__ grp_base, int g_first,
                                     const float *__restrict__ fac_t, const double *__restrict__ rhs, double *__restrict__ z, int accumulate,
                                     const int *__restrict__ grp_row0, const int *__restrict__ col_slot, int ngrp, int K, int k0)
{
   extern __shared__ double lds[];
   constexpr int gw = 32, CH = 16, STRIDE = NCH * CH + 1;
   constexpr LdspSchedule<NCH, P * CH, (P + 1) * CH> S;
   const int g = blockIdx.x + g_first;
   const int lane = threadIdx.x;
   const int ml = grp_maxlen[g];
   const int nch = ml / CH, mlq = ml >> 2;
   const int R0 = grp_row0[g];
   const int cl = lane & (gw - 1);
   const int s = col_slot[g * gw + cl], len = col_slot[(ngrp + g) * gw + cl];
   const float4 *f4 = reinterpret_cast<const float4 *> (fac_t + grp_base[g]) + cl;
   PackChunk<P> F[NCH], Bq[NCH];
#pragma unroll
   for (int t = 0; t < NCH; t++)
      if (t < S.f_upfront) ldsp_load_fwd<P> (F[t], f4, mlq, LDSP_FWD_K0 (t), gw);
#pragma unroll
   for (int t = 0; t < NCH; t++)
      if (t < S.b_upfront) ldsp_load_bwd<P> (Bq[t], f4, mlq, LDSP_BWD_K0 (t), gw);
#pragma unroll
   for (int c0 = 0; c0 < gw; c0 += 8) {
      double2 t[8], t2[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
         const int sc = __builtin_amdgcn_readlane (s, c0 + u), lc = __builtin_amdgcn_readlane (len, c0 + u);
         t[u] = (lane < lc) ? *reinterpret_cast<const double2 *> (rhs + ((int64_t) R0 + sc + lane) * K + k0) : make_double2 (0.0, 0.0);
         if (NCH > 4) t2[u] = (lane + NKP_WAVE < lc) ? *reinterpret_cast<const double2 *> (rhs + ((int64_t) R0 + sc + lane + NKP_WAVE) * K + k0) : make_double2 (0.0, 0.0);
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
         lds[(c0 + u) * STRIDE + lane] = t[u].x;
         lds[(gw + c0 + u) * STRIDE + lane] = t[u].y;
         if (NCH > 4 && lane < STRIDE - 1 - NKP_WAVE) {
            lds[(c0 + u) * STRIDE + lane + NKP_WAVE] = t2[u].x;
            lds[(gw + c0 + u) * STRIDE + lane + NKP_WAVE] = t2[u].y;
         }
      }
   }
   __syncthreads ();
   {
      double *col = lds + lane * STRIDE;                    // slot lane = (system half, column)
      double w[P];
#pragma unroll
      for (int q = 0; q < P; q++) w[q] = 0.0;
#pragma unroll
      for (int c = 0; c < NCH; c++) {
         if (c < nch) ldsp_step_fwd<P> (F[c], col, c * CH, w);
#pragma unroll
         for (int t = 0; t < NCH; t++)
            if (t >= (c ? S.f_after[c - 1] : S.f_upfront) && t < S.f_after[c]) ldsp_load_fwd<P> (F[t], f4, mlq, LDSP_FWD_K0 (t), gw);
#pragma unroll
         for (int t = 0; t < NCH; t++)
            if (t >= (c ? S.b_after_f[c - 1] : S.b_upfront) && t < S.b_after_f[c]) ldsp_load_bwd<P> (Bq[t], f4, mlq, LDSP_BWD_K0 (t), gw);
      }
#pragma unroll
      for (int q = 0; q < P; q++) w[q] = 0.0;
#pragma unroll
      for (int j = 0; j < NCH; j++) {
         if (j < nch) ldsp_step_bwd<P> (Bq[j], col, (nch - 1 - j) * CH, w);
#pragma unroll
         for (int t = 0; t < NCH; t++)
            if (t >= (j ? S.b_after_b[j - 1] : S.b_after_f[NCH - 1]) && t < S.b_after_b[j]) ldsp_load_bwd<P> (Bq[t], f4, mlq, LDSP_BWD_K0 (t), gw);
      }
   }
   __syncthreads ();
#pragma unroll
   for (int c0 = 0; c0 < gw; c0 += 8) {
      double2 t[8], t2[8];
      int sc[8], lc[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
         sc[u] = __builtin_amdgcn_readlane (s, c0 + u);
         lc[u] = __builtin_amdgcn_readlane (len, c0 + u);
         t[u] = (accumulate && lane < lc[u]) ? *reinterpret_cast<const double2 *> (z + ((int64_t) R0 + sc[u] + lane) * K + k0) : make_double2 (0.0, 0.0);
         if (NCH > 4) t2[u] = (accumulate && lane + NKP_WAVE < lc[u]) ? *reinterpret_cast<const double2 *> (z + ((int64_t) R0 + sc[u] + lane + NKP_WAVE) * K + k0) : make_double2 (0.0, 0.0);
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
         if (lane < lc[u])
            *reinterpret_cast<double2 *> (z + ((int64_t) R0 + sc[u] + lane) * K + k0) = make_double2 (t[u].x + lds[(c0 + u) * STRIDE + lane], t[u].y + lds[(gw + c0 + u) * STRIDE + lane]);
         if (NCH > 4 && lane + NKP_WAVE < lc[u])
            *reinterpret_cast<double2 *> (z + ((int64_t) R0 + sc[u] + lane + NKP_WAVE) * K + k0) =
               make_double2 (t2[u].x + lds[(c0 + u) * STRIDE + lane + NKP_WAVE], t2[u].y + lds[(gw + c0 + u) * STRIDE + lane + NKP_WAVE]);
      }
   }
}

// FOUR right-hand sides in one launch: a wave takes 16 of a group's 32 columns (block 2 g + h = half h of group g) for all four
// systems -- lane = system * 16 + column.  The factors are read once for the four systems (the 16 lanes of every system address
// the same 256 bytes), the staging moves whole 32-byte rows of the interleaved vectors.  The two-system kernel above takes two
// launches for K = 4 and its 33 KB of LDS per wave leave a colour's 1469 waves in 1.4 rounds of 4 per CU: 53 us per launch
// at 1 degree, slower per system than the single-vector kernel; here the same LDS holds 4 x 16 slots and the waves are twice as many.
template <int P, int NCH>
__global__ __launch_bounds__ (NKP_WAVE, 2)
void colblock_apply_ldspack4_kernel (const int *__restrict__ grp_maxlen, const long long *__restrict__ grp_base, int g_first,
                                     const float *__restrict__ fac_t, const double *__restrict__ rhs, double *__restrict__ z, int accumulate,
                                     const int *__restrict__ grp_row0, const int *__restrict__ col_slot, int ngrp, int K /* vectors interleaved */, int k0 /* first of this launch's four */)
{
   extern __shared__ double lds[];
   constexpr int gw = 32, hw = 16, CH = 16, STRIDE = NCH * CH + 1;
   rhs += k0;
   z += k0;
   constexpr LdspSchedule<NCH, P * CH, (P + 1) * CH> S;
   const int g = (int) (blockIdx.x >> 1) + g_first, half = blockIdx.x & 1;
   const int lane = threadIdx.x;
   const int ml = grp_maxlen[g];
   const int nch = ml / CH, mlq = ml >> 2;
   const int R0 = grp_row0[g];
   const int cl = half * hw + (lane & (hw - 1));             // this lane's column within the group
   const int s = col_slot[g * gw + cl], len = col_slot[(ngrp + g) * gw + cl];
   const float4 *f4 = reinterpret_cast<const float4 *> (fac_t + grp_base[g]) + cl;
   PackChunk<P> F[NCH], Bq[NCH];
#pragma unroll
   for (int t = 0; t < NCH; t++)
      if (t < S.f_upfront) ldsp_load_fwd<P> (F[t], f4, mlq, LDSP_FWD_K0 (t), gw);
#pragma unroll
   for (int t = 0; t < NCH; t++)
      if (t < S.b_upfront) ldsp_load_bwd<P> (Bq[t], f4, mlq, LDSP_BWD_K0 (t), gw);
   // slot (system q, column c) at (q * 16 + c) * STRIDE; one column per step, lane = row, the row's four values in two 16-byte loads
#pragma unroll
   for (int c0 = 0; c0 < hw; c0 += 4) {
      double2 ta[4], tb[4], ua[4], ub[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
         const int sc = __builtin_amdgcn_readlane (s, c0 + u), lc = __builtin_amdgcn_readlane (len, c0 + u);
         const double *src = rhs + ((int64_t) R0 + sc + lane) * K;
         ta[u] = (lane < lc) ? *reinterpret_cast<const double2 *> (src) : make_double2 (0.0, 0.0);
         tb[u] = (lane < lc) ? *reinterpret_cast<const double2 *> (src + 2) : make_double2 (0.0, 0.0);
         if (NCH > 4) {
            ua[u] = (lane + NKP_WAVE < lc) ? *reinterpret_cast<const double2 *> (src + (int64_t) NKP_WAVE * K) : make_double2 (0.0, 0.0);
            ub[u] = (lane + NKP_WAVE < lc) ? *reinterpret_cast<const double2 *> (src + (int64_t) NKP_WAVE * K + 2) : make_double2 (0.0, 0.0);
         }
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
         lds[(0 * hw + c0 + u) * STRIDE + lane] = ta[u].x;
         lds[(1 * hw + c0 + u) * STRIDE + lane] = ta[u].y;
         lds[(2 * hw + c0 + u) * STRIDE + lane] = tb[u].x;
         lds[(3 * hw + c0 + u) * STRIDE + lane] = tb[u].y;
         if (NCH > 4 && lane < STRIDE - 1 - NKP_WAVE) {
            lds[(0 * hw + c0 + u) * STRIDE + lane + NKP_WAVE] = ua[u].x;
            lds[(1 * hw + c0 + u) * STRIDE + lane + NKP_WAVE] = ua[u].y;
            lds[(2 * hw + c0 + u) * STRIDE + lane + NKP_WAVE] = ub[u].x;
            lds[(3 * hw + c0 + u) * STRIDE + lane + NKP_WAVE] = ub[u].y;
         }
      }
   }
   __syncthreads ();
   {
      double *col = lds + lane * STRIDE;                    // slot lane = (system, column)
      double w[P];
#pragma unroll
      for (int q = 0; q < P; q++) w[q] = 0.0;
#pragma unroll
      for (int c = 0; c < NCH; c++) {
         if (c < nch) ldsp_step_fwd<P> (F[c], col, c * CH, w);
#pragma unroll
         for (int t = 0; t < NCH; t++)
            if (t >= (c ? S.f_after[c - 1] : S.f_upfront) && t < S.f_after[c]) ldsp_load_fwd<P> (F[t], f4, mlq, LDSP_FWD_K0 (t), gw);
#pragma unroll
         for (int t = 0; t < NCH; t++)
            if (t >= (c ? S.b_after_f[c - 1] : S.b_upfront) && t < S.b_after_f[c]) ldsp_load_bwd<P> (Bq[t], f4, mlq, LDSP_BWD_K0 (t), gw);
      }
#pragma unroll
      for (int q = 0; q < P; q++) w[q] = 0.0;
#pragma unroll
      for (int j = 0; j < NCH; j++) {
         if (j < nch) ldsp_step_bwd<P> (Bq[j], col, (nch - 1 - j) * CH, w);
#pragma unroll
         for (int t = 0; t < NCH; t++)
            if (t >= (j ? S.b_after_b[j - 1] : S.b_after_f[NCH - 1]) && t < S.b_after_b[j]) ldsp_load_bwd<P> (Bq[t], f4, mlq, LDSP_BWD_K0 (t), gw);
      }
   }
#undef LDSP_FWD_K0
#undef LDSP_BWD_K0
   __syncthreads ();
#pragma unroll
   for (int c0 = 0; c0 < hw; c0 += 4) {
      double2 ta[4], tb[4], ua[4], ub[4];
      int sc[4], lc[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
         sc[u] = __builtin_amdgcn_readlane (s, c0 + u);
         lc[u] = __builtin_amdgcn_readlane (len, c0 + u);
         const double *src = z + ((int64_t) R0 + sc[u] + lane) * K;
         ta[u] = (accumulate && lane < lc[u]) ? *reinterpret_cast<const double2 *> (src) : make_double2 (0.0, 0.0);
         tb[u] = (accumulate && lane < lc[u]) ? *reinterpret_cast<const double2 *> (src + 2) : make_double2 (0.0, 0.0);
         if (NCH > 4) {
            ua[u] = (accumulate && lane + NKP_WAVE < lc[u]) ? *reinterpret_cast<const double2 *> (src + (int64_t) NKP_WAVE * K) : make_double2 (0.0, 0.0);
            ub[u] = (accumulate && lane + NKP_WAVE < lc[u]) ? *reinterpret_cast<const double2 *> (src + (int64_t) NKP_WAVE * K + 2) : make_double2 (0.0, 0.0);
         }
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
         double *dst = z + ((int64_t) R0 + sc[u] + lane) * K;
         if (lane < lc[u]) {
            *reinterpret_cast<double2 *> (dst) = make_double2 (ta[u].x + lds[(0 * hw + c0 + u) * STRIDE + lane], ta[u].y + lds[(1 * hw + c0 + u) * STRIDE + lane]);
            *reinterpret_cast<double2 *> (dst + 2) = make_double2 (tb[u].x + lds[(2 * hw + c0 + u) * STRIDE + lane], tb[u].y + lds[(3 * hw + c0 + u) * STRIDE + lane]);
         }
         if (NCH > 4 && lane + NKP_WAVE < lc[u]) {
            double *d2 = dst + (int64_t) NKP_WAVE * K;
            *reinterpret_cast<double2 *> (d2) = make_double2 (ua[u].x + lds[(0 * hw + c0 + u) * STRIDE + lane + NKP_WAVE], ua[u].y + lds[(1 * hw + c0 + u) * STRIDE + lane + NKP_WAVE]);
            *reinterpret_cast<double2 *> (d2 + 2) = make_double2 (ub[u].x + lds[(2 * hw + c0 + u) * STRIDE + lane + NKP_WAVE], ub[u].y + lds[(3 * hw + c0 + u) * STRIDE + lane + NKP_WAVE]);
         }
      }
   }
}

// ================================================================ selection, opt-in, launch
// f (kernel) for the single-vector instantiation the arguments name: the launcher passes the level's values, the opt-in walks the lists
template <class F>
static void with_ldspack_kernel (int P, int nch, F &&f)
{
   with_band (P, [&] (auto p) { with_int<4, 5> (nch, [&] (auto n) { f (colblock_apply_ldspack_kernel<decltype (p)::value, decltype (n)::value>); }); });
}

void colblock_ldspack_opt_in (int lds_bytes)
{
   for (int P : { 1, 2, 4 })
      for (int nch : { 4, 5 }) with_ldspack_kernel (P, nch, [&] (auto kernel) { colblock_opt_in ((const void *) kernel, lds_bytes); });
}

void launch_colblock_apply_ldspack (const ColBlocksDev &B, int g0, int g1, const double *r, double *z, int accumulate, hipStream_t st)
{
   const size_t lds = (size_t) B.lds_doubles * sizeof (double);
   with_ldspack_kernel (B.P, B.kern.nch, [&] (auto kernel) {
      hipLaunchKernelGGL (kernel, dim3 (g1 - g0), dim3 (NKP_WAVE), lds, st, B.grp_nb, B.grp_maxlen, B.grp_base, g0, (const float *) B.fac_tf, r, z, accumulate, B.grp_row0,
                          B.col_slot, B.ngrp);
   });
}

// groups [g0, g1) of a level whose layout is the packed one, K-interleaved right-hand sides: K / 4 launches of the four-system
// kernel or K / 2 of the two-system kernel, as col_plan.cpp chose for this K.  Returns non-zero (nothing launched) for a level
// that takes the wave-per-column batch kernel instead.
int launch_colblock_apply_lanes_batch (int K, const ColBlocksDev &B, int g0, int g1, const double *r, double *z, int accumulate, hipStream_t st)
{
   const int kind = K % 4 == 0 ? B.kern.batch4 : B.kern.batch_other;
   if (kind == COL_BATCH_WAVE) return 1;
   if (g1 <= g0) return 0;
   const size_t lds = (size_t) 64 * (size_t) (B.kern.nch * NKP_LDSRES_CH + 1) * sizeof (double);
   with_band (B.P, [&] (auto p) {
      constexpr int P = decltype (p)::value;
      with_int<4, 5> (B.kern.nch, [&] (auto nch_) {
         constexpr int NCH = decltype (nch_)::value;
         // four systems per launch, two waves (16 columns each) per group; K / 2 launches of the two-system kernel otherwise
         if (kind == COL_BATCH_LDSPACK4)
            for (int k0 = 0; k0 < K; k0 += 4)
               hipLaunchKernelGGL ((colblock_apply_ldspack4_kernel<P, NCH>), dim3 (2 * (g1 - g0)), dim3 (NKP_WAVE), lds, st, B.grp_maxlen, B.grp_base, g0,
                                   B.fac_tf, r, z, accumulate, B.grp_row0, B.col_slot, B.ngrp, K, k0);
         else
            for (int k0 = 0; k0 < K; k0 += 2)
               hipLaunchKernelGGL ((colblock_apply_ldspack2_kernel<P, NCH>), dim3 (g1 - g0), dim3 (NKP_WAVE), lds, st, B.grp_maxlen, B.grp_base, g0,
                                   B.fac_tf, r, z, accumulate, B.grp_row0, B.col_slot, B.ngrp, K, k0);
      });
   });
   return 0;
}
