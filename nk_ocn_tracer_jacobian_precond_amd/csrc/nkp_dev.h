// Internal device-side interfaces of libnkp_hip (gfx950 only).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nkp.h"
#include "col_plan.h"
#include "tuning.h"

#include <type_traits>
#include <utility>
#include <vector>

#define NKP_WAVE 64
#define NKP_MAX_K 512           // most basis vectors a fused update kernel takes (LDS coefficients)
#define NKP_SPMV_LDS_NNZ 2048    // CSR-stream row block: entries staged in LDS ...
#define NKP_SPMV_MAX_ROWS 256    // ... and rows (= threads of the SpMV workgroup) at most

// ---------------------------------------------------------------- CSR matrix on the device
// per-column diagonals (below): what one wave of the diagonal kernels needs of its tile, in aligned scalar loads (48 bytes)
struct alignas (16) DgTile {
   int row0, rows;                    // first row of the tile, its rows (<= 64)
   int kl0, len;                      // position of row0 inside its column, rows of the column
   int k0, nk;                        // the column's keys: dg_key[k0 .. k0 + nk)
   int g0, ng;                        // the column's groups of consecutive keys: dg_grp[g0 .. g0 + ng)
   long long voff;                    // the column's value block: dg_val[voff + s * len + kl]
};
// a run of m consecutive keys key0, key0 + 1, .. of a column, slots s0 .. s0 + m - 1 of it: one 64-lane window of x serves them
struct DgGroup {
   int key0;
   int slots;                         // s0 | m << 16
};
#define DG_RUN_MAX 5             // keys of a group at most

struct CsrDev {
   int64_t n = 0, nnz = 0;
   int *rowptr = nullptr;      // [n+1]
   int *colind = nullptr;      // [nnz]
   double *val = nullptr;      // [nnz]
   float *valf = nullptr;      // [nnz] optional f32 copy of val (preconditioner operators: f32 storage, f64 arithmetic)
   // CSR-stream row blocks: block b owns rows [rowblk[b], rowblk[b+1]) whose entries fit the
   // LDS staging buffer (or a single long row)
   int *rowblk = nullptr;      // [nrowblk+1]
   int nrowblk = 0;
   // optional 2-byte column codes (internal format; the int32 colind stays for the setup kernels and
   // as the fallback): entry e of row block b holds (row - rowblk[b]) | id << 8 and its column is
   // row + dict[dict_ptr[b] + id], the block's dictionary of distinct (column - row) offsets.
   // dict_ptr[b+1] == dict_ptr[b] marks a block whose dictionary would exceed 256 entries (plain path).
   unsigned short *codes = nullptr;   // [nnz]
   int *dict = nullptr;
   int *dict_ptr = nullptr;           // [nrowblk+1]
   // optional per-column diagonals of a level operator (tuning ml_diag) or of the solver's own A (tuning spmv_diag, f64 values
   // in dg_vald) (diagop.hip; all NULL = the operator runs on CSR).  Rows of a water
   // column are contiguous and depth-ordered, so with kl = the position of a row inside its column, colind - kl takes few
   // distinct values ("keys") over a column: one per (neighbour column, depth offset).  Column c keeps its keys ascending in
   // dg_key[dg_ptr[c] .. dg_ptr[c+1]) and one dense diagonal per key: dg_val[dg_voff[c] + s * len + kl] is the entry of row
   // kl in column key_s + kl, exactly 0.0f where the row has none.  Ascending keys = ascending columns within every row.
   int *dg_ptr = nullptr;             // [ncol+1]
   int *dg_key = nullptr;             // [dg_nkey = dg_ptr[ncol]] (+ 8 zeros behind them, which no kernel reads)
   long long *dg_voff = nullptr;      // [ncol]
   float *dg_val = nullptr;           // [dg_nval] (a level operator: the values of valf)
   double *dg_vald = nullptr;         // [dg_nval] (a matrix without valf, the solver's own A: the values of val); one of the two at most
   DgTile *dg_tile = nullptr;         // [dg_ntile] ceil (len / 64) per column, of equal heights (67 rows: 34 + 33), in row order
   // groups (pattern only, built once): column c cuts its keys into maximal runs of consecutive keys of at most DG_RUN_MAX and
   // at most 64 - rows + 1 keys (rows: of the column's tallest tile), so that row l of a tile finds x for the group's d-th key
   // in lane l + d <= 63 of one contiguous load of x.  A tile of 64 rows has groups of one key.
   int *dg_gptr = nullptr;            // [ncol+1]
   DgGroup *dg_grp = nullptr;         // [dg_ngrp = dg_gptr[ncol]]
   int dg_ntile = 0, dg_ncol = 0, dg_nkey = 0, dg_ngrp = 0;
   int64_t dg_nval = 0;
   const nkp_tuning *tune = nullptr;  // launch shape knobs of the owning solver (NULL: built-in defaults)
};

// host helper: build the codes for a CSR matrix and its row blocks; returns the fraction of entries coded
double build_spmv_codes_host (int64_t n, const int *rowptr, const int *colind, const int *rowblk, int nrowblk,
                              unsigned short **codes_out, int **dict_out, int *ndict_out, int **dict_ptr_out);
// upload them into A (device); 0 = ok
int attach_spmv_codes (CsrDev &A, const int *h_rowptr, const int *h_colind, const int *h_rowblk, size_t *device_bytes);

// y = A x (mode 0) or y = b - A x (mode 1)
void launch_csr_spmv (const CsrDev &A, const double *x, double *y, const double *b, int mode, hipStream_t st);
// rows of the row blocks [rb0, rb1) only: y_rows = b_rows - (A x)_rows  (Gauss-Seidel colour sweep)
void launch_csr_residual_range (const CsrDev &A, int rb0, int rb1, const double *x, const double *b, double *y, hipStream_t st);
// rows of the row blocks [rb0, rb1) only, any mode (0: y = A x, 1: y = b - A x, 2: y = |A||x| + |b|)
void launch_csr_spmv_range (const CsrDev &A, int rb0, int rb1, const double *x, double *y, const double *b, int mode, hipStream_t st);
// y = |A| |x| + |b|   (denominator of the componentwise backward error)
void launch_csr_abs_spmv (const CsrDev &A, const double *x, const double *b, double *y, hipStream_t st);
// ---- per-column diagonals (diagop.hip)
// Build the layout of L from its CSR arrays (the f32 values valf into dg_val; without valf the f64 values val into dg_vald) if
// every column gets by with at most cap keys, no column is longer than 256 rows and the padded slots stay within 1.5 nnz;
// h_blk_start / d_blk_start: row offsets of the ncol columns, the first ncol0 of them colour 0.  Returns 1 (built:
// color_tile[c] .. color_tile[c+1] are colour c's tiles) or 0 (L stays on CSR: not eligible, or out of device memory, which is
// answered here).
int diag_build (CsrDev &L, const int *h_blk_start, const int *d_blk_start, int ncol, int ncol0, int max_len, int cap, int color_tile[3],
                size_t *device_bytes, hipStream_t st);
// dg_val from L.valf, dg_vald from L.val (new values on the same pattern)
void launch_diag_fill (const CsrDev &L, hipStream_t st);
// rows of the tiles [tile0, tile1): y_rows = b_rows - (L x)_rows, every row summed in stored order like the CSR kernels
void launch_diag_residual (const CsrDev &L, int tile0, int tile1, const double *x, const double *b, double *y, hipStream_t st);
// all rows of a matrix with f64 diagonals (dg_vald): y = A x (mode 0) or y = b - A x (mode 1), the bits of launch_csr_spmv
void launch_diag_spmv (const CsrDev &A, const double *x, double *y, const double *b, int mode, hipStream_t st);
// host helper: greedy row-block partition (host arrays)
void build_rowblocks_host (int64_t n, const int *rowptr, int **rowblk_out, int *nrowblk_out);

// nkp_value_gradient (valgrad.hip): g[e] (+)= alpha * sum_{c < nk} lam_c[row of e] * x_c[colind[e]] on the pattern of A, the sum taken
// in ascending c, every product and sum rounded.  K in {1, 2, 4, 8}: interleave width of lam and x (1 = plain vectors), nk <= K
void launch_value_gradient (int K, int nk, const CsrDev &A, const double *lam, const double *x, double alpha, int accumulate, double *g, hipStream_t st);
// nkp_values_product (valprod.hip): y_c[i] (+)= alpha * sum_e val[e] * x_c[colind[e]] over the stored entries of row i in stored order, c < nk,
// with the bits of the SpMV kernels on a matrix that stores val.  K in {1, 2, 4, 8}: interleave width of x (1 = a plain vector), nk <= K;
// y is column-major, vector c at c * ldy.  Every row is written, also of a matrix without entries
void launch_values_product (int K, int nk, const CsrDev &A, const double *val, const double *x, double alpha, int accumulate, double *y, int64_t ldy, hipStream_t st);
// nkp_values_product_trans (valprod.hip): the same kernel text on the pattern T of A^T (rowptr, colind, rowblk only), the value of its entry p
// gathered from val[src[p]] -- val stays in A's order; the bits of the SpMV kernels on a matrix that stores the transposed values
void launch_values_product_trans (int K, int nk, const CsrDev &T, const int *src, const double *val, const double *x, double alpha, int accumulate, double *y,
                                  int64_t ldy, hipStream_t st);
// nkp_values_product_trans_dist (valprod.hip): the same on the row block of A^T a rank assembled; src[p] < 0 marks a product a peer shipped,
// which sits in x at row T.colind[p] and takes the value 1.0
void launch_values_product_trans_recv (int K, int nk, const CsrDev &T, const int *src, const double *val, const double *x, double alpha, int accumulate, double *y,
                                       int64_t ldy, hipStream_t st);
// nkp_residual_batch (residual.hip): one pass over A for c < nk: r_c = b_c - A x_c into R (column-major, vector c at c * ldr; NULL: not
// stored; may be B, never x) and out[c] = sum r_c^2, out[K + c] = sum b_c^2, out[2 K + c] = max_or_nan over the rows of |r| / (|A||x| + |b|)
// by berr_kernel's rule; the rows' sums have the bits of the SpMV kernels (modes 0 and 2).  K in {1, 2, 4, 8}: interleave width of x
// (1 = a plain vector), nk <= K; columns c >= nk of out get +0.0.  partial: 3 K doubles per row block of A
void launch_residual_batch (int K, int nk, const CsrDev &A, const double *x, const double *B, int64_t ldb, double *R, int64_t ldr, double *partial, double *out,
                            hipStream_t st);

// ---------------------------------------------------------------- water-column blocks
// Banded LU (no pivoting) of every diagonal block, half-bandwidth P in {1,2,4}; SoA by
// diagonal: fac[(d+P)*n + row] holds, for d<0 the L multiplier l(row,row+d), for d=0 the
// RECIPROCAL of the U diagonal, for d>0 u(row,row+d).
struct ColBlocksDev {
   int64_t n = 0;
   int nblk = 0;
   int *blk_start = nullptr;   // [nblk+1]
   int P = 0;                  // half bandwidth actually stored
   int max_len = 0;            // longest block
   int dropped = 0;            // 1 if in-block entries beyond the band were dropped
   double *fac = nullptr;      // [(2P+1)*n]
   // lane-per-column layout for the apply kernel: groups of <= 64 consecutive blocks; group g's
   // factors live at fac_t + grp_base[g] as [(2P+1)][grp_maxlen[g]][64] (coalesced per step k)
   int ngrp = 0;
   int *grp_b0 = nullptr;      // [ngrp] first block of the group
   int *grp_nb = nullptr;      // [ngrp] blocks in the group (<= 64)
   int *grp_maxlen = nullptr;  // [ngrp] longest block of the group
   long long *grp_base = nullptr;   // [ngrp] offset into fac_t (doubles)
   int *grp_row0 = nullptr;    // [ngrp] first row of the group, [ngrp..2ngrp) its row count (no dependent blk_start lookups)
   int *col_slot = nullptr;    // [ngrp*gw] row offset of lane's column inside the group, [ngrp*gw..) its length
   double *fac_t = nullptr;
   float *fac_tf = nullptr;    // same layout in f32 (preconditioner: f32 storage, f64 arithmetic)
   int lds_doubles = 0;        // LDS staging need of the largest group (padded)
   int gw = 64;                // columns (lanes in use) per group
   int rhs_slots = 0;          // LDS doubles reserved for the staged right-hand side
   // fused Gauss-Seidel half sweep (gs_fused_kernel): row blocks of every group's rows
   int stream = 0;             // 1: 64 columns per wave, factors read straight from HBM (colblock_apply_stream_kernel)
   int ldsres = 0;             // 1: 32 columns per wave, factors streamed, the column resident in LDS (colblock_apply_ldsres_kernel);
                               // 2: the same with the factors packed four steps to a load and a static prefetch schedule (colblock_apply_ldspack_kernel)
   int gs_ok = 0;              // 1 if the level can run it (no row longer than GS_NNZ, LDS need within 64 KB)
   int gs_lds_bytes = 0;
   int *gs_rb_ptr = nullptr;   // [ngrp+1] first row-block boundary of the group
   int *gs_rb = nullptr;       // row-block boundaries (rows), groups back to back
   int *wave_desc = nullptr;   // levels run by gs_wave_kernel: per column {first row, rows, first entry, entries} -- one load instead of two dependent ones
   int *grp_tile = nullptr;    // kern.lane_fused: [ngrp*gw] the tile of the level operator's diagonals that is the lane's column, -1 = none (pattern only)
   int grp_tile_cnt = 0;       // ... the tiles the map counts on: columns with rows, each one tile
   const nkp_tuning *tune = nullptr;   // kernel selection knobs of the owning solver (NULL: built-in defaults)
   int ml_level = 0;           // 1: a level of the multilevel cycle (set before the layout is built), which may run one column per wave
   ColKernel kern;             // the kernel choice col_plan resolved when the layout was built: what the launchers branch on
   // HOST: the columns of every group's lanes when the groups were formed from sorted columns (else NULL), for the repack of
   // nkp_refactor.  Owned, shared with clones and freed like the device arrays above
   std::vector<int> *grp_cols = nullptr;
};

// ---------------------------------------------------------------- kernel selection (host side)
// A launcher turns each run-time value that picks a kernel instantiation into a compile-time tag and names the kernel, with its
// argument list, once inside a generic lambda:
//    with_band (B.P, [&] (auto p) { constexpr int P = decltype (p)::value; hipLaunchKernelGGL ((kernel<P>), ...); });
// The lambda's body is compiled for every value of the list, so nested selectors instantiate the product of their lists
// (`if constexpr` on a tag leaves out a combination that has no kernel).  The lambda's result, if any, is passed on.

template <int V> using int_tag = std::integral_constant<int, V>;
// f (int_tag<V>) for the first V of the list that v equals; any other v takes the last one
template <int V0, int... Vs, class F>
inline auto with_int (int v, F &&f)
{
   if constexpr (sizeof... (Vs) == 0) return f (int_tag<V0> ());
   else {
      if (v == V0) return f (int_tag<V0> ());
      return with_int<Vs...> (v, f);
   }
}
template <class F> inline auto with_band (int P, F &&f) { return with_int<1, 2, 4> (P, f); }   // half bandwidth stored
template <class F> inline auto with_k (int K, F &&f) { return with_int<2, 4, 8> (K, f); }       // interleaved right-hand sides
template <class F> inline auto with_bool (bool b, F &&f) { return b ? f (std::true_type ()) : f (std::false_type ()); }
// f (vf) when the f32 copy exists, f (vd) otherwise; inside, elem_t<decltype (v)> is the storage type of the pointer f was given
template <class F> inline auto with_storage (const float *vf, const double *vd, F &&f) { return vf ? f (vf) : f (vd); }
template <class PTR> using elem_t = std::remove_cv_t<std::remove_pointer_t<PTR>>;
// wave-per-column kernels: f (band tag, rows-per-lane tag) -- a lane holds one row of a column, two where a column can exceed the wave
template <class F>
inline auto with_band_rows (const ColBlocksDev &B, F &&f)
{
   return with_band (B.P, [&] (auto p) { return with_int<1, 2> (B.max_len <= NKP_WAVE ? 1 : 2, [&] (auto rpl) { return f (p, rpl); }); });
}

// ---------------------------------------------------------------- band substitution, one water column per wave (device side)
// f (int_tag<0>), ..., f (int_tag<N - 1>) in this order: the index is a constant inside every call
template <int... Is, class F>
__device__ __forceinline__ void static_for_seq (std::integer_sequence<int, Is...>, F &&f) { (f (int_tag<Is> ()), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for (F &&f) { static_for_seq (std::make_integer_sequence<int, N> (), f); }

template <int LANE>
__device__ __forceinline__ double readlane_const_f64 (double v)
{
   int lo = __double2loint (v), hi = __double2hiint (v);
   lo = __builtin_amdgcn_readlane (lo, LANE);
   hi = __builtin_amdgcn_readlane (hi, LANE);
   return __hiloint2double (hi, lo);
}

// the same for a wave-uniform lane that is no constant
__device__ __forceinline__ double readlane_f64 (double v, int lane)
{
   int lo = __double2loint (v), hi = __double2hiint (v);
   lo = __builtin_amdgcn_readlane (lo, lane);
   hi = __builtin_amdgcn_readlane (hi, lane);
   return __hiloint2double (hi, lo);
}

// y <- (LU)^-1 y for the column a wave holds: lane l owns row s * 64 + l in y[s][.] (RPL = 2: columns of 65-128 rows), K
// right-hand sides side by side, L[s][q - 1] = l(r, r - q), U[s][q - 1] = u(r, r + q), invd = 1 / u(r, r), all zero behind
// the column's end.  Both sweeps are written out step by step, so the lane a step broadcasts and the lanes it updates are
// constants: no lane compare or register select sits between two broadcasts, only
//    forward:   v_readlane (y_k) -> multiply by l(k+1, k) -> subtract -> v_readlane (y_{k+1})
//    backward:  v_readlane (x_k) -> multiply by u(k-1, k) -> subtract -> multiply by invd -> v_readlane (x_{k-1})
// computed on all lanes, of which the next step reads the one that is complete; the masked write into y and the updates of
// the rows further off (q >= 2) are issued behind that and are off the chain.  Each step is guarded by the wave-uniform
// k < len - 1 (forward) or k < len (backward), so no step runs beyond the column's end.  Per row the operations and their
// order are those of the lane-per-column kernels: row r takes - l(r, r-q) y_{r-q} for q = P first down to q = 1, then
// - u(r, r+q) x_{r+q} for q = P first down to q = 1, then * invd; a product and a difference each rounded (no FMA).
template <int P, int RPL, int K>
__device__ __forceinline__ void wave_band_sweeps (int len, int lane, double (&y)[RPL][K], const double (&invd)[RPL], const double (&L)[RPL][P],
                                                  const double (&U)[RPL][P])
{
   constexpr int ROWS = RPL * NKP_WAVE;
   len = __builtin_amdgcn_readfirstlane (len);
   double bc[K];                                   // the step's broadcast: y_k, then x_k
#pragma unroll
   for (int j = 0; j < K; j++) bc[j] = readlane_const_f64<0> (y[0][j]);
   static_for<ROWS - 1> ([&] (auto kc) __attribute__ ((always_inline)) {
      constexpr int k = decltype (kc)::value;
      if (__builtin_expect (k < len - 1, 1)) {
         constexpr int s1 = (k + 1) / NKP_WAVE, l1 = (k + 1) % NKP_WAVE;
         double t[K], nb[K];
#pragma unroll
         for (int j = 0; j < K; j++) {
            t[j] = y[s1][j] - L[s1][0] * bc[j];             // row k + 1 is complete in lane l1
            nb[j] = readlane_const_f64<l1> (t[j]);
         }
#pragma unroll
         for (int j = 0; j < K; j++) y[s1][j] = lane == l1 ? t[j] : y[s1][j];
#pragma unroll
         for (int q = 2; q <= P; q++)
            if (k + q < ROWS) {
               const int s = (k + q) / NKP_WAVE, l = (k + q) % NKP_WAVE;
#pragma unroll
               for (int j = 0; j < K; j++) {
                  const double u = y[s][j] - L[s][q - 1] * bc[j];
                  y[s][j] = lane == l ? u : y[s][j];
               }
            }
#pragma unroll
         for (int j = 0; j < K; j++) bc[j] = nb[j];
      }
   });
   // (the backward guards test a copy of len the compiler cannot see through: left to itself it keeps every forward guard's
   // outcome in a register pair for the backward sweep and spills them)
   asm volatile ("" : "+s" (len));
   // c: lane k holds row k with its subtractions done when step k begins; the sweep enters at row len - 1
   double c[K];
#pragma unroll
   for (int j = 0; j < K; j++) {
      c[j] = y[0][j];
      if (RPL == 2 && len > NKP_WAVE) c[j] = y[RPL - 1][j];
   }
   static_for<ROWS> ([&] (auto ic) __attribute__ ((always_inline)) {
      constexpr int k = ROWS - 1 - decltype (ic)::value;
      if (__builtin_expect (k < len, 1)) {
         constexpr int s0 = k / NKP_WAVE, l0 = k % NKP_WAVE;
         double v[K];
#pragma unroll
         for (int j = 0; j < K; j++) {
            v[j] = c[j] * invd[s0];                           // x_k in lane l0
            bc[j] = readlane_const_f64<l0> (v[j]);
         }
         if (k > 0) {
            constexpr int s1 = (k > 0 ? k - 1 : 0) / NKP_WAVE;
#pragma unroll
            for (int j = 0; j < K; j++) c[j] = y[s1][j] - U[s1][0] * bc[j];
         }
#pragma unroll
         for (int j = 0; j < K; j++) y[s0][j] = lane == l0 ? v[j] : y[s0][j];
#pragma unroll
         for (int q = 2; q <= P; q++)
            if (k - q >= 0) {
               const int s = (k - q) / NKP_WAVE, l = (k - q) % NKP_WAVE;
#pragma unroll
               for (int j = 0; j < K; j++) {
                  const double u = y[s][j] - U[s][q - 1] * bc[j];
                  y[s][j] = lane == l ? u : y[s][j];
               }
            }
      }
   });
}

// Build the lane-per-column layout.  ranges: nranges+1 block offsets; a group never straddles a
// range boundary (Gauss-Seidel colours).  grp_first[r] = first group of range r (nranges+1 out).
// Returns 0 or a HIP error code cast to int.
int colblock_build_lane_layout (ColBlocksDev &B, const int *h_blk_start, const int *ranges, int nranges,
                                int *grp_first, size_t *device_bytes, hipStream_t st, int f32 = 0, const int *h_rowptr = nullptr);
// new factors (B.fac) into the layout built above, which depends on the pattern only (nkp_refactor).  d_gcols: a device
// copy of *B.grp_cols when the groups were formed from sorted columns, else NULL
int colblock_repack_lane_layout (const ColBlocksDev &B, const int *d_gcols, hipStream_t st);
// one Gauss-Seidel half sweep over the groups [g0, g1) of one colour in ONE launch: r = b - L x on the groups' rows
// (x rows < split from xa, the others from xb), column solves, xout_rows = x_rows + z.  Returns non-zero (and does
// nothing) when the level cannot run the fused kernel.
int launch_gs_fused (const CsrDev &L, const ColBlocksDev &B, int g0, int g1, const double *xa, const double *xb, int split,
                     const double *b, double *xout, hipStream_t st);
// groups [g0, g1): z (+)= M^-1 r, one water column per LANE, rhs staged through LDS
void launch_colblock_apply_lanes (const ColBlocksDev &B, int g0, int g1, const double *r, double *z, int accumulate, hipStream_t st);

// max over blocks of the in-block half bandwidth and of the block length (device reduction)
void launch_colblock_measure (const CsrDev &A, const ColBlocksDev &B, int *d_out2 /* [bw, zero_diag_rows] */, hipStream_t st);
// extract + factor; *d_status receives the first row with a (near-)zero pivot + 1, else 0
void launch_colblock_factor (const CsrDev &A, ColBlocksDev &B, int *d_status, hipStream_t st);
// z = M^-1 r
void launch_colblock_apply (const ColBlocksDev &B, const double *r, double *z, hipStream_t st);
// blocks [b0, b1) only; accumulate: z_blk += M_blk^-1 r_blk, else z_blk = M_blk^-1 r_blk
void launch_colblock_apply_range (const ColBlocksDev &B, int b0, int b1, const double *r, double *z, int accumulate, hipStream_t st);
void launch_colblock_apply_range_r32 (const ColBlocksDev &B, int b0, int b1, const double *r, double *z, int accumulate, hipStream_t st);
// blocks [b0, b1) of one colour in ONE launch, one column per wave: xout_rows = x_rows + M_blk^-1 (b - L x)_rows, x taken from
// xa (rows < split) and xb (the others); r32 as above
void launch_build_wave_desc (const CsrDev &L, ColBlocksDev &B, hipStream_t st);   // fills B.wave_desc (allocated by the caller: 4 ints per column)
void launch_gs_wave (const CsrDev &L, const ColBlocksDev &B, int b0, int b1, const double *xa, const double *xb, int split, const double *b, double *xout,
                     int r32, hipStream_t st);
// the same half sweep on L's per-column diagonals (diagop.hip), tiles [tile0, tile1) of one colour, for a level whose columns
// are one tile each (at most 64 rows): the bits of launch_gs_wave
void launch_gs_wave_diag (const CsrDev &L, const ColBlocksDev &B, int tile0, int tile1, const double *xa, const double *xb, int split, const double *b,
                          double *xout, int r32, hipStream_t st);
// the same half sweep for a level on the packed lane-per-column layout (col_gs_lanes.hip), groups [g0, g1) of one colour: L on its
// diagonals, B.grp_tile built, columns of at most 64 rows, P <= 2 (B.kern.lane_fused); the bits of launch_diag_residual +
// launch_colblock_apply_lanes
void launch_gs_lanes_diag (const CsrDev &L, const ColBlocksDev &B, int g0, int g1, const double *xa, const double *xb, int split, const double *b,
                           double *xout, hipStream_t st);

// ---------------------------------------------------------------- BLAS-1 style kernels
#define NKP_BATCH_MAX 8            // right-hand sides per sweep at most (interleave widths 2, 4, 8)
#define NKP_RED_BLOCKS 1024        // partial sums per reduction (fixed => deterministic)
#define NKP_DOT_CHUNK 8

// partial[(chunk*NKP_RED_BLOCKS + blk)*8 + c] ; then finish sums over blk in fixed order
// out[j] = sum_i V[j*ld+i] * w[i]  j<k ;  out[k] = sum_i w[i]^2
void launch_multi_dot (const void *V, int v_f32, int64_t ld, int k, const double *w, int64_t n, double *partial, double *out, hipStream_t st);
// w -= sum_j h[j] V_j (j<k);  out_nrm2[0] = ||w_new||^2 (via partial, deterministic)
void launch_update_w (const void *V, int v_f32, int64_t ld, int k, const double *h, double *w, int64_t n, double *partial, double *out_nrm2, hipStream_t st);
// y = alpha[0] * x   (alpha on device)
void launch_scale_to (const double *x, const double *alpha_dev, double *y, float *yf, int64_t n, hipStream_t st);
// x += sum_j c[j] Z_j (j<k)   (c on device)
void launch_axpy_multi (const double *Z, int64_t ld, int k, const double *c, double *x, int64_t n, hipStream_t st);
// out[0] = sum x_i*y_i
void launch_dot (const double *x, const double *y, int64_t n, double *partial, double *out, hipStream_t st);
// out[0] = max_i |r_i| / den_i  (den_i == 0 -> ignored when r_i == 0); NaN when any r_i or den_i is NaN, or both are Inf
void launch_berr (const double *r, const double *den, int64_t n, double *partial, double *out, hipStream_t st);
// out[0] = number of NaN / Inf entries of x, out[1] = number of entries != 0 (partial: 2 * NKP_RED_BLOCKS doubles)
void launch_count_entries (const double *x, int64_t n, double *partial, double *out, hipStream_t st);
// small device-side scalar programs of the Krylov drivers
// h[j] += h2[j] (j<k); h[k] = sqrt(nrm2); inv[0] = 1/h[k] (0 if h[k]==0)
void launch_finish_column (double *h, const double *h2, int k, const double *nrm2, double *inv, hipStream_t st);
// the same behind a launch_update_w with out_nrm2 = NULL (tuning step_glue bit 8): adds up that launch's partial sums of the n-vector
// itself (to nrm2_out, same order) and stores h[0 .. k] to host_col too, pinned host memory
void launch_finish_column_host (double *h, const double *h2, int k, const double *partial, int64_t n, double *nrm2_out, double *inv, double *host_col, hipStream_t st);
void launch_finish_column_pythagoras (double *h, int k, double *inv, hipStream_t st);
// The Gram-Schmidt kernels above for a group of R systems in one launch each (batched solve of the row-distributed flavour):
// system r has its own basis, w and partial sums; its dots form row r of ONE message msg[r * (k + 1) + j] (j <= k) that a
// single allreduce reduces for the group.  Per system the operations and their order are those of the kernels above.
struct GsGroup {
   const double *V[NKP_BATCH_MAX];
   double *w[NKP_BATCH_MAX];
   double *partial[NKP_BATCH_MAX];
   double *vnext[NKP_BATCH_MAX];
};
void launch_multi_dot_group (int R, const GsGroup &G, int64_t ld, int k, int64_t n, double *msg, hipStream_t st);
// w_r -= V_r msg[r]; nrm2[r] = ||w_r||^2
void launch_update_w_group (int R, const GsGroup &G, int64_t ld, int k, const double *msg, int64_t n, double *nrm2, hipStream_t st);
// msg[r][j] += msg2[r][j] (msg2 != NULL); msg[r][k] = sqrt (nrm2[r]); inv[r] = 1 / msg[r][k]; or the Pythagoras form (nrm2 NULL)
void launch_finish_column_group (int R, double *msg, const double *msg2, int k, const double *nrm2, double *inv, hipStream_t st);
// vnext_r = inv[r] * w_r
void launch_scale_to_group (int R, const GsGroup &G, const double *inv, int64_t n, hipStream_t st);
// y = a*x + b*y style helpers for BiCGStab
void launch_axpby (double a, const double *x, double b, double *y, int64_t n, hipStream_t st);
void launch_copy (const double *x, double *y, int64_t n, hipStream_t st);
// y[i] = x[i] * w[i]   (y may alias x)
void launch_vmul (const double *x, const double *w, double *y, int64_t n, hipStream_t st);
void launch_fill (double *y, double v, int64_t n, hipStream_t st);

// ---------------------------------------------------------------- grid transfer / permutation
// coarse[I] = sum_{q in [rptr[I], rptr[I+1])} fine[ridx[q]]   (restriction = P^T, fixed order)
// coarse_x (tuning step_glue bit 4): also zeroed, nc doubles
void launch_restrict_sum (const int *rptr, const int *ridx, const double *fine, double *coarse, int64_t nc, hipStream_t st, double *coarse_x = nullptr);
// vnext[perm[i]] = b0[i] = w[perm[i]] * inv[0], x0[i] = 0 (tuning step_glue bit 8)
void launch_cycle_entry (const int *perm, const double *w, const double *inv, double *vnext, double *b0, double *x0, int64_t n, hipStream_t st);
// fine[i] += coarse[cmap[i]]                                  (prolongation = P)
void launch_prolong_add (const int *cmap, const double *coarse, double *fine, int64_t nf, double omega, hipStream_t st);
// out[i] = in[perm[i]]
void launch_gather (const int *perm, const double *in, double *out, int64_t n, hipStream_t st);
// out[perm[i]] = in[i]
void launch_scatter (const int *perm, const double *in, double *out, int64_t n, hipStream_t st);
// y = Minv x, dense row-major n x n (coarsest level)
void launch_dense_matvec (const double *Minv, const double *x, double *y, int n, hipStream_t st);
void launch_dense_matvec_f32 (const float *Minv, int ld, const double *x, double *y, int n, hipStream_t st);
void launch_dense_matvec_f32_batch (int K, const float *Minv, int ld, const double *x, double *y, int n, hipStream_t st);
int dense_inverse_blocked_device (int n, const int *h_rowptr, const int *h_col, const double *h_val, double **inv_out, float **invf_out, int *ldf_out,
                                  size_t *bytes, hipStream_t st);
// the pivoted routine: unblocked Gauss-Jordan with partial pivoting on the dense matrix host_a (row-major n x n); *inv_out
// receives a device buffer with the inverse; false if singular / no memory
bool dense_inverse_device (int n, const std::vector<double> &host_a, double **inv_out, size_t *bytes, hipStream_t st);

// ---------------------------------------------------------------- K interleaved right-hand sides (batch.hip; X[i * K + k], K = 2 or 4)
// scale (may be NULL), here and below: the row scaling of the row-weighted iteration folded into the kernel, one rounded
// multiplication per value (what launch_vmul does): on the way in src_k[i] * scale[i], on the way out (A x)_i * scale[i]
void launch_interleave (int K, const double *const *src /* K pointers, NULL = zeros */, double *X, int64_t n, hipStream_t st, const double *scale = nullptr);
void launch_deinterleave (int K, const double *X, double *const *dst /* K pointers, NULL = skip */, int64_t n, hipStream_t st);
// row blocks [rb0, rb1) of A: y = A x (mode 0) or y = b - A x (mode 1) on K columns
void launch_csr_spmv_batch (int K, const CsrDev &A, int rb0, int rb1, const double *x, double *y, const double *b, int mode, hipStream_t st,
                            const double *scale = nullptr /* mode 0 only */);
void launch_restrict_sum_batch (int K, const int *rptr, const int *ridx, const double *fine, double *coarse, int64_t nc, hipStream_t st);
void launch_prolong_add_batch (int K, const int *cmap, const double *coarse, double *fine, int64_t nf, double omega, hipStream_t st);
void launch_gather_batch (int K, const int *perm, const double *in, double *out, int64_t n, hipStream_t st);
// out[i * K + k] = src_k[idx[i]], the entry of a batched cycle or the rows of a K-wide message; the
// exit: z[perm[i] * K + k] = dst_k[perm[i]] = in[i * K + k]
void launch_gather_interleave (int K, const int *idx, const double *const *src, double *out, int64_t n, hipStream_t st, const double *scale = nullptr);
void launch_scatter_split (int K, const int *perm, const double *in, double *z, double *const *dst, int64_t n, hipStream_t st);
void launch_csr_spmv_batch_split_range (int K, const CsrDev &A, int rb0, int rb1, const double *x, double *const *dst, hipStream_t st, const double *scale = nullptr);
// chained cycles: dst_k = b_k - A x_k from and to per-system vectors (b_k times bscale when given; dst_k NULL: system k takes no
// part), and z_k += p_k on the interleaved z and the systems' own vectors at once (dst_k NULL: column k of z stays as it is)
void launch_csr_residual_batch_split_range (int K, const CsrDev &A, int rb0, int rb1, const double *x, const double *const *b, const double *bscale,
                                            double *const *dst, hipStream_t st);
void launch_add_split (int K, const double *p, double *z, double *const *dst, int64_t n, hipStream_t st);
// row-distributed flavour: the entry / exit of a batched cycle on the extended rows [own | overlap] (overlap rows read from the
// K-interleaved rows ext: the halo at sel[.], or with sel NULL a block of the overlap rows alone; only own rows written back)
void launch_gather_interleave_ext (int K, const int *perm, const double *const *src, const double *ext, const int *sel, int64_t n_own, double *out, int64_t n,
                                   hipStream_t st);
void launch_scatter_split_own (int K, const int *perm, const double *in, double *z, double *const *dst, int64_t n_own, int64_t n, hipStream_t st);
void launch_dense_matvec_batch (int K, const double *Minv, const double *x, double *y, int n, hipStream_t st);
// water-column solves of blocks [b0, b1), one column per wave / the fused half sweep, K columns
void launch_colblock_apply_wave_batch (int K, const ColBlocksDev &B, int b0, int b1, const double *r, double *z, int accumulate, int r32, hipStream_t st);
void launch_gs_wave_batch (int K, const CsrDev &L, const ColBlocksDev &B, int b0, int b1, const double *xa, const double *xb, int split, const double *b, double *xout,
                           int r32, hipStream_t st);
// groups [g0, g1) with the packed lane layout (col_packed.hip); non-zero = the level takes the wave kernel (B.kern.batch4 / batch_other)
int launch_colblock_apply_lanes_batch (int K, const ColBlocksDev &B, int g0, int g1, const double *r, double *z, int accumulate, hipStream_t st);
