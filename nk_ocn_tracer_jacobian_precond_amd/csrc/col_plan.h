// Lane-per-column band solves: which kernel serves a level and how its columns are grouped (col_plan.cpp).  Plain C++, no
// HIP: the rule is integer arithmetic on the column lengths and the nkp_tuning, written once here and run on the CPU by
// tests/col_plan_main.cpp.  The device units (col_layout.hip and the kernel families) upload the tables and branch on ColKernel.
#pragma once
#include "../../include/nkp.h"

#include <vector>

#define NKP_LDSRES_CH 16         // substitution steps per factor chunk of colblock_apply_ldsres_kernel (group lengths are padded to it)
#define GS_THREADS 256           // gs_fused_kernel: threads of a workgroup = rows of a row block at most
#define GS_NNZ 2048              // ... and the entries of a row block at most (products parked in LDS)
#define LDS_PAD(i) ((i) + ((i) >> 5))       // break the lane stride (column length) bank pattern

#define COL_GROUP_LDS_BYTES (56 * 1024)      // col_group is halved until a group's staged factors + right-hand side fit this: LDS several times per CU
#define COL_LDS_DEFAULT_BYTES (48 * 1024)    // dynamic LDS a kernel gets without an opt-in (hipFuncSetAttribute)
#define COL_GS_LDS_BYTES (64 * 1024)         // gs_fused_kernel: beyond it, not worth running one workgroup per CU
#define COL_LDS_MAX_BYTES (160 * 1024)       // LDS of a CU: a layout that needs more is refused
// fewest columns of a level that uses the streamed kernel (col_stream_min < 0).  Measured at 1 degree (93 MB per colour of
// the fine level): 8 columns per wave with LDS-staged factors 44.7 us, 64 streamed 33.6 us, 32 streamed 26.2 us (3.55 TB/s);
// on levels below ~50 000 columns the fewer, longer waves of the streamed kernel lose to the small-group kernel (whole cycle
// 2.69 -> 2.52 ms with the fine level only, 2.55 with the first two levels, 2.61 with three)
#define COL_STREAM_MIN_COLS 50000
// the column resident in LDS (colblock_apply_ldsres_kernel): the default from 20 000 columns (8000 when the columns are
// longer than 64 levels, where the alternative runs at half the rate).  Same box, 1 degree, cycle time twice each:
// LDS-resident on levels 0 and 1: 2.385 / 2.394 ms; streamed on level 0, small groups on level 1: 2.410 / 2.427;
// streamed on level 0, LDS-resident on level 1: 2.434 / 2.409.  NKP_COL_LDSRES=1 keeps it to the long columns (and
// the streamed kernel on the largest levels), =0 switches it off.
#define COL_LDSRES_MIN_COLS 20000
#define COL_LDSRES_MIN_COLS_LONG 8000

enum ColFamily {
   COL_LANES = 0,      // gw <= 64 columns per wave, factors staged in LDS (colblock_apply_lanes_kernel, ..._lanes_pipe_kernel)
   COL_STREAM,         // 32 or 64 columns per wave, factors read straight from HBM, the column in registers (colblock_apply_stream_kernel)
   COL_LDSRES,         // 32 columns per wave, factors streamed, the column resident in LDS (colblock_apply_ldsres_kernel)
   COL_LDSPACK         // the same with the factors packed four steps to a load and a static prefetch schedule (colblock_apply_ldspack_kernel)
};
enum ColBatch { COL_BATCH_WAVE = 0, COL_BATCH_LDSPACK2, COL_BATCH_LDSPACK4 };   // K interleaved right-hand sides: one column per wave, or the packed kernels

// the resolved kernel choice of a level: what the launchers branch on (ColBlocksDev carries a copy)
struct ColKernel {
   int family = COL_LANES;
   int maxl = 64, wpe = 1;     // COL_LANES: <P, MAXL, FT, WPE> is <., 64, ., 1> up to 64 rows, <., 80, ., 3> up to 80 rows with col_w3, else <., 128, ., 1>
   int nch = 4;                // COL_LDSPACK: chunks of 16 steps (4 up to 64 rows, else 5)
   // col_ldsres_early = 1: first factor chunks and the accumulate target requested before the right-hand side is staged
   // (247 instead of 172 VGPRs).  Measured twice on one box: 26.9 / 26.6 us per colour of the 1 degree fine level with it,
   // 26.8 / 27.0 without -- no difference, so it stays off
   int early = 0;              // COL_LDSRES: the EARLY instantiation
   // pipelined persistent variant: f32 factors, <= 64 levels, 8 columns per wave, band <= 2, LDS within the default limit.
   // OFF unless col_pipe_min = <groups> is set: it needs 256 VGPRs (one wave per SIMD), and with nothing to interleave the
   // recurrence's own dependency stalls cost more than the hidden load latency saves -- 1 degree V-cycle 3.10 ms
   // against 2.70 ms for the one-group-per-wave kernel (bit-identical results)
   int pipe_min = 0;           // COL_LANES: > 0 = a launch of at least that many groups takes colblock_apply_lanes_pipe_kernel
   int batch4 = COL_BATCH_WAVE, batch_other = COL_BATCH_WAVE;   // K interleaved right-hand sides with K % 4 == 0 / any other K
   int wave_columns = 0;       // a level of the multilevel cycle with few columns: one column per WAVE (colblock_apply_kernel)
   int wave_fused = 0;         // ... and its half sweeps are one launch each (gs_wave_kernel)
   // COL_LDSPACK level of the cycle, not one column per wave, columns of at most 64 rows, P <= 2 (the group's factors beside
   // its columns twice in a CU's LDS), at most ml_lane_fused columns: its half sweeps may run as one launch each on the level
   // operator's diagonals (gs_lanes_diag_kernel); the plan then carries grp_tile
   int lane_fused = 0;
};

struct ColPlanInput {
   int P = 1;                          // half bandwidth stored
   int max_len = 0;                    // longest column
   int dropped = 0;                    // in-column entries beyond the band were dropped
   int f32 = 0;                        // factors stored in f32
   const int *h_blk_start = nullptr;   // row offsets of the columns
   const int *ranges = nullptr;        // nranges + 1 column offsets; a group never straddles a range boundary (Gauss-Seidel colours)
   int nranges = 0;
   const int *h_rowptr = nullptr;      // the level operator's row offsets when the fused sweep (gs_fused_kernel) is wanted, else NULL
   int ncol = -1;                      // columns of a level of the multilevel cycle; -1: the column preconditioner (never one column per wave)
};

struct ColPlan {
   ColKernel kern;
   int gw = 8;                         // columns (lanes in use) per group
   int stream = 0, ldsres = 0;         // the family as nkp_get_int / nkp_ml_level_array report it (ldsres: 1 = COL_LDSRES, 2 = COL_LDSPACK)
   int sorted = 0;                     // groups formed from the colour's columns sorted by chunk count (COL_LDSPACK with col_sort_groups)
   int ngrp = 0;
   std::vector<int> grp_first;         // [nranges + 1] first group of every range
   std::vector<int> grp_b0, grp_nb, grp_maxlen;   // [ngrp] first column, columns, padded longest column of the group
   std::vector<long long> grp_base;    // [ngrp] offset of the group's factors [(2P+1)][grp_maxlen][gw]
   std::vector<int> grp_row0;          // [ngrp] first row of the group (0 when sorted), then [ngrp] its rows (0 when sorted)
   std::vector<int> col_slot;          // [ngrp * gw] first row of the lane's column relative to grp_row0, then [ngrp * gw] its length (0: no column)
   std::vector<int> grp_cols;          // sorted only: [ngrp * gw] the lane's column, -1 = none
   std::vector<int> grp_tile;          // kern.lane_fused only: [ngrp * gw] the lane's column counted in columns that have rows (= its tile in the level operator's diagonals), -1 = none
   int ntile = 0;                      // ... and how many such columns there are
   std::vector<int> gs_rb_ptr, gs_rb;  // fused sweep: [ngrp + 1] first row block of the group; first rows of the blocks + the end (empty: a row exceeds GS_NNZ, or not wanted)
   long long fac_total = 0;            // elements of the factor array
   int rhs_slots = 0;                  // LDS doubles reserved for the staged right-hand side
   int lds_doubles = 0;                // dynamic LDS of the lane kernels
   int gs_ok = 0;                      // the fused sweep can run (before the storage-match test of the multilevel setup)
   int gs_lds_bytes = 0;
};

// 0, or 1 when the layout needs more LDS than a CU has
int col_plan (const ColPlanInput &in, const nkp_tuning &T, ColPlan &pl);
