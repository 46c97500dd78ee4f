// The kernel selection rule and the group tables of the lane-per-column band solves (col_plan.h).  Plain C++, no HIP, no
// environment: everything follows from the column lengths, the band and the caller's nkp_tuning.
#include "col_plan.h"

#include <algorithm>

static inline int chunks (int len) { return (len + NKP_LDSRES_CH - 1) / NKP_LDSRES_CH; }

// ---------------------------------------------------------------- which layout, which kernel
// sets gw, stream, ldsres, sorted and what of kern does not depend on the group tables
static void choose_family (const ColPlanInput &in, const nkp_tuning &T, ColPlan &pl)
{
   const int ncols = in.ranges[in.nranges] - in.ranges[0];
   // columns per wave: the group's factors + right-hand side must fit LDS several times per CU
   int gw = T.col_group;
   if (gw != 8 && gw != 16 && gw != 32 && gw != 64) gw = 8;
   // levels with many columns: 32 or 64 columns per wave, factors streamed from HBM instead of staged in LDS
   // (colblock_apply_stream_kernel); col_stream = 0 disables, col_stream_min = fewest columns of a level that uses it
   const int on = T.col_stream != 0, sgw = T.col_stream_gw == 64 ? 64 : 32;
   const bool env_min = T.col_stream_min >= 0;
   const int min_cols = env_min ? T.col_stream_min : COL_STREAM_MIN_COLS;
   // the column lives in registers: beyond 64 levels the kernel needs all 256 VGPRs (one wave per SIMD) and loses --
   // 0.25 degree x 80 levels: cycle 46.2 ms with it against 32.8 ms with the small-group kernel
   pl.stream = on && ncols >= min_cols && in.max_len <= 64;
   if (pl.stream) gw = sgw;
   const int lr = T.col_ldsres;
   int min_long = env_min ? min_cols : COL_LDSRES_MIN_COLS_LONG, min_short = env_min ? min_cols : COL_LDSRES_MIN_COLS;
   if (T.col_ldsres_min > 0) min_long = min_short = T.col_ldsres_min;     // A/B: the LDS-resident kernels from that many columns only
   pl.ldsres = lr > 0 && on && in.max_len <= 128 && ((in.max_len > 64 && ncols >= min_long) || (lr == 2 && ncols >= min_short));
   if (pl.ldsres) { pl.stream = 0; gw = 32; }
   // 2 = factors packed four steps to a 16-byte load (colblock_apply_ldspack_kernel): f32 storage, at most 5 chunks of 16
   // levels; the fused half sweep and the tail kernel read the plain layout
   if (pl.ldsres && in.f32 && in.max_len <= 80 && T.col_ldsres_packed && !in.h_rowptr && T.ml_tail_rows <= 0) pl.ldsres = 2;
   while (!pl.stream && !pl.ldsres && gw > 8 && (size_t) ((2 * in.P + 2) * ((in.max_len + 7) & ~7) * gw) * sizeof (double) > COL_GROUP_LDS_BYTES) gw >>= 1;
   pl.gw = gw;
   // packed layout (colblock_apply_ldspack_kernel addresses every column through its own (first row, length) pair): the groups
   // of a colour are formed from its columns SORTED BY LENGTH, so that a group's zero padding (to its longest column, in chunks
   // of 16 steps) and its step count follow the columns it holds -- at 1 degree the factor stream shrinks from 1.23 to 1.09 of its
   // algorithmic size and three quarters of the waves run 48 instead of 64 steps
   pl.sorted = pl.ldsres == 2 && T.col_sort_groups != 0;

   ColKernel &k = pl.kern;
   k.family = pl.ldsres == 2 ? COL_LDSPACK : pl.ldsres ? COL_LDSRES : pl.stream ? COL_STREAM : COL_LANES;
   // WPE = 3 for the 80-level instantiations only (colblock_apply_lanes_kernel says why)
   if (in.max_len <= 64) { k.maxl = 64; k.wpe = 1; }
   else if (in.max_len <= 80 && T.col_w3) { k.maxl = 80; k.wpe = 3; }
   else { k.maxl = 128; k.wpe = 1; }
   k.nch = in.max_len <= 64 ? 4 : 5;
   k.early = T.col_ldsres_early != 0;
   // levels with few columns run one column per WAVE: with thousands of idle wave slots its ~5 us beat the 12-16 us latency
   // floor of the lane-per-column kernels, which only win when the chip is full
   k.wave_columns = in.ncol >= 0 && in.ncol <= T.col_wave_max && in.dropped == 0;
   k.wave_fused = k.wave_columns && (T.ml_wave_fused == 1 || (T.ml_wave_fused > 1 && in.ncol <= T.ml_wave_fused));
   // the packed lane layout has kernels for two and for four systems; every other level takes the wave-per-column batch kernel
   // (which reads the f64 factors and rounds them like the f32 layouts store them: same values)
   const bool packed_batch = k.family == COL_LDSPACK && !k.wave_columns;
   k.batch4 = packed_batch ? COL_BATCH_LDSPACK4 : COL_BATCH_WAVE;
   k.batch_other = packed_batch ? COL_BATCH_LDSPACK2 : COL_BATCH_WAVE;
   k.lane_fused = k.family == COL_LDSPACK && !k.wave_columns && in.max_len <= 64 && in.P <= 2 && in.ncol >= 0 && T.ml_lane_fused > 0 && in.ncol <= T.ml_lane_fused;
}

// ---------------------------------------------------------------- groups
// row blocks of the fused sweep kernel: consecutive rows of the group [r, rend), <= GS_NNZ entries and <= GS_THREADS rows
// each, every block as long as both allow; false = a row alone exceeds GS_NNZ
static bool row_blocks (const int *h_rowptr, int r, int rend, std::vector<int> &rb)
{
   while (r < rend) {
      int r2 = r + 1;
      if (h_rowptr[r2] - h_rowptr[r] > GS_NNZ) return false;
      while (r2 < rend && r2 - r < GS_THREADS && h_rowptr[r2 + 1] - h_rowptr[r] <= GS_NNZ) r2++;
      rb.push_back (r);
      r = r2;
   }
   return true;
}

// the groups of every range: gw columns each in the order of the range (natural, or stably sorted by chunk count, longest
// first); fac_need = elements of the largest group's factor block, rows_need = LDS doubles of the largest staged right-hand side
static void form_groups (const ColPlanInput &in, ColPlan &pl, int &rows_need, int &fac_need, bool &rb_ok)
{
   const int *bs = in.h_blk_start;
   const int gw = pl.gw, ndiag = 2 * in.P + 1;
   const auto len = [bs] (int col) { return bs[col + 1] - bs[col]; };
   std::vector<int> nrow, clen, order, tile_of;
   if (pl.kern.lane_fused) {
      // a column of at most 64 rows is one tile of the diagonals, a column without rows none: tiles follow the columns
      tile_of.resize ((size_t) in.ranges[in.nranges]);
      for (int col = 0; col < in.ranges[in.nranges]; col++) tile_of[(size_t) col] = len (col) > 0 ? pl.ntile++ : -1;
   }
   rows_need = fac_need = 0;
   rb_ok = in.h_rowptr != nullptr;
   pl.grp_first.assign ((size_t) in.nranges + 1, 0);
   for (int r = 0; r < in.nranges; r++) {
      pl.grp_first[r] = (int) pl.grp_b0.size ();
      order.resize ((size_t) (in.ranges[r + 1] - in.ranges[r]));
      for (size_t q = 0; q < order.size (); q++) order[q] = in.ranges[r] + (int) q;
      if (pl.sorted) std::stable_sort (order.begin (), order.end (), [&] (int a, int c) { return chunks (len (a)) > chunks (len (c)); });
      for (size_t q0 = 0; q0 < order.size (); q0 += (size_t) gw) {
         const int cnt = (int) std::min ((size_t) gw, order.size () - q0);
         int m = 0;
         for (int c = 0; c < cnt; c++) m = std::max (m, len (order[q0 + c]));
         m = pl.ldsres ? chunks (m) * NKP_LDSRES_CH : (m + 7) & ~7;      // the apply kernels step in chunks (zero-padded factors)
         // consecutive columns: one contiguous stretch of rows, slots relative to its first; sorted: slots are absolute first rows
         const int first = order[q0];
         const int row0 = pl.sorted ? 0 : bs[first], rows = pl.sorted ? 0 : bs[first + cnt] - bs[first];
         rows_need = std::max (rows_need, LDS_PAD (rows) + 2);
         fac_need = std::max (fac_need, ndiag * m * gw);
         pl.grp_row0.push_back (row0);
         nrow.push_back (rows);
         for (int c = 0; c < gw; c++) {
            const int col = c < cnt ? order[q0 + c] : -1;
            if (pl.sorted) pl.grp_cols.push_back (col);
            if (pl.kern.lane_fused) pl.grp_tile.push_back (col >= 0 ? tile_of[(size_t) col] : -1);
            pl.col_slot.push_back (col >= 0 ? bs[col] - row0 : 0);
            clen.push_back (col >= 0 ? len (col) : 0);
         }
         pl.grp_b0.push_back (first);
         pl.grp_nb.push_back (cnt);
         pl.grp_maxlen.push_back (m);
         pl.grp_base.push_back (pl.fac_total);
         pl.fac_total += (long long) ndiag * m * gw;
         if (rb_ok) {
            pl.gs_rb_ptr.push_back ((int) pl.gs_rb.size ());
            rb_ok = row_blocks (in.h_rowptr, bs[first], bs[first + cnt], pl.gs_rb);
         }
      }
   }
   pl.grp_first[in.nranges] = (int) pl.grp_b0.size ();
   pl.ngrp = (int) pl.grp_b0.size ();
   pl.grp_row0.insert (pl.grp_row0.end (), nrow.begin (), nrow.end ());
   pl.col_slot.insert (pl.col_slot.end (), clen.begin (), clen.end ());
   if (rb_ok) {
      pl.gs_rb_ptr.push_back ((int) pl.gs_rb.size ());
      pl.gs_rb.push_back (in.ranges[in.nranges] > 0 ? bs[in.ranges[in.nranges]] : 0);
   } else {
      pl.gs_rb_ptr.clear ();
      pl.gs_rb.clear ();
   }
}

int col_plan (const ColPlanInput &in, const nkp_tuning &T, ColPlan &pl)
{
   pl = ColPlan ();
   choose_family (in, T, pl);
   int lds_need = 0, fac_need = 0;
   bool gs_ok = false;
   form_groups (in, pl, lds_need, fac_need, gs_ok);
   if (pl.ldsres == 2) lds_need = std::max (lds_need, 32 * (pl.kern.nch * NKP_LDSRES_CH + 1));     // one fixed-stride slot per column
   lds_need = (lds_need + 1) & ~1;                 // keep the factor area 16-byte aligned
   pl.rhs_slots = lds_need;
   const int fac_doubles = in.f32 ? (fac_need + 1) / 2 : fac_need;
   if (pl.kern.family == COL_LANES) lds_need += fac_doubles;
   pl.lds_doubles = lds_need;
   if (gs_ok) {
      // gs_fused_kernel stages the group's factors behind the right-hand side under EVERY layout; the streamed and the
      // LDS-resident lane kernels read them from memory, so lds_need has no room for them there
      pl.gs_lds_bytes = (GS_NNZ + pl.rhs_slots + fac_doubles) * (int) sizeof (double);
      if (pl.gs_lds_bytes > COL_GS_LDS_BYTES) gs_ok = false;
   }
   pl.gs_ok = gs_ok ? 1 : 0;
   const int lds_bytes = lds_need * (int) sizeof (double);
   if (lds_bytes > COL_LDS_MAX_BYTES) return 1;
   ColKernel &k = pl.kern;
   if (k.family == COL_LANES && in.f32 && in.max_len <= 64 && pl.gw == 8 && in.P <= 2 && T.col_pipe_min > 0 && lds_bytes <= COL_LDS_DEFAULT_BYTES)
      k.pipe_min = T.col_pipe_min;
   return 0;
}
