// csrc/col_plan.cpp run alone (tests/test_col_plan.py builds this with the address and undefined-behaviour sanitizers; it links
// col_plan.cpp and tuning.cpp and nothing else).  Reads a case from every file named on the command line, one item per line:
//    tune <nkp_tuning field> <value>      any number of them, on top of nkp_builtin_tuning
//    P | dropped | max_len | f32 | multilevel <value>
//    blk_start | ranges | rowptr <count> <values ...>     (rowptr: the fused sweep is wanted)
// and prints "case <file>" and the plan, one "name values ..." line per field.
#include "../nk_ocn_tracer_jacobian_precond_amd/csrc/col_plan.h"
#include "../nk_ocn_tracer_jacobian_precond_amd/csrc/tuning.h"

#include <stdio.h>

#include <fstream>
#include <sstream>
#include <string>

static bool set_knob (nkp_tuning &T, const std::string &name, long long v)
{
#define KNOB(field) if (name == #field) { T.field = (decltype (T.field)) v; return true; }
   KNOB (col_ldsres) KNOB (col_stream) KNOB (col_stream_min) KNOB (col_stream_gw) KNOB (col_wave_max) KNOB (col_w3) KNOB (col_group)
   KNOB (col_pipe_min) KNOB (col_ldsres_early) KNOB (col_ldsres_packed) KNOB (col_sort_groups) KNOB (col_ldsres_min)
   KNOB (ml_fused) KNOB (ml_wave_fused) KNOB (ml_tail_rows) KNOB (ml_coarsest_rows)
#undef KNOB
   return false;
}

template <class T>
static void print (const char *name, const std::vector<T> &v)
{
   printf ("%s", name);
   for (const T &x : v) printf (" %lld", (long long) x);
   printf ("\n");
}

static int run_case (const char *path)
{
   std::ifstream f (path);
   if (!f) { fprintf (stderr, "cannot read %s\n", path); return 2; }
   printf ("case %s\n", path);
   nkp_tuning T = nkp_builtin_tuning ();
   ColPlanInput in;
   std::vector<int> blk_start, ranges, rowptr;
   int multilevel = 0;
   std::string line, key;
   while (std::getline (f, line)) {
      std::istringstream w (line);
      if (!(w >> key)) continue;
      if (key == "tune") {
         std::string name;
         long long v;
         if (!(w >> name >> v) || !set_knob (T, name, v)) { fprintf (stderr, "bad knob: %s\n", line.c_str ()); return 2; }
      } else if (key == "blk_start" || key == "ranges" || key == "rowptr") {
         std::vector<int> &dst = key == "blk_start" ? blk_start : key == "ranges" ? ranges : rowptr;
         size_t cnt;
         if (!(w >> cnt)) { fprintf (stderr, "bad line: %s\n", key.c_str ()); return 2; }
         dst.resize (cnt);
         for (int &x : dst)
            if (!(w >> x)) { fprintf (stderr, "short line: %s\n", key.c_str ()); return 2; }
      } else {
         int v;
         if (!(w >> v)) { fprintf (stderr, "bad line: %s\n", line.c_str ()); return 2; }
         if (key == "P") in.P = v;
         else if (key == "dropped") in.dropped = v;
         else if (key == "max_len") in.max_len = v;
         else if (key == "f32") in.f32 = v;
         else if (key == "multilevel") multilevel = v;
         else { fprintf (stderr, "unknown item: %s\n", key.c_str ()); return 2; }
      }
   }
   if (ranges.size () < 2 || blk_start.size () != (size_t) ranges.back () + 1 || (!rowptr.empty () && rowptr.size () != (size_t) blk_start.back () + 1)) {
      fprintf (stderr, "inconsistent case\n");
      return 2;
   }
   in.h_blk_start = blk_start.data ();
   in.ranges = ranges.data ();
   in.nranges = (int) ranges.size () - 1;
   in.h_rowptr = rowptr.empty () ? nullptr : rowptr.data ();
   in.ncol = multilevel ? ranges.back () : -1;
   ColPlan pl;
   const int rc = col_plan (in, T, pl);
   const ColKernel &k = pl.kern;
   printf ("rc %d\n", rc);
   printf ("family %d\nmaxl %d\nwpe %d\nnch %d\nearly %d\npipe_min %d\nbatch4 %d\nbatch_other %d\nwave_columns %d\nwave_fused %d\n", k.family, k.maxl, k.wpe, k.nch, k.early,
           k.pipe_min, k.batch4, k.batch_other, k.wave_columns, k.wave_fused);
   printf ("gw %d\nstream %d\nldsres %d\nsorted %d\nngrp %d\nfac_total %lld\nrhs_slots %d\nlds_doubles %d\ngs_ok %d\ngs_lds_bytes %d\n", pl.gw, pl.stream, pl.ldsres, pl.sorted,
           pl.ngrp, pl.fac_total, pl.rhs_slots, pl.lds_doubles, pl.gs_ok, pl.gs_lds_bytes);
   print ("grp_first", pl.grp_first);
   print ("grp_b0", pl.grp_b0);
   print ("grp_nb", pl.grp_nb);
   print ("grp_maxlen", pl.grp_maxlen);
   print ("grp_base", pl.grp_base);
   print ("grp_row0", pl.grp_row0);
   print ("col_slot", pl.col_slot);
   print ("grp_cols", pl.grp_cols);
   print ("gs_rb_ptr", pl.gs_rb_ptr);
   print ("gs_rb", pl.gs_rb);
   return 0;
}

int main (int argc, char **argv)
{
   if (argc < 2) { fprintf (stderr, "usage: col_plan_main CASE ...\n"); return 2; }
   for (int a = 1; a < argc; a++)
      if (const int rc = run_case (argv[a])) return rc;
   return 0;
}
