// csrc/col_plan.cpp run alone on the one-launch half sweep's part of the plan (ColKernel::lane_fused, ColPlan::grp_tile):
// tests/test_col_plan_lane_fused.py builds this with the address and undefined-behaviour sanitizers; it links col_plan.cpp and
// tuning.cpp and nothing else.  Reads a case from every file named on the command line, one item per line:
//    tune <ml_lane_fused | col_wave_max | col_ldsres_min | col_ldsres_packed | col_sort_groups | ml_tail_rows> <value>
//    P | dropped | max_len | f32 | multilevel <value>
//    blk_start | ranges <count> <values ...>
// and prints "case <file>" and one "name values ..." line per field.
#include "../nk_ocn_tracer_jacobian_precond_amd/csrc/col_plan.h"
#include "../nk_ocn_tracer_jacobian_precond_amd/csrc/tuning.h"

#include <stdio.h>

#include <fstream>
#include <sstream>
#include <string>

static bool set_knob (nkp_tuning &T, const std::string &name, long long v)
{
#define KNOB(field) if (name == #field) { T.field = (decltype (T.field)) v; return true; }
   KNOB (ml_lane_fused) KNOB (col_wave_max) KNOB (col_ldsres_min) KNOB (col_ldsres_packed) KNOB (col_sort_groups) KNOB (ml_tail_rows)
#undef KNOB
   return false;
}

static void print (const char *name, const std::vector<int> &v)
{
   printf ("%s", name);
   for (int x : v) printf (" %d", x);
   printf ("\n");
}

static int run_case (const char *path)
{
   std::ifstream f (path);
   if (!f) { fprintf (stderr, "cannot read %s\n", path); return 2; }
   printf ("case %s\n", path);
   nkp_tuning T = nkp_builtin_tuning ();
   printf ("builtin_ml_lane_fused %d\n", T.ml_lane_fused);
   ColPlanInput in;
   std::vector<int> blk_start, ranges;
   int multilevel = 0;
   std::string line, key;
   while (std::getline (f, line)) {
      std::istringstream w (line);
      if (!(w >> key)) continue;
      if (key == "tune") {
         std::string name;
         long long v;
         if (!(w >> name >> v) || !set_knob (T, name, v)) { fprintf (stderr, "bad knob: %s\n", line.c_str ()); return 2; }
      } else if (key == "blk_start" || key == "ranges") {
         std::vector<int> &dst = key == "blk_start" ? blk_start : ranges;
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
   if (ranges.size () < 2 || blk_start.size () != (size_t) ranges.back () + 1) { fprintf (stderr, "inconsistent case\n"); return 2; }
   in.h_blk_start = blk_start.data ();
   in.ranges = ranges.data ();
   in.nranges = (int) ranges.size () - 1;
   in.ncol = multilevel ? ranges.back () : -1;
   ColPlan pl;
   const int rc = col_plan (in, T, pl);
   printf ("rc %d\nfamily %d\nnch %d\nwave_columns %d\nwave_fused %d\nlane_fused %d\ngw %d\nsorted %d\nngrp %d\nntile %d\n", rc, pl.kern.family, pl.kern.nch,
           pl.kern.wave_columns, pl.kern.wave_fused, pl.kern.lane_fused, pl.gw, pl.sorted, pl.ngrp, pl.ntile);
   print ("grp_first", pl.grp_first);
   print ("grp_b0", pl.grp_b0);
   print ("grp_nb", pl.grp_nb);
   print ("grp_cols", pl.grp_cols);
   print ("grp_tile", pl.grp_tile);
   return 0;
}

int main (int argc, char **argv)
{
   if (argc < 2) { fprintf (stderr, "usage: col_plan_lane_main CASE ...\n"); return 2; }
   for (int a = 1; a < argc; a++)
      if (const int rc = run_case (argv[a])) return rc;
   return 0;
}
