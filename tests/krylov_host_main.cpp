// Stand-alone driver of the host arithmetic of FGMRES (csrc/krylov_host.cpp) for tests/test_krylov_host.py, which builds the two
// files under the address and undefined-behaviour sanitizers: no HIP runtime, no solver object, no Python.
//
//    krylov_host_main solve.txt
//
// solve.txt, numbers separated by white space (doubles in any form strtod reads, hexadecimal included):
//    m max_iters steps_now bnorm target            the head: restart length, iteration budget, cycles per application, ||b||, target
//    R beta           a restart with the true residual norm beta: prints "restart <todo> <finished> <status> <steps_now>
//                     <stalled_cycles> <relres> <inner_scale>"; unless the solve is over the next cycle starts (fg_start_cycle)
//    S h[0 .. j+1]    the Hessenberg column of step j of the running cycle: prints "step <its> <ends> <breakdown> <est>"
//    E                the end of the cycle: prints "end <k>", then "y", "cs", "sn" (k numbers each), "g" (k + 1 numbers: what y was
//                     solved from, and the entry behind it) and "H" (the rotated upper triangle, column by column: c + 1 numbers
//                     of column c)
//    V bnorm2 target nonfinite nonzero    the verdict on a right-hand side (rhs_needs_counts, rhs_verdict), at any point of the
//                     file: prints "verdict <needs counts> <RHS_* code>"
// Doubles are printed as hexadecimal floats, so that nothing is lost on the way.  The driver does what krylov.hip does between
// two calls and nothing else: it lowers steps_now when the verdict says so.
#include "../nk_ocn_tracer_jacobian_precond_amd/csrc/krylov_host.h"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

static void usage_error (const char *what)
{
   fprintf (stderr, "krylov_host_main: %s\n", what);
   exit (2);
}

static double read_double (FILE *f)
{
   char tok[64];
   if (fscanf (f, "%63s", tok) != 1) usage_error ("a number is missing");
   char *end = nullptr;
   const double v = strtod (tok, &end);
   if (end == tok || *end) usage_error ("not a number");
   return v;
}

static void print_row (const char *name, const double *v, int count)
{
   printf ("%s", name);
   for (int i = 0; i < count; i++) printf (" %a", v[i]);
   printf ("\n");
}

int main (int argc, char **argv)
{
   if (argc != 2) usage_error ("usage: krylov_host_main solve.txt");
   FILE *f = fopen (argv[1], "r");
   if (!f) usage_error ("cannot open the input");
   int m = 0, max_iters = 0, steps_now = 0;
   if (fscanf (f, "%d %d %d", &m, &max_iters, &steps_now) != 3 || m < 1) usage_error ("bad head");
   FgmresState F;
   fg_init (F, m);
   F.bnorm = read_double (f);
   F.target = read_double (f);
   char cmd[8];
   std::vector<double> h ((size_t) m + 1);
   while (fscanf (f, "%7s", cmd) == 1) {
      if (cmd[0] == 'R') {
         const double beta = read_double (f);
         const int todo = fg_restart_verdict (F, beta, max_iters, steps_now);
         if (todo & FG_LOWER_STEPS) steps_now = 1;
         printf ("restart %d %d %d %d %d %a %a\n", todo, F.finished ? 1 : 0, F.status, steps_now, F.stalled_cycles, F.relres, F.inner_scale);
         if (!(todo & FG_STOP)) fg_start_cycle (F);
      } else if (cmd[0] == 'S') {
         if (F.finished || F.j >= m) usage_error ("a column beyond the cycle");
         for (int i = 0; i <= F.j + 1; i++) h[(size_t) i] = read_double (f);
         const bool ends = fg_column_step (F, h.data (), max_iters);
         printf ("step %d %d %d %a\n", F.its, ends ? 1 : 0, F.breakdown_in_cycle ? 1 : 0, F.est);
      } else if (cmd[0] == 'E') {
         const int k = F.j;
         fg_back_substitute (F);
         printf ("end %d\n", k);
         print_row ("y", F.y.data (), k);
         print_row ("cs", F.cs.data (), k);
         print_row ("sn", F.sn.data (), k);
         print_row ("g", F.g.data (), k + 1);
         printf ("H");
         for (int c = 0; c < k; c++)
            for (int i = 0; i <= c; i++) printf (" %a", F.H[(size_t) c * (size_t) (m + 1) + (size_t) i]);
         printf ("\n");
      } else if (cmd[0] == 'V') {
         const double bnorm2 = read_double (f), target = read_double (f), nonfinite = read_double (f), nonzero = read_double (f);
         printf ("verdict %d %d\n", rhs_needs_counts (bnorm2, target) ? 1 : 0, rhs_verdict (bnorm2, target, nonfinite, nonzero));
      } else
         usage_error ("unknown command");
   }
   fclose (f);
   return 0;
}
