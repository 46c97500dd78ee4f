// rtol, atol and max_iters after creation: nkp_set_solve_controls / nkp_get_solve_controls on a handle, and per column of one
// call in nkp_solve_batch_device_ex (contracts: nkp.h).
//
// The three values live in nkp_solver::opt, where every driver reads them when a solve starts (fg_begin, fg_restart, fg_post_step,
// bicgstab, the NKP_OK_BERR verdicts of krylov.hip and batch_solve.hip) -- nothing is sized by them and nothing else keeps a
// copy, so writing them there IS creating the solver with them.  This unit validates, agrees between the ranks and writes; the
// solves themselves are batch_solve.hip's (solve_batch_columns).  No HIP call is made here.
#include "solver_impl.h"

#include <math.h>
#include <string.h>

#include <vector>

namespace {

int64_t bits_of (double v)
{
   int64_t b;
   memcpy (&b, &v, sizeof b);
   return b;
}

// One number from every rank, made whatever happened locally.  false: the transport failed
bool gather (nkp_solver *s, int64_t mine, std::vector<int64_t> &all)
{
   const nkp_comm_ops &c = s->dist.ops;
   all.assign ((size_t) c.nranks + 1, 0);
   return c.allgather_i64_host (c.ctx, mine, all.data ()) == 0;
}

// the lowest rank whose number is not rank 0's (0: rank 0 itself sent `bad`), -1: all equal and none is `bad`
int odd_rank (const std::vector<int64_t> &all, int nranks, int64_t bad)
{
   for (int p = 0; p < nranks; p++)
      if (all[(size_t) p] == bad || all[(size_t) p] != all[0]) return p;
   return -1;
}

}      // namespace

extern "C" int nkp_get_solve_controls (nkp_solver *s, nkp_solve_controls *out)
{
   const char *who = "nkp_get_solve_controls";
   if (!out) return fail (NKP_EINVAL, "%s: NULL argument out", who);
   if (out->struct_size != (int) sizeof (nkp_solve_controls))
      return fail (NKP_EINVAL, "%s: nkp_solve_controls.struct_size mismatch (%d != %zu)", who, out->struct_size, sizeof (nkp_solve_controls));
   if (!s) return fail (NKP_EINVAL, "%s: NULL solver (argument s)", who);
   out->max_iters = s->opt.max_iters;
   out->rtol = s->opt.rtol;
   out->atol = s->opt.atol;
   return NKP_OK;
}

extern "C" int nkp_set_solve_controls (nkp_solver *s, const nkp_solve_controls *c)
{
   const char *who = "nkp_set_solve_controls";
   if (!s) return fail (NKP_EINVAL, "%s: NULL solver (argument s)", who);
   // ---- what this rank would have in force afterwards
   SolveControls v = c ? controls_of (s) : s->created;
   int rc = NKP_OK;
   if (c) {
      if (c->struct_size != (int) sizeof (nkp_solve_controls))
         rc = fail (NKP_EINVAL, "%s: nkp_solve_controls.struct_size mismatch (%d != %zu); nothing changed", who, c->struct_size, sizeof (nkp_solve_controls));
      else if (!is_finite (c->rtol) || !is_finite (c->atol))
         rc = fail (NKP_EINVAL, "%s: rtol = %g, atol = %g: NaN and Inf are not tolerances; nothing changed", who, c->rtol, c->atol);
      else if (c->max_iters < 0)
         rc = fail (NKP_EINVAL, "%s: max_iters = %d < 0 (0 leaves it as it is); nothing changed", who, c->max_iters);
      else {
         if (c->max_iters > 0) v.max_iters = c->max_iters;
         if (c->rtol >= 0.0) v.rtol = c->rtol;
         if (c->atol >= 0.0) v.atol = c->atol;
      }
   }
   if (!s->dist.on) {
      if (rc) return rc;
      controls_into (s, v);
      return NKP_OK;
   }
   // ---- row-distributed: the ranks' stopping tests must be one test, or their collectives part.  Three allgathers, always all
   // three and in this order -- rtol, atol, max_iters, as they would be in force -- whatever this rank found; a rank whose own check
   // failed sends -1, which no valid value is (the bits of a double >= 0 are >= 0 as an integer; max_iters > 0)
   const int nranks = s->dist.ops.nranks;
   const std::string text = rc ? last_error_message () : std::string ();
   const int64_t mine[3] = { rc ? -1 : bits_of (v.rtol), rc ? -1 : bits_of (v.atol), rc ? -1 : (int64_t) v.max_iters };
   const char *name[3] = { "rtol", "atol", "max_iters" };
   bool comm_ok = true;
   int odd = -1, odd_at = -1;
   for (int i = 0; i < 3; i++) {
      std::vector<int64_t> all;
      if (!gather (s, mine[i], all)) { comm_ok = false; continue; }
      const int p = odd_rank (all, nranks, -1);
      if (p >= 0 && (odd < 0 || p < odd)) { odd = p; odd_at = all[(size_t) p] == -1 ? -1 : i; }
   }
   if (!comm_ok) return fail (NKP_ECOMM, "%s: allgather failed; nothing changed", who);
   if (odd >= 0) {
      if (odd_at < 0 && rc && odd == s->dist.ops.rank) return fail (NKP_EINVAL, "%s: rank %d: its own check failed (%s)", who, odd, text.c_str ());
      if (odd_at < 0) return fail (NKP_EINVAL, "%s: rank %d failed its own check of the values; see its message; no rank changed anything", who, odd);
      return fail (NKP_EINVAL, "%s: rank %d would run at another %s than rank 0: the call is collective, all ranks pass the same values; no rank changed anything", who, odd,
                   name[odd_at]);
   }
   controls_into (s, v);
   return NKP_OK;
}

// FNV-1a over the bytes of the per-column arrays, NULL-ness included; the top bit is cleared so that -1 can mean "my check failed"
static int64_t hash_columns (int nrhs, const double *rtol, const double *atol, const int *max_iters, const int *use_guess)
{
   uint64_t h = 1469598103934665603ull;
   auto eat = [&h] (const void *p, size_t bytes) {
      const unsigned char *q = (const unsigned char *) p;
      for (size_t i = 0; i < bytes; i++) { h ^= q[i]; h *= 1099511628211ull; }
   };
   auto array = [&] (const void *p, size_t elem) {
      const unsigned char there = p ? 1 : 0;
      eat (&there, 1);
      if (p && nrhs > 0) eat (p, elem * (size_t) nrhs);
   };
   eat (&nrhs, sizeof nrhs);
   array (rtol, sizeof (double));
   array (atol, sizeof (double));
   array (max_iters, sizeof (int));
   array (use_guess, sizeof (int));
   return (int64_t) (h & 0x7fffffffffffffffull);
}

extern "C" int nkp_solve_batch_device_ex (nkp_solver *s, int nrhs, const void *d_B, void *d_X, int64_t ldb, const double *rtol, const double *atol, const int *max_iters,
                                          const int *use_guess, double *berr, int *iters, double *relres)
{
   const char *who = "nkp_solve_batch_device_ex";
   if (!s) return fail (NKP_EINVAL, "%s: NULL solver (argument s)", who);
   if (nrhs > 0 && !d_B) return fail (NKP_EINVAL, "%s: NULL argument d_B", who);
   if (nrhs > 0 && !d_X) return fail (NKP_EINVAL, "%s: NULL argument d_X", who);
   int rc = NKP_OK;
   if (nrhs < 0) rc = fail (NKP_EINVAL, "%s: nrhs = %d < 0", who, nrhs);
   else if (nrhs > 0 && ldb < s->n) rc = fail (NKP_EINVAL, "%s: ldb = %lld < n = %lld", who, (long long) ldb, (long long) s->n);
   for (int c = 0; c < nrhs && !rc; c++) {
      if (rtol && !is_finite (rtol[c])) rc = fail (NKP_EINVAL, "%s: rtol[%d] = %g is not a tolerance", who, c, rtol[c]);
      else if (atol && !is_finite (atol[c])) rc = fail (NKP_EINVAL, "%s: atol[%d] = %g is not a tolerance", who, c, atol[c]);
      else if (max_iters && max_iters[c] < 0) rc = fail (NKP_EINVAL, "%s: max_iters[%d] = %d < 0 (0 means the solver's)", who, c, max_iters[c]);
      else if (use_guess && use_guess[c] != 0 && d_X == d_B)
         rc = fail (NKP_EINVAL, "%s: d_X == d_B with use_guess[%d] set: the initial guess and the right-hand side would be the same memory", who, c);
   }
   if (s->dist.on) {
      // the ranks must pass identical arrays: ONE allgather of their hash, always made, before any collective of the solve
      const int nranks = s->dist.ops.nranks;
      const std::string text = rc ? last_error_message () : std::string ();
      std::vector<int64_t> all;
      const bool comm_ok = gather (s, rc ? -1 : hash_columns (nrhs, rtol, atol, max_iters, use_guess), all);
      if (rc) { restore_error_message (text); return rc; }
      if (!comm_ok) return fail (NKP_ECOMM, "%s: allgather failed (per-column arrays); nothing solved", who);
      const int p = odd_rank (all, nranks, -1);
      if (p >= 0 && all[(size_t) p] == -1) return fail (NKP_EINVAL, "%s: rank %d refused its arguments; see its message; nothing solved", who, p);
      if (p >= 0)
         return fail (NKP_EINVAL, "%s: rank %d passed other per-column arrays (rtol, atol, max_iters, use_guess, or nrhs) than rank 0: the call is collective; nothing solved", who, p);
   }
   if (rc) return rc;
   const ColumnControls cc = { rtol, atol, max_iters, use_guess };
   return solve_batch_columns (s, nrhs, d_B, d_X, ldb, &cc, berr, iters, relres);
}
