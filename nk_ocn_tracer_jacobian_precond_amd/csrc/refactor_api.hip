// New matrix values on an existing solver: nkp_refactor, nkp_refactor_device and their row-distributed forms nkp_refactor_dist,
// nkp_refactor_dist_device.  Host orchestration only: the value passes and their kernels are refactor.hip and refactor_dist.hip.
//
// One sequence serves both flavours.  Nothing a solve reads is written before the last check that can refuse the call:
//   (a) the new values are staged and their diagonals checked on the device;
//   (b) either (fast path) the hierarchy's new values are computed into work buffers and their pattern drift counted, or
//       (rebuild: asked for, drift, or a construction the fast path does not cover) a whole new hierarchy is built beside the
//       old one;
//   (c) only then are the matrix, the row scaling and the hierarchy overwritten (the commit).
// A row-distributed solver is the same sequence made collective: the overlap rows of restricted additive Schwarz get their
// values from their owners through one alltoallv of device doubles before (b), and an agreement through allgather_i64_host
// after each step keeps the ranks together --
//   after (a) and (b) a failure anywhere leaves every rank unchanged, after (c) it leaves every rank's solver unusable.
// A rank whose own step failed returns its code and message, every other rank NKP_ECOMM naming it.  The callbacks are reached
// in the same order on every rank (allgather, [alltoallv], allgather, allgather) whatever path each rank takes locally.  A
// distributed solver never has user clones (nkp_clone refuses them), so the live-clone checks only ever act on one GPU.
#include "solver_impl.h"

#include <stdio.h>
#include <time.h>

// The matrix the hierarchy is built from, with its new values on the device: the solver's own matrix with the staged values on
// one GPU, the plan's [own rows | overlap rows] source on a distributed rank.
struct HierarchySource {
   const CsrDev &pat;         // pattern (val unused)
   const double *val;
   int64_t n, nnz;
   bool filter;               // nkp_create's inter-tracer filter (developer switch) applies: the hierarchy is always rebuilt
   const CsrDev *dev;         // what ml_setup may read in place of an upload of the unfiltered matrix, or NULL
};

// A new hierarchy H2 from a host copy of the matrix the hierarchy is built from, with new values, exactly as nkp_create builds
// it (with its inter-tracer filter when `filter`; dev = a device copy of the unfiltered matrix, or NULL).  0 or an nkp error
// code with the message in err; H2 is empty on failure.
static int rebuild_hierarchy (nkp_solver *s, MlHierarchy &H2, int64_t n, const int32_t *rowptr, const int32_t *colind, const double *val, bool filter,
                              const CsrDev *dev, char *err, size_t errlen)
{
   std::vector<int32_t> f_rowptr, f_colind;
   std::vector<double> f_val;
   if (filter) {
      drop_intertracer (n, s->tracer_cnt, rowptr, colind, val, f_rowptr, f_colind, f_val);
      rowptr = f_rowptr.data ();
      colind = f_colind.data ();
      val = f_val.data ();
   }
   auto opt_ptr = [] (const std::vector<int> &a) { return a.empty () ? nullptr : a.data (); };
   const int mrc = ml_setup (H2, n, rowptr, colind, val, s->h_blk.data (), (int64_t) s->h_blk.size () - 1, opt_ptr (s->h_col_i), opt_ptr (s->h_col_j), opt_ptr (s->h_col_t),
                             s->tracer_cnt, s->opt.ml_levels, s->opt.ml_smooth, s->tune.ml_coarsest_rows, s->opt.verbose, s->opt.rank, s->stream, err, errlen, s->tune,
                             f_rowptr.empty () ? dev : nullptr);
   if (mrc != 0) {
      (void) hipStreamSynchronize (s->stream);
      ml_free (H2);
      (void) hipGetLastError ();
   }
   return mrc;
}

// (a) The caller's values into W.aval; a row of the solver's matrix without a (non-zero) diagonal refuses them.
static int refactor_stage (nkp_solver *s, const double *h_val, const void *d_val, const char *who)
{
   const int64_t nnz = s->A.nnz;
   hipStream_t st = s->stream;
   HIPCHK (hipSetDevice (s->device));
   HIPCHK (hipStreamSynchronize (st));
   if (!s->rf) s->rf = new RefactorWork;
   RefactorWork &W = *s->rf;
   const bool staged = W.aval != nullptr;
   if (rf_stage (W, nnz, (int) s->ml.lev.size ()) != 0) return fail (NKP_ENOMEM, "%s: no device memory for the staged values", who);
   if (!staged) s->device_bytes += ((size_t) nnz + 2) * sizeof (double) + (4 + 2 * 64) * sizeof (int);
   if (nnz) HIPCHK (hipMemcpyAsync (W.aval, h_val ? (const void *) h_val : d_val, (size_t) nnz * sizeof (double), h_val ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
   if (s->opt.precond != NKP_PRECOND_NONE) {
      // own rows only on a distributed rank: the halo columns (>= m_loc) are never a diagonal; an overlap row's diagonal is
      // checked by its owner
      rf_launch_diag_check (s->A, W.aval, W.dcnt, st);
      int c[3] = { 0, 0, 0 };
      HIPCHK (hipMemcpyAsync (c, W.dcnt, sizeof c, hipMemcpyDeviceToHost, st));
      HIPCHK (hipStreamSynchronize (st));
      if (c[1] && s->dist.on)
         return fail (NKP_ESINGULAR, "%s: row %lld (global) has no (or a zero) diagonal entry (%d such rows on rank %d); no rank's solver is changed", who,
                      (long long) (s->dist.fst + c[2] - 1), c[1], s->dist.ops.rank);
      if (c[1]) return fail (NKP_ESINGULAR, "%s: row %d has no (or a zero) diagonal entry (%d such rows); the solver is unchanged", who, c[2] - 1, c[1]);
   }
   return NKP_OK;
}

// (b) The hierarchy's new values beside the current ones: prepared in W (fast path), or a whole new hierarchy in H2 (*rebuild,
// which the caller may ask for and this step may decide).  Neither the solver nor H2 is changed when it fails.
static int refactor_prepare (nkp_solver *s, const HierarchySource &src, bool *rebuild, MlHierarchy &H2, const char *who)
{
   RefactorWork &W = *s->rf;
   hipStream_t st = s->stream;
   const bool dist = s->dist.on;
   // the fast path covers the default construction of the whole matrix
   if (src.filter) *rebuild = true;
   if (!*rebuild && !W.maps) {
      const int mrc = rf_build_maps (W, s->ml, src.pat, st);
      if (mrc == 0) s->device_bytes += W.bytes;
      else {
         rf_free_maps (W);
         if (mrc < 0) return fail (mrc == -2 ? NKP_ENOMEM : NKP_EDEVICE, "%s: the value maps of the hierarchy could not be built (%s)", who, mrc == -2 ? "out of device memory" : "HIP failure");
         *rebuild = true;
      }
   }
   if (!*rebuild) {
      rf_values (W, s->ml, src.pat, src.val, st);
      int drift = 0;
      HIPCHK (hipMemcpyAsync (&drift, W.dcnt, sizeof drift, hipMemcpyDeviceToHost, st));
      HIPCHK (hipStreamSynchronize (st));
      HIPCHK (hipGetLastError ());
      if (drift) {
         msg (s, 1, "%s: %d couplings of %s hierarchy appear or vanish with the new values: rebuilding it\n", who, drift, dist ? "this rank's" : "the");
         *rebuild = true;
      }
   }
   const int live = s->shared->clones.load () - (int) s->batch_members.size ();
   if (!*rebuild) {
      // the coarsest inverse of the new values, before the commit point: a singular operator, or one whose inverse needs
      // other storage than the clones point at, is refused with the solver unchanged
      char err[256] = "";
      const int irc = rf_prepare_inverse (W, s->ml, st, err, sizeof err);
      if (irc) return fail (irc == -4 ? NKP_ESINGULAR : irc == -2 ? NKP_ENOMEM : NKP_EDEVICE, "%s", err);
      if (live > 0 && !rf_inverse_same_storage (W, s->ml)) {
         rf_drop_inverse (W);
         return fail (NKP_EINVAL, "%s: the coarsest inverse of the new values needs other storage, which %d live clone(s) would not see; destroy them first", who, live);
      }
      return NKP_OK;
   }
   if (live > 0) return fail (NKP_EINVAL, "%s: the hierarchy has to be rebuilt, which %d live clone(s) would not see; destroy them first", who, live);
   // the hierarchy's matrix read back from the device, as nkp_create / nkp_create_dist passed it to ml_setup
   std::vector<int32_t> rp ((size_t) src.n + 1), ci ((size_t) src.nnz);
   std::vector<double> v ((size_t) src.nnz);
   HIPCHK (hipStreamSynchronize (st));
   HIPCHK (hipMemcpy (rp.data (), src.pat.rowptr, rp.size () * sizeof (int32_t), hipMemcpyDeviceToHost));
   if (src.nnz) {
      HIPCHK (hipMemcpy (ci.data (), src.pat.colind, ci.size () * sizeof (int32_t), hipMemcpyDeviceToHost));
      HIPCHK (hipMemcpy (v.data (), src.val, v.size () * sizeof (double), hipMemcpyDeviceToHost));
   }
   char err[256] = "";
   const int mrc = rebuild_hierarchy (s, H2, src.n, rp.data (), ci.data (), v.data (), src.filter, src.dev, err, sizeof err);
   if (mrc != 0) return fail (mrc, "%s: %s (%s)", who, err, dist ? "no rank's solver is changed" : "the solver is unchanged");
   return NKP_OK;
}

// (c) The commit: A's values, row scaling, the hierarchy (rebuild: H2 replaces it; otherwise rf_commit writes the prepared
// values), the column factors.  0 or -2 / -3 / -4 with a message in err; after a failure nobody knows what the solver holds.
static int refactor_commit (nkp_solver *s, bool rebuilt, MlHierarchy &H2, char *err, size_t errlen)
{
   RefactorWork &W = *s->rf;
   hipStream_t st = s->stream;
   const bool multilevel = s->opt.precond == NKP_PRECOND_MULTILEVEL;
   if (s->A.nnz && hipMemcpyAsync (s->A.val, W.aval, (size_t) s->A.nnz * sizeof (double), hipMemcpyDeviceToDevice, st) != hipSuccess) {
      snprintf (err, errlen, "copy of the new values failed");
      if (rebuilt) ml_free (H2);
      return -3;
   }
   launch_diag_fill (s->A, st);            // A's own per-column diagonals (tuning spmv_diag) hold the same values
   if (s->equil) rf_launch_row_scale (s->A, W.aval, s->rscale, s->rinv, st);
   int rc = 0;
   if (multilevel && rebuilt) {
      for (nkp_solver *c : s->batch_members) solver_free (c);      // they copied the old hierarchy; batch_prepare makes new ones
      s->batch_members.clear ();
      (void) hipStreamSynchronize (st);
      s->device_bytes -= s->ml.device_bytes;
      ml_free (s->ml);
      s->ml = H2;
      s->device_bytes += s->ml.device_bytes;
      s->device_bytes -= rf_free_maps (W);
      // the fine-level exchange addresses level-0 positions, and the new hierarchy has its own perm0; a new level 0 that runs
      // other sweeps than the ranks agreed on would leave the peers waiting in an exchange
      if (s->dist.smooth && (!ml_level0_hookable (s->ml) || smooth_build_lists (s) != 0)) {
         rc = -3;
         snprintf (err, errlen, "the index lists of the fine-level exchange could not be rebuilt for the new hierarchy");
      }
   } else if (multilevel) {
      int replaced = 0;
      const size_t before = s->ml.device_bytes;
      rc = rf_commit (W, s->ml, st, err, errlen, &replaced);
      s->device_bytes += s->ml.device_bytes - before;
      if (replaced) {                                                 // new coarsest buffers: the batch members copied the old pointers
         for (nkp_solver *c : s->batch_members) solver_free (c);
         s->batch_members.clear ();
      }
   } else if (s->opt.precond == NKP_PRECOND_COLUMN_JACOBI) {
      // the distributed flavour's A also holds the halo columns: they lie outside every water-column block, and the factor
      // kernel skips columns outside the block (colblock_factor_kernel), as it did in nkp_create_dist
      const size_t before = W.bytes;
      rc = rf_column_factor (W, s->A, s->B, st, err, errlen);
      s->device_bytes += W.bytes - before;
   }
   if (hipStreamSynchronize (st) != hipSuccess || hipGetLastError () != hipSuccess) {
      if (!rc) { rc = -3; snprintf (err, errlen, "a HIP call failed"); }
   }
   return rc;
}

// collective: the entry point is one every rank calls (nkp_refactor_dist*), so a row-distributed solver is accepted
static int refactor_impl (nkp_solver *s, const double *h_val, const void *d_val, int flags, const char *who, bool collective)
{
   if (!s || (!h_val && !d_val)) return fail (NKP_EINVAL, "%s: NULL argument", who);
   if (s->borrowed) return fail (NKP_EINVAL, "%s: a clone shares its matrix; refactor the solver it was cloned from", who);
   if (s->dist.on && !collective) return fail (NKP_EINVAL, "%s: not available for the row-distributed flavour; every rank calls nkp_refactor_dist instead", who);
   const bool dist = s->dist.on;      // false behind nkp_refactor_dist too where nkp_create_dist made a plain solver
   const bool multilevel = s->opt.precond == NKP_PRECOND_MULTILEVEL;
   DistRefactorPlan *Q = s->dplan;
   hipStream_t st = s->stream;
   auto agree = [&] (int local_rc, const char *where) { return dist ? dist_agree (s, local_rc, who, where) : local_rc; };
   // a rank that rebuilds its hierarchy drops its batch members (refactor_commit) and has to allocate them again, which can
   // fail on that rank alone: the next batched solve agrees on its width anew on every rank
   if (dist) s->dist.agreed_K = 0;
   struct timespec ts0;
   clock_gettime (CLOCK_MONOTONIC, &ts0);

   // ---- (a) this rank's arguments, its staged values and their diagonals, the device copies of the plan
   int rc = NKP_OK;
   if (flags & ~NKP_REFACTOR_REBUILD) rc = fail (NKP_EINVAL, "%s: unknown flags 0x%x", who, flags);
   else if (dist && multilevel && !Q) rc = fail (NKP_EINVAL, "%s: the solver kept no plan of its hierarchy's matrix", who);
   else rc = refactor_stage (s, h_val, d_val, who);
   if (!rc && dist && multilevel && !Q->uploaded) {
      const int urc = rf_dist_upload (*Q, st);
      if (urc) rc = fail (urc == -2 ? NKP_ENOMEM : NKP_EDEVICE, "%s: the value maps of the hierarchy's matrix could not be uploaded", who);
      else s->device_bytes += Q->bytes;
   }
   if ((rc = agree (rc, "arguments and own diagonals"))) return rc;
   RefactorWork &W = *s->rf;

   // ---- (b) the overlap values from their owners, then the hierarchy's new values beside the current ones
   bool rebuild = multilevel && (flags & NKP_REFACTOR_REBUILD);
   MlHierarchy H2;
   int64_t halo_values = 0;
   if (multilevel) {
      if (dist && Q->exchange) {
         rf_dist_launch_pack (*Q, W.aval, st);
         if (s->dist.ops.alltoallv (s->dist.ops.ctx, Q->sendbuf, Q->ship_counts.data (), Q->recvbuf, Q->recv_counts.data (), (void *) st))
            rc = fail (NKP_ECOMM, "%s: the exchange of the overlap values failed", who);
         halo_values = Q->n_recv;
      }
      if (!rc) {
         // nkp_create's inter-tracer filter applies to the diagonal block only
         const bool filter = s->tune.ml_drop_intertracer && s->tracer_cnt > 1 && !s->dist.ras;
         if (dist) {
            rf_dist_launch_assemble (*Q, W.aval, st);
            rc = refactor_prepare (s, HierarchySource { Q->src, Q->sval, Q->n_src, Q->nnz_src, filter, nullptr }, &rebuild, H2, who);
         } else {
            // the staged values on the device stand in for A's (as A does in nkp_create), so the device passes need no upload
            CsrDev staged_A = s->A;
            staged_A.val = W.aval;
            rc = refactor_prepare (s, HierarchySource { s->A, W.aval, s->n, s->A.nnz, filter, &staged_A }, &rebuild, H2, who);
         }
      }
   }
   const bool built = !rc && rebuild;
   if ((rc = agree (rc, "new values of the hierarchy"))) {
      if (built) {
         (void) hipStreamSynchronize (st);
         ml_free (H2);
      }
      rf_drop_inverse (W);
      return rc;
   }

   // ---- (c) commit point: from here on the solver's own buffers are written; all ranks commit, or none of them solves
   char err[256] = "";
   const int lrc = refactor_commit (s, built, H2, err, sizeof err);
   rc = lrc ? fail (lrc == -4 ? NKP_ESINGULAR : lrc == -2 ? NKP_ENOMEM : NKP_EDEVICE, "%s: %s", who, err) : NKP_OK;
   if ((rc = agree (rc, "commit"))) {
      const std::string part = std::string (who) + " failed after writing part of the new values (" + err + "); ";
      s->shared->broken = true;
      s->shared->why = !dist ? part + "this solver and its clones cannot solve until a refactor succeeds"
                       : lrc ? part + "this solver cannot solve until nkp_refactor_dist succeeds on every rank"
                             : last_error_message () + "; the new values are written on this rank, so it cannot solve until nkp_refactor_dist succeeds on every rank";
      return rc;
   }
   s->shared->broken = false;
   s->refactor_count++;
   s->refactor_rebuilt = rebuild ? 1 : 0;
   if (dist) s->refactor_halo_values = halo_values;
   struct timespec ts1;
   clock_gettime (CLOCK_MONOTONIC, &ts1);
   s->refactor_seconds = (double) (ts1.tv_sec - ts0.tv_sec) + 1e-9 * (double) (ts1.tv_nsec - ts0.tv_nsec);
   if (dist) msg (s, 1, "%s: %s, %lld overlap values received, %.3f s\n", who, rebuild ? "hierarchy rebuilt" : "coarse cells kept", (long long) halo_values, s->refactor_seconds);
   else msg (s, 1, "%s: %s, %.3f s\n", who, rebuild ? "hierarchy rebuilt" : "coarse cells kept", s->refactor_seconds);
   return NKP_OK;
}

// The entry points.  A solver that owns a transposed one (nkp_transpose) keeps it in step: once its own refactor has succeeded
// the new values are gathered through the value map on the device and the same sequence, with the same flags, runs on the
// transposed solver.  A transposed solver that cannot follow is freed -- the next nkp_transpose rebuilds it from the new matrix
// and reports its own error -- and the call still returns the owner's code.  On a row-distributed solver (nkp_transpose_dist) the
// gather is a gather, one alltoallv and an assembly (trans_dist_follow), every step is agreed between the ranks, and the sequence
// on the transposed solver is the collective one: all ranks keep their transposed solvers, or all free them.
static int refactor_entry (nkp_solver *s, const double *h_val, const void *d_val, int flags, const char *who, bool collective)
{
   if (!s || (!h_val && !d_val)) return refactor_impl (s, h_val, d_val, flags, who, collective);      // refused before s is looked at
   if (s->trans_of) return fail (NKP_EINVAL, "%s: a transposed solver follows its source; refactor the solver it was transposed from", who);
   const int rc = refactor_impl (s, h_val, d_val, flags, who, collective);
   if (!s->trans) return rc;
   if (rc != NKP_OK) {
      if (s->shared->broken) {      // failed after the commit point: nobody knows which matrix the owner holds
         const std::string keep = last_error_message ();
         msg (s, 1, "%s: the transposed solver is freed with the failed refactor\n", who);
         trans_release (s);
         restore_error_message (keep);
      }
      return rc;
   }
   const double *d_valT = nullptr;
   int trc;
   if (s->dist.on) {
      // nkp_transpose_dist: collective, and every step agreed, so that all ranks keep or free their transposed solvers together
      trc = trans_dist_follow (s, flags, who, [] (nkp_solver *t, const void *d_val, int fl, const char *w) { return refactor_impl (t, nullptr, d_val, fl, w, true); });
   } else {
      trc = trans_gather_values (s, &d_valT);
      if (!trc) trc = refactor_impl (s->trans, nullptr, d_valT, flags, who, false);
   }
   if (trc) {
      msg (s, 1, "%s: the transposed solver could not follow (%d: %s); it is freed, the next %s builds a new one\n", who, trc, last_error_message ().c_str (),
           s->dist.on ? "nkp_transpose_dist" : "nkp_transpose");
      (void) hipStreamSynchronize (s->stream);
      trans_release (s);
      (void) hipGetLastError ();
   }
   return rc;      // the code of s
}

extern "C" int nkp_refactor (nkp_solver *s, const double *val, int flags) { return refactor_entry (s, val, nullptr, flags, "nkp_refactor", false); }

extern "C" int nkp_refactor_device (nkp_solver *s, const void *d_val, int flags) { return refactor_entry (s, nullptr, d_val, flags, "nkp_refactor_device", false); }

extern "C" int nkp_refactor_dist (nkp_solver *s, const double *val_loc, int flags) { return refactor_entry (s, val_loc, nullptr, flags, "nkp_refactor_dist", true); }

extern "C" int nkp_refactor_dist_device (nkp_solver *s, const void *d_val_loc, int flags) { return refactor_entry (s, nullptr, d_val_loc, flags, "nkp_refactor_dist_device", true); }
