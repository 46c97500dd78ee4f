// K right-hand sides in lockstep: the driver (nkp_solve_batch_device).  The K-wide kernels it launches are batch.hip.
//
// The reference's RHS loop (src/solve_ABglobal.c:370-409) as ONE pass over the matrix and the hierarchy per Krylov step for K
// systems: every system keeps its own FGMRES recurrence (own basis, own Hessenberg matrix, own restart decisions -- the state
// machine of krylov.hip), but the K applications of the cycle and of A in a step are one application to K interleaved vectors
// (batch.hip).  Per system the operations and their order are those of a solve done alone, so are the bits.
//
// Row equilibration and chained preconditioner cycles are fixed linear changes around those same applications and are batched
// with them (batch_step_apply).  What is NOT covered takes its right-hand sides one at a time, with the same answers:
//   a clone                    its work vectors are one system's, and it may run next to its siblings
//   BiCGStab                   the lockstep driver is FGMRES's state machine
//   an f32 Krylov basis        the batched kernels read an f64 basis
//   row equilibration on a row-distributed solver      the K-wide overlap exchange carries unscaled rows
#include "solver_impl.h"

#include <math.h>
#include <string.h>

#include <string>
#include <vector>

const char *batch_unsupported (const nkp_solver *s)
{
   if (s->borrowed) return "a clone";
   if (s->opt.krylov != NKP_KRYLOV_FGMRES) return "BiCGStab";
   if (s->equil && s->dist.on) return "row equilibration on a row-distributed solver";
   if (s->vf32) return "an f32 Krylov basis";
   return nullptr;
}

void note_fallback (const nkp_solver *s, const char *who, const char *why, int nrhs)
{
   msg (s, 1, "%s: %d right-hand sides one at a time: the batched path does not cover %s\n", who, nrhs, why);
}

// a set of device buffers of `count` doubles per unit of width each, all or nothing (see batch_prepare)
static int buffer_set (nkp_solver *s, const std::vector<std::pair<double **, size_t>> &set, int *width, int K_new)
{
   auto drop = [s, &set] (int K_old) {
      for (auto &e : set)
         if (*e.first) {
            const size_t count = e.second * (size_t) K_old;
            (void) hipFree (*e.first);
            *e.first = nullptr;
            s->device_bytes -= (count ? count : 1) * sizeof (double);      // what dev_alloc added
         }
   };
   drop (*width);
   *width = 0;
   int rc = NKP_OK;
   for (auto &e : set) {
      const size_t count = e.second * (size_t) K_new;
      if ((rc = dev_alloc (s, e.first, count)) != NKP_OK) break;
      if (hipMemset (*e.first, 0, (count ? count : 1) * sizeof (double)) != hipSuccess) { rc = fail (NKP_EDEVICE, "nkp_solve_batch: hipMemset failed"); break; }
   }
   if (rc == NKP_OK) { *width = K_new; return NKP_OK; }
   drop (K_new);
   (void) hipGetLastError ();
   return rc;
}

// the row-distributed part of batch_prepare (solver_impl.h): the buffers of the K-wide exchanges, for s->dist.bK < K
int batch_prepare_exchange (nkp_solver *s, int K)
{
   // the host mirror of the Hessenberg columns is small: made once for the widest group
   if (!s->dist.ghpin && hipHostMalloc ((void **) &s->dist.ghpin, (size_t) NKP_BATCH_MAX * (size_t) (s->m + 2) * sizeof (double), hipHostMallocDefault) != hipSuccess) {
      s->dist.ghpin = nullptr;
      (void) hipGetLastError ();
      return fail (NKP_ENOMEM, "nkp_solve_batch: pinned host memory for the Gram-Schmidt messages");
   }
   const size_t gcount = 2 * (size_t) (s->m + 2) + 2;
   std::vector<std::pair<double **, size_t>> set = { { &s->dist.bxe, (size_t) (s->n + s->dist.n_halo) }, { &s->dist.gmsg, gcount } };
   s->dist.each_exchange ([&set] (RowExchange &X, bool in_force) { push_wide (X, in_force, set); });
   return buffer_set (s, set, &s->dist.bK, K);
}

// Everything K systems in flight need.  Transactional per buffer set: after a failed allocation the set is gone and its
// recorded width is 0 (never a width whose buffers are missing or short), and the sticky out-of-memory error is cleared, so
// the narrower retry of the caller starts clean.
static int batch_prepare (nkp_solver *s, int K)
{
   while ((int) s->batch_members.size () < K - 1) {
      nkp_solver *c = nullptr;
      const int rc = clone_impl (s, &c, true);
      if (rc) { (void) hipGetLastError (); return rc; }
      if (c->own_stream && c->stream) (void) hipStreamDestroy (c->stream);
      c->stream = s->stream;
      c->own_stream = false;
      s->batch_members.push_back (c);
   }
   if (s->batch_K < K) {
      const int rc = buffer_set (s, { { &s->bvin, (size_t) s->ld }, { &s->bz, (size_t) s->ld }, { &s->bw, (size_t) s->ld } }, &s->batch_K, K);
      if (rc) return rc;
   }
   if (s->dist.on && s->dist.bK < K) {
      const int rc = batch_prepare_exchange (s, K);
      if (rc) return rc;
   }
   if (s->opt.precond == NKP_PRECOND_MULTILEVEL) {
      const size_t before = s->ml.device_bytes;
      const int mrc = ml_batch_prepare (s->ml, K);
      s->device_bytes += s->ml.device_bytes - before;      // (unsigned wrap-around on a shrink is the intended subtraction)
      if (mrc) return fail (NKP_ENOMEM, "nkp_solve_batch: device memory for the level vectors of %d right-hand sides", K);
   }
   return NKP_OK;
}

// The group's Krylov step applies the cycle and the operator to K vectors, one or several times each (chained cycles), so the
// two are separate routines: "precondition K vectors" and "apply A to K vectors".  Both work from / to per-system vectors
// (src[k] / dst[k], NULL = system k takes no part: zeros in, nothing out) around ONE K-interleaved vector.
//
// Row-distributed flavour: each routine has the exchange of ONE system, K rows wide -- the overlap rows of the preconditioner,
// the halo of the SpMV.  The interleaved operator input is bxe = [own | halo] x K, so the column indices of A (halo slots
// at >= n) address it unchanged; its halo part also receives the overlap residuals (it is rewritten by the operator's
// exchange before A reads it).

// zi[i * K + k] = dz[k][i] = (M src_k)[i] on the own rows (dz NULL: the interleaved result alone); src_scale: src_k times it
static void batch_precond (nkp_solver *s, int K, const double *const *src, const double *src_scale, double *zi, double *const *dz)
{
   const int64_t n = s->n;
   hipStream_t st = s->stream;
   auto &D = s->dist;
   double *const none[NKP_BATCH_MAX] = {};
   if (s->opt.precond == NKP_PRECOND_MULTILEVEL && D.on && D.ras) {
      // several rings: the overlap rows alone, K wide, in the hierarchy's order; one ring: the SpMV's halo, picked from by sel_idx
      RowExchange &X = D.ras_sep ? D.x_ras : D.x_halo;
      double *ext = D.ras_sep ? X.recv_for (K) : halo_rows_of (s, K);
      launch_gather_interleave (K, X.send_idx, src, X.send_for (K), X.nsend, st);
      exchange_rows (s, X, K, X.send_for (K), ext, st);
      ml_apply_batch_split_ext (s->ml, K, src, ext, D.ras_sep ? nullptr : D.sel_idx, n, zi, dz ? dz : none, st, smooth_hook_of (s));
   } else if (s->opt.precond == NKP_PRECOND_MULTILEVEL) {
      // permutation into the hierarchy's row order and the (de-)interleave in one kernel each
      ml_apply_batch_split (s->ml, K, src, zi, dz ? dz : none, st, src_scale);
   } else {
      launch_interleave (K, src, s->bvin, n, st, src_scale);
      if (s->opt.precond == NKP_PRECOND_COLUMN_JACOBI) {
         if (launch_colblock_apply_lanes_batch (K, s->B, 0, s->B.ngrp, s->bvin, zi, 0, st) != 0)
            launch_colblock_apply_wave_batch (K, s->B, 0, s->B.nblk, s->bvin, zi, 0, s->B.fac_tf ? 1 : 0, st);
      } else
         launch_copy (s->bvin, zi, n * K, st);
      if (dz) launch_deinterleave (K, zi, dz, n, st);
   }
}

// dst_k = A x_k (b NULL; times out_scale when given) or dst_k = b_k - A x_k (b_k times b_scale when given) for the K columns
// of xi -- s->bz, or the own rows of s->dist.bxe (K >= 2: halo_fetch copies nothing), whose halo rows arrive here as spmv_op fetches them
static void batch_operator (nkp_solver *s, int K, const double *xi, const double *const *b, const double *b_scale, const double *out_scale, double *const *dst)
{
   const int64_t n = s->n;
   hipStream_t st = s->stream;
   auto &D = s->dist;
   const bool split = s->tune.batch_spmv_rows != 0;
   // the products-in-LDS layout works on interleaved vectors: right-hand side in through bvin, result out through bw
   if (!split && b) launch_interleave (K, b, s->bvin, n, st, b_scale);
   auto rows = [&] (int rb0, int rb1) {
      if (split && b) launch_csr_residual_batch_split_range (K, s->A, rb0, rb1, xi, b, b_scale, dst, st);
      else if (split) launch_csr_spmv_batch_split_range (K, s->A, rb0, rb1, xi, dst, st, out_scale);
      else launch_csr_spmv_batch (K, s->A, rb0, rb1, xi, s->bw, b ? s->bvin : nullptr, b ? 1 : 0, st, out_scale);
   };
   if (D.on && D.overlap) halo_product_overlapped (s, K, xi, rows);
   else {
      if (D.on) halo_fetch (s, K, xi, nullptr, st);
      rows (0, s->A.nrowblk);
   }
   if (!split) launch_deinterleave (K, s->bw, dst, n, st);
}

// One Krylov step's applications for the running systems of a group, arnoldi_apply / apply_precond operation by operation:
//   z_k = M v_k;  for c = 1 .. steps - 1:  p1_k = v_k - A z_k,  z_k += M p1_k;  w_k = A z_k
// and in the row-weighted iteration v_k R^-1 on the way in and R on the way out, folded into the kernels that read v and write w.
// Each stage is one pass for the group (one exchange in the row-distributed flavour).
static void batch_step_apply (nkp_solver *s, int K, nkp_solver *const *mem, const bool *running, int j)
{
   const int64_t ld = s->ld, n = s->n;
   hipStream_t st = s->stream;
   const double *src[NKP_BATCH_MAX] = {};
   double *dz[NKP_BATCH_MAX] = {}, *dw[NKP_BATCH_MAX] = {};
   int steps = 1;
   for (int k = 0; k < K; k++)
      if (mem[k] && running[k]) {
         src[k] = mem[k]->V + (int64_t) j * ld; dz[k] = mem[k]->Z + (int64_t) j * ld; dw[k] = mem[k]->w;
         if (mem[k]->p1 && mem[k]->steps_now > steps) steps = mem[k]->steps_now;
      }
   const double *rinv = s->equil ? s->rinv : nullptr, *rscale = s->equil ? s->rscale : nullptr;
   double *zi = s->dist.on ? s->dist.bxe : s->bz;
   batch_precond (s, K, src, rinv, zi, dz);
   for (int c = 1; c < steps; c++) {
      // The run-time guard of fg_restart is per system: one whose steps_now it has lowered takes no part in the further
      // cycles (NULL pointers, like a system that is not running) and keeps the z of its single solve.  On a row-distributed
      // solver steps_now follows from allreduced residual norms, so every rank builds the same mask and `steps` is the same
      // everywhere: the ranks' sequences of exchanges stay together.
      const double *rin[NKP_BATCH_MAX] = {}, *p1c[NKP_BATCH_MAX] = {};
      double *p1[NKP_BATCH_MAX] = {}, *zc[NKP_BATCH_MAX] = {};
      for (int k = 0; k < K; k++)
         if (src[k] && mem[k]->p1 && mem[k]->steps_now > c) { rin[k] = src[k]; p1[k] = mem[k]->p1; p1c[k] = mem[k]->p1; zc[k] = dz[k]; }
      batch_operator (s, K, zi, rin, rinv, nullptr, p1);
      batch_precond (s, K, p1c, nullptr, s->bw, nullptr);
      launch_add_split (K, s->bw, zi, zc, n, st);
   }
   batch_operator (s, K, zi, nullptr, nullptr, rscale, dw);
}

// Gram-Schmidt of the running systems (run[0 .. R-1], at column j) with the allreduces of ONE system: row r of each message
// belongs to system run[r].  Per system this is arnoldi_orthogonalise, operation by operation.
static void orthogonalise_group (nkp_solver *s, int R, nkp_solver *const *run, int j)
{
   const int64_t ld = s->ld, n = s->n;
   hipStream_t st = s->stream;
   const int k = j + 1, K = s->dist.bK;
   double *msg = s->dist.gmsg, *msg2 = msg + (size_t) K * (size_t) (s->m + 2), *nrm = msg2 + (size_t) K * (size_t) (s->m + 2), *inv = nrm + K;
   GsGroup G = {};
   for (int r = 0; r < R; r++) { G.V[r] = run[r]->V; G.w[r] = run[r]->w; G.partial[r] = run[r]->partial; G.vnext[r] = run[r]->V + (int64_t) (j + 1) * ld; }
   launch_multi_dot_group (R, G, ld, k, n, msg, st);
   allreduce_dev (s, msg, R * (k + 1), 0);
   launch_update_w_group (R, G, ld, k, msg, n, nrm, st);
   if (s->opt.reorth) {
      launch_multi_dot_group (R, G, ld, k, n, msg2, st);
      allreduce_dev (s, msg2, R * (k + 1), 0);
      launch_update_w_group (R, G, ld, k, msg2, n, nrm, st);
      allreduce_dev (s, nrm, R, 0);
      launch_finish_column_group (R, msg, msg2, k, nrm, inv, st);
   } else if (s->tune.dist_one_reduce) launch_finish_column_group (R, msg, nullptr, k, nullptr, inv, st);
   else {
      allreduce_dev (s, nrm, R, 0);
      launch_finish_column_group (R, msg, nullptr, k, nrm, inv, st);
   }
   launch_scale_to_group (R, G, inv, n, st);
}

// mem[k]->b / ->x hold right-hand side and initial guess of system k (k < nact); on return ->x holds the solutions
static int fgmres_batch (nkp_solver *s, int K, int nact, nkp_solver *const *mem, FgmresState *F)
{
   int rc;
   for (int k = 0; k < nact; k++)
      if ((rc = fg_begin (mem[k], F[k]))) return rc;
   for (;;) {
      bool running[NKP_BATCH_MAX] = {}, in_cycle[NKP_BATCH_MAX] = {};
      int nrun = 0;
      for (int k = 0; k < nact; k++) {
         if (F[k].finished) continue;
         if ((rc = fg_restart (mem[k], F[k]))) return rc;
         running[k] = in_cycle[k] = !F[k].finished;
         nrun += running[k] ? 1 : 0;
      }
      if (!nrun) break;
      // the running systems advance together: all of them are at column j of their cycle
      for (int j = 0; nrun; j++) {
         s->batch_steps++;
         batch_step_apply (s, K, mem, running, j);
         if (s->dist.on) {
            nkp_solver *run[NKP_BATCH_MAX] = {};
            int R = 0;
            for (int k = 0; k < nact; k++)
               if (running[k]) run[R++] = mem[k];
            orthogonalise_group (s, R, run, j);
            HIPCHK (hipMemcpyAsync (s->dist.ghpin, s->dist.gmsg, (size_t) R * (size_t) (j + 2) * sizeof (double), hipMemcpyDeviceToHost, s->stream));
            HIPCHK (hipStreamSynchronize (s->stream));
            // stale halo rows or partial sums: no verdict is taken from them (the ranks' sequences of collectives would part)
            if (s->comm_failed) return fail (NKP_ECOMM, "nkp_solve_batch: a collective of the distributed solve failed (lockstep step %lld)", (long long) s->batch_steps);
            for (int r = 0; r < R; r++) memcpy (run[r]->hpin, s->dist.ghpin + (size_t) r * (size_t) (j + 2), (size_t) (j + 2) * sizeof (double));
            for (int k = 0; k < nact; k++)
               if (running[k] && fg_post_step (mem[k], F[k])) { running[k] = false; nrun--; }
            continue;
         }
         for (int k = 0; k < nact; k++) {
            if (!running[k]) continue;
            arnoldi_orthogonalise (mem[k], j);
            HIPCHK (hipMemcpyAsync (mem[k]->hpin, mem[k]->h_dev (), (size_t) (j + 2) * sizeof (double), hipMemcpyDeviceToHost, s->stream));
         }
         HIPCHK (hipStreamSynchronize (s->stream));
         for (int k = 0; k < nact; k++)
            if (running[k] && fg_post_step (mem[k], F[k])) { running[k] = false; nrun--; }      // this system's cycle is over; it waits for the others
      }
      for (int k = 0; k < nact; k++)
         if (in_cycle[k] && (rc = fg_end_cycle (mem[k], F[k]))) return rc;
   }
   HIPCHK (hipGetLastError ());
   return NKP_OK;
}

// all ranks leave a step together (solver_impl.h)
int dist_allgather (nkp_solver *s, int local_rc, int64_t mine, std::vector<int64_t> &all, const char *who, const char *where)
{
   const nkp_comm_ops &c = s->dist.ops;
   all.assign ((size_t) c.nranks + 1, 0);
   const std::string text = local_rc ? last_error_message () : std::string ();
   const bool comm_ok = c.allgather_i64_host (c.ctx, local_rc ? -1 : mine, all.data ()) == 0;
   if (local_rc) { restore_error_message (text); return local_rc; }
   if (!comm_ok) return fail (NKP_ECOMM, "%s: allgather failed (%s)", who, where);
   return NKP_OK;
}

int dist_agree (nkp_solver *s, int local_rc, const char *who, const char *where)
{
   std::vector<int64_t> all;
   if (const int rc = dist_allgather (s, local_rc, 0, all, who, where)) return rc;
   const int p = failed_rank (all);
   return p < 0 ? NKP_OK : fail (NKP_ECOMM, "%s: rank %d failed (%s); see its message", who, p, where);
}

extern "C" int nkp_solve_batch_device (nkp_solver *s, int nrhs, const void *d_B, void *d_X, int64_t ldb, double *berr, int *iters, double *relres)
{
   if (!s || nrhs < 0 || (nrhs > 0 && (!d_B || !d_X))) return fail (NKP_EINVAL, "nkp_solve_batch_device: NULL argument");
   if (nrhs > 0 && ldb < s->n) return fail (NKP_EINVAL, "nkp_solve_batch_device: ldb < n");
   return solve_batch_columns (s, nrhs, d_B, d_X, ldb, nullptr, berr, iters, relres);
}

// The solver's own controls come back when the call ends, however it ends: the columns' values sit in s->opt (and in the members'
// own options) only while their systems are solved
namespace {
struct ControlsGuard {
   nkp_solver *s;
   SolveControls own;
   explicit ControlsGuard (nkp_solver *solver) : s (solver), own (controls_of (solver)) {}
   ~ControlsGuard () { controls_into (s, own); }
   // what column c runs at: its entries where they say something, else the solver's
   SolveControls column (const ColumnControls *cc, int c) const
   {
      SolveControls v = own;
      if (cc && cc->max_iters && cc->max_iters[c] > 0) v.max_iters = cc->max_iters[c];
      if (cc && cc->rtol && cc->rtol[c] >= 0.0) v.rtol = cc->rtol[c];
      if (cc && cc->atol && cc->atol[c] >= 0.0) v.atol = cc->atol[c];
      return v;
   }
};
}      // namespace

int solve_batch_columns (nkp_solver *s, int nrhs, const void *d_B, void *d_X, int64_t ldb, const ColumnControls *cc, double *berr, int *iters, double *relres)
{
   if (s->shared->broken) return refactor_broken (s);
   HIPCHK (hipSetDevice (s->device));
   const double *B = (const double *) d_B;
   double *X = (double *) d_X;
   const size_t bytes = (size_t) s->n * sizeof (double);
   int worst = NKP_OK;
   ControlsGuard ctl (s);
   auto guess_of = [cc] (int c) { return cc && cc->use_guess && cc->use_guess[c] != 0; };
   // one system alone, at its column's controls and from its column's guess: the single remainder of a group, every fallback
   auto alone = [&] (int c) {
      controls_into (s, ctl.column (cc, c));
      return nkp_solve_device (s, B + (size_t) c * (size_t) ldb, X + (size_t) c * (size_t) ldb, guess_of (c) ? 1 : 0, berr ? berr + c : nullptr, iters ? iters + c : nullptr,
                               relres ? relres + c : nullptr);
   };
   const char *why = batch_unsupported (s);
   if (why || nrhs < 2 || !s->tune.rhs_batch) {
      // one at a time (the reference's loop); `why` names what the batched path does not cover
      if (why && nrhs >= 2 && s->tune.rhs_batch) note_fallback (s, "nkp_solve_batch", why, nrhs);
      for (int c = 0; c < nrhs; c++) {
         const int status = alone (c);
         if (status < 0) return status;
         if (sev_of (status) > sev_of (worst)) worst = status;
      }
      return worst;
   }
   int kmax = s->tune.rhs_batch >= 8 ? 8 : s->tune.rhs_batch >= 4 || s->tune.rhs_batch == 1 ? 4 : 2;      // widest interleave (nkp_tuning.rhs_batch: 1 = 4)
   int nact = 0;
   for (int c0 = 0; c0 < nrhs; c0 += nact) {
      nact = nrhs - c0 < kmax ? nrhs - c0 : kmax;
      if (nact == 1) {
         const int status = alone (c0);
         if (status < 0) return status;
         if (sev_of (status) > sev_of (worst)) worst = status;
         continue;
      }
      int K = nact <= 2 ? 2 : nact <= 4 ? 4 : 8;
      const int K_wanted = K;
      int rc = NKP_OK;
      controls_into (s, ctl.own);      // (a member made now starts from the solver's own values)
      if (!s->dist.on || K > s->dist.agreed_K) {
         rc = batch_prepare (s, K);
         // every further system in flight costs a set of work vectors: out of device memory => narrower interleave, then one at a time
         while (rc == NKP_ENOMEM && K > 2) {
            K /= 2;
            rc = batch_prepare (s, K);
         }
         if (rc == NKP_ENOMEM) { K = 1; rc = NKP_OK; }
      }
      if (s->dist.on && K_wanted > s->dist.agreed_K) {
         // the width is a collective decision: every rank takes the narrowest one any rank reached, so that all of them run the
         // same sequence of collectives; a rank with a hard failure returns its code, the others NKP_ECOMM naming it
         std::vector<int64_t> all;
         if ((rc = dist_allgather (s, rc, K, all, "nkp_solve_batch", "interleave width"))) return rc;
         const int bad = failed_rank (all);
         if (bad >= 0) return fail (NKP_ECOMM, "nkp_solve_batch: rank %d failed while preparing %d right-hand sides; see its message", bad, K_wanted);
         for (int p = 0; p < s->dist.ops.nranks; p++)
            if (all[(size_t) p] < K) K = (int) all[(size_t) p];
         if (K == K_wanted) s->dist.agreed_K = K;
      }
      if (rc) return rc;
      if (K < K_wanted) {
         kmax = K;
         if (K == 1) { nact = 0; continue; }
         if (nact > K) nact = K;
      }
      s->batch_width = K;
      nkp_solver *mem[NKP_BATCH_MAX] = { s };
      for (int k = 1; k < K; k++) mem[k] = s->batch_members[(size_t) k - 1];
      for (int k = 0; k < nact; k++) {
         // every system at its own column's controls (a member follows its owner at every call) and from its own start vector
         controls_into (mem[k], ctl.column (cc, c0 + k));
         if (guess_of (c0 + k)) HIPCHK (hipMemcpyAsync (mem[k]->x, X + (size_t) (c0 + k) * (size_t) ldb, bytes, hipMemcpyDeviceToDevice, s->stream));
         else HIPCHK (hipMemsetAsync (mem[k]->x, 0, bytes, s->stream));
         HIPCHK (hipMemcpyAsync (mem[k]->b, B + (size_t) (c0 + k) * (size_t) ldb, bytes, hipMemcpyDeviceToDevice, s->stream));
         mem[k]->stagnated = false;
      }
      FgmresState F[NKP_BATCH_MAX];
      if ((rc = fgmres_batch (s, K, nact, mem, F)) < 0) return rc;
      for (int k = 0; k < nact; k++)
         if (mem[k]->comm_failed) return fail (NKP_ECOMM, "nkp_solve_batch: a collective of the distributed solve failed");
      for (int k = 0; k < nact; k++) {
         // the verdict of one system, exactly as solve_resident gives it for a solve done alone
         nkp_solver *q = mem[k];
         int status = F[k].status;
         double be = 0.0;
         if (berr || q->stagnated) {
            if ((rc = backward_error (q, &be))) return rc;
            if (q->comm_failed) return fail (NKP_ECOMM, "nkp_solve_batch: a collective of the distributed solve failed");
            if (berr) berr[c0 + k] = be;
         }
         if (status == NKP_NOT_CONVERGED && q->stagnated && be <= fmax (NKP_BERR_ROUNDING_LEVEL, 1.0e-2 * q->opt.rtol)) status = NKP_OK_BERR;
         if (iters) iters[c0 + k] = F[k].its;
         if (relres) relres[c0 + k] = F[k].relres;
         msg (s, 1, "nkp_solve_batch: right-hand side %d: %s after %d iterations, ||b-Ax||/||b|| = %.3e\n", c0 + k,
              status == NKP_OK ? "converged" : status == NKP_OK_BERR ? "at the attainable accuracy (backward error accepted)" : status == NKP_BREAKDOWN ? "breakdown" : "NOT converged", F[k].its, F[k].relres);
         if (q->rhs_class == RHS_NONFINITE || q->rhs_class == RHS_OUT_OF_RANGE) rhs_refused (q->rhs_class, ("nkp_solve_batch: right-hand side " + std::to_string (c0 + k)).c_str ());
         else if (status != NKP_OK) fail (status, "nkp_solve_batch: right-hand side %d: %s after %d iterations (relres %.3e, rtol %.1e)", c0 + k,
                                     status == NKP_OK_BERR ? "stopped above rtol at the attainable accuracy" : status == NKP_BREAKDOWN ? "breakdown" : "not converged", F[k].its, F[k].relres, q->opt.rtol);
         if (sev_of (status) > sev_of (worst)) worst = status;
         HIPCHK (hipMemcpyAsync (X + (size_t) (c0 + k) * (size_t) ldb, q->x, bytes, hipMemcpyDeviceToDevice, s->stream));
      }
      HIPCHK (hipStreamSynchronize (s->stream));
   }
   return worst;
}
