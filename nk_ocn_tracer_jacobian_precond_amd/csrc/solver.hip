// libnkp_hip: C ABI (include/nkp.h) + host-orchestrated, device-resident Krylov drivers.
//
// Replaces the pdgssvx_ABglobal / pdgssvx calls of the reference (src/solve_ABglobal.c:353,395;
// src/solve_ABdist.c:518,571): setup once (nkp_create), then one solve per right-hand side
// with B overwritten by X.  All vectors live in HBM for the whole solve; the host only sees
// one Hessenberg column (<= m+2 doubles) per iteration for the Givens recurrences.
//
// There is NO CPU fallback in this library: every entry point that computes needs a gfx950
// device and fails with NKP_EDEVICE otherwise.
//
// New matrix values on an existing solver (nkp_refactor and its kin) are refactor_api.hip; the solver object both units work on
// is solver_impl.h.
#include "solver_impl.h"

#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

extern "C" int nkp_device_count (void)
{
   int n = 0;
   if (hipGetDeviceCount (&n) != hipSuccess) return 0;
   return n;
}

// ---------------------------------------------------------------- solver object
#define NKP_BERR_ROUNDING_LEVEL 1.0e-14     // 45 eps

void solver_free (nkp_solver *s)
{
   if (!s) return;
   if (s->borrowed) {           // a clone owns its work vectors, its level vectors and its stream, nothing else
      void *own[] = { s->V, s->vcur, s->Z, s->w, s->r, s->x, s->b, s->t1, s->t2, s->p1, s->p2, s->eqtmp, s->partial, s->dscal, s->dint };
      for (void *p : own)
         if (p) (void) hipFree (p);
      for (MlLevel &L : s->ml.lev) {
         void *lv[] = { L.x, L.x2, L.b, L.r };
         for (void *p : lv)
            if (p) (void) hipFree (p);
      }
      valgrad_release (s);
      valprod_release (s);
      if (s->hpin) (void) hipHostFree (s->hpin);
      if (s->own_stream && s->stream) (void) hipStreamDestroy (s->stream);
      s->shared->clones--;
      delete s;
      return;
   }
   if (s->trans_of) trans_detach (s);
   if (s->trans) trans_release (s);      // before the stream it shares goes
   valgrad_release (s);
   valprod_release (s);
   for (nkp_solver *c : s->batch_members) solver_free (c);
   s->batch_members.clear ();
   for (double *p : { s->bvin, s->bz, s->bw })
      if (p) (void) hipFree (p);
   void *ptrs[] = { s->A.rowptr, s->A.colind, s->A.val, s->A.rowblk, s->A.codes, s->A.dict, s->A.dict_ptr, s->A.dg_ptr, s->A.dg_key, s->A.dg_voff, s->A.dg_vald, s->A.dg_tile, s->A.dg_gptr, s->A.dg_grp, s->B.blk_start, s->B.fac, s->B.grp_b0, s->B.grp_nb, s->B.grp_maxlen, s->B.grp_base, s->B.grp_row0, s->B.col_slot, s->B.fac_t, s->B.gs_rb_ptr, s->B.gs_rb, s->V, s->vcur, s->Z, s->w, s->r,
                    s->x, s->b, s->t1, s->t2, s->p1, s->p2, s->partial, s->dscal, s->dint, s->rscale, s->rinv, s->eqtmp };
   for (void *p : ptrs)
      if (p) (void) hipFree (p);
   ml_free (s->ml);
   if (s->rf) { rf_free (*s->rf); delete s->rf; }
   if (s->dplan) { rf_dist_free (*s->dplan); delete s->dplan; }
   if (s->dist.send_idx) (void) hipFree (s->dist.send_idx);
   if (s->dist.sendbuf) (void) hipFree (s->dist.sendbuf);
   if (s->dist.xe) (void) hipFree (s->dist.xe);
   if (s->dist.sel_idx) (void) hipFree (s->dist.sel_idx);
   if (s->dist.ras_send_idx) (void) hipFree (s->dist.ras_send_idx);
   if (s->dist.ras_sendbuf) (void) hipFree (s->dist.ras_sendbuf);
   if (s->dist.rext) (void) hipFree (s->dist.rext);
   if (s->dist.zext) (void) hipFree (s->dist.zext);
   for (double *p : { s->dist.bxe, s->dist.bsend, s->dist.gmsg, s->dist.bras_send, s->dist.bras_recv })
      if (p) (void) hipFree (p);
   if (s->dist.ghpin) (void) hipHostFree (s->dist.ghpin);
   if (s->dist.ev_packed) (void) hipEventDestroy (s->dist.ev_packed);
   if (s->dist.ev_halo) (void) hipEventDestroy (s->dist.ev_halo);
   if (s->dist.comm_stream) (void) hipStreamDestroy (s->dist.comm_stream);
   if (s->hpin) (void) hipHostFree (s->hpin);
   if (s->own_stream && s->stream) (void) hipStreamDestroy (s->stream);
   delete s;
}

extern "C" void nkp_destroy (nkp_solver *s) { solver_free (s); }

void msg (const nkp_solver *s, int lvl, const char *fmt, ...)
{
   if (s->opt.verbose < lvl) return;
   va_list ap;
   va_start (ap, fmt);
   printf ("(%d) ", s->opt.rank);
   vprintf (fmt, ap);
   va_end (ap);
   fflush (stdout);
}

// the two device collectives of a solve; a failure leaves stale data behind and is checked before any verdict is returned
static inline void alltoallv_dev (nkp_solver *s, const double *send, const int *send_counts, double *recv, const int *recv_counts, hipStream_t st)
{
   s->shared->alltoallv_calls++;
   if (s->dist.ops.alltoallv (s->dist.ops.ctx, send, send_counts, recv, recv_counts, (void *) st)) s->comm_failed = true;
}

static void apply_precond_once (nkp_solver *s, const double *rin, double *zout)
{
   if (s->opt.precond == NKP_PRECOND_NONE) launch_copy (rin, zout, s->n, s->stream);
   else if (s->opt.precond == NKP_PRECOND_MULTILEVEL && s->dist.ras) {
      if (s->dist.ras_sep) {
         // several rings: the overlap rows alone, straight into place behind the own rows
         if (s->dist.ras_nsend) launch_gather (s->dist.ras_send_idx, rin, s->dist.ras_sendbuf, s->dist.ras_nsend, s->stream);
         alltoallv_dev (s, s->dist.ras_sendbuf, s->dist.ras_send_counts.data (), s->dist.rext + s->n, s->dist.ras_recv_counts.data (), s->stream);
         launch_copy (rin, s->dist.rext, s->n, s->stream);
      } else {
         // the residual on the overlap rows comes from their owners (same exchange pattern as the SpMV's halo)
         if (s->dist.nsend) launch_gather (s->dist.send_idx, rin, s->dist.sendbuf, s->dist.nsend, s->stream);
         alltoallv_dev (s, s->dist.sendbuf, s->dist.send_counts.data (), s->dist.xe + s->n, s->dist.recv_counts.data (), s->stream);
         launch_copy (rin, s->dist.rext, s->n, s->stream);
         if (s->dist.n_sel) launch_gather (s->dist.sel_idx, s->dist.xe + s->n, s->dist.rext + s->n, s->dist.n_sel, s->stream);
      }
      ml_apply (s->ml, s->dist.rext, s->dist.zext, s->stream);
      launch_copy (s->dist.zext, zout, s->n, s->stream);
   } else if (s->opt.precond == NKP_PRECOND_MULTILEVEL) ml_apply (s->ml, rin, zout, s->stream);
   else launch_colblock_apply_lanes (s->B, 0, s->B.ngrp, rin, zout, 0, s->stream);
}

static void spmv_op (nkp_solver *s, const double *x, double *y, const double *b, int mode);

// z = M r, optionally followed by defect-correction steps against the true operator: z += M (r - A z)
// (NKP_PRECOND_STEPS, default 1; still a fixed linear operator, so FGMRES and BiCGStab are both fine with it)
static void apply_precond (nkp_solver *s, const double *rin, double *zout)
{
   apply_precond_once (s, rin, zout);
   for (int k = 1; k < s->steps_now && s->p1 && s->p2; k++) {
      spmv_op (s, zout, s->p1, rin, 1);
      apply_precond_once (s, s->p1, s->p2);
      launch_axpby (1.0, s->p2, 1.0, zout, s->n, s->stream);
   }
}

// y = A x (0), y = b - A x (1), y = |A||x| + |b| (2); in the distributed flavour the rows other
// ranks own are fetched first (pack -> alltoallv -> extended input vector)
static void spmv_op (nkp_solver *s, const double *x, double *y, const double *b, int mode)
{
   const double *xin = x;
   if (s->dist.on) {
      launch_copy (x, s->dist.xe, s->n, s->stream);
      if (s->dist.nsend) launch_gather (s->dist.send_idx, x, s->dist.sendbuf, s->dist.nsend, s->stream);
      xin = s->dist.xe;
      if (s->dist.overlap) {
         // the exchange runs on its own stream behind the packing; the interior rows (no off-rank column) are multiplied
         // meanwhile, the boundary rows once the halo has landed -- every row is still summed in stored order, so the
         // result is the bit pattern of the serial version
         (void) hipEventRecord (s->dist.ev_packed, s->stream);
         (void) hipStreamWaitEvent (s->dist.comm_stream, s->dist.ev_packed, 0);
         alltoallv_dev (s, s->dist.sendbuf, s->dist.send_counts.data (), s->dist.xe + s->n, s->dist.recv_counts.data (), s->dist.comm_stream);
         (void) hipEventRecord (s->dist.ev_halo, s->dist.comm_stream);
         launch_csr_spmv_range (s->A, s->dist.seg_rb[1], s->dist.seg_rb[2], xin, y, b, mode, s->stream);
         (void) hipStreamWaitEvent (s->stream, s->dist.ev_halo, 0);
         launch_csr_spmv_range (s->A, s->dist.seg_rb[0], s->dist.seg_rb[1], xin, y, b, mode, s->stream);
         launch_csr_spmv_range (s->A, s->dist.seg_rb[2], s->dist.seg_rb[3], xin, y, b, mode, s->stream);
         return;
      }
      alltoallv_dev (s, s->dist.sendbuf, s->dist.send_counts.data (), s->dist.xe + s->n, s->dist.recv_counts.data (), s->stream);
   }
   if (mode == 2) launch_csr_abs_spmv (s->A, xin, b, y, s->stream);
   else if (s->A.dg_vald) launch_diag_spmv (s->A, xin, y, b, mode, s->stream);      // tuning spmv_diag: same bits, no column indices
   else launch_csr_spmv (s->A, xin, y, b, mode, s->stream);
}

// A's per-column diagonals (tuning spmv_diag) from the caller's water columns.  Any reason not to have them -- columns that do
// not tile the rows, too many keys, too much padding, no device memory -- leaves A on CSR and is no error.
static void build_matrix_diagonals (nkp_solver *s, const int32_t *blk_start, int64_t nblk)
{
   const int64_t n = s->n;
   if (s->tune.spmv_diag <= 0 || !blk_start || nblk <= 0 || nblk >= INT_MAX || n <= 0 || blk_start[0] != 0 || blk_start[nblk] != n) return;
   int max_len = 0;
   for (int64_t c = 0; c < nblk; c++) {
      const int len = blk_start[c + 1] - blk_start[c];
      if (len <= 0) return;
      max_len = std::max (max_len, len);
   }
   void *d_blk = nullptr;
   const size_t bytes = ((size_t) nblk + 1) * sizeof (int);
   if (hipMalloc (&d_blk, bytes) != hipSuccess || hipMemcpy (d_blk, blk_start, bytes, hipMemcpyHostToDevice) != hipSuccess) {
      if (d_blk) (void) hipFree (d_blk);
      (void) hipGetLastError ();
      return;
   }
   int color_tile[3];
   (void) diag_build (s->A, blk_start, (const int *) d_blk, (int) nblk, (int) nblk, max_len, s->tune.spmv_diag, color_tile, &s->device_bytes, s->stream);
   (void) hipFree (d_blk);
}

static inline void allreduce_dev (nkp_solver *s, double *dev, int count, int op)
{
   if (!s->dist.on) return;
   s->shared->allreduce_calls++;
   if (s->dist.ops.allreduce (s->dist.ops.ctx, dev, count, op, (void *) s->stream)) s->comm_failed = true;
}

// the SpMV matrix (device copy; columns may address halo slots >= n) and the matrix the preconditioner
// is built from (host only) are the same arrays except in the distributed flavour
struct SpmvMatrixHost {
   int64_t nnz, ncols;
   const int32_t *rowptr, *colind;
   const double *val;
};
// the matrix the multilevel hierarchy is built from when it is not the solver's own n x n block (distributed flavour
// with overlap: own rows followed by the overlap rows, columns renumbered accordingly)
struct PrecondMatrixHost {
   int64_t n, nblk;
   const int32_t *rowptr, *colind;
   const double *val;
   const int32_t *blk_start, *col_i, *col_j, *col_t;
};

// nkp_create's developer switch ml_drop_intertracer, again in a rebuild of the hierarchy (solver_impl.h)
void drop_intertracer (int64_t n, int tracer_cnt, const int32_t *rowptr, const int32_t *colind, const double *val,
                       std::vector<int32_t> &f_rowptr, std::vector<int32_t> &f_colind, std::vector<double> &f_val)
{
   const int64_t tsl = n / tracer_cnt;
   f_rowptr.assign ((size_t) n + 1, 0);
   for (int64_t i = 0; i < n; i++) {
      for (int32_t e = rowptr[i]; e < rowptr[i + 1]; e++)
         if (colind[e] / tsl == i / tsl) { f_colind.push_back (colind[e]); f_val.push_back (val[e]); }
      f_rowptr[(size_t) i + 1] = (int32_t) f_colind.size ();
   }
}

// The work vectors of one system in flight (a solver's own, a clone's, a batch member's), for s->m, s->ld, s->precond_steps and
// s->equil as they stand.  A batch member never applies the preconditioner on its own: of the scratch of the chained cycles it
// needs p1 only (the residual between two cycles; the second cycle's correction stays interleaved), and no eqtmp (the
// batched kernels scale on the way in).  A failure leaves what was allocated to solver_free.
static int alloc_work_vectors (nkp_solver *s, bool member = false)
{
   const size_t ld = (size_t) s->ld, m = (size_t) s->m, nscal = 3 * (m + 2) + 16 + 8;
   const struct { double **p; size_t count; } vec[] = {
      { &s->V, ld * (m + 1) }, { &s->vcur, ld }, { &s->Z, ld * m }, { &s->w, ld }, { &s->r, ld }, { &s->x, ld }, { &s->b, ld }, { &s->t1, ld }, { &s->t2, ld },
      { &s->p1, s->precond_steps > 1 ? ld : 0 }, { &s->p2, s->precond_steps > 1 && !member ? ld : 0 }, { &s->eqtmp, s->equil && !member ? ld : 0 },
      { &s->partial, ((m + 1 + NKP_DOT_CHUNK) / NKP_DOT_CHUNK + 1) * NKP_RED_BLOCKS * (NKP_DOT_CHUNK + 1) }, { &s->dscal, nscal } };
   int rc = NKP_OK;
   for (const auto &v : vec)
      if (v.count && (rc = dev_alloc (s, v.p, v.count))) return rc;
   if ((rc = dev_alloc (s, &s->dint, 8))) return rc;
   HIPCHK (hipHostMalloc ((void **) &s->hpin, (m + 16) * sizeof (double), hipHostMallocDefault));
   HIPCHK (hipMemset (s->dscal, 0, nscal * sizeof (double)));
   return NKP_OK;
}

// create_impl and clone_impl: a failed step frees the solver under construction and returns its code
#define TRY(x) do { rc = (x); if (rc != NKP_OK) { solver_free (s); return rc; } } while (0)
#define TRYHIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { rc = fail (NKP_EDEVICE, "%s failed: %s", #call, hipGetErrorString (e_)); solver_free (s); return rc; } } while (0)

static int create_impl (nkp_solver **out, const nkp_options *opt_in, int64_t n, int64_t nnz,
                        const int32_t *rowptr, const int32_t *colind, const double *val,
                        const int32_t *blk_start, int64_t nblk, int coupled_tracer_cnt, const SpmvMatrixHost *spmv_mat,
                        const PrecondMatrixHost *pm = nullptr)
{
   if (!out) return fail (NKP_EINVAL, "nkp_create: out is NULL");
   *out = nullptr;
   nkp_options opt;
   if (opt_in) {
      if (opt_in->struct_size != (int) sizeof (nkp_options)) return fail (NKP_EINVAL, "nkp_create: nkp_options.struct_size mismatch (%d != %zu)", opt_in->struct_size, sizeof (nkp_options));
      opt = *opt_in;
   } else
      nkp_default_options (&opt);
   if (n < 0 || nnz < 0 || !rowptr || (nnz > 0 && (!colind || !val))) return fail (NKP_EINVAL, "nkp_create: bad matrix arguments");
   if (n >= 2147483647LL || nnz >= 2147483647LL) return fail (NKP_EINVAL, "nkp_create: n/nnz exceed the int32 index schema");
   if (rowptr[0] != 0 || rowptr[n] != nnz) return fail (NKP_EINVAL, "nkp_create: rowptr[0]=%d rowptr[n]=%d inconsistent with nnz=%lld", rowptr[0], rowptr[n], (long long) nnz);
   if (opt.restart < 1) opt.restart = 1;
   if (opt.restart > NKP_MAX_K - 2) opt.restart = NKP_MAX_K - 2;
   if (opt.precond != NKP_PRECOND_NONE && opt.precond != NKP_PRECOND_COLUMN_JACOBI && opt.precond != NKP_PRECOND_MULTILEVEL)
      return fail (NKP_EINVAL, "nkp_create: unknown preconditioner %d", opt.precond);
   nkp_tuning tune;
   { const int trc = resolve_tuning (&opt, &tune); if (trc) return trc; }
   opt.tuning = nullptr;            // the caller's struct is not kept
   // host-side validation of what the kernels will trust (row chunks in parallel; the lowest offending row is reported)
   {
      struct Bad { int64_t row = -1; int kind = 0; int col = 0; };
      const int nt = (n >= 200000) ? (int) std::min (16u, std::max (1u, std::thread::hardware_concurrency ())) : 1;
      std::vector<Bad> bad ((size_t) nt);
      auto check = [&] (int t) {
         const int64_t r0 = n * t / nt, r1 = n * (t + 1) / nt;
         for (int64_t r = r0; r < r1 && bad[(size_t) t].row < 0; r++) {
            Bad b;
            if (rowptr[r + 1] < rowptr[r]) b.kind = 1;
            else {
               bool have_diag = false;
               for (int e = rowptr[r]; e < rowptr[r + 1] && !b.kind; e++) {
                  if (colind[e] < 0 || colind[e] >= n) { b.kind = 2; b.col = colind[e]; }
                  else if (colind[e] == r && val[e] != 0.0) have_diag = true;
                  else if (opt.precond == NKP_PRECOND_MULTILEVEL && e > rowptr[r] && colind[e] <= colind[e - 1]) b.kind = 4;
               }
               if (!b.kind && opt.precond != NKP_PRECOND_NONE && !have_diag) b.kind = 3;
            }
            if (b.kind) { b.row = r; bad[(size_t) t] = b; }
         }
      };
      if (nt == 1) check (0);
      else {
         std::vector<std::thread> pool;
         for (int t = 0; t < nt; t++) pool.emplace_back (check, t);
         for (std::thread &th : pool) th.join ();
      }
      for (const Bad &b : bad) {
         if (b.row < 0) continue;
         if (b.kind == 1) return fail (NKP_EINVAL, "nkp_create: rowptr decreases at row %lld", (long long) b.row);
         if (b.kind == 2) return fail (NKP_EINVAL, "nkp_create: column index %d out of range in row %lld", b.col, (long long) b.row);
         if (b.kind == 3) return fail (NKP_ESINGULAR, "nkp_create: row %lld has no (or a zero) diagonal entry; the water-column preconditioners need one (the reference only reports this: src/matrix.c:3692-3727)", (long long) b.row);
         return fail (NKP_EINVAL, "nkp_create: row %lld is not sorted by column (the multilevel setup needs the sorted rows gen_A writes)", (long long) b.row);
      }
   }
   std::vector<int> blk_default;
   if (opt.precond != NKP_PRECOND_NONE) {
      if (!blk_start) {
         for (int64_t r = 0; r < n; r += NKP_WAVE) blk_default.push_back ((int) r);
         blk_default.push_back ((int) n);
         blk_start = blk_default.data ();
         nblk = (int64_t) blk_default.size () - 1;
      }
      if (nblk < 0 || blk_start[0] != 0 || blk_start[nblk] != n) return fail (NKP_EINVAL, "nkp_create: blk_start must run from 0 to n");
      for (int64_t b = 0; b < nblk; b++) {
         int len = blk_start[b + 1] - blk_start[b];
         if (len <= 0) return fail (NKP_EINVAL, "nkp_create: empty or descending block %lld", (long long) b);
         if (len > 2 * NKP_WAVE) return fail (NKP_EINVAL, "nkp_create: block %lld has %d rows; this build supports water columns of at most %d levels", (long long) b, len, 2 * NKP_WAVE);
      }
   }

   int ndev = 0;
   if (hipGetDeviceCount (&ndev) != hipSuccess || ndev == 0) return fail (NKP_EDEVICE, "nkp_create: no HIP device available (this library has no CPU fallback)");
   nkp_solver *s = new nkp_solver;
   s->opt = opt;
   s->tune = tune;
   s->A.tune = &s->tune;
   s->B.tune = &s->tune;
   if (opt.device >= 0) {
      if (opt.device >= ndev) { delete s; return fail (NKP_EDEVICE, "nkp_create: device %d of %d does not exist", opt.device, ndev); }
      if (hipSetDevice (opt.device) != hipSuccess) { delete s; return fail (NKP_EDEVICE, "hipSetDevice(%d) failed", opt.device); }
   }
   (void) hipGetDevice (&s->device);
   {
      hipDeviceProp_t prop;
      if (hipGetDeviceProperties (&prop, s->device) == hipSuccess && strncmp (prop.gcnArchName, "gfx950", 6) != 0)
         msg (s, 1, "warning: device %d is %s, kernels are built and tuned for gfx950\n", s->device, prop.gcnArchName);
   }
   int rc = NKP_OK;
   struct timespec ts0_;
   clock_gettime (CLOCK_MONOTONIC, &ts0_);
   auto since0 = [&] () { struct timespec t; clock_gettime (CLOCK_MONOTONIC, &t); return (double) (t.tv_sec - ts0_.tv_sec) + 1e-9 * (double) (t.tv_nsec - ts0_.tv_nsec); };
   TRYHIP (hipStreamCreateWithFlags (&s->stream, hipStreamNonBlocking));
   s->own_stream = true;
   s->n = n;
   s->ld = (n + 63) & ~(int64_t) 63;
   if (s->ld == 0) s->ld = 64;
   s->m = opt.restart;
   // cycles per preconditioner application (defect correction against A between them).  Round 1 chained 2-3 cycles
   // on large systems because every Krylov iteration dragged a 200-vector basis through HBM; with the connectivity-aware
   // aggregates a 1 degree solve needs 78 iterations with one cycle (0.29 s) against 48 with two (0.33 s), 0.25 degree
   // 167 / 6.8 s against 89 / 6.7 s, so one cycle is the automatic choice everywhere (and no rank-dependent choice
   // can desynchronise the collectives of the distributed flavour); the option stays
   s->precond_steps = 1;
   if (opt.precond_steps > 0) s->precond_steps = opt.precond_steps;
   if (tune.precond_steps > 0) s->precond_steps = tune.precond_steps;
   s->steps_now = s->precond_steps;
   s->equil = opt.equil > 0;
   if (tune.equil >= 0 && opt.equil == 0) s->equil = tune.equil != 0;
   if (opt.krylov != NKP_KRYLOV_FGMRES) s->equil = false;

   // matrix
   const SpmvMatrixHost own = { nnz, n, rowptr, colind, val };
   const SpmvMatrixHost &M = spmv_mat ? *spmv_mat : own;
   s->A.n = n;
   s->A.nnz = M.nnz;
   TRY (dev_alloc (s, &s->A.rowptr, (size_t) n + 1));
   TRY (dev_alloc (s, &s->A.colind, (size_t) M.nnz + 2));      // +2: the SpMV reads entries in aligned pairs
   TRY (dev_alloc (s, &s->A.val, (size_t) M.nnz + 2));
   TRYHIP (hipMemcpy (s->A.rowptr, M.rowptr, ((size_t) n + 1) * sizeof (int), hipMemcpyHostToDevice));
   if (M.nnz) {
      TRYHIP (hipMemcpy (s->A.colind, M.colind, (size_t) M.nnz * sizeof (int), hipMemcpyHostToDevice));
      TRYHIP (hipMemcpy (s->A.val, M.val, (size_t) M.nnz * sizeof (double), hipMemcpyHostToDevice));
   }
   {
      int *rb = nullptr, nrb = 0;
      if (spmv_mat) {
         // distributed flavour: row blocks per segment [head boundary | interior | tail boundary], where the interior is
         // the longest run of rows without an off-rank (halo) column -- with latitude bands it is everything but the two
         // or three latitude rows at either end of the band
         int64_t lo = 0, hi = 0, run0 = 0;
         for (int64_t r = 0; r <= n; r++) {
            bool boundary = r == n;
            for (int e = boundary ? 0 : M.rowptr[r]; !boundary && e < M.rowptr[r + 1]; e++) boundary = M.colind[e] >= n;
            if (boundary) {
               if (r - run0 > hi - lo) { lo = run0; hi = r; }
               run0 = r + 1;
            }
         }
         const int64_t seg[4] = { 0, lo, hi, n };
         std::vector<int> all (1, 0);
         for (int q = 0; q < 3; q++) {
            s->dist.seg_rb[q] = (int) all.size () - 1;
            int *part = nullptr, np = 0;
            if (seg[q + 1] > seg[q]) build_rowblocks_host (seg[q + 1] - seg[q], M.rowptr + seg[q], &part, &np);
            for (int i = 1; i <= np; i++) all.push_back ((int) seg[q] + part[i]);
            free (part);
         }
         s->dist.seg_rb[3] = (int) all.size () - 1;
         nrb = (int) all.size () - 1;
         rb = (int *) malloc (all.size () * sizeof (int));
         memcpy (rb, all.data (), all.size () * sizeof (int));
      } else
         build_rowblocks_host (n, M.rowptr, &rb, &nrb);
      s->A.nrowblk = nrb;
      rc = dev_alloc (s, &s->A.rowblk, (size_t) nrb + 1);
      if (rc == NKP_OK && hipMemcpy (s->A.rowblk, rb, ((size_t) nrb + 1) * sizeof (int), hipMemcpyHostToDevice) != hipSuccess)
         rc = fail (NKP_EDEVICE, "copy of row blocks failed");
      if (rc == NKP_OK && attach_spmv_codes (s->A, M.rowptr, M.colind, rb, &s->device_bytes)) rc = fail (NKP_ENOMEM, "column codes could not be uploaded");
      free (rb);
      if (rc != NKP_OK) { solver_free (s); return rc; }
   }
   // the caller's own water columns only; a row-distributed rank keeps CSR (its halo columns live behind n)
   if (!spmv_mat && blk_default.empty ()) build_matrix_diagonals (s, blk_start, nblk);

   if (s->equil) {
      // R_i = 1 / max_j |a_ij| (the row half of dgsequ); rows without entries keep 1
      std::vector<double> rs ((size_t) n, 1.0), ri ((size_t) n, 1.0);
      for (int64_t r = 0; r < n; r++) {
         double mx = 0.0;
         for (int e = M.rowptr[r]; e < M.rowptr[r + 1]; e++) mx = fmax (mx, fabs (M.val[e]));
         if (mx > 0.0) { rs[(size_t) r] = 1.0 / mx; ri[(size_t) r] = mx; }
      }
      TRY (dev_alloc (s, &s->rscale, (size_t) s->ld));
      TRY (dev_alloc (s, &s->rinv, (size_t) s->ld));
      TRYHIP (hipMemcpy (s->rscale, rs.data (), (size_t) n * sizeof (double), hipMemcpyHostToDevice));
      TRYHIP (hipMemcpy (s->rinv, ri.data (), (size_t) n * sizeof (double), hipMemcpyHostToDevice));
   }

   const double t_matrix = since0 ();
   // work space
   s->vf32 = opt.basis_f32 != 0;
   TRY (alloc_work_vectors (s));

   const double t_work = since0 ();
   if (opt.precond != NKP_PRECOND_NONE && !pm) {
      // what a rebuild of the hierarchy (nkp_refactor) passes to ml_setup again, and nkp_transpose to nkp_create
      s->h_blk.assign (blk_start, blk_start + nblk + 1);
      s->tracer_cnt = coupled_tracer_cnt;
      if (blk_default.empty ()) {
         if (opt.col_i) s->h_col_i.assign (opt.col_i, opt.col_i + nblk);
         if (opt.col_j) s->h_col_j.assign (opt.col_j, opt.col_j + nblk);
         if (opt.col_t) s->h_col_t.assign (opt.col_t, opt.col_t + nblk);
      }
   }
   if (opt.precond == NKP_PRECOND_MULTILEVEL) {
      char err[256] = "";
      // developer switch: build the hierarchy without the couplings between tracers, i.e. exactly the
      // preconditioner a tracer-per-rank partition applies (one rank-local hierarchy per tracer), to measure its
      // iteration count on one GPU
      std::vector<int32_t> f_rowptr, f_colind;
      std::vector<double> f_val;
      if (tune.ml_drop_intertracer && coupled_tracer_cnt > 1) {
         drop_intertracer (n, coupled_tracer_cnt, rowptr, colind, val, f_rowptr, f_colind, f_val);
         rowptr = f_rowptr.data ();
         colind = f_colind.data ();
         val = f_val.data ();
      }
      const int coarsest_rows = tune.ml_coarsest_rows;   // 8000: a dense last level costs its bytes, an iterated one ~200 us of launch latencies (dense.hip)
      const int mrc = pm ? ml_setup (s->ml, pm->n, pm->rowptr, pm->colind, pm->val, pm->blk_start, pm->nblk, pm->col_i, pm->col_j, pm->col_t, coupled_tracer_cnt, opt.ml_levels,
                                     opt.ml_smooth, coarsest_rows, opt.verbose, opt.rank, s->stream, err, sizeof err, s->tune)
                         : ml_setup (s->ml, n, rowptr, colind, val, blk_start, nblk, blk_default.empty () ? opt.col_i : nullptr, blk_default.empty () ? opt.col_j : nullptr, blk_default.empty () ? opt.col_t : nullptr,
                                     coupled_tracer_cnt, opt.ml_levels, opt.ml_smooth, coarsest_rows, opt.verbose, opt.rank, s->stream, err, sizeof err, s->tune,
                                     // the SpMV's device copy is this very matrix unless the columns were renumbered (distributed flavour) or filtered
                                     (!spmv_mat && f_rowptr.empty ()) ? &s->A : nullptr);
      if (mrc != 0) {
         rc = fail (mrc, "nkp_create: %s", err);
         solver_free (s);
         return rc;
      }
      s->device_bytes += s->ml.device_bytes;
   }
   // water-column blocks
   if (opt.precond == NKP_PRECOND_COLUMN_JACOBI) {
      s->B.n = n;
      s->B.nblk = (int) nblk;
      TRY (dev_alloc (s, &s->B.blk_start, (size_t) nblk + 1));
      TRYHIP (hipMemcpy (s->B.blk_start, blk_start, ((size_t) nblk + 1) * sizeof (int), hipMemcpyHostToDevice));
      TRYHIP (hipMemsetAsync (s->dint, 0, 8 * sizeof (int), s->stream));
      launch_colblock_measure (s->A, s->B, s->dint, s->stream);
      int meas[3] = { 0, 0, 0 };
      TRYHIP (hipMemcpyAsync (meas, s->dint, sizeof meas, hipMemcpyDeviceToHost, s->stream));
      TRYHIP (hipStreamSynchronize (s->stream));
      if (meas[1] > 0) {
         rc = fail (NKP_ESINGULAR, "nkp_create: %d rows have no (or a zero) diagonal entry; the column-block preconditioner needs one (the reference only reports this: src/matrix.c:3692-3727)", meas[1]);
         solver_free (s);
         return rc;
      }
      s->B.max_len = meas[2];
      s->B.P = meas[0] <= 1 ? 1 : meas[0] <= 2 ? 2 : 4;
      TRY (dev_alloc (s, &s->B.fac, (size_t) (2 * s->B.P + 1) * (size_t) n));
      TRYHIP (hipMemsetAsync (s->dint, 0, 8 * sizeof (int), s->stream));
      launch_colblock_factor (s->A, s->B, s->dint, s->stream);
      int st2[2] = { 0, 0 };
      TRYHIP (hipMemcpyAsync (st2, s->dint, sizeof st2, hipMemcpyDeviceToHost, s->stream));
      TRYHIP (hipStreamSynchronize (s->stream));
      if (st2[0] != 0) {
         rc = fail (NKP_ESINGULAR, "nkp_create: zero pivot at row %d while factoring its water-column block", st2[0] - 1);
         solver_free (s);
         return rc;
      }
      s->B.dropped = st2[1];
      {
         const int ranges[2] = { 0, (int) nblk };
         int grp_first[2];
         const int lrc = colblock_build_lane_layout (s->B, blk_start, ranges, 1, grp_first, &s->device_bytes, s->stream);
         if (lrc != 0) {
            rc = fail (NKP_EDEVICE, "nkp_create: lane layout of the column blocks failed (HIP error %d)", lrc);
            solver_free (s);
            return rc;
         }
      }
      msg (s, 1, "column blocks: %lld blocks, longest %d rows, in-block half bandwidth %d stored as %d%s\n", (long long) nblk,
           s->B.max_len, meas[0], s->B.P, s->B.dropped ? " (entries beyond the band dropped)" : "");
   }
   TRYHIP (hipStreamSynchronize (s->stream));
   TRYHIP (hipGetLastError ());
   msg (s, 1, "nkp_create: n = %lld, nnz = %lld, %d SpMV row blocks, %.1f MB on device %d; %.2f s matrix upload + row blocks, %.2f s work vectors, %.2f s preconditioner\n",
        (long long) n, (long long) M.nnz, s->A.nrowblk, (double) s->device_bytes / 1.0e6, s->device, t_matrix, t_work - t_matrix, since0 () - t_work);
   s->create_seconds = since0 ();
   *out = s;
   return NKP_OK;
}

// ---------------------------------------------------------------- hierarchy introspection (tests)
extern "C" int64_t nkp_ml_level_array (nkp_solver *s, int level, const char *what, void *dst, int64_t capacity_bytes)
{
   if (!s || !what || s->opt.precond != NKP_PRECOND_MULTILEVEL || level < 0 || level >= (int) s->ml.lev.size ()) return fail (NKP_EINVAL, "nkp_ml_level_array: bad argument");
   const MlLevel &V = s->ml.lev[(size_t) level];
   const bool last = level == (int) s->ml.lev.size () - 1;
   const void *src = nullptr;
   int64_t count = 0;
   size_t elem = 4;
   bool host = false;
   int col_kernel[11];
   if (!strcmp (what, "rowptr")) { src = V.L.rowptr; count = V.n + 1; }
   else if (!strcmp (what, "colind")) { src = V.L.colind; count = V.L.nnz; }
   else if (!strcmp (what, "valf")) { src = V.L.valf; count = V.L.valf ? V.L.nnz : 0; }
   else if (!strcmp (what, "val")) { src = V.L.val; count = V.L.val ? V.L.nnz : 0; elem = 8; }
   else if (!strcmp (what, "dg_ptr")) { src = V.L.dg_ptr; count = src ? V.L.dg_ncol + 1 : 0; }
   else if (!strcmp (what, "dg_key")) { src = V.L.dg_key; count = src ? (int64_t) V.L.dg_nkey : 0; }
   else if (!strcmp (what, "dg_voff")) { src = V.L.dg_voff; count = src ? V.L.dg_ncol : 0; elem = 8; }
   else if (!strcmp (what, "dg_val")) { src = V.L.dg_val; count = src ? V.L.dg_nval : 0; }
   else if (!strcmp (what, "dg_gptr")) { src = V.L.dg_gptr; count = src ? V.L.dg_ncol + 1 : 0; }
   else if (!strcmp (what, "dg_grp")) { src = V.L.dg_grp; count = src ? 2 * (int64_t) V.L.dg_ngrp : 0; }
   else if (!strcmp (what, "cmap")) { src = V.cmap; count = V.cmap ? V.n : 0; }
   else if (!strcmp (what, "rptr")) { src = V.rptr; count = V.rptr ? V.nc + 1 : 0; }
   else if (!strcmp (what, "ridx")) { src = V.ridx; count = V.ridx ? V.n : 0; }
   else if (!strcmp (what, "blk_start")) { src = V.B.blk_start; count = V.B.blk_start ? V.B.nblk + 1 : 0; }
   else if (!strcmp (what, "fac")) { src = V.B.fac; count = V.B.fac ? (int64_t) (2 * V.B.P + 1) * V.n : 0; elem = 8; }
   else if (!strcmp (what, "perm0")) { src = level == 0 ? s->ml.perm0 : nullptr; count = src ? V.n : 0; }
   else if (!strcmp (what, "coarse_inv")) { src = last ? s->ml.coarse_inv : nullptr; count = src ? V.n * V.n : 0; elem = 8; }
   else if (!strcmp (what, "color_blk")) { src = V.B.blk_start ? V.color_blk : nullptr; count = src ? 3 : 0; host = true; }
   else if (!strcmp (what, "col_kernel")) {      // which column-solve kernels the level was given (read-only, host values)
      const ColBlocksDev &B = V.B;
      const int v[11] = { V.wave_columns ? 1 : 0, V.wave_fused ? 1 : 0, B.stream ? 1 : 0, B.ldsres, B.gw, B.P, B.dropped, B.max_len, B.gs_ok, B.ngrp, B.lds_doubles };
      memcpy (col_kernel, v, sizeof v);
      src = B.blk_start ? col_kernel : nullptr; count = src ? 11 : 0; host = true;
   }
   else return fail (NKP_EINVAL, "nkp_ml_level_array: unknown array '%s'", what);
   if (!dst) return count;
   if (count * (int64_t) elem > capacity_bytes) return fail (NKP_EINVAL, "nkp_ml_level_array: buffer too small");
   if (host) {                                  // kept on the host: no device call
      if (count) memcpy (dst, src, (size_t) count * elem);
      return count;
   }
   HIPCHK (hipSetDevice (s->device));
   HIPCHK (hipStreamSynchronize (s->stream));
   if (count) HIPCHK (hipMemcpy (dst, src, (size_t) count * elem, hipMemcpyDeviceToHost));
   return count;
}

// the per-column diagonals of the solver's own matrix (tuning spmv_diag), same contract as nkp_ml_level_array
extern "C" int64_t nkp_matrix_array (nkp_solver *s, const char *what, void *dst, int64_t capacity_bytes)
{
   if (!s || !what) return fail (NKP_EINVAL, "nkp_matrix_array: bad argument");
   const CsrDev &A = s->A;
   const bool have = A.dg_vald != nullptr;
   const void *src = nullptr;
   int64_t count = 0;
   size_t elem = 4;
   if (!strcmp (what, "dg_ptr")) { src = A.dg_ptr; count = have ? A.dg_ncol + 1 : 0; }
   else if (!strcmp (what, "dg_key")) { src = A.dg_key; count = have ? (int64_t) A.dg_nkey : 0; }
   else if (!strcmp (what, "dg_voff")) { src = A.dg_voff; count = have ? A.dg_ncol : 0; elem = 8; }
   else if (!strcmp (what, "dg_val")) { src = A.dg_vald; count = have ? A.dg_nval : 0; elem = 8; }
   else if (!strcmp (what, "dg_gptr")) { src = A.dg_gptr; count = have ? A.dg_ncol + 1 : 0; }
   else if (!strcmp (what, "dg_grp")) { src = A.dg_grp; count = have ? 2 * (int64_t) A.dg_ngrp : 0; }
   else return fail (NKP_EINVAL, "nkp_matrix_array: unknown array '%s'", what);
   if (!dst) return count;
   if (count * (int64_t) elem > capacity_bytes) return fail (NKP_EINVAL, "nkp_matrix_array: buffer too small");
   HIPCHK (hipSetDevice (s->device));
   HIPCHK (hipStreamSynchronize (s->stream));
   if (count) HIPCHK (hipMemcpy (dst, src, (size_t) count * elem, hipMemcpyDeviceToHost));
   return count;
}

extern "C" int nkp_create (nkp_solver **out, const nkp_options *opt, int64_t n, int64_t nnz,
                           const int32_t *rowptr, const int32_t *colind, const double *val,
                           const int32_t *blk_start, int64_t nblk, int coupled_tracer_cnt)
{
   return create_impl (out, opt, n, nnz, rowptr, colind, val, blk_start, nblk, coupled_tracer_cnt, nullptr);
}

extern "C" int nkp_create64 (nkp_solver **out, const nkp_options *opt, int64_t n, const int64_t *rowptr, const int32_t *colind, const double *val,
                             const int32_t *blk_start, int64_t nblk, int coupled_tracer_cnt)
{
   if (!out) return fail (NKP_EINVAL, "nkp_create64: out is NULL");
   *out = nullptr;
   if (n < 0 || !rowptr) return fail (NKP_EINVAL, "nkp_create64: bad matrix arguments");
   if (n >= 2147483647LL || rowptr[n] >= 2147483647LL || rowptr[n] < 0)
      return fail (NKP_EINVAL, "nkp_create64: %lld rows / %lld entries: one GPU stores entry offsets in 32 bits (at most 2^31 - 1 rows and entries); "
                   "row-partition the system with nkp_create_dist, where the limit applies per rank", (long long) n, (long long) rowptr[n]);
   std::vector<int32_t> rp ((size_t) n + 1);
   for (int64_t r = 0; r <= n; r++) {
      if (rowptr[r] < 0 || rowptr[r] > rowptr[n]) return fail (NKP_EINVAL, "nkp_create64: rowptr[%lld] = %lld out of range", (long long) r, (long long) rowptr[r]);
      rp[(size_t) r] = (int32_t) rowptr[r];
   }
   return create_impl (out, opt, n, rowptr[n], rp.data (), colind, val, blk_start, nblk, coupled_tracer_cnt, nullptr);
}

extern "C" int nkp_set_stream (nkp_solver *s, void *hip_stream)
{
   if (!s) return fail (NKP_EINVAL, "nkp_set_stream: NULL solver");
   if (s->trans_of) return fail (NKP_EINVAL, "nkp_set_stream: a transposed solver runs on the stream of the solver it was transposed from; set that one's stream");
   if (s->own_stream && s->stream) { (void) hipStreamSynchronize (s->stream); (void) hipStreamDestroy (s->stream); }
   // NULL is a stream too: the device's default stream (what torch.cuda.current_stream() is unless the
   // caller switched streams), so work enqueued here stays ordered with the caller's own kernels
   s->stream = (hipStream_t) hip_stream;
   s->own_stream = false;
   for (nkp_solver *c : s->batch_members) c->stream = s->stream;      // the members of a batch share the solver's stream
   trans_set_stream (s);                                               // ... and so does the transposed solver
   return NKP_OK;
}

extern "C" int64_t nkp_get_int (nkp_solver *s, const char *key)
{
   if (!s || !key) return -1;
   if (!strcmp (key, "n")) return s->n;
   if (!strcmp (key, "nnz")) return s->A.nnz;
   if (!strcmp (key, "nblk")) return s->B.nblk;
   if (!strcmp (key, "band")) return s->B.P;
   if (!strcmp (key, "band_dropped")) return s->B.dropped;
   if (!strcmp (key, "col_stream")) return s->B.stream ? 1 : 0;
   if (!strcmp (key, "col_ldsres")) return s->B.ldsres;
   if (!strcmp (key, "col_gw")) return s->B.gw;
   if (!strcmp (key, "col_max_len")) return s->B.max_len;
   if (!strcmp (key, "col_lds_bytes")) return (int64_t) s->B.lds_doubles * (int64_t) sizeof (double);
   if (!strcmp (key, "levels")) return s->opt.precond == NKP_PRECOND_MULTILEVEL ? (int64_t) s->ml.lev.size () : 1;
   if (!strcmp (key, "ml_rows")) { int64_t t = 0; for (auto &v : s->ml.lev) t += v.n; return t; }
   if (!strcmp (key, "ml_nnz")) { int64_t t = 0; for (auto &v : s->ml.lev) t += v.L.nnz; return t; }
   if (!strcmp (key, "rowblocks")) return s->A.nrowblk;
   if (!strcmp (key, "spmv_bytes")) return 12 * s->A.nnz + 4 * (s->n + 1) + 16 * s->n;
   if (!strcmp (key, "spmv_diag")) return s->A.dg_vald ? 1 : 0;
   // compulsory bytes of one product on the diagonals, counted as ml_bytes counts a level's: values, tiles, groups, x and y
   if (!strcmp (key, "spmv_diag_bytes"))
      return s->A.dg_vald ? 8 * s->A.dg_nval + (int64_t) s->A.dg_ntile * (int64_t) sizeof (DgTile) + (int64_t) s->A.dg_ngrp * (int64_t) sizeof (DgGroup) + 16 * s->n : 0;
   if (!strcmp (key, "precond_bytes")) return s->opt.precond == NKP_PRECOND_NONE ? 16 * s->n : (int64_t) (2 * s->B.P + 1) * 8 * s->n + 16 * s->n;
   if (!strcmp (key, "device_bytes")) return (int64_t) s->device_bytes;
   if (!strcmp (key, "precond_steps")) return s->precond_steps;
   if (!strcmp (key, "equil")) return s->equil ? 1 : 0;
   if (!strcmp (key, "dist_overlap")) return s->dist.overlap ? 1 : 0;
   if (!strcmp (key, "dist_ras")) return s->dist.ras ? 1 : 0;
   if (!strcmp (key, "dist_ras_rows")) return s->dist.n_sel;
   if (!strcmp (key, "dist_ras_rings")) return s->dist.ras ? s->dist.ras_rings : 0;
   if (!strcmp (key, "dist_halo_rows")) return s->dist.n_halo;
   // rows received per preconditioner application: the SpMV halo with one ring, the overlap rows alone with more
   if (!strcmp (key, "dist_ras_recv_rows")) return !s->dist.ras ? 0 : s->dist.ras_sep ? s->dist.n_sel : s->dist.n_halo;
   if (!strcmp (key, "dist_interior_rowblocks")) return s->dist.seg_rb[2] - s->dist.seg_rb[1];
   if (!strcmp (key, "smoother_spmv_bytes")) return s->opt.precond == NKP_PRECOND_MULTILEVEL ? ml_bytes (s->ml, 0) : 0;
   if (!strcmp (key, "column_solve_bytes")) return s->opt.precond == NKP_PRECOND_MULTILEVEL ? ml_bytes (s->ml, 1) : 0;
   if (!strcmp (key, "cycle_bytes")) return s->opt.precond == NKP_PRECOND_MULTILEVEL ? ml_bytes (s->ml, 2) : 0;
   if (!strcmp (key, "ml_levels_on_device")) return s->ml.levels_on_device;
   if (!strcmp (key, "ml_inverse_pivoted")) return s->ml.inverse_pivoted;
   if (!strcmp (key, "ml_setup_us")) return (int64_t) (s->ml.setup_seconds * 1.0e6);
   if (!strcmp (key, "create_us")) return (int64_t) (s->create_seconds * 1.0e6);
   if (!strcmp (key, "refactor_count")) return s->refactor_count;
   if (!strcmp (key, "refactor_rebuilt")) return s->refactor_rebuilt;
   if (!strcmp (key, "refactor_us")) return (int64_t) (s->refactor_seconds * 1.0e6);
   if (!strcmp (key, "refactor_halo_values")) return s->refactor_halo_values;
   if (!strcmp (key, "is_transpose")) return s->trans_of ? 1 : 0;
   if (!strcmp (key, "trans_device_bytes")) return trans_device_bytes (s);
   if (!strcmp (key, "trans_us")) return (int64_t) (s->trans_seconds * 1.0e6);
   if (!strcmp (key, "trans_kernel_us")) return (int64_t) (s->trans_kernel_seconds * 1.0e6);
   if (!strcmp (key, "trans_sent_entries")) return s->trans_sent;
   if (!strcmp (key, "trans_recv_entries")) return s->trans_received;
   if (!strcmp (key, "dist_alltoallv_calls")) return s->shared->alltoallv_calls.load ();
   if (!strcmp (key, "dist_allreduce_calls")) return s->shared->allreduce_calls.load ();
   if (!strcmp (key, "value_gradient_calls")) return s->vg.calls;
   if (!strcmp (key, "value_gradient_us")) return (int64_t) (s->vg.seconds * 1.0e6);
   if (!strcmp (key, "values_product_calls")) return s->vp.calls;
   if (!strcmp (key, "values_product_us")) return (int64_t) (s->vp.seconds * 1.0e6);
   if (!strcmp (key, "tangent_calls")) return s->vp.tangent_calls;
   if (!strcmp (key, "batch_steps")) return s->batch_steps;
   if (!strcmp (key, "batch_width")) return s->batch_width;
   if (!strcmp (key, "batch_member_bytes")) {      // the further sets of work vectors a batched group keeps (not part of device_bytes)
      size_t sum = 0;
      for (const nkp_solver *c : s->batch_members) sum += c->device_bytes;
      return (int64_t) sum;
   }
   return -1;
}

// ---------------------------------------------------------------- device-side building blocks
static int dot_host (nkp_solver *s, const double *x, const double *y, double *out)
{
   launch_dot (x, y, s->n, s->partial, s->misc_dev () + 2, s->stream);
   allreduce_dev (s, s->misc_dev () + 2, 1, 0);
   HIPCHK (hipMemcpyAsync (s->hpin, s->misc_dev () + 2, sizeof (double), hipMemcpyDeviceToHost, s->stream));
   HIPCHK (hipStreamSynchronize (s->stream));
   // a collective that failed on this rank leaves stale halo rows / partial sums behind: no host decision may be taken
   // on them (the ranks' decisions would diverge and their collective sequences with them)
   if (s->comm_failed) return fail (NKP_ECOMM, "nkp_solve: a collective of the distributed solve failed");
   *out = s->hpin[0];
   return NKP_OK;
}

// one Arnoldi step on the device in two halves: (1) z_j = M^-1 v_j, w = A z_j; (2) orthogonalise w against V[0..j],
// v_{j+1} = w / ||w||, which leaves the Hessenberg column h[0..j+1] in s->h_dev().  The batched driver below replaces (1) by
// ONE application of the cycle and of A to K interleaved vectors and runs (2) per system.
static void arnoldi_apply (nkp_solver *s, int j)
{
   const int64_t ld = s->ld;
   double *zj = s->Z + (int64_t) j * ld;
   const double *vj = s->vf32 ? s->vcur : s->V + (int64_t) j * ld;
   if (s->equil) {
      // row-weighted iteration: the basis lives in the scaled space, operator R A M R^-1
      launch_vmul (vj, s->rinv, s->eqtmp, s->n, s->stream);
      apply_precond (s, s->eqtmp, zj);
      spmv_op (s, zj, s->w, nullptr, 0);
      launch_vmul (s->w, s->rscale, s->w, s->n, s->stream);
   } else {
      apply_precond (s, vj, zj);
      spmv_op (s, zj, s->w, nullptr, 0);
   }
}

static void arnoldi_orthogonalise (nkp_solver *s, int j)
{
   const int64_t ld = s->ld;
   launch_multi_dot (s->V, s->vf32, ld, j + 1, s->w, s->n, s->partial, s->h_dev (), s->stream);
   allreduce_dev (s, s->h_dev (), j + 2, 0);                 // one allreduce per Gram-Schmidt pass
   launch_update_w (s->V, s->vf32, ld, j + 1, s->h_dev (), s->w, s->n, s->partial, s->misc_dev (), s->stream);
   if (s->opt.reorth) {
      launch_multi_dot (s->V, s->vf32, ld, j + 1, s->w, s->n, s->partial, s->h2_dev (), s->stream);
      allreduce_dev (s, s->h2_dev (), j + 2, 0);
      launch_update_w (s->V, s->vf32, ld, j + 1, s->h2_dev (), s->w, s->n, s->partial, s->misc_dev (), s->stream);
      allreduce_dev (s, s->misc_dev (), 1, 0);
      launch_finish_column (s->h_dev (), s->h2_dev (), j + 1, s->misc_dev (), s->misc_dev () + 1, s->stream);
   } else if (s->dist.on && s->tune.dist_one_reduce) {
      // ||w||^2 after the update from the message that is already reduced (w.w rode along with the dots): one allreduce per step
      launch_finish_column_pythagoras (s->h_dev (), j + 1, s->misc_dev () + 1, s->stream);
   } else {
      allreduce_dev (s, s->misc_dev (), 1, 0);
      launch_finish_column (s->h_dev (), nullptr, j + 1, s->misc_dev (), s->misc_dev () + 1, s->stream);
   }
   if (s->vf32) launch_scale_to (s->w, s->misc_dev () + 1, s->vcur, (float *) s->V + (int64_t) (j + 1) * ld, s->n, s->stream);
   else launch_scale_to (s->w, s->misc_dev () + 1, s->V + (int64_t) (j + 1) * ld, nullptr, s->n, s->stream);
}

static void arnoldi_step_device (nkp_solver *s, int j)
{
   arnoldi_apply (s, j);
   arnoldi_orthogonalise (s, j);
}

// ---------------------------------------------------------------- FGMRES as a state machine
// One right-hand side's restarted FGMRES, cut at the points where the host looks at device results, so that the same code
// drives one system (fgmres) or K of them in lockstep around batched operator applications (fgmres_batch).
//
// The recurrence's residual estimate assumes an orthonormal basis; with one Gram-Schmidt pass it can run ahead of the true
// residual.  When a cycle stops on the estimate and the true residual disagrees, the next cycle aims lower by the observed
// factor (inner_scale).  Attainable-accuracy guard: three such cycles in a row that gain less than 30 % mean rounding has
// decoupled the two for good, and the iteration is stopped instead of spinning to max_iters.
struct FgmresState {
   std::vector<double> H, cs, sn, g, y;
   double bnorm = 0.0, target = 0.0, relres = 0.0;
   double beta = 0.0, beta_prev = 0.0, est_at_exit = 0.0, inner_scale = 1.0, beta_it = 0.0, target_it = 0.0;
   int its = 0, status = NKP_NOT_CONVERGED, stalled_cycles = 0;
   int j = 0;                              // columns of the running restart cycle
   bool cycle_ended_on_estimate = false;
   bool finished = false;                  // the solve is over (status says how)
   bool breakdown_in_cycle = false;
};

// ||b||, the trivial case b = 0; returns a negative code on failure
static int fg_begin (nkp_solver *s, FgmresState &F)
{
   const int m = s->m;
   F = FgmresState ();
   F.H.assign ((size_t) (m + 1) * m, 0.0);
   F.cs.assign (m, 0.0); F.sn.assign (m, 0.0); F.g.assign (m + 1, 0.0); F.y.assign (m, 0.0);
   double bnorm2 = 0.0;
   int rc = dot_host (s, s->b, s->b, &bnorm2);
   if (rc) return rc;
   F.bnorm = sqrt (bnorm2);
   s->stagnated = false;
   s->steps_now = s->precond_steps;      // the run-time guard below lowers it for this solve only
   if (!(F.bnorm > 0.0)) {         // b == 0 -> x = 0
      launch_fill (s->x, 0.0, s->n, s->stream);
      F.finished = true;
      F.status = NKP_OK;
      F.relres = 0.0;
      return NKP_OK;
   }
   F.target = fmax (s->opt.rtol * F.bnorm, s->opt.atol);
   return NKP_OK;
}

// true residual, verdict, start vector of the next restart cycle.  After it either F.finished, or v_0 is in place (F.j = 0).
static int fg_restart (nkp_solver *s, FgmresState &F)
{
   hipStream_t st = s->stream;
   const int64_t n = s->n;
   int rc;
   // true residual (unscaled: the stopping test is ||b - A x||_2 <= rtol ||b||_2 whatever norm the iteration minimises)
   spmv_op (s, s->x, s->r, s->b, 1);
   double r2 = 0.0;
   if ((rc = dot_host (s, s->r, s->r, &r2))) return rc;
   const double beta = sqrt (r2);
   F.beta = beta;
   F.relres = beta / F.bnorm;
   msg (s, 2, "fgmres: its = %d, true relres = %.3e\n", F.its, F.relres);
   if (s->comm_failed) return fail (NKP_ECOMM, "nkp_solve: a collective of the distributed solve failed");
   if (!(beta == beta)) { F.status = NKP_BREAKDOWN; F.finished = true; return NKP_OK; }
   if (beta <= F.target) { F.status = NKP_OK; F.finished = true; return NKP_OK; }
   if (F.its >= s->opt.max_iters) { F.status = NKP_NOT_CONVERGED; F.finished = true; return NKP_OK; }
   if (s->steps_now > 1 && F.its > 0 && !(beta < F.beta_prev)) {
      // a whole restart cycle without progress: the chained cycles are not helping on this right-hand side
      msg (s, 1, "fgmres: no progress over a restart cycle with %d preconditioner cycles per iteration; continuing with one\n", s->steps_now);
      s->steps_now = 1;
   }
   F.stalled_cycles = (F.cycle_ended_on_estimate && beta > 0.7 * F.beta_prev) ? F.stalled_cycles + 1 : 0;
   if (F.stalled_cycles >= 3) { F.status = NKP_NOT_CONVERGED; s->stagnated = true; F.finished = true; return NKP_OK; }
   if (F.cycle_ended_on_estimate && F.est_at_exit > 0.0) F.inner_scale = fmax (1e-3, fmin (F.inner_scale, 0.5 * F.est_at_exit / beta));
   F.beta_prev = beta;
   F.cycle_ended_on_estimate = false;
   // v0 = r / beta; in the row-weighted iteration v0 = R r / ||R r|| and the inner target is the same relative
   // reduction in that norm (the inner_scale logic above corrects it from what the next true residual shows)
   F.beta_it = beta;
   F.target_it = F.target;
   if (s->equil) {
      launch_vmul (s->r, s->rscale, s->r, n, st);
      double q2 = 0.0;
      if ((rc = dot_host (s, s->r, s->r, &q2))) return rc;
      F.beta_it = sqrt (q2);
      if (!(F.beta_it > 0.0)) { F.status = NKP_BREAKDOWN; F.finished = true; return NKP_OK; }
      F.target_it = F.target * (F.beta_it / beta);
   }
   s->hpin[0] = 1.0 / F.beta_it;
   HIPCHK (hipMemcpyAsync (s->misc_dev () + 1, s->hpin, sizeof (double), hipMemcpyHostToDevice, st));
   if (s->vf32) launch_scale_to (s->r, s->misc_dev () + 1, s->vcur, (float *) s->V, n, st);
   else launch_scale_to (s->r, s->misc_dev () + 1, s->V, nullptr, n, st);
   HIPCHK (hipStreamSynchronize (st));      // hpin is reused below
   F.g[0] = F.beta_it;
   F.j = 0;
   F.breakdown_in_cycle = false;
   return NKP_OK;
}

// column j of the Hessenberg matrix is in s->hpin[0 .. j+1] (copied and synchronised by the caller): Givens rotations, the
// residual estimate.  Returns true when this system's restart cycle ends here (estimate met, breakdown, column budget).
static bool fg_post_step (nkp_solver *s, FgmresState &F)
{
   const int m = s->m, j = F.j;
   double *hc = &F.H[(size_t) j * (m + 1)];
   for (int i = 0; i <= j + 1; i++) hc[i] = s->hpin[i];
   // a negative sub-diagonal entry is finish_column_pythagoras_kernel's mark: its magnitude is short of digits, the cycle ends here
   const bool weak_norm = hc[j + 1] < 0.0;
   if (weak_norm) hc[j + 1] = -hc[j + 1];
   for (int i = 0; i < j; i++) {
      const double t = F.cs[i] * hc[i] + F.sn[i] * hc[i + 1];
      hc[i + 1] = -F.sn[i] * hc[i] + F.cs[i] * hc[i + 1];
      hc[i] = t;
   }
   const double hjj = hc[j], hj1 = hc[j + 1];
   const double d = hypot (hjj, hj1);
   if (!(d > 0.0) || !(d == d)) { F.status = NKP_BREAKDOWN; F.breakdown_in_cycle = true; return true; }     // column j is unusable: keep k = j
   F.cs[j] = hjj / d;
   F.sn[j] = hj1 / d;
   hc[j] = d;
   hc[j + 1] = 0.0;
   F.g[j + 1] = -F.sn[j] * F.g[j];
   F.g[j] = F.cs[j] * F.g[j];
   F.its++;
   const double est = fabs (F.g[j + 1]);
   msg (s, 3, "fgmres: its = %d, est relres = %.3e\n", F.its, est / F.bnorm);
   F.j = j + 1;
   if (est <= F.target_it * F.inner_scale || hj1 == 0.0) {
      F.cycle_ended_on_estimate = true;
      F.est_at_exit = est * (F.beta / F.beta_it);
      return true;
   }
   return weak_norm || F.j >= m || F.its >= s->opt.max_iters;
}

// y = H^-1 g (upper triangular, size F.j), x += Z y; after a breakdown the true residual of what we have decides
static int fg_end_cycle (nkp_solver *s, FgmresState &F)
{
   const int m = s->m, k = F.j;
   hipStream_t st = s->stream;
   for (int i = k - 1; i >= 0; i--) {
      double t = F.g[i];
      for (int c = i + 1; c < k; c++) t -= F.H[(size_t) c * (m + 1) + i] * F.y[c];
      F.y[i] = t / F.H[(size_t) i * (m + 1) + i];
   }
   for (int i = 0; i < k; i++) s->hpin[i] = F.y[i];
   HIPCHK (hipMemcpyAsync (s->y_dev (), s->hpin, (size_t) k * sizeof (double), hipMemcpyHostToDevice, st));
   launch_axpy_multi (s->Z, s->ld, k, s->y_dev (), s->x, s->n, st);
   HIPCHK (hipStreamSynchronize (st));
   if (F.breakdown_in_cycle) {
      // report the true residual of what we have
      int rc;
      double r2 = 0.0;
      spmv_op (s, s->x, s->r, s->b, 1);
      if ((rc = dot_host (s, s->r, s->r, &r2))) return rc;
      F.relres = sqrt (r2) / F.bnorm;
      F.status = sqrt (r2) <= F.target ? NKP_OK : NKP_BREAKDOWN;
      F.finished = true;
   }
   return NKP_OK;
}

static int fgmres (nkp_solver *s, int *iters_out, double *relres_out)
{
   FgmresState F;
   int rc = fg_begin (s, F);
   if (rc) return rc;
   while (!F.finished) {
      if ((rc = fg_restart (s, F))) return rc;
      if (F.finished) break;
      for (;;) {
         arnoldi_step_device (s, F.j);
         HIPCHK (hipMemcpyAsync (s->hpin, s->h_dev (), (size_t) (F.j + 2) * sizeof (double), hipMemcpyDeviceToHost, s->stream));
         HIPCHK (hipStreamSynchronize (s->stream));
         if (s->comm_failed) return fail (NKP_ECOMM, "nkp_solve: a collective of the distributed solve failed (Arnoldi step %d)", F.its + 1);
         if (fg_post_step (s, F)) break;
      }
      if ((rc = fg_end_cycle (s, F))) return rc;
   }
   HIPCHK (hipGetLastError ());
   *iters_out = F.its;
   *relres_out = F.relres;
   return F.status;
}

// right-preconditioned BiCGStab; every inner product is a deterministic two-stage reduction
static int bicgstab (nkp_solver *s, int *iters_out, double *relres_out)
{
   const int64_t n = s->n, ld = s->ld;
   hipStream_t st = s->stream;
   if (s->m < 2) return fail (NKP_EINVAL, "bicgstab needs restart >= 2 (it borrows the Krylov basis storage)");
   double *r = s->r, *r0 = s->V, *p = s->V + ld, *v = s->V + 2 * ld;
   double *ph = s->Z, *sh = s->Z + ld, *t = s->t2, *sv = s->t1;
   int rc;
   double bnorm2, rho = 1.0, alpha = 1.0, omega = 1.0, tmp;
   if ((rc = dot_host (s, s->b, s->b, &bnorm2))) return rc;
   const double bnorm = sqrt (bnorm2);
   if (!(bnorm > 0.0)) { launch_fill (s->x, 0.0, n, st); *iters_out = 0; *relres_out = 0.0; return NKP_OK; }
   const double target = fmax (s->opt.rtol * bnorm, s->opt.atol);
   spmv_op (s, s->x, r, s->b, 1);
   launch_copy (r, r0, n, st);
   launch_fill (p, 0.0, n, st);
   launch_fill (v, 0.0, n, st);
   int its = 0, status = NKP_NOT_CONVERGED;
   double rn2;
   if ((rc = dot_host (s, r, r, &rn2))) return rc;
   double relres = sqrt (rn2) / bnorm;
   while (its < s->opt.max_iters) {
      if (sqrt (rn2) <= target) { status = NKP_OK; break; }
      double rho_new;
      if ((rc = dot_host (s, r0, r, &rho_new))) return rc;
      if (rho_new == 0.0 || !(rho_new == rho_new)) { status = NKP_BREAKDOWN; break; }
      const double beta = (rho_new / rho) * (alpha / omega);
      // p = r + beta (p - omega v)
      launch_axpby (-omega, v, 1.0, p, n, st);
      launch_axpby (1.0, r, beta, p, n, st);
      apply_precond (s, p, ph);
      spmv_op (s, ph, v, nullptr, 0);
      if ((rc = dot_host (s, r0, v, &tmp))) return rc;
      if (tmp == 0.0 || !(tmp == tmp)) { status = NKP_BREAKDOWN; break; }
      alpha = rho_new / tmp;
      // s = r - alpha v
      launch_copy (r, sv, n, st);
      launch_axpby (-alpha, v, 1.0, sv, n, st);
      apply_precond (s, sv, sh);
      spmv_op (s, sh, t, nullptr, 0);
      double ts, tt;
      if ((rc = dot_host (s, t, sv, &ts))) return rc;
      if ((rc = dot_host (s, t, t, &tt))) return rc;
      if (tt == 0.0 || !(tt == tt)) { status = NKP_BREAKDOWN; break; }
      omega = ts / tt;
      // x += alpha ph + omega sh ; r = s - omega t
      launch_axpby (alpha, ph, 1.0, s->x, n, st);
      launch_axpby (omega, sh, 1.0, s->x, n, st);
      launch_copy (sv, r, n, st);
      launch_axpby (-omega, t, 1.0, r, n, st);
      rho = rho_new;
      its++;
      if ((rc = dot_host (s, r, r, &rn2))) return rc;
      relres = sqrt (rn2) / bnorm;
      msg (s, 3, "bicgstab: its = %d, recurrence relres = %.3e\n", its, relres);
      if (omega == 0.0) { status = NKP_BREAKDOWN; break; }
   }
   // true residual
   spmv_op (s, s->x, r, s->b, 1);
   if ((rc = dot_host (s, r, r, &rn2))) return rc;
   relres = sqrt (rn2) / bnorm;
   if (sqrt (rn2) <= target * 1.0001) status = NKP_OK;
   else if (status == NKP_OK) status = NKP_NOT_CONVERGED;
   HIPCHK (hipGetLastError ());
   *iters_out = its;
   *relres_out = relres;
   return status;
}

// componentwise backward error of s->x for s->b, like SuperLU's berr
static int backward_error (nkp_solver *s, double *berr)
{
   spmv_op (s, s->x, s->r, s->b, 1);
   spmv_op (s, s->x, s->t1, s->b, 2);
   launch_berr (s->r, s->t1, s->n, s->partial, s->misc_dev () + 3, s->stream);
   allreduce_dev (s, s->misc_dev () + 3, 1, 1);
   HIPCHK (hipMemcpyAsync (s->hpin, s->misc_dev () + 3, sizeof (double), hipMemcpyDeviceToHost, s->stream));
   HIPCHK (hipStreamSynchronize (s->stream));
   *berr = s->hpin[0];
   return NKP_OK;
}

static int refactor_broken (const nkp_solver *s) { return fail (NKP_ESINGULAR, "%s", s->shared->why.c_str ()); }

static int solve_resident (nkp_solver *s, double *berr, int *iters, double *relres)
{
   if (s->shared->broken) return refactor_broken (s);
   int it = 0;
   double rr = 0.0;
   s->stagnated = false;
   int status = (s->opt.krylov == NKP_KRYLOV_BICGSTAB) ? bicgstab (s, &it, &rr) : fgmres (s, &it, &rr);
   if (status < 0) return status;
   double be = 0.0;
   if (berr || s->stagnated) {
      int rc = backward_error (s, &be);
      if (rc) return rc;
      if (berr) *berr = be;
   }
   // the reference's only accuracy measure is SuperLU's componentwise backward error: a solve that has reached
   // the attainable accuracy with berr at rounding level, or two orders below the requested tolerance (berr bounds
   // the normwise backward error), is as converged as f64 allows, whatever ||r||/||b|| is
   if (s->comm_failed) return fail (NKP_ECOMM, "nkp_solve: a collective of the distributed solve failed");
   if (status == NKP_NOT_CONVERGED && s->stagnated && be <= fmax (NKP_BERR_ROUNDING_LEVEL, 1.0e-2 * s->opt.rtol)) {
      msg (s, 1, "nkp_solve: residual stagnated at %.3e (rtol %.1e) with backward error %.3e: NKP_OK_BERR\n", rr, s->opt.rtol, be);
      status = NKP_OK_BERR;
   }
   if (iters) *iters = it;
   if (relres) *relres = rr;
   msg (s, 1, "nkp_solve: %s after %d iterations, ||b-Ax||/||b|| = %.3e\n", status == NKP_OK ? "converged" : status == NKP_OK_BERR ? "at the attainable accuracy (backward error accepted)" : status == NKP_BREAKDOWN ? "breakdown" : "NOT converged", it, rr);
   if (status == NKP_OK_BERR) fail (status, "nkp_solve: ||b-Ax||/||b|| = %.3e stopped above rtol %.1e at the attainable accuracy after %d iterations; componentwise backward error %.3e", rr, s->opt.rtol, it, be);
   else if (status != NKP_OK) fail (status, "nkp_solve: %s after %d iterations (relres %.3e, rtol %.1e)", status == NKP_BREAKDOWN ? "breakdown" : s->stagnated ? "stagnated at the attainable accuracy, not converged" : "not converged", it, rr, s->opt.rtol);
   return status;
}

extern "C" int nkp_solve_device (nkp_solver *s, const void *d_b, void *d_x, int use_guess, double *berr, int *iters, double *relres)
{
   if (!s || !d_b || !d_x) return fail (NKP_EINVAL, "nkp_solve_device: NULL argument");
   HIPCHK (hipSetDevice (s->device));
   const size_t bytes = (size_t) s->n * sizeof (double);
   if (use_guess) HIPCHK (hipMemcpyAsync (s->x, d_x, bytes, hipMemcpyDeviceToDevice, s->stream));
   else HIPCHK (hipMemsetAsync (s->x, 0, bytes, s->stream));
   HIPCHK (hipMemcpyAsync (s->b, d_b, bytes, hipMemcpyDeviceToDevice, s->stream));
   int status = solve_resident (s, berr, iters, relres);
   if (status < 0) return status;
   HIPCHK (hipMemcpyAsync (d_x, s->x, bytes, hipMemcpyDeviceToDevice, s->stream));
   HIPCHK (hipStreamSynchronize (s->stream));
   return status;
}

// A second set of work vectors (Krylov basis, level vectors, scalars) and a second stream on the SAME device-resident
// matrix, factors and hierarchy: several right-hand sides can then be solved concurrently from different host threads,
// one clone per thread.  Single-GPU solvers only.
//
// member: the work vectors of one more system of a batched solve.  A member of a row-distributed solver shares its parent's
// matrix, hierarchy, stream, plan and exchange buffers (all of its work is ordered on that one stream) and is only ever driven
// from inside the parent's collective calls, so it adds no collective of its own.
static int clone_impl (nkp_solver *src, nkp_solver **out, bool member)
{
   if (!src || !out) return fail (NKP_EINVAL, "nkp_clone: NULL argument");
   *out = nullptr;
   if (src->dist.on && !member) return fail (NKP_EINVAL, "nkp_clone: not available for the row-distributed flavour");
   if (src->borrowed) return fail (NKP_EINVAL, "nkp_clone: clone the original solver, not a clone");
   if (src->trans_of && !member) return fail (NKP_EINVAL, "nkp_clone: not available on a transposed solver (its owner may free it at a refactor)");
   HIPCHK (hipSetDevice (src->device));
   nkp_solver *s = new (std::nothrow) nkp_solver (*src);
   if (!s) return fail (NKP_ENOMEM, "nkp_clone: out of host memory");
   s->borrowed = true;
   s->rf = nullptr;
   s->shared->clones++;
   s->stagnated = false;
   s->batch_members.clear ();
   s->bvin = s->bz = s->bw = nullptr;
   s->batch_K = 0;
   s->dist.bxe = s->dist.bsend = s->dist.gmsg = s->dist.ghpin = s->dist.bras_send = s->dist.bras_recv = nullptr;
   s->dist.bK = s->dist.agreed_K = 0;
   s->dplan = nullptr;
   s->trans = s->trans_of = nullptr;
   s->trans_src = nullptr;
   s->trans_val = nullptr;
   s->trans_map_bytes = 0;
   s->trans_ship = nullptr;
   s->trans_send = s->trans_recv = nullptr;
   s->vg = decltype (s->vg) ();      // nkp_value_gradient's work space and counters are per handle
   s->vp = decltype (s->vp) ();      // and nkp_values_product's
   s->A.tune = &s->tune;
   s->B.tune = &s->tune;
   s->ml.tune = &s->tune;
   for (MlLevel &L : s->ml.lev) L.L.tune = L.B.tune = &s->tune;
   s->stream = nullptr;
   s->own_stream = false;
   s->device_bytes = 0;
   s->V = s->vcur = s->Z = s->w = s->r = s->x = s->b = s->t1 = s->t2 = s->p1 = s->p2 = s->eqtmp = s->partial = s->dscal = s->hpin = nullptr;
   s->dint = nullptr;
   for (MlLevel &L : s->ml.lev) L.x = L.x2 = L.b = L.r = nullptr;
   int rc = NKP_OK;
   TRYHIP (hipStreamCreateWithFlags (&s->stream, hipStreamNonBlocking));
   s->own_stream = true;
   TRY (alloc_work_vectors (s, member));
   for (MlLevel &L : s->ml.lev) {
      TRY (dev_alloc (s, &L.x, (size_t) L.n));
      TRY (dev_alloc (s, &L.x2, (size_t) L.n));
      TRY (dev_alloc (s, &L.b, (size_t) L.n));
      TRY (dev_alloc (s, &L.r, (size_t) L.n));
      TRYHIP (hipMemset (L.x, 0, (size_t) (L.n ? L.n : 1) * sizeof (double)));
      TRYHIP (hipMemset (L.x2, 0, (size_t) (L.n ? L.n : 1) * sizeof (double)));
      TRYHIP (hipMemset (L.b, 0, (size_t) (L.n ? L.n : 1) * sizeof (double)));
      TRYHIP (hipMemset (L.r, 0, (size_t) (L.n ? L.n : 1) * sizeof (double)));
   }
   *out = s;
   return NKP_OK;
}

#undef TRY
#undef TRYHIP

extern "C" int nkp_clone (nkp_solver *src, nkp_solver **out) { return clone_impl (src, out, false); }

// ---------------------------------------------------------------- K right-hand sides in lockstep
// The reference's RHS loop (src/solve_ABglobal.c:370-409) as ONE pass over the matrix and the hierarchy per Krylov step for K
// systems: every system keeps its own FGMRES recurrence (own basis, own Hessenberg matrix, own restart decisions -- the state
// machine above), but the K applications of the cycle and of A in a step are one application to K interleaved vectors
// (batch.hip).  Per system the operations and their order are those of a solve done alone, so are the bits.
//
// Row equilibration and chained preconditioner cycles are fixed linear changes around those same applications and are batched
// with them (batch_step_apply).  What is NOT covered takes its right-hand sides one at a time, with the same answers:
//   a clone                    its work vectors are one system's, and it may run next to its siblings
//   BiCGStab                   the lockstep driver is FGMRES's state machine
//   an f32 Krylov basis        the batched kernels read an f64 basis
//   row equilibration on a row-distributed solver      the K-wide overlap exchange carries unscaled rows
static const char *batch_unsupported (const nkp_solver *s)
{
   if (s->borrowed) return "a clone";
   if (s->opt.krylov != NKP_KRYLOV_FGMRES) return "BiCGStab";
   if (s->equil && s->dist.on) return "row equilibration on a row-distributed solver";
   if (s->vf32) return "an f32 Krylov basis";
   return nullptr;
}

// the one line a batched call that falls back leaves at -D1
static void note_fallback (const nkp_solver *s, const char *who, const char *why, int nrhs)
{
   msg (s, 1, "%s: %d right-hand sides one at a time: the batched path does not cover %s\n", who, nrhs, why);
}

// a set of device buffers of `count` doubles per unit of width each, all or nothing (see batch_prepare)
static int buffer_set (nkp_solver *s, std::initializer_list<std::pair<double **, size_t>> set, int *width, int K_new)
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
   return s->dist.ras_sep
             ? buffer_set (s, { { &s->dist.bxe, (size_t) (s->n + s->dist.n_halo) }, { &s->dist.bsend, (size_t) s->dist.nsend }, { &s->dist.gmsg, gcount },
                                { &s->dist.bras_send, (size_t) s->dist.ras_nsend }, { &s->dist.bras_recv, (size_t) s->dist.n_sel } }, &s->dist.bK, K)
             : buffer_set (s, { { &s->dist.bxe, (size_t) (s->n + s->dist.n_halo) }, { &s->dist.bsend, (size_t) s->dist.nsend }, { &s->dist.gmsg, gcount } }, &s->dist.bK, K);
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
      double *halo = D.bxe + n * K;
      if (D.ras_sep) {
         // several rings: the overlap rows alone, K wide, into a block of their own in the hierarchy's order
         D.ras_send_counts_k.resize (D.ras_send_counts.size ());
         D.ras_recv_counts_k.resize (D.ras_recv_counts.size ());
         for (size_t p = 0; p < D.ras_send_counts.size (); p++) D.ras_send_counts_k[p] = D.ras_send_counts[p] * K;
         for (size_t p = 0; p < D.ras_recv_counts.size (); p++) D.ras_recv_counts_k[p] = D.ras_recv_counts[p] * K;
         if (D.ras_nsend) launch_pack_rows_split (K, D.ras_send_idx, src, D.bras_send, D.ras_nsend, st);
         alltoallv_dev (s, D.bras_send, D.ras_send_counts_k.data (), D.bras_recv, D.ras_recv_counts_k.data (), st);
         ml_apply_batch_split_ext (s->ml, K, src, D.bras_recv, nullptr, n, zi, dz ? dz : none, st);
      } else {
         if (D.nsend) launch_pack_rows_split (K, D.send_idx, src, D.bsend, D.nsend, st);
         alltoallv_dev (s, D.bsend, D.send_counts_k.data (), halo, D.recv_counts_k.data (), st);
         ml_apply_batch_split_ext (s->ml, K, src, halo, D.sel_idx, n, zi, dz ? dz : none, st);
      }
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
// of xi -- s->bz, or the own rows of s->dist.bxe, whose halo rows arrive here as spmv_op fetches them for one vector
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
   if (!D.on) rows (0, s->A.nrowblk);
   else {
      double *halo = D.bxe + n * K;
      if (D.nsend) launch_gather_batch (K, D.send_idx, xi, D.bsend, D.nsend, st);
      if (D.overlap) {
         (void) hipEventRecord (D.ev_packed, st);
         (void) hipStreamWaitEvent (D.comm_stream, D.ev_packed, 0);
         alltoallv_dev (s, D.bsend, D.send_counts_k.data (), halo, D.recv_counts_k.data (), D.comm_stream);
         (void) hipEventRecord (D.ev_halo, D.comm_stream);
         rows (D.seg_rb[1], D.seg_rb[2]);
         (void) hipStreamWaitEvent (st, D.ev_halo, 0);
         rows (D.seg_rb[0], D.seg_rb[1]);
         rows (D.seg_rb[2], D.seg_rb[3]);
      } else {
         alltoallv_dev (s, D.bsend, D.send_counts_k.data (), halo, D.recv_counts_k.data (), st);
         rows (0, s->A.nrowblk);
      }
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
   if (s->dist.on) {
      auto &D = s->dist;
      D.send_counts_k.resize (D.send_counts.size ());
      D.recv_counts_k.resize (D.recv_counts.size ());
      for (size_t p = 0; p < D.send_counts.size (); p++) D.send_counts_k[p] = D.send_counts[p] * K;
      for (size_t p = 0; p < D.recv_counts.size (); p++) D.recv_counts_k[p] = D.recv_counts[p] * K;
   }
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
int dist_agree (nkp_solver *s, int local_rc, const char *who, const char *where)
{
   const nkp_comm_ops &c = s->dist.ops;
   std::vector<int64_t> all ((size_t) c.nranks + 1, 0);
   const std::string mine = local_rc ? last_error_message () : std::string ();
   const bool comm_ok = c.allgather_i64_host (c.ctx, local_rc ? 1 : 0, all.data ()) == 0;
   if (local_rc) { restore_error_message (mine); return local_rc; }
   if (!comm_ok) return fail (NKP_ECOMM, "%s: allgather failed (%s)", who, where);
   for (int p = 0; p < c.nranks; p++)
      if (all[(size_t) p]) return fail (NKP_ECOMM, "%s: rank %d failed (%s); see its message", who, p, where);
   return NKP_OK;
}

static int sev_of (int c) { return c == NKP_OK ? 0 : c == NKP_OK_BERR ? 1 : c == NKP_NOT_CONVERGED ? 2 : 3; }

extern "C" int nkp_solve_batch_device (nkp_solver *s, int nrhs, const void *d_B, void *d_X, int64_t ldb, double *berr, int *iters, double *relres)
{
   if (!s || nrhs < 0 || (nrhs > 0 && (!d_B || !d_X))) return fail (NKP_EINVAL, "nkp_solve_batch_device: NULL argument");
   if (nrhs > 0 && ldb < s->n) return fail (NKP_EINVAL, "nkp_solve_batch_device: ldb < n");
   if (s->shared->broken) return refactor_broken (s);
   HIPCHK (hipSetDevice (s->device));
   const double *B = (const double *) d_B;
   double *X = (double *) d_X;
   const size_t bytes = (size_t) s->n * sizeof (double);
   int worst = NKP_OK;
   const char *why = batch_unsupported (s);
   if (why || nrhs < 2 || !s->tune.rhs_batch) {
      // one at a time (the reference's loop); `why` names what the batched path does not cover
      if (why && nrhs >= 2 && s->tune.rhs_batch) note_fallback (s, "nkp_solve_batch", why, nrhs);
      for (int c = 0; c < nrhs; c++) {
         const int status = nkp_solve_device (s, B + (size_t) c * (size_t) ldb, X + (size_t) c * (size_t) ldb, 0, berr ? berr + c : nullptr, iters ? iters + c : nullptr, relres ? relres + c : nullptr);
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
         const int status = nkp_solve_device (s, B + (size_t) c0 * (size_t) ldb, X + (size_t) c0 * (size_t) ldb, 0, berr ? berr + c0 : nullptr, iters ? iters + c0 : nullptr, relres ? relres + c0 : nullptr);
         if (status < 0) return status;
         if (sev_of (status) > sev_of (worst)) worst = status;
         continue;
      }
      int K = nact <= 2 ? 2 : nact <= 4 ? 4 : 8;
      const int K_wanted = K;
      int rc = NKP_OK;
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
         const nkp_comm_ops &c = s->dist.ops;
         std::vector<int64_t> all ((size_t) c.nranks + 1, 0);
         const std::string mine = rc ? last_error_message () : std::string ();
         const bool comm_ok = c.allgather_i64_host (c.ctx, rc ? -1 : K, all.data ()) == 0;
         if (rc) { restore_error_message (mine); return rc; }
         if (!comm_ok) return fail (NKP_ECOMM, "nkp_solve_batch: allgather failed (interleave width)");
         for (int p = 0; p < c.nranks; p++) {
            if (all[(size_t) p] < 0) return fail (NKP_ECOMM, "nkp_solve_batch: rank %d failed while preparing %d right-hand sides; see its message", p, K_wanted);
            if (all[(size_t) p] < K) K = (int) all[(size_t) p];
         }
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
         HIPCHK (hipMemsetAsync (mem[k]->x, 0, bytes, s->stream));
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
         if (status == NKP_NOT_CONVERGED && q->stagnated && be <= fmax (NKP_BERR_ROUNDING_LEVEL, 1.0e-2 * s->opt.rtol)) status = NKP_OK_BERR;
         if (iters) iters[c0 + k] = F[k].its;
         if (relres) relres[c0 + k] = F[k].relres;
         msg (s, 1, "nkp_solve_batch: right-hand side %d: %s after %d iterations, ||b-Ax||/||b|| = %.3e\n", c0 + k,
              status == NKP_OK ? "converged" : status == NKP_OK_BERR ? "at the attainable accuracy (backward error accepted)" : status == NKP_BREAKDOWN ? "breakdown" : "NOT converged", F[k].its, F[k].relres);
         if (status != NKP_OK) fail (status, "nkp_solve_batch: right-hand side %d: %s after %d iterations (relres %.3e, rtol %.1e)", c0 + k,
                                     status == NKP_OK_BERR ? "stopped above rtol at the attainable accuracy" : status == NKP_BREAKDOWN ? "breakdown" : "not converged", F[k].its, F[k].relres, s->opt.rtol);
         if (sev_of (status) > sev_of (worst)) worst = status;
         HIPCHK (hipMemcpyAsync (X + (size_t) (c0 + k) * (size_t) ldb, q->x, bytes, hipMemcpyDeviceToDevice, s->stream));
      }
      HIPCHK (hipStreamSynchronize (s->stream));
   }
   return worst;
}

extern "C" int nkp_solve (nkp_solver *s, double *b_in_x_out, int nrhs, int64_t ldb, double *berr, int *iters, double *relres)
{
   if (!s || (nrhs > 0 && !b_in_x_out)) return fail (NKP_EINVAL, "nkp_solve: NULL argument");
   if (nrhs < 0 || (nrhs > 0 && ldb < s->n)) return fail (NKP_EINVAL, "nkp_solve: bad nrhs/ldb");
   HIPCHK (hipSetDevice (s->device));
   const size_t bytes = (size_t) s->n * sizeof (double);
   int worst = NKP_OK;
   if (nrhs >= 2 && s->tune.rhs_batch && !batch_unsupported (s)) {
      // several right-hand sides share the sweeps over the matrix and the hierarchy (same bits per column as one at a time)
      double *dB = nullptr;
      const int64_t ldd = s->ld;
      int status = NKP_OK;
      if (hipMalloc ((void **) &dB, (size_t) ldd * (size_t) nrhs * sizeof (double)) != hipSuccess) {
         dB = nullptr;
         (void) hipGetLastError ();
         status = fail (NKP_ENOMEM, "nkp_solve: device memory for %d right-hand sides", nrhs);
      }
      for (int c = 0; c < nrhs && status == NKP_OK; c++)
         if (hipMemcpy (dB + (size_t) c * (size_t) ldd, b_in_x_out + (size_t) c * (size_t) ldb, bytes, hipMemcpyHostToDevice) != hipSuccess) status = fail (NKP_EDEVICE, "nkp_solve: upload of right-hand side %d failed", c);
      // row-distributed: a rank that could not stage its right-hand sides must not leave the others alone in the collectives
      if (s->dist.on) status = dist_agree (s, status, "nkp_solve", "staging the right-hand sides on the device");
      if (status != NKP_OK) { if (dB) (void) hipFree (dB); return status; }
      if (status == NKP_OK) status = nkp_solve_batch_device (s, nrhs, dB, dB, ldd, berr, iters, relres);
      if (status >= 0)
         for (int c = 0; c < nrhs; c++)
            if (hipMemcpy (b_in_x_out + (size_t) c * (size_t) ldb, dB + (size_t) c * (size_t) ldd, bytes, hipMemcpyDeviceToHost) != hipSuccess) status = fail (NKP_EDEVICE, "nkp_solve: download of solution %d failed", c);
      (void) hipFree (dB);
      return status;
   }
   if (nrhs >= 2 && s->tune.rhs_batch) note_fallback (s, "nkp_solve", batch_unsupported (s), nrhs);
   for (int c = 0; c < nrhs; c++) {          // nrhs = 0 is the reference's factor-only call: nothing to do
      double *col = b_in_x_out + (size_t) c * (size_t) ldb;
      HIPCHK (hipMemcpyAsync (s->b, col, bytes, hipMemcpyHostToDevice, s->stream));
      HIPCHK (hipMemsetAsync (s->x, 0, bytes, s->stream));
      int status = solve_resident (s, berr ? berr + c : nullptr, iters ? iters + c : nullptr, relres ? relres + c : nullptr);
      if (status < 0) return status;
      HIPCHK (hipMemcpyAsync (col, s->x, bytes, hipMemcpyDeviceToHost, s->stream));
      HIPCHK (hipStreamSynchronize (s->stream));
      // severity: OK < OK_BERR < NOT_CONVERGED < BREAKDOWN
      if (sev_of (status) > sev_of (worst)) worst = status;
   }
   return worst;
}

// ---------------------------------------------------------------- exposed pieces (parity / roofline)
extern "C" int nkp_spmv_device (nkp_solver *s, const void *d_x, void *d_y)
{
   if (!s || !d_x || !d_y) return fail (NKP_EINVAL, "nkp_spmv_device: NULL argument");
   HIPCHK (hipSetDevice (s->device));
   spmv_op (s, (const double *) d_x, (double *) d_y, nullptr, 0);
   HIPCHK (hipStreamSynchronize (s->stream));
   HIPCHK (hipGetLastError ());
   return NKP_OK;
}

extern "C" int nkp_spmv (nkp_solver *s, const double *x, double *y)
{
   if (!s || !x || !y) return fail (NKP_EINVAL, "nkp_spmv: NULL argument");
   HIPCHK (hipSetDevice (s->device));
   const size_t bytes = (size_t) s->n * sizeof (double);
   HIPCHK (hipMemcpyAsync (s->t1, x, bytes, hipMemcpyHostToDevice, s->stream));
   spmv_op (s, s->t1, s->t2, nullptr, 0);
   HIPCHK (hipMemcpyAsync (y, s->t2, bytes, hipMemcpyDeviceToHost, s->stream));
   HIPCHK (hipStreamSynchronize (s->stream));
   HIPCHK (hipGetLastError ());
   return NKP_OK;
}

extern "C" int nkp_precond_apply (nkp_solver *s, const double *r, double *z)
{
   if (!s || !r || !z) return fail (NKP_EINVAL, "nkp_precond_apply: NULL argument");
   if (s->shared->broken) return refactor_broken (s);
   HIPCHK (hipSetDevice (s->device));
   const size_t bytes = (size_t) s->n * sizeof (double);
   HIPCHK (hipMemcpyAsync (s->t1, r, bytes, hipMemcpyHostToDevice, s->stream));
   apply_precond_once (s, s->t1, s->t2);      // one cycle: what the parity tests and the cycle timing mean
   HIPCHK (hipMemcpyAsync (z, s->t2, bytes, hipMemcpyDeviceToHost, s->stream));
   HIPCHK (hipStreamSynchronize (s->stream));
   HIPCHK (hipGetLastError ());
   return NKP_OK;
}

extern "C" int nkp_multi_dot (nkp_solver *s, const double *V, int64_t ld, int k, const double *w, double *out)
{
   if (!s || !V || !w || !out || k < 0 || k > s->m + 1 || ld < s->n) return fail (NKP_EINVAL, "nkp_multi_dot: bad argument (k must be <= restart+1)");
   HIPCHK (hipSetDevice (s->device));
   std::vector<float> vf;
   for (int j = 0; j < k; j++) {
      if (s->vf32) {
         vf.assign (V + (int64_t) j * ld, V + (int64_t) j * ld + s->n);
         HIPCHK (hipMemcpyAsync ((float *) s->V + (int64_t) j * s->ld, vf.data (), (size_t) s->n * sizeof (float), hipMemcpyHostToDevice, s->stream));
         HIPCHK (hipStreamSynchronize (s->stream));        // vf is reused
      } else
         HIPCHK (hipMemcpyAsync (s->V + (int64_t) j * s->ld, V + (int64_t) j * ld, (size_t) s->n * sizeof (double), hipMemcpyHostToDevice, s->stream));
   }
   HIPCHK (hipMemcpyAsync (s->w, w, (size_t) s->n * sizeof (double), hipMemcpyHostToDevice, s->stream));
   launch_multi_dot (s->V, s->vf32, s->ld, k, s->w, s->n, s->partial, s->h_dev (), s->stream);
   allreduce_dev (s, s->h_dev (), k + 1, 0);
   HIPCHK (hipMemcpyAsync (out, s->h_dev (), (size_t) (k + 1) * sizeof (double), hipMemcpyDeviceToHost, s->stream));
   HIPCHK (hipStreamSynchronize (s->stream));
   HIPCHK (hipGetLastError ());
   return NKP_OK;
}

extern "C" int nkp_time_kernel (nkp_solver *s, int which, int arg, int reps, double *avg_ms)
{
   if (!s || !avg_ms || reps < 1) return fail (NKP_EINVAL, "nkp_time_kernel: bad argument");
   if (which == 8 && !s->A.dg_vald) return fail (NKP_EINVAL, "nkp_time_kernel: the matrix has no per-column diagonals (tuning spmv_diag)");
   HIPCHK (hipSetDevice (s->device));
   if (which == 5) {      // the gradient kernel of nkp_value_gradient at interleave width arg, on scratch operands of its own
      const int prc = valgrad_time_prepare (s, arg);
      if (prc) return prc;
   }
   if (which == 6 || which == 7) {      // the product kernel of nkp_values_product at interleave width arg, likewise; 7: what it replaces
      const int prc = valprod_time_prepare (s, arg, which);
      if (prc) return prc;
   }
   hipEvent_t e0, e1;
   HIPCHK (hipEventCreate (&e0));
   HIPCHK (hipEventCreate (&e1));
   // operands: whatever is in the work vectors (made finite first)
   launch_fill (s->t1, 1.0, s->n, s->stream);
   if (which == 2) {
      if (arg < 0 || arg >= s->m) return fail (NKP_EINVAL, "nkp_time_kernel: restart position out of range");
      // finite operands in whichever basis precision is active (f32 vectors are filled through their f64 twin)
      for (int j = 0; j <= arg + 1; j++) {
         launch_fill (s->t2, 1.0 / (1.0 + j), s->n, s->stream);
         s->hpin[0] = 1.0;
         HIPCHK (hipMemcpyAsync (s->misc_dev () + 1, s->hpin, sizeof (double), hipMemcpyHostToDevice, s->stream));
         if (s->vf32) launch_scale_to (s->t2, s->misc_dev () + 1, s->vcur, (float *) s->V + (int64_t) j * s->ld, s->n, s->stream);
         else launch_scale_to (s->t2, s->misc_dev () + 1, s->V + (int64_t) j * s->ld, nullptr, s->n, s->stream);
         HIPCHK (hipStreamSynchronize (s->stream));
      }
   }
   for (int pass = 0; pass < 2; pass++) {      // pass 0 = warm-up
      const int cnt = pass == 0 ? (reps < 3 ? reps : 3) : reps;
      HIPCHK (hipEventRecord (e0, s->stream));
      for (int i = 0; i < cnt; i++) {
         if (which == 0 && s->A.dg_vald) launch_csr_spmv (s->A, s->t1, s->t2, nullptr, 0, s->stream);      // 0 stays the CSR kernel
         else if (which == 0) spmv_op (s, s->t1, s->t2, nullptr, 0);
         else if (which == 8) launch_diag_spmv (s->A, s->t1, s->t2, nullptr, 0, s->stream);
         else if (which == 1) apply_precond_once (s, s->t1, s->t2);
         else if (which == 2) arnoldi_step_device (s, arg);
         else if (which == 5) valgrad_time_launch (s, arg);
         else if (which == 6) valprod_time_launch (s, arg);
         else if (which == 7) valprod_time_composition (s, arg);
         else if (s->opt.precond == NKP_PRECOND_MULTILEVEL) ml_time_piece (s->ml, which - 3, s->stream);   // 3: smoother residual rows, 4: column solves (level 0, colour 0)
      }
      HIPCHK (hipEventRecord (e1, s->stream));
      HIPCHK (hipEventSynchronize (e1));
      float ms = 0.f;
      HIPCHK (hipEventElapsedTime (&ms, e0, e1));
      *avg_ms = (double) ms / cnt;
   }
   (void) hipEventDestroy (e0);
   (void) hipEventDestroy (e1);
   HIPCHK (hipGetLastError ());
   return NKP_OK;
}

// ---------------------------------------------------------------- distributed flavour (its host-side plan: dist_plan.cpp)
extern "C" int nkp_create_dist (nkp_solver **out, const nkp_options *opt, int64_t n_global, int64_t fst_row, int64_t m_loc,
                                int64_t nnz_loc, const int32_t *rowptr_loc, const int32_t *colind_glob, const double *val,
                                const int32_t *blk_start_loc, int64_t nblk_loc, int coupled_tracer_cnt, const nkp_comm_ops *comm)
{
   if (!out) return fail (NKP_EINVAL, "nkp_create_dist: out is NULL");
   *out = nullptr;
   nkp_tuning tune;
   {
      // a dist_ras_rings out of range is refused by every rank together (dist_plan) when there are peers to tell
      bool range_error = false;
      const int trc = resolve_tuning (opt, &tune, &range_error);
      if (trc && !(range_error && comm && comm->nranks > 1)) return trc;
   }
   if (!comm || (comm->nranks <= 1 && !tune.force_dist)) {
      if (fst_row != 0 || m_loc != n_global) return fail (NKP_EINVAL, "nkp_create_dist: a single rank must own all rows");
      return create_impl (out, opt, n_global, nnz_loc, rowptr_loc, colind_glob, val, blk_start_loc, nblk_loc, coupled_tracer_cnt, nullptr);
   }
   if (!comm->allreduce || !comm->alltoallv || !comm->alltoallv_i32_host || !comm->allgather_i64_host)
      return fail (NKP_EINVAL, "nkp_create_dist: incomplete nkp_comm_ops");
   if (!rowptr_loc || m_loc < 0 || nnz_loc < 0 || (nnz_loc > 0 && (!colind_glob || !val))) return fail (NKP_EINVAL, "nkp_create_dist: bad matrix arguments");
   const int P = comm->nranks, rank = comm->rank;
   std::vector<int64_t> starts (P + 1, 0);
   if (comm->allgather_i64_host (comm->ctx, fst_row, starts.data ())) return fail (NKP_ECOMM, "nkp_create_dist: allgather failed");
   starts[P] = n_global;
   for (int p = 0; p < P; p++)
      if (starts[p + 1] < starts[p] || starts[0] != 0) return fail (NKP_EINVAL, "nkp_create_dist: row blocks must be contiguous and ascending over the ranks");
   // (whether m_loc matches the next rank's fst_row is a per-rank finding: dist_plan checks it and all ranks leave together)

   nkp_options o;
   if (opt) o = *opt;
   else nkp_default_options (&o);
   o.rank = rank;
   o.tuning = &tune;               // resolved once for the plan and the create call below
   DistPlan D;
   int rc = dist_plan (D, comm, o, starts, fst_row, m_loc, nnz_loc, rowptr_loc, colind_glob, val, blk_start_loc, nblk_loc, coupled_tracer_cnt);
   if (rc) return rc;
   // diagonal block: what the create path validates and what the hierarchy is built from without overlap
   std::vector<int32_t> drow ((size_t) m_loc + 1, 0), dcol;
   std::vector<double> dval;
   dcol.reserve ((size_t) nnz_loc);
   dval.reserve ((size_t) nnz_loc);
   for (int64_t r = 0; r < m_loc; r++) {
      for (int e = rowptr_loc[r]; e < rowptr_loc[r + 1]; e++)
         if (D.colind_ext[e] < m_loc) { dcol.push_back (D.colind_ext[e]); dval.push_back (val[e]); }
      drow[r + 1] = (int32_t) dcol.size ();
   }
   SpmvMatrixHost M = { nnz_loc, m_loc + D.n_halo, rowptr_loc, D.colind_ext.data (), val };
   PrecondMatrixHost PM = { m_loc + D.n_sel, (int64_t) D.e_blk.size () - 1, D.e_rowptr.data (), D.e_colind.data (), D.e_val.data (), D.e_blk.data (), D.e_ci.data (), D.e_cj.data (), D.e_ct.data () };
   nkp_solver *s = nullptr;
   rc = create_impl (&s, &o, m_loc, (int64_t) dcol.size (), drow.data (), dcol.data (), dval.data (), blk_start_loc, nblk_loc, coupled_tracer_cnt, &M, D.ras ? &PM : nullptr);
   // every rank must reach the collectives below even if its own setup failed: agree on success first
   {
      int64_t flag = rc ? 1 : 0;
      std::vector<int64_t> all (P + 1, 0);
      if (comm->allgather_i64_host (comm->ctx, flag, all.data ())) { if (s) solver_free (s); return fail (NKP_ECOMM, "nkp_create_dist: allgather failed"); }
      for (int p = 0; p < P; p++)
         if (all[p]) {
            if (s) solver_free (s);
            return rc ? rc : fail (NKP_ECOMM, "nkp_create_dist: setup failed on rank %d", p);
         }
   }
   s->dist.ops = *comm;
   s->dist.n_global = n_global;
   s->dist.fst = fst_row;
   s->dist.n_halo = D.n_halo;
   s->dist.nsend = D.nsend;
   s->dist.send_counts.assign (D.give.begin (), D.give.end ());
   s->dist.recv_counts.assign (D.need.begin (), D.need.end ());
   bool ok = dev_alloc (s, &s->dist.send_idx, (size_t) D.nsend) == NKP_OK && dev_alloc (s, &s->dist.sendbuf, (size_t) D.nsend) == NKP_OK &&
             dev_alloc (s, &s->dist.xe, (size_t) (m_loc + D.n_halo)) == NKP_OK;
   if (ok && D.nsend) ok = hipMemcpy (s->dist.send_idx, D.send_rows.data (), (size_t) D.nsend * sizeof (int), hipMemcpyHostToDevice) == hipSuccess;
   if (ok && D.ras) {
      s->dist.n_sel = D.n_sel;
      s->dist.n_ext = m_loc + D.n_sel;
      s->dist.ras_rings = D.rings;
      s->dist.ras_sep = D.rings >= 2;
      ok = dev_alloc (s, &s->dist.rext, (size_t) (m_loc + D.n_sel)) == NKP_OK && dev_alloc (s, &s->dist.zext, (size_t) (m_loc + D.n_sel)) == NKP_OK;
      if (!s->dist.ras_sep) {
         ok = ok && dev_alloc (s, &s->dist.sel_idx, (size_t) D.n_sel) == NKP_OK;
         if (ok && D.n_sel) ok = hipMemcpy (s->dist.sel_idx, D.sel_hpos.data (), (size_t) D.n_sel * sizeof (int), hipMemcpyHostToDevice) == hipSuccess;
      } else {
         s->dist.ras_nsend = (int64_t) D.ras_send_rows.size ();
         s->dist.ras_send_counts.assign (D.ras_give.begin (), D.ras_give.end ());
         s->dist.ras_recv_counts.assign (D.ras_need.begin (), D.ras_need.end ());
         ok = ok && dev_alloc (s, &s->dist.ras_send_idx, (size_t) s->dist.ras_nsend) == NKP_OK && dev_alloc (s, &s->dist.ras_sendbuf, (size_t) s->dist.ras_nsend) == NKP_OK;
         if (ok && s->dist.ras_nsend)
            ok = hipMemcpy (s->dist.ras_send_idx, D.ras_send_rows.data (), (size_t) s->dist.ras_nsend * sizeof (int), hipMemcpyHostToDevice) == hipSuccess;
      }
      s->dist.ras = ok;
   }
   {
      // once more all ranks together: a rank without halo buffers must not leave its peers to a first SpMV that never completes
      std::vector<int64_t> all (P + 1, 0);
      const bool comm_ok = comm->allgather_i64_host (comm->ctx, ok ? 0 : 1, all.data ()) == 0;
      int bad_rank = -1;
      for (int p = 0; p < P && comm_ok; p++) if (all[p] && bad_rank < 0) bad_rank = p;
      if (!ok || !comm_ok || bad_rank >= 0) {
         solver_free (s);
         if (!ok) return fail (NKP_ENOMEM, "nkp_create_dist: halo buffers could not be allocated");
         return fail (NKP_ECOMM, comm_ok ? "nkp_create_dist: halo buffers could not be allocated on rank %d" : "nkp_create_dist: allgather failed (%d)", bad_rank);
      }
   }
   {
      const bool want = s->tune.dist_overlap != 0;
      const int interior_blocks = s->dist.seg_rb[2] - s->dist.seg_rb[1];
      if (want && interior_blocks > 0 && hipStreamCreateWithFlags (&s->dist.comm_stream, hipStreamNonBlocking) == hipSuccess &&
          hipEventCreateWithFlags (&s->dist.ev_packed, hipEventDisableTiming) == hipSuccess &&
          hipEventCreateWithFlags (&s->dist.ev_halo, hipEventDisableTiming) == hipSuccess)
         s->dist.overlap = true;
   }
   s->dist.on = true;
   // nkp_transpose_dist builds A^T's row block from these and passes the caller's own block data to nkp_create_dist again
   s->dist.starts = starts;
   s->dist.h_halo_rows.assign (D.halo_rows.begin (), D.halo_rows.begin () + D.n_halo);
   s->dist.h_send_rows.assign (D.send_rows.begin (), D.send_rows.begin () + D.nsend);
   s->dist.own_has_blk = blk_start_loc != nullptr;
   if (blk_start_loc) s->dist.own_blk.assign (blk_start_loc, blk_start_loc + nblk_loc + 1);
   if (o.col_i) s->dist.own_ci.assign (o.col_i, o.col_i + nblk_loc);
   if (o.col_j) s->dist.own_cj.assign (o.col_j, o.col_j + nblk_loc);
   if (o.col_t) s->dist.own_ct.assign (o.col_t, o.col_t + nblk_loc);
   s->dist.own_tracer_cnt = coupled_tracer_cnt;
   if (s->opt.precond == NKP_PRECOND_MULTILEVEL) {
      // nkp_refactor_dist: the hierarchy's source matrix and where its values come from (host memory only until the first call)
      DistRefactorPlan *Q = new DistRefactorPlan;
      if (D.ras) {
         Q->n_src = m_loc + D.n_sel;
         Q->src_rowptr.swap (D.e_rowptr);
         Q->src_colind.swap (D.e_colind);
         Q->origin.swap (D.e_org);
         Q->ship.swap (D.ship_e);
         Q->ship_counts = D.ent_give;
         Q->recv_counts = D.ent_need;
         for (int c : Q->recv_counts) Q->n_recv += c;
         Q->exchange = true;
         // what a rebuild passes to ml_setup again (nkp_create's own copies are made for the diagonal block only)
         s->h_blk.swap (D.e_blk);
         s->h_col_i.swap (D.e_ci);
         s->h_col_j.swap (D.e_cj);
         s->h_col_t.swap (D.e_ct);
         s->tracer_cnt = coupled_tracer_cnt;
      } else {
         Q->n_src = m_loc;
         Q->origin.reserve (dcol.size ());
         for (int64_t e = 0; e < nnz_loc; e++)
            if (D.colind_ext[(size_t) e] < m_loc) Q->origin.push_back ((int32_t) e);
         Q->src_rowptr.swap (drow);
         Q->src_colind.swap (dcol);
      }
      Q->nnz_src = (int64_t) Q->src_colind.size ();
      s->dplan = Q;
   }
   msg (s, 1, "nkp_create_dist: %d of %d SpMV row blocks are interior (multiplied while the halo travels: %s)\n", s->dist.seg_rb[2] - s->dist.seg_rb[1],
        s->dist.seg_rb[3], s->dist.overlap ? "yes" : "no");
   msg (s, 1, "nkp_create_dist: rows [%lld, %lld) of %lld, %lld halo rows in, %lld rows out; overlap (restricted additive Schwarz): %s, %lld rows of other ranks in this rank's hierarchy (overlap depth %d)\n",
        (long long) fst_row, (long long) (fst_row + m_loc), (long long) n_global, (long long) D.n_halo, (long long) D.nsend, s->dist.ras ? "on" : "off", (long long) s->dist.n_sel,
        s->dist.ras ? s->dist.ras_rings : 0);
   *out = s;
   return NKP_OK;
}

extern "C" int nkp_set_device (int device)
{
   HIPCHK (hipSetDevice (device));
   return NKP_OK;
}

extern "C" int nkp_gather_root (nkp_solver *s, const double *x_loc, double *x_global)
{
   if (!s || !x_loc) return fail (NKP_EINVAL, "nkp_gather_root: NULL argument");
   HIPCHK (hipSetDevice (s->device));
   if (!s->dist.on) {
      if (!x_global) return fail (NKP_EINVAL, "nkp_gather_root: NULL argument");
      memcpy (x_global, x_loc, (size_t) s->n * sizeof (double));
      return NKP_OK;
   }
   const int P = s->dist.ops.nranks, rank = s->dist.ops.rank;
   std::vector<int64_t> sizes (P + 1, 0);
   if (s->dist.ops.allgather_i64_host (s->dist.ops.ctx, s->n, sizes.data ())) return fail (NKP_ECOMM, "nkp_gather_root: allgather failed");
   std::vector<int> scnt (P, 0), rcnt (P, 0);
   scnt[0] = (int) s->n;                                  // everything goes to rank 0
   int64_t total = 0;
   if (rank == 0)
      for (int p = 0; p < P; p++) { rcnt[p] = (int) sizes[p]; total += sizes[p]; }
   double *dsend = s->t1, *drecv = nullptr;
   HIPCHK (hipMemcpyAsync (dsend, x_loc, (size_t) s->n * sizeof (double), hipMemcpyHostToDevice, s->stream));
   if (rank == 0) {
      if (!x_global) return fail (NKP_EINVAL, "nkp_gather_root: rank 0 needs x_global");
      HIPCHK (hipMalloc ((void **) &drecv, (size_t) (total ? total : 1) * sizeof (double)));
   }
   const int crc = s->dist.ops.alltoallv (s->dist.ops.ctx, dsend, scnt.data (), drecv ? (void *) drecv : (void *) s->t2, rcnt.data (), (void *) s->stream);
   if (!crc && rank == 0) {
      hipError_t e = hipMemcpyAsync (x_global, drecv, (size_t) total * sizeof (double), hipMemcpyDeviceToHost, s->stream);
      if (e != hipSuccess) { (void) hipFree (drecv); return fail (NKP_EDEVICE, "nkp_gather_root: copy back failed"); }
   }
   HIPCHK (hipStreamSynchronize (s->stream));
   if (drecv) (void) hipFree (drecv);
   return crc ? fail (NKP_ECOMM, "nkp_gather_root: exchange failed") : NKP_OK;
}
