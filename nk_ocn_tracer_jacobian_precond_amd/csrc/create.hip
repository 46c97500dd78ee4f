// Creation and cloning of a solver (nkp_create, nkp_create64, nkp_clone): what the kernels will trust is validated on the host,
// the matrix and its row blocks go to the device, then the work vectors and the preconditioner (hierarchy or column factors).
// create_impl also builds the rank-local solver of nkp_create_dist (create_dist.hip).
#include "solver_impl.h"

#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <thread>
#include <vector>

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

// ---------------------------------------------------------------- the steps of create_impl, in the order it takes them
// the caller's options (or the defaults) with the restart length clamped, and the tuning resolved once
static int check_arguments (const nkp_options *opt_in, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colind, const double *val,
                            nkp_options &opt, nkp_tuning &tune)
{
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
   { const int trc = resolve_tuning (&opt, &tune); if (trc) return trc; }
   opt.tuning = nullptr;            // the caller's struct is not kept
   return NKP_OK;
}

// host-side validation of what the kernels will trust (row chunks in parallel; the lowest offending row is reported)
static int check_rows (const nkp_options &opt, int64_t n, const int32_t *rowptr, const int32_t *colind, const double *val)
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
            // A is the sum of its stored entries: so is the diagonal, in stored order (colblock_measure_kernel and rf_diag_kernel
            // sum it the same way).  The order test covers every entry, the diagonal included.
            double diag = 0.0;
            for (int e = rowptr[r]; e < rowptr[r + 1] && !b.kind; e++) {
               if (colind[e] < 0 || colind[e] >= n) { b.kind = 2; b.col = colind[e]; }
               else if (opt.precond == NKP_PRECOND_MULTILEVEL && e > rowptr[r] && colind[e] <= colind[e - 1]) b.kind = 4;
               else if (colind[e] == r) diag += val[e];
            }
            if (!b.kind && opt.precond != NKP_PRECOND_NONE && !(diag != 0.0)) b.kind = 3;
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
   return NKP_OK;
}

// the water columns of a preconditioner: the caller's, or blocks of one wave (blk_default, which then owns them)
static int check_blocks (const nkp_options &opt, int64_t n, const int32_t *&blk_start, int64_t &nblk, std::vector<int> &blk_default)
{
   if (opt.precond == NKP_PRECOND_NONE) return NKP_OK;
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
   return NKP_OK;
}

// the solver object on the device the options name
static int new_solver_on_device (const nkp_options &opt, const nkp_tuning &tune, nkp_solver **out)
{
   int ndev = 0;
   if (hipGetDeviceCount (&ndev) != hipSuccess || ndev == 0) return fail (NKP_EDEVICE, "nkp_create: no HIP device available (this library has no CPU fallback)");
   nkp_solver *s = new nkp_solver;
   s->opt = opt;
   s->created = controls_of (s);
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
   *out = s;
   return NKP_OK;
}

// the steps below work on the solver under construction: a failed one frees it and returns its code (so does clone_impl)
#define TRY(x) do { rc = (x); if (rc != NKP_OK) { solver_free (s); return rc; } } while (0)
#define TRYHIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { rc = fail (NKP_EDEVICE, "%s failed: %s", #call, hipGetErrorString (e_)); solver_free (s); return rc; } } while (0)

// stream, sizes, and the options that the tuning may override
static int configure (nkp_solver *s, int64_t n)
{
   const nkp_options &opt = s->opt;
   const nkp_tuning &tune = s->tune;
   int rc = NKP_OK;
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
   return rc;
}

// Row blocks of a row-distributed rank, per segment [head boundary | interior | tail boundary], where the interior is
// the longest run of rows without an off-rank (halo) column -- with latitude bands it is everything but the two
// or three latitude rows at either end of the band.  *rb is malloc'ed.
static void segmented_rowblocks (nkp_solver *s, const SpmvMatrixHost &M, int **rb, int *nrb)
{
   const int64_t n = s->n;
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
   *nrb = (int) all.size () - 1;
   *rb = (int *) malloc (all.size () * sizeof (int));
   memcpy (*rb, all.data (), all.size () * sizeof (int));
}

// the SpMV matrix, its row blocks and column codes on the device
static int upload_matrix (nkp_solver *s, const SpmvMatrixHost &M, bool distributed)
{
   const int64_t n = s->n;
   int rc = NKP_OK;
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
   int *rb = nullptr, nrb = 0;
   if (distributed) segmented_rowblocks (s, M, &rb, &nrb);
   else build_rowblocks_host (n, M.rowptr, &rb, &nrb);
   s->A.nrowblk = nrb;
   rc = dev_alloc (s, &s->A.rowblk, (size_t) nrb + 1);
   if (rc == NKP_OK && hipMemcpy (s->A.rowblk, rb, ((size_t) nrb + 1) * sizeof (int), hipMemcpyHostToDevice) != hipSuccess)
      rc = fail (NKP_EDEVICE, "copy of row blocks failed");
   if (rc == NKP_OK && attach_spmv_codes (s->A, M.rowptr, M.colind, rb, &s->device_bytes)) rc = fail (NKP_ENOMEM, "column codes could not be uploaded");
   free (rb);
   if (rc != NKP_OK) { solver_free (s); return rc; }
   return NKP_OK;
}

// R_i = 1 / max_j |a_ij| (the row half of dgsequ); rows without entries keep 1
static int upload_row_scales (nkp_solver *s, const SpmvMatrixHost &M)
{
   const int64_t n = s->n;
   int rc = NKP_OK;
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
   return rc;
}

// The multilevel hierarchy from pm, or from the solver's own n x n block (own_blocks: the water columns and grid positions are
// the caller's; A_is_source: the SpMV's device copy holds this very matrix).
static int build_hierarchy (nkp_solver *s, int64_t n, const int32_t *rowptr, const int32_t *colind, const double *val, const int32_t *blk_start, int64_t nblk,
                            bool own_blocks, int coupled_tracer_cnt, bool A_is_source, const PrecondMatrixHost *pm)
{
   const nkp_options &opt = s->opt;
   const nkp_tuning &tune = s->tune;
   int rc = NKP_OK;
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
                      : ml_setup (s->ml, n, rowptr, colind, val, blk_start, nblk, own_blocks ? opt.col_i : nullptr, own_blocks ? opt.col_j : nullptr, own_blocks ? opt.col_t : nullptr,
                                  coupled_tracer_cnt, opt.ml_levels, opt.ml_smooth, coarsest_rows, opt.verbose, opt.rank, s->stream, err, sizeof err, s->tune,
                                  // the SpMV's device copy is this very matrix unless the columns were renumbered (distributed flavour) or filtered
                                  (A_is_source && f_rowptr.empty ()) ? &s->A : nullptr);
   if (mrc != 0) {
      rc = fail (mrc, "nkp_create: %s", err);
      solver_free (s);
      return rc;
   }
   s->device_bytes += s->ml.device_bytes;
   return NKP_OK;
}

// column Jacobi: measure the water-column blocks, factor them, lay them out for the lanes kernels
static int factor_columns (nkp_solver *s, const int32_t *blk_start, int64_t nblk)
{
   const int64_t n = s->n;
   int rc = NKP_OK;
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
   return NKP_OK;
}

int create_impl (nkp_solver **out, const nkp_options *opt_in, int64_t n, int64_t nnz,
                 const int32_t *rowptr, const int32_t *colind, const double *val,
                 const int32_t *blk_start, int64_t nblk, int coupled_tracer_cnt, const SpmvMatrixHost *spmv_mat,
                 const PrecondMatrixHost *pm)
{
   if (!out) return fail (NKP_EINVAL, "nkp_create: out is NULL");
   *out = nullptr;
   nkp_options opt;
   nkp_tuning tune;
   std::vector<int> blk_default;
   int rc;
   if ((rc = check_arguments (opt_in, n, nnz, rowptr, colind, val, opt, tune))) return rc;
   if ((rc = check_rows (opt, n, rowptr, colind, val))) return rc;
   if ((rc = check_blocks (opt, n, blk_start, nblk, blk_default))) return rc;

   nkp_solver *s = nullptr;
   if ((rc = new_solver_on_device (opt, tune, &s))) return rc;
   struct timespec ts0_;
   clock_gettime (CLOCK_MONOTONIC, &ts0_);
   auto since0 = [&] () { struct timespec t; clock_gettime (CLOCK_MONOTONIC, &t); return (double) (t.tv_sec - ts0_.tv_sec) + 1e-9 * (double) (t.tv_nsec - ts0_.tv_nsec); };
   if ((rc = configure (s, n))) return rc;

   // matrix
   const SpmvMatrixHost own = { nnz, n, rowptr, colind, val };
   const SpmvMatrixHost &M = spmv_mat ? *spmv_mat : own;
   if ((rc = upload_matrix (s, M, spmv_mat != nullptr))) return rc;
   // the caller's own water columns only; a row-distributed rank keeps CSR (its halo columns live behind n)
   if (!spmv_mat && blk_default.empty ()) build_matrix_diagonals (s, blk_start, nblk);
   if (s->equil && (rc = upload_row_scales (s, M))) return rc;

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
   if (opt.precond == NKP_PRECOND_MULTILEVEL &&
       (rc = build_hierarchy (s, n, rowptr, colind, val, blk_start, nblk, blk_default.empty (), coupled_tracer_cnt, !spmv_mat, pm))) return rc;
   // water-column blocks
   if (opt.precond == NKP_PRECOND_COLUMN_JACOBI && (rc = factor_columns (s, blk_start, nblk))) return rc;
   TRYHIP (hipStreamSynchronize (s->stream));
   TRYHIP (hipGetLastError ());
   msg (s, 1, "nkp_create: n = %lld, nnz = %lld, %d SpMV row blocks, %.1f MB on device %d; %.2f s matrix upload + row blocks, %.2f s work vectors, %.2f s preconditioner\n",
        (long long) n, (long long) M.nnz, s->A.nrowblk, (double) s->device_bytes / 1.0e6, s->device, t_matrix, t_work - t_matrix, since0 () - t_work);
   s->create_seconds = since0 ();
   *out = s;
   return NKP_OK;
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

// (what a clone and a batch member are: solver_impl.h)
int clone_impl (nkp_solver *src, nkp_solver **out, bool member)
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
   s->dist.bxe = s->dist.gmsg = s->dist.ghpin = nullptr;
   s->dist.each_exchange ([] (RowExchange &X, bool) { X.drop_wide (); });
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
   s->vt = decltype (s->vt) ();      // the transposed index stays with the owner
   s->rb = decltype (s->rb) ();      // nkp_residual_batch's work space and counters are per handle too
   s->A.tune = &s->tune;
   s->B.tune = &s->tune;
   s->ml.tune = &s->tune;
   for (MlLevel &L : s->ml.lev) L.L.tune = L.B.tune = &s->tune;
   s->stream = nullptr;
   s->own_stream = false;
   s->device_bytes = 0;
   s->V = s->vcur = s->Z = s->w = s->r = s->x = s->b = s->t1 = s->t2 = s->p1 = s->p2 = s->eqtmp = s->partial = s->dscal = s->hpin = nullptr;
   s->dint = nullptr;
   for (MlLevel &L : s->ml.lev) L.one = MlVecs ();
   int rc = NKP_OK;
   TRYHIP (hipStreamCreateWithFlags (&s->stream, hipStreamNonBlocking));
   s->own_stream = true;
   TRY (alloc_work_vectors (s, member));
   for (MlLevel &L : s->ml.lev) {
      for (double **p : { &L.one.x, &L.one.x2, &L.one.b, &L.one.r }) {
         TRY (dev_alloc (s, p, (size_t) L.n));
         TRYHIP (hipMemset (*p, 0, (size_t) (L.n ? L.n : 1) * sizeof (double)));
      }
   }
   *out = s;
   return NKP_OK;
}

#undef TRY
#undef TRYHIP

extern "C" int nkp_clone (nkp_solver *src, nkp_solver **out) { return clone_impl (src, out, false); }
