// nkp_transpose: a solver for A^T made from the matrix a solver already holds on the device -- the stand-in of SuperLU's
// options.Trans (reference src/solve_ABglobal.c:327-335 sets the options pdgssvx_ABglobal reads), for adjoint tracer problems.
//
// Two parts.
//   The device transpose: count the entries of every column (integer atomics), scan, scatter every entry to its column through
//   per-column cursors, then give every entry of a row of A^T its rank among that row's source rows.  The atomics decide only
//   where an entry waits between the scatter and the ranking; the ranks depend on the keys alone (source row, then stored
//   position), so the output is the same on every run.  The ranking reads a row of A^T once per entry of that row: no cap on
//   its length, no LDS slot, quadratic in it (a 700-entry row costs 490 000 four-byte reads that sit in L2).
//   The solver: the transposed CSR goes to the host once and through nkp_create with the options and tuning the source solver
//   resolved, so the result is bit for bit what nkp_create builds from the host transpose.  The map src (valT[p] = val[src[p]])
//   stays on the device: a refactor of the source gathers the new values through it and refactors the transposed solver too.
#include "solver_impl.h"
#include "transpose.h"

#include <stdio.h>
#include <time.h>

#define TR_T 256
static inline dim3 tr_grid (int64_t n) { return dim3 ((unsigned) ((n + TR_T - 1) / TR_T)); }

// the row r with ptr[r] <= e < ptr[r + 1] (ptr ascending, ptr[0] = 0, e < ptr[n]; empty rows are skipped)
__device__ static inline int tr_row_of (const int *__restrict__ ptr, int n, int e)
{
   int lo = 0, hi = n;
   while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (ptr[mid + 1] <= e) lo = mid + 1;
      else hi = mid;
   }
   return lo;
}

__global__ __launch_bounds__ (TR_T)
void tr_count_kernel (const int *__restrict__ colind, int64_t nnz, int *__restrict__ cnt)
{
   const int64_t e = (int64_t) blockIdx.x * TR_T + threadIdx.x;
   if (e < nnz) atomicAdd (&cnt[colind[e]], 1);
}

// entry e = (r, c) waits at some position of row c of A^T with its source row and its stored position
__global__ __launch_bounds__ (TR_T)
void tr_fill_kernel (const int *__restrict__ rowptr, const int *__restrict__ colind, int n, int64_t nnz, const int *__restrict__ rowptrT,
                     int *__restrict__ cursor, int *__restrict__ row_tmp, int *__restrict__ src_tmp)
{
   const int64_t e = (int64_t) blockIdx.x * TR_T + threadIdx.x;
   if (e >= nnz) return;
   const int c = colind[e];
   const int p = rowptrT[c] + atomicAdd (&cursor[c], 1);
   row_tmp[p] = tr_row_of (rowptr, n, (int) e);
   src_tmp[p] = (int) e;
}

// rank of every waiting entry inside its row of A^T by (source row, stored position); the values come along
__global__ __launch_bounds__ (TR_T)
void tr_rank_kernel (const int *__restrict__ rowptrT, int n, int64_t nnz, const int *__restrict__ row_tmp, const int *__restrict__ src_tmp,
                     const double *__restrict__ val, int *__restrict__ colindT, int *__restrict__ src, double *__restrict__ valT)
{
   const int64_t p = (int64_t) blockIdx.x * TR_T + threadIdx.x;
   if (p >= nnz) return;
   const int c = tr_row_of (rowptrT, n, (int) p);
   const int b = rowptrT[c], e = rowptrT[c + 1];
   const int key = row_tmp[p], pos = src_tmp[p];
   int rank = 0;
   for (int q = b; q < e; q++) {
      const int k = row_tmp[q];
      rank += (k < key || (k == key && src_tmp[q] < pos)) ? 1 : 0;
   }
   colindT[b + rank] = key;
   src[b + rank] = pos;
   valT[b + rank] = val[pos];
}

__global__ __launch_bounds__ (TR_T)
void tr_gather_kernel (const double *__restrict__ val, const int *__restrict__ src, int64_t nnz, double *__restrict__ out)
{
   const int64_t p = (int64_t) blockIdx.x * TR_T + threadIdx.x;
   if (p < nnz) out[p] = val[src[p]];
}

static double seconds_since (const struct timespec &t0)
{
   struct timespec t;
   clock_gettime (CLOCK_MONOTONIC, &t);
   return (double) (t.tv_sec - t0.tv_sec) + 1e-9 * (double) (t.tv_nsec - t0.tv_nsec);
}

// A^T of the device CSR A of A.n rows and ncols columns (nkp_transpose_dist: the rectangle [own | halo]): rowptrT[ncols + 1],
// colindT / valT / src[nnz], every row sorted by column.  0, or a hipError_t
#define TRCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return (int) e_; } while (0)
int transpose_device (const CsrDev &A, int64_t ncols, mls::DBuf<int> &rowptrT, mls::DBuf<int> &colindT, mls::DBuf<double> &valT, mls::DBuf<int> &src, hipStream_t st)
{
   const int64_t n = ncols, nnz = A.nnz;
   mls::DBuf<int> cursor, row_tmp, src_tmp;
   TRCHK (rowptrT.alloc ((size_t) n + 1));
   TRCHK (colindT.alloc ((size_t) nnz));
   TRCHK (valT.alloc ((size_t) nnz));
   TRCHK (src.alloc ((size_t) nnz));
   TRCHK (cursor.alloc ((size_t) n));
   TRCHK (row_tmp.alloc ((size_t) nnz));
   TRCHK (src_tmp.alloc ((size_t) nnz));
   TRCHK (hipMemsetAsync (rowptrT.p, 0, ((size_t) n + 1) * sizeof (int), st));
   TRCHK (hipMemsetAsync (cursor.p, 0, (size_t) (n ? n : 1) * sizeof (int), st));
   if (nnz > 0) hipLaunchKernelGGL (tr_count_kernel, tr_grid (nnz), dim3 (TR_T), 0, st, A.colind, nnz, rowptrT.p);
   int64_t total = 0;
   const int rc = mls::scan_exclusive (rowptrT.p, rowptrT.p, n, st, &total);
   if (rc) return rc;
   if (total != nnz) return 1000;
   if (nnz > 0) {
      hipLaunchKernelGGL (tr_fill_kernel, tr_grid (nnz), dim3 (TR_T), 0, st, A.rowptr, A.colind, (int) A.n, nnz, rowptrT.p, cursor.p, row_tmp.p, src_tmp.p);
      hipLaunchKernelGGL (tr_rank_kernel, tr_grid (nnz), dim3 (TR_T), 0, st, rowptrT.p, (int) n, nnz, row_tmp.p, src_tmp.p, A.val, colindT.p, src.p, valT.p);
   }
   TRCHK (hipStreamSynchronize (st));      // the work buffers are freed on return
   TRCHK (hipGetLastError ());
   return 0;
}

// ---------------------------------------------------------------- ownership
static void trans_free_maps (nkp_solver *s)
{
   if (s->trans_src) (void) hipFree (s->trans_src);
   if (s->trans_val) (void) hipFree (s->trans_val);
   if (s->trans_ship) (void) hipFree (s->trans_ship);
   if (s->trans_send) (void) hipFree (s->trans_send);
   if (s->trans_recv) (void) hipFree (s->trans_recv);
   s->trans_src = s->trans_ship = nullptr;
   s->trans_val = s->trans_send = s->trans_recv = nullptr;
   s->trans_map_bytes = 0;
}

void trans_release (nkp_solver *s)
{
   nkp_solver *t = s->trans;
   s->trans = nullptr;
   if (t) {
      t->trans_of = nullptr;
      solver_free (t);
   }
   trans_free_maps (s);
}

void trans_detach (nkp_solver *t)
{
   nkp_solver *s = t->trans_of;
   t->trans_of = nullptr;
   if (!s) return;
   s->trans = nullptr;
   trans_free_maps (s);
}

void trans_set_stream (nkp_solver *s)
{
   nkp_solver *t = s->trans;
   if (!t) return;
   t->stream = s->stream;
   for (nkp_solver *c : t->batch_members) c->stream = s->stream;
}

int64_t trans_device_bytes (const nkp_solver *s)
{
   if (!s->trans) return 0;
   size_t sum = s->trans->device_bytes + s->trans_map_bytes;
   for (const nkp_solver *c : s->trans->batch_members) sum += c->device_bytes;
   return (int64_t) sum;
}

void launch_tr_gather (const double *val, const int *src, int64_t nnz, double *out, hipStream_t st)
{
   if (nnz > 0) hipLaunchKernelGGL (tr_gather_kernel, tr_grid (nnz), dim3 (TR_T), 0, st, val, src, nnz, out);
}

// ---------------------------------------------------------------- the refactor of the source reaches the transposed solver
int trans_gather_values (nkp_solver *s, const double **d_valT)
{
   const int64_t nnz = s->A.nnz;
   if (!s->trans_val) {
      void *q = nullptr;
      const size_t bytes = (size_t) (nnz ? nnz : 1) * sizeof (double);
      if (hipMalloc (&q, bytes) != hipSuccess) {
         (void) hipGetLastError ();
         return fail (NKP_ENOMEM, "no device memory for the %zu bytes of transposed values", bytes);
      }
      s->trans_val = (double *) q;
      s->trans_map_bytes += bytes;
   }
   launch_tr_gather (s->A.val, s->trans_src, nnz, s->trans_val, s->stream);
   HIPCHK (hipGetLastError ());
   *d_valT = s->trans_val;
   return NKP_OK;
}

// ---------------------------------------------------------------- C ABI
extern "C" int nkp_transpose (nkp_solver *s, nkp_solver **out)
{
   if (out) *out = nullptr;
   if (!s || !out) return fail (NKP_EINVAL, "nkp_transpose: NULL argument");
   if (s->borrowed) return fail (NKP_EINVAL, "nkp_transpose: a clone shares its matrix; transpose the solver it was cloned from");
   if (s->trans_of) return fail (NKP_EINVAL, "nkp_transpose: this solver is itself a transposed handle; the solver it was transposed from holds A");
   if (s->dist.on) return fail (NKP_EINVAL, "nkp_transpose: not available for the row-distributed flavour (the transpose of a row block needs an exchange between the ranks: every rank calls nkp_transpose_dist instead)");
   if (s->trans) { *out = s->trans; return NKP_OK; }
   if (s->shared->broken) return fail (NKP_ESINGULAR, "nkp_transpose: %s", s->shared->why.c_str ());
   HIPCHK (hipSetDevice (s->device));
   HIPCHK (hipStreamSynchronize (s->stream));
   struct timespec t0;
   clock_gettime (CLOCK_MONOTONIC, &t0);
   const int64_t n = s->n, nnz = s->A.nnz;
   std::vector<int32_t> rp ((size_t) n + 1), ci ((size_t) nnz);
   std::vector<double> v ((size_t) nnz);
   mls::DBuf<int> src;
   double kernel_seconds = 0.0;
   {
      mls::DBuf<int> rowptrT, colindT;
      mls::DBuf<double> valT;
      const int trc = transpose_device (s->A, s->n, rowptrT, colindT, valT, src, s->stream);
      if (trc) {
         (void) hipStreamSynchronize (s->stream);
         (void) hipGetLastError ();      // an out-of-memory error is sticky until read
         if (trc == (int) hipErrorOutOfMemory) return fail (NKP_ENOMEM, "nkp_transpose: no device memory for the transposed matrix (%lld entries); the solver is unchanged", (long long) nnz);
         return fail (NKP_EDEVICE, "nkp_transpose: the device transpose failed (%s)", trc >= 1000 ? "inconsistent column counts" : hipGetErrorString ((hipError_t) trc));
      }
      kernel_seconds = seconds_since (t0);
      HIPCHK (hipMemcpy (rp.data (), rowptrT.p, rp.size () * sizeof (int32_t), hipMemcpyDeviceToHost));
      if (nnz) {
         HIPCHK (hipMemcpy (ci.data (), colindT.p, ci.size () * sizeof (int32_t), hipMemcpyDeviceToHost));
         HIPCHK (hipMemcpy (v.data (), valT.p, v.size () * sizeof (double), hipMemcpyDeviceToHost));
      }
   }
   // the options and tuning the source resolved at its creation; the block offsets and grid positions it kept
   nkp_options opt = s->opt;
   opt.device = s->device;
   nkp_tuning tune = s->tune;
   tune.spmv_diag = 0;                 // the transposed handle keeps its products on CSR
   opt.tuning = &tune;
   opt.col_i = s->h_col_i.empty () ? nullptr : s->h_col_i.data ();
   opt.col_j = s->h_col_j.empty () ? nullptr : s->h_col_j.data ();
   opt.col_t = s->h_col_t.empty () ? nullptr : s->h_col_t.data ();
   const bool blocks = opt.precond != NKP_PRECOND_NONE;
   nkp_solver *t = nullptr;
   const int rc = nkp_create (&t, &opt, n, nnz, rp.data (), ci.data (), v.data (), blocks ? s->h_blk.data () : nullptr, blocks ? (int64_t) s->h_blk.size () - 1 : 0, s->tracer_cnt);
   if (rc) {
      (void) hipGetLastError ();
      const std::string why = last_error_message ();
      return fail (rc, "nkp_transpose: %s; the solver is unchanged", why.c_str ());
   }
   // same stream as the source
   if (t->own_stream && t->stream) { (void) hipStreamSynchronize (t->stream); (void) hipStreamDestroy (t->stream); }
   t->stream = s->stream;
   t->own_stream = false;
   t->trans_of = s;
   s->trans = t;
   s->trans_src = src.release ();
   s->trans_map_bytes = (size_t) (nnz ? nnz : 1) * sizeof (int);
   s->trans_seconds = seconds_since (t0);
   s->trans_kernel_seconds = kernel_seconds;
   msg (s, 1, "nkp_transpose: n = %lld, nnz = %lld, %.1f MB on device %d; %.3f s device transpose, %.3f s in all\n", (long long) n, (long long) nnz,
        (double) trans_device_bytes (s) / 1.0e6, s->device, kernel_seconds, s->trans_seconds);
   *out = t;
   return NKP_OK;
}
