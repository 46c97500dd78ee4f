// The envelope of the K-vector calls on the solver's pattern: nkp_value_gradient*, nkp_values_product*,
// nkp_values_product_trans*, nkp_solve_tangent_device, nkp_values_product_trans_dist*, nkp_residual_batch*.  Each takes up to
// NKP_BATCH_MAX column vectors with a leading dimension, in a host or a device flavour, on a single-GPU or a row-distributed solver;
// what is the same in all of them is written here once.  A body calls the phases of OperandCall in order and keeps what is its own:
// its argument checks, its Want list, its staging layout, its operand fetch or own exchange, its kernel and what it copies back.
#pragma once
#include "solver_impl.h"

#include <time.h>

// Everything here is hidden (NKP_PRIVATE): an inline function the compiler does not inline must not join the library's symbols
struct NKP_PRIVATE Stopwatch {
   double t0;
   Stopwatch () : t0 (now ()) {}
   void start () { t0 = now (); }
   double seconds () const { return now () - t0; }
   static double now ()
   {
      struct timespec t;
      clock_gettime (CLOCK_MONOTONIC, &t);
      return (double) t.tv_sec + 1e-9 * (double) t.tv_nsec;
   }
};

// ---- column staging: nrhs columns of n doubles between a host array of leading dimension ld and a device buffer of leading
// dimension n, queued on st; the first error ends it
NKP_PRIVATE inline hipError_t stage_columns (double *dst, int64_t ldd, const double *src, int64_t lds, int nrhs, int64_t n, hipMemcpyKind kind, hipStream_t st)
{
   hipError_t e = hipSuccess;
   for (int c = 0; c < nrhs && e == hipSuccess && n; c++)
      e = hipMemcpyAsync (dst + (size_t) c * (size_t) ldd, src + (size_t) c * (size_t) lds, (size_t) n * sizeof (double), kind, st);
   return e;
}
NKP_PRIVATE inline hipError_t upload_columns (double *dst, const double *src, int64_t ld, int nrhs, int64_t n, hipStream_t st) { return stage_columns (dst, n, src, ld, nrhs, n, hipMemcpyHostToDevice, st); }
NKP_PRIVATE inline hipError_t download_columns (double *dst, int64_t ld, const double *src, int nrhs, int64_t n, hipStream_t st) { return stage_columns (dst, ld, src, n, nrhs, n, hipMemcpyDeviceToHost, st); }

// ---- argument refusals (no HIP call); hint: what the message says after the range, rows: "n" or "m_loc"
NKP_PRIVATE inline int refuse_nrhs (const char *who, int nrhs, const char *hint)
{
   return nrhs >= 1 && nrhs <= NKP_BATCH_MAX ? NKP_OK : fail (NKP_EINVAL, "%s: nrhs = %d, must be 1 .. %d%s", who, nrhs, NKP_BATCH_MAX, hint);
}
NKP_PRIVATE inline int refuse_ld (const char *who, const char *name, int64_t ld, const char *rows, int64_t n)
{
   return ld >= n ? NKP_OK : fail (NKP_EINVAL, "%s: %s = %lld < %s = %lld", who, name, (long long) ld, rows, (long long) n);
}

// ---- the call.  halo: the call reads x through the solver's own halo exchange (fetch_x_operand), whose K-wide buffers it shares
// with the batched solve.  On a row-distributed solver every rank reaches both agreements whatever happened locally, unless the
// first one fails: then every rank returns after it, and nothing else is exchanged.
struct NKP_PRIVATE OperandCall {
   nkp_solver *s;
   const char *who;
   int nrhs, K = 1;
   bool host, dist, halo;
   int rc = NKP_OK;
   Stopwatch watch;      // from the body's entry; a body whose time runs from its run phase starts it again there

   OperandCall (nkp_solver *s_, const char *who_, int nrhs_, bool host_, bool halo_ = true)
      : s (s_), who (who_), nrhs (nrhs_), host (host_), dist (s_->dist.on), halo (halo_) {}

   // verdict: what this rank's argument checks said.  true: return rc now -- a single-GPU solver refuses before any HIP call; a
   // row-distributed one carries the code to the first agreement, and every step from here on is skipped once rc is set
   bool begin (int verdict)
   {
      rc = verdict;
      if (rc && !dist) return true;
      K = width_of (nrhs);
      if (!rc && hipSetDevice (s->device) != hipSuccess) rc = fail (NKP_EDEVICE, "%s: hipSetDevice (%d) failed", who, s->device);
      return false;
   }

   // the call's work space, all of it or none; fetch: the K-wide buffers of the halo exchange too, when they are narrower than K
   void reserve (std::initializer_list<Want> set, bool fetch)
   {
      if (!rc) rc = ::reserve (s, set, who);
      if (!rc && fetch && dist && K >= 2 && s->dist.bK < K) rc = batch_prepare_exchange (s, K);
   }

   void uploaded (hipError_t e, const char *what)
   {
      if (e != hipSuccess) rc = fail (NKP_EDEVICE, "%s: upload of the host %s failed: %s", who, what, hipGetErrorString (e));
   }

   // the first agreement, or (agreed) the verdict of a caller's own variant of it.  Non-zero: return it.  After a failed agreement
   // nothing this call queued still reads the caller's arrays, and a rank whose K-wide exchange buffers are gone is not a rank
   // "known to have buffers": the next batched solve agrees anew
   int agree (const char *where) { return agreed (dist ? dist_agree (s, rc, who, where) : rc); }
   int agreed (int verdict)
   {
      rc = verdict;
      if (rc && dist) {
         if (halo) s->dist.agreed_K = 0;
         (void) hipStreamSynchronize (s->stream);
      }
      return rc;
   }

   // e: what queueing the copies of the results said.  The stream is synchronised on every path; then the second agreement (where),
   // and only a call that succeeded on every rank sets its time and counts
   int finish (hipError_t e, const char *kernel, const char *where, double &seconds, int64_t &calls)
   {
      if (!rc) {
         if (e == hipSuccess) e = hipStreamSynchronize (s->stream);
         if (e == hipSuccess) e = hipGetLastError ();
         if (e != hipSuccess) rc = fail (NKP_EDEVICE, "%s: the %s kernel or its copies failed: %s", who, kernel, hipGetErrorString (e));
      }
      if (rc) (void) hipStreamSynchronize (s->stream);
      if (dist) rc = dist_agree (s, rc, who, where);
      if (rc) return rc;
      seconds = watch.seconds ();
      calls++;
      return NKP_OK;
   }
};

// ---- defined in valprod_api.hip: the operands of a product with caller-supplied values (nkp_values_product*, also _trans_dist).
// product_stage reserves the call's work space -- xbuf and the staging buffer of the host flavour, val | x | y at ld n -- and, host
// flavour, queues the uploads and points o, which came with the caller's device pointers, at the staged copies
struct ProductOperands { const double *val, *x; double *y; int64_t ldx, ldy; };
NKP_PRIVATE void product_stage (OperandCall &c, Want xbuf, const double *h_val, const double *h_x, const double *h_y, int accumulate, ProductOperands &o, bool fetch);

// ---- work space made by reserve, given back: every buffer freed takes its bytes off device_bytes, whoever calls
NKP_PRIVATE inline void release_buffers (nkp_solver *s, std::initializer_list<Want> set)
{
   for (const Want &w : set) {
      if (*w.p) {
         (void) hipFree (*w.p);
         s->device_bytes -= *w.cap * sizeof (double);
      }
      *w.p = nullptr;
      *w.cap = 0;
   }
}

// ---- nkp_time_kernel: the kernels of these calls are timed on single-GPU solvers at interleave width K
NKP_PRIVATE inline int time_width_ok (const nkp_solver *s, int K, int which, const char *what)
{
   if (s->dist.on) return fail (NKP_EINVAL, "nkp_time_kernel: the %s kernel (which = %d) is timed on single-GPU solvers only", what, which);
   if (K != 1 && K != 2 && K != 4 && K != 8) return fail (NKP_EINVAL, "nkp_time_kernel: which = %d takes arg = K in {1, 2, 4, 8}", which);
   return NKP_OK;
}
