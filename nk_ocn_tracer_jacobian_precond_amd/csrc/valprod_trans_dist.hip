// nkp_values_product_trans_dist / nkp_values_product_trans_dist_device (include/nkp.h): y_c (+)= alpha * G^T x_c on a row-distributed
// solver, G the global matrix that holds every rank's values on the global pattern; every rank passes and gets its own rows, and
// its slice of y has the bits nkp_values_product_trans_device gives on a single-GPU solver of the whole matrix.
//
//   The products travel, not partial sums.  Column j of G is summed in ascending (global row, stored position) order; with a row
//   partition that is rank 0's entries, then rank 1's, ... -- so for every entry in one of its halo columns a rank ships the
//   rounded product val[e] * x_c[row of e] (K of them, interleaved) to the owner of the column, and the owner walks the assembled
//   row of G^T in order, adding own and received products alike, one rounded add each.
//   The transposed index, built collectively at the first call and kept: the local transpose of the [own | halo] rectangle, the
//   entry counts of the halo rows to their owners and the placement plan, all three the steps of nkp_transpose_dist
//   (transpose_dist.h) -- but no source rows and no values travel, only where every contribution sits.  Kept: the row offsets of
//   the assembled block and its row blocks, per assembled entry its origin (a position in val_loc, or -1 - q for received product
//   q) and its x row (a local row, or m_loc + q), and the ship list (position in val_loc and local row, grouped by destination).
//   A call: x interleaved into xe = [ own rows | received products ] x K, the pack kernel below, ONE alltoallv straight into the
//   receive area of xe, and the product kernel of valprod.hip in its RECV mode (a received product takes the value 1.0).
#include "operand_call.h"
#include "transpose_dist.h"

#include <limits.h>
#include <stdlib.h>

#include <memory>

#define VTD_T 256

// shipped entry k = (e, i): send[k * K + c] = val[e] * xe[i * K + c], one rounded product per vector; the ship list is read
// coalesced, a row of xe and of send moves in 16-byte pieces for K >= 2
template <int K>
__global__ __launch_bounds__ (VTD_T)
void vtd_pack_kernel (int64_t n, const int *__restrict__ ship_e, const int *__restrict__ ship_i, const double *__restrict__ val, const double *__restrict__ xe,
                      double *__restrict__ send)
{
   const int64_t k = (int64_t) blockIdx.x * VTD_T + threadIdx.x;
   if (k >= n) return;
   const double v = val[ship_e[k]];
   const double *xr = xe + (int64_t) ship_i[k] * K;
   double *out = send + k * K;
   if constexpr (K == 1) out[0] = __dmul_rn (v, xr[0]);
   else {
#pragma unroll
      for (int g = 0; g < K / 2; g++) {
         const double2 q = *reinterpret_cast<const double2 *> (xr + 2 * g);
         double2 r;
         r.x = __dmul_rn (v, q.x);
         r.y = __dmul_rn (v, q.y);
         *reinterpret_cast<double2 *> (out + 2 * g) = r;
      }
   }
}

namespace {

// xe and the K-wide send buffer for width K, both or neither (a buffer of no element holds one)
int work_reserve (nkp_solver *s, int K, int64_t n_ship, int64_t n_recv, const char *who)
{
   auto &I = s->vt;
   const size_t xe = (size_t) (s->n + n_recv) * (size_t) K, send = (size_t) n_ship * (size_t) K;
   return reserve (s, { { &I.xe, &I.xe_cap, xe ? xe : 1 }, { &I.send, &I.send_cap, send ? send : 1 } }, who);
}

void work_release (nkp_solver *s)
{
   release_buffers (s, { { &s->vt.xe, &s->vt.xe_cap, 0 }, { &s->vt.send, &s->vt.send_cap, 0 } });
}

// what the index build holds beside the steps of transpose_dist.h until every rank has built its part
struct IndexBuild {
   TransDistBuild B;
   mls::DBuf<int> rowptrF, rowblk, ship_e, ship_i;
   int nrb = 0;
   Stopwatch watch;
   explicit IndexBuild (const nkp_solver *s) : B (s) {}
};

#define VTDHIP(call)                                                                                         \
   do {                                                                                                      \
      hipError_t e_ = (call);                                                                                \
      if (e_ != hipSuccess) {                                                                                \
         (void) hipGetLastError ();      /* an out-of-memory error is sticky until read */                  \
         return fail (e_ == hipErrorOutOfMemory ? NKP_ENOMEM : NKP_EDEVICE, "%s: the transposed index: %s failed: %s; the solver is unchanged", who, #call, \
                      hipGetErrorString (e_));                                                               \
      }                                                                                                      \
   } while (0)

// rank-local, after the entry counts arrived: the placement, the arrays of the index and the work space for width K
int index_build (nkp_solver *s, IndexBuild &X, int K, const char *who)
{
   TransDistBuild &B = X.B;
   if (const int rc = td_plan_placement (s, B, who)) return rc;
   if (B.n_ship > INT_MAX / NKP_BATCH_MAX || B.n_recv > INT_MAX / NKP_BATCH_MAX)
      return fail (NKP_EINVAL, "%s: %lld entries to ship and %lld to receive, times %d vectors, exceed the int counts of the exchange", who, (long long) B.n_ship,
                   (long long) B.n_recv, NKP_BATCH_MAX);
   if (const int rc = td_place_entries (s, B, false, 0, (int) B.m_loc, who)) return rc;
   VTDHIP (X.rowptrF.alloc ((size_t) B.m_loc + 1));
   VTDHIP (hipMemcpy (X.rowptrF.p, B.rowptrF.data (), ((size_t) B.m_loc + 1) * sizeof (int), hipMemcpyHostToDevice));
   int *h_rb = nullptr;
   build_rowblocks_host (B.m_loc, B.rowptrF.data (), &h_rb, &X.nrb);
   hipError_t e = X.rowblk.alloc ((size_t) X.nrb + 1);
   if (e == hipSuccess) e = hipMemcpy (X.rowblk.p, h_rb, ((size_t) X.nrb + 1) * sizeof (int), hipMemcpyHostToDevice);
   free (h_rb);
   VTDHIP (e);
   VTDHIP (X.ship_e.alloc ((size_t) B.n_ship));
   VTDHIP (X.ship_i.alloc ((size_t) B.n_ship));
   if (B.n_ship) {
      VTDHIP (hipMemcpy (X.ship_e.p, B.src.p + B.n_own, (size_t) B.n_ship * sizeof (int), hipMemcpyDeviceToDevice));
      VTDHIP (hipMemcpy (X.ship_i.p, B.colindT.p + B.n_own, (size_t) B.n_ship * sizeof (int), hipMemcpyDeviceToDevice));
   }
   return work_reserve (s, K, B.n_ship, B.n_recv, who);
}

// every rank built its part: the solver takes it (nothing here can fail)
void index_commit (nkp_solver *s, IndexBuild &X, const char *who)
{
   auto &I = s->vt;
   TransDistBuild &B = X.B;
   const auto held = [] (int64_t c) { return (size_t) (c ? c : 1); };      // as the allocations were made
   I.bytes = (held (B.m_loc + 1) + 2 * held (B.nnzF) + held (X.nrb + 1) + 2 * held (B.n_ship)) * sizeof (int);
   I.T.n = B.m_loc;
   I.T.nnz = B.nnzF;
   I.T.rowptr = X.rowptrF.release ();
   I.T.colind = B.colF.release ();
   I.T.rowblk = X.rowblk.release ();
   I.T.nrowblk = X.nrb;
   I.src = B.origin.release ();
   I.ship_e = X.ship_e.release ();
   I.ship_i = X.ship_i.release ();
   I.n_ship = B.n_ship;
   I.n_recv = B.n_recv;
   I.send_entries = B.ent_send;
   I.recv_entries = B.ent_recv;
   I.send_k.clear ();
   I.recv_k.clear ();
   s->device_bytes += I.bytes;
   I.build_seconds = X.watch.seconds ();
   msg (s, 1, "%s: transposed index of rows [%lld, %lld): %lld entries, %lld shipped, %lld received, %d row blocks, %.1f MB, %.3f s\n", who, (long long) s->dist.fst,
        (long long) (s->dist.fst + B.m_loc), (long long) B.nnzF, (long long) B.n_ship, (long long) B.n_recv, X.nrb, (double) I.bytes / 1.0e6, I.build_seconds);
}

// Host flavour: h_* given, d_* NULL; device flavour the other way round.  The entry points have refused NULL arguments, clones and
// transposed handles on the calling rank; from here on every rank makes the same collective calls whatever happens locally.
int product_trans_dist (nkp_solver *s, int nrhs, const double *h_val, const double *h_x, const double *d_val, const double *d_x, int64_t ldx, double alpha,
                        int accumulate, double *h_y, double *d_y, int64_t ldy, const char *who)
{
   OperandCall c (s, who, nrhs, h_y != nullptr, false);      // its own exchange: the K-wide halo buffers are not touched
   auto &I = s->vt;
   const int64_t n = s->n;
   hipStream_t st = s->stream;

   // ---- (a) this rank's arguments, without an index the local transpose, the work space, the host arrays staged
   int rc = refuse_nrhs (who, nrhs, " (more vectors: call again)");
   if (!rc) rc = refuse_ld (who, "ldx", ldx, "m_loc", n);
   if (!rc) rc = refuse_ld (who, "ldy", ldy, "m_loc", n);
   if (!rc && (c.host ? (const double *) h_y == h_x : (const double *) d_y == d_x)) rc = fail (NKP_EINVAL, "%s: y and x are the same buffer (the product is not done in place)", who);
   c.begin (rc);      // row-distributed: never returns here
   const int K = c.K;
   const bool building = !I.src;      // all ranks or none: the index is committed after an agreement
   std::unique_ptr<IndexBuild> X;
   if (building) {
      X.reset (new IndexBuild (s));
      if (!c.rc) c.rc = td_local_transpose (s, X->B, who);
      X->B.valT.reset ();      // comes along with the transpose; the index holds no values
   } else if (!c.rc)
      c.rc = work_reserve (s, K, I.n_ship, I.n_recv, who);
   ProductOperands o = { d_val, d_x, d_y, ldx, ldy };
   product_stage (c, { &s->vp.x, &s->vp.x_cap, 0 }, h_val, h_x, h_y, accumulate, o, false);
   if (c.agree (building ? "arguments, local transpose and work space" : "arguments and work space")) return c.rc;

   // ---- (b) only in a call that builds the index: the entry counts, then placement, arrays and work space; all ranks or none
   if (building) {
      if (!(rc = td_exchange_counts (s, X->B, who))) rc = index_build (s, *X, K, who);
      if (rc) { (void) hipStreamSynchronize (st); (void) hipGetLastError (); }
      if ((rc = dist_agree (s, rc, who, "transposed index"))) {
         work_release (s);      // X frees what this rank built: the solver is as it was
         return rc;
      }
      index_commit (s, *X, who);
      X.reset ();
   }

   // ---- (c) x into xe, the products to ship, ONE alltoallv into the receive area of xe (always made), the kernel, the agreement;
   // the time of a product runs from here
   c.watch.start ();
   I.send_k = I.send_entries;
   I.recv_k = I.recv_entries;
   for (int &v : I.send_k) v *= K;
   for (int &v : I.recv_k) v *= K;
   hipError_t e = hipSuccess;
   if (K == 1) {
      if (n) e = hipMemcpyAsync (I.xe, o.x, (size_t) n * sizeof (double), hipMemcpyDeviceToDevice, st);
   } else {
      const double *xp[NKP_BATCH_MAX] = {};
      for (int k = 0; k < nrhs; k++) xp[k] = o.x + (size_t) k * (size_t) o.ldx;
      launch_interleave (K, xp, I.xe, n, st);
   }
   if (e == hipSuccess && I.n_ship)
      with_int<1, 2, 4, 8> (K, [&] (auto k) {
         hipLaunchKernelGGL ((vtd_pack_kernel<decltype (k)::value>), dim3 ((unsigned) ((I.n_ship + VTD_T - 1) / VTD_T)), dim3 (VTD_T), 0, st, I.n_ship,
                             (const int *) I.ship_e, (const int *) I.ship_i, o.val, (const double *) I.xe, I.send);
      });
   if (e != hipSuccess) c.rc = fail (NKP_EDEVICE, "%s: the copy of x failed: %s", who, hipGetErrorString (e));
   if (alltoallv_dev (s, I.send, I.send_k.data (), I.xe + (size_t) n * (size_t) K, I.recv_k.data (), st, false)) {
      if (!c.rc) c.rc = fail (NKP_ECOMM, "%s: the exchange of the products failed", who);
   } else if (!c.rc) {
      launch_values_product_trans_recv (K, nrhs, I.T, I.src, o.val, I.xe, alpha, accumulate, o.y, o.ldy, st);
      if (c.host) e = download_columns (h_y, ldy, o.y, nrhs, n, st);
   }
   return c.finish (e, "product", "exchange and kernel", I.seconds, I.calls);
}

// refused on the calling rank, before any collective
int refuse_handle (const nkp_solver *s, const char *who)
{
   if (s->borrowed) return fail (NKP_EINVAL, "%s: a clone shares its matrix; call it on the solver it was cloned from", who);
   if (s->trans_of) return fail (NKP_EINVAL, "%s: this solver is itself a transposed handle; call it on its owner, the solver it was transposed from", who);
   return NKP_OK;
}

}   // namespace

extern "C" int nkp_values_product_trans_dist_device (nkp_solver *s, int nrhs, const void *d_val_loc, const void *d_x, int64_t ldx, double alpha, int accumulate,
                                                     void *d_y, int64_t ldy)
{
   static const char who[] = "nkp_values_product_trans_dist_device";
   if (!s) return fail (NKP_EINVAL, "%s: NULL solver (argument s)", who);
   if (!d_val_loc) return fail (NKP_EINVAL, "%s: NULL argument d_val_loc", who);
   if (!d_x) return fail (NKP_EINVAL, "%s: NULL argument d_x", who);
   if (!d_y) return fail (NKP_EINVAL, "%s: NULL argument d_y", who);
   if (!s->dist.on) return nkp_values_product_trans_device (s, nrhs, d_val_loc, d_x, ldx, alpha, accumulate, d_y, ldy);
   if (const int rc = refuse_handle (s, who)) return rc;
   return product_trans_dist (s, nrhs, nullptr, nullptr, (const double *) d_val_loc, (const double *) d_x, ldx, alpha, accumulate, nullptr, (double *) d_y, ldy, who);
}

extern "C" int nkp_values_product_trans_dist (nkp_solver *s, int nrhs, const double *val_loc, const double *x, int64_t ldx, double alpha, int accumulate, double *y,
                                              int64_t ldy)
{
   static const char who[] = "nkp_values_product_trans_dist";
   if (!s) return fail (NKP_EINVAL, "%s: NULL solver (argument s)", who);
   if (!val_loc) return fail (NKP_EINVAL, "%s: NULL argument val_loc", who);
   if (!x) return fail (NKP_EINVAL, "%s: NULL argument x", who);
   if (!y) return fail (NKP_EINVAL, "%s: NULL argument y", who);
   if (!s->dist.on) return nkp_values_product_trans (s, nrhs, val_loc, x, ldx, alpha, accumulate, y, ldy);
   if (const int rc = refuse_handle (s, who)) return rc;
   return product_trans_dist (s, nrhs, val_loc, x, nullptr, nullptr, ldx, alpha, accumulate, y, nullptr, ldy, who);
}
