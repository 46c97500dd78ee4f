// nkp_transpose_dist: a row-distributed solver for A^T with the row partition of the solver it is made from, built from the row
// block every rank holds on the device.
//
//   The local transpose.  A rank's matrix is m_loc rows by m_loc + n_halo columns in [own | halo] numbering.  The kernels of
//   transpose.hip run over that rectangle: rows [0, m_loc) of the result are the own part of A^T's row block (their columns are
//   local source rows, global = fst + r), rows [m_loc, m_loc + n_halo) are the entries other ranks own.  The halo is ascending
//   in global row, hence grouped by owner: the second part is the send stream as it stands, every shipped column's entries
//   sorted by source row.  The ranking step of transpose.hip reads a row of A^T once per entry of that row -- quadratic in its
//   length, accepted here as there (the long rows of A^T are assembled from the ranks' shorter pieces).
//   The exchange.  The owner of a halo row knows which of its rows a peer holds as halo (the send rows of the SpMV plan, in the
//   peer's halo order), so only the entry count of every such row, the global source rows (both alltoallv_i32_host) and the
//   values (the device alltoallv) travel.  Halo rows that exist only to complete a water column carry count 0.
//   The placement.  A row of A^T sorted by global column is the concatenation, in rank order, of what every rank contributed,
//   the own part at this rank's position: row lengths are sums, row starts a scan, and two kernels write every own and every
//   received entry to row start + segment offset + index.  No sort, no atomics: the output depends on the keys alone.
//   The solver.  The assembled block goes to the host once and through nkp_create_dist with the options, tuning and block data
//   the source kept, which makes it bit for bit the solver nkp_create_dist builds from the host transpose's row slice.
// Kept on the device for refactors: origin (per entry of the assembled block: a position in the source's values, or -1 - a
// position in the received values), the ship list (positions in the source's values, by destination) and, from the first
// refactor on, the send / receive / assembled value buffers.
// The local transpose, the exchange of the entry counts, the placement plan and the placing kernels are declared in
// transpose_dist.h: the transposed index of nkp_values_product_trans_dist (valprod_trans_dist.hip) is built from the same steps.
#include "transpose_dist.h"

#include <stdio.h>
#include <time.h>


#define TD_T 256
static inline dim3 td_grid (int64_t n) { return dim3 ((unsigned) ((n + TD_T - 1) / TD_T)); }

// the segment k with ptr[k] <= e < ptr[k + 1] (ptr ascending, ptr[0] = 0, e < ptr[n]; empty segments are skipped)
__device__ static inline int td_seg_of (const int *__restrict__ ptr, int n, int e)
{
   int lo = 0, hi = n;
   while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (ptr[mid + 1] <= e) lo = mid + 1;
      else hi = mid;
   }
   return lo;
}

// own part: entry e of row c < m_loc of the local transpose goes to own_dst[c] + (e - rowptrT[c]) with the column col_add + its
// source row (col_add = the rank's first row: the global column; 0: the local row); valT / valF NULL: no values are placed
__global__ __launch_bounds__ (TD_T)
void td_place_own_kernel (const int *__restrict__ rowptrT, int m_loc, int n_own, const int *__restrict__ own_dst, const int *__restrict__ colindT,
                          const int *__restrict__ src, const double *__restrict__ valT, int col_add, int *__restrict__ colF, double *__restrict__ valF,
                          int *__restrict__ origin)
{
   const int e = blockIdx.x * TD_T + threadIdx.x;
   if (e >= n_own) return;
   const int c = td_seg_of (rowptrT, m_loc, e);
   const int d = own_dst[c] + (e - rowptrT[c]);
   colF[d] = col_add + colindT[e];
   if (valF) valF[d] = valT[e];
   origin[d] = src[e];
}

// received part: entry i of segment k (one row a peer holds as halo) goes to seg_dst[k] + (i - seg_ptr[k]); without recv_col its
// column is col_add + i, its place in the received stream
__global__ __launch_bounds__ (TD_T)
void td_place_recv_kernel (const int *__restrict__ seg_ptr, int nseg, int n_recv, const int *__restrict__ seg_dst, const int *__restrict__ recv_col,
                           const double *__restrict__ recv_val, int col_add, int *__restrict__ colF, double *__restrict__ valF, int *__restrict__ origin)
{
   const int i = blockIdx.x * TD_T + threadIdx.x;
   if (i >= n_recv) return;
   const int k = td_seg_of (seg_ptr, nseg, i);
   const int d = seg_dst[k] + (i - seg_ptr[k]);
   colF[d] = recv_col ? recv_col[i] : col_add + i;
   if (valF) valF[d] = recv_val[i];
   origin[d] = -1 - i;
}

// a refactor of the source: the values to ship, and the assembled values of A^T's row block
__global__ __launch_bounds__ (TD_T)
void td_pack_kernel (int64_t n, const int *__restrict__ ship, const double *__restrict__ aval, double *__restrict__ out)
{
   const int64_t k = (int64_t) blockIdx.x * TD_T + threadIdx.x;
   if (k < n) out[k] = aval[ship[k]];
}

__global__ __launch_bounds__ (TD_T)
void td_assemble_kernel (int64_t n, const int *__restrict__ origin, const double *__restrict__ aval, const double *__restrict__ recv, double *__restrict__ out)
{
   const int64_t k = (int64_t) blockIdx.x * TD_T + threadIdx.x;
   if (k >= n) return;
   const int o = origin[k];
   out[k] = o >= 0 ? aval[o] : recv[-1 - o];
}

static double td_since (const struct timespec &t0)
{
   struct timespec t;
   clock_gettime (CLOCK_MONOTONIC, &t);
   return (double) (t.tv_sec - t0.tv_sec) + 1e-9 * (double) (t.tv_nsec - t0.tv_nsec);
}

// a HIP call of a rank-local step of `who`: its failure becomes that step's code (the agreement after the step carries it to the peers)
#define TDHIP(call)                                                                                          \
   do {                                                                                                      \
      hipError_t e_ = (call);                                                                                \
      if (e_ != hipSuccess) {                                                                                \
         (void) hipGetLastError ();                                                                          \
         return fail (e_ == hipErrorOutOfMemory ? NKP_ENOMEM : NKP_EDEVICE, "%s: %s failed: %s", who, #call, hipGetErrorString (e_)); \
      }                                                                                                      \
   } while (0)

// ---------------------------------------------------------------- the steps shared with the transposed index (transpose_dist.h)
int td_local_transpose (nkp_solver *s, TransDistBuild &B, const char *who)
{
   hipStream_t st = s->stream;
   TDHIP (hipSetDevice (s->device));
   TDHIP (hipStreamSynchronize (st));
   struct timespec t0;
   clock_gettime (CLOCK_MONOTONIC, &t0);
   const int64_t ncols = B.m_loc + B.n_halo;
   const int trc = transpose_device (s->A, ncols, B.rowptrT, B.colindT, B.valT, B.src, st);
   if (trc) {
      (void) hipStreamSynchronize (st);
      (void) hipGetLastError ();      // an out-of-memory error is sticky until read
      if (trc == (int) hipErrorOutOfMemory) return fail (NKP_ENOMEM, "%s: no device memory for the transposed row block (%lld entries); the solver is unchanged", who, (long long) B.nnz);
      return fail (NKP_EDEVICE, "%s: the device transpose failed (%s)", who, trc >= 1000 ? "inconsistent column counts" : hipGetErrorString ((hipError_t) trc));
   }
   B.kernel_seconds = td_since (t0);
   B.h_rpT.assign ((size_t) ncols + 1, 0);
   TDHIP (hipMemcpy (B.h_rpT.data (), B.rowptrT.p, B.h_rpT.size () * sizeof (int32_t), hipMemcpyDeviceToHost));
   B.n_own = B.h_rpT[(size_t) B.m_loc];
   B.n_ship = B.nnz - B.n_own;
   if (B.h_rpT[(size_t) ncols] != B.nnz || B.n_own < 0 || B.n_ship < 0) return fail (NKP_EDEVICE, "%s: the device transpose returned inconsistent row offsets", who);
   B.cnt_send.assign ((size_t) B.n_halo + 1, 0);
   for (int64_t h = 0; h < B.n_halo; h++) B.cnt_send[(size_t) h] = B.h_rpT[(size_t) (B.m_loc + h + 1)] - B.h_rpT[(size_t) (B.m_loc + h)];
   // the halo rows of owner p follow each other: recv_counts[p] of them
   B.ent_send.assign ((size_t) B.P, 0);
   int64_t h = 0;
   for (int p = 0; p < B.P; p++)
      for (int k = 0; k < s->dist.x_halo.recv_counts[(size_t) p]; k++, h++) B.ent_send[(size_t) p] += B.cnt_send[(size_t) h];
   if (h != B.n_halo) return fail (NKP_EINVAL, "%s: the halo plan of this solver is inconsistent", who);
   return NKP_OK;
}

int td_exchange_counts (nkp_solver *s, TransDistBuild &B, const char *who)
{
   const nkp_comm_ops &c = s->dist.ops;
   B.cnt_recv.assign ((size_t) B.nseg + 1, 0);
   if (c.alltoallv_i32_host (c.ctx, B.cnt_send.data (), s->dist.x_halo.recv_counts.data (), B.cnt_recv.data (), s->dist.x_halo.send_counts.data ()))
      return fail (NKP_ECOMM, "%s: the exchange of the entry counts failed", who);
   return NKP_OK;
}

int td_plan_placement (nkp_solver *s, TransDistBuild &B, const char *who)
{
   const std::vector<int32_t> &rows = s->dist.h_send_rows;
   B.ent_recv.assign ((size_t) B.P, 0);
   B.seg_ptr.assign ((size_t) B.nseg + 1, 0);
   std::vector<int64_t> len ((size_t) B.m_loc + 1, 0);
   for (int64_t c = 0; c < B.m_loc; c++) len[(size_t) c] = B.h_rpT[(size_t) c + 1] - B.h_rpT[(size_t) c];
   int64_t k = 0, total = 0;
   for (int p = 0; p < B.P; p++) {
      int64_t t = 0;
      for (int q = 0; q < s->dist.x_halo.send_counts[(size_t) p]; q++, k++) {
         const int32_t cnt = B.cnt_recv[(size_t) k], c = rows[(size_t) k];
         if (cnt < 0 || c < 0 || c >= B.m_loc) return fail (NKP_ECOMM, "%s: rank %d sent an entry count this rank cannot place", who, p);
         t += cnt;
         len[(size_t) c] += cnt;
      }
      total += t;
      if (total >= 2147483647LL) return fail (NKP_EINVAL, "%s: the entries received exceed the int32 exchange counts", who);
      B.ent_recv[(size_t) p] = (int) t;
   }
   B.n_recv = total;
   B.nnzF = B.n_own + B.n_recv;
   if (B.nnzF >= 2147483647LL) return fail (NKP_EINVAL, "%s: the row block of A^T exceeds the int32 index schema", who);
   for (int64_t q = 0; q < B.nseg; q++) B.seg_ptr[(size_t) q + 1] = B.seg_ptr[(size_t) q] + B.cnt_recv[(size_t) q];
   B.rowptrF.assign ((size_t) B.m_loc + 1, 0);
   for (int64_t c = 0; c < B.m_loc; c++) B.rowptrF[(size_t) c + 1] = (int32_t) (B.rowptrF[(size_t) c] + len[(size_t) c]);
   // the contributions of a row in rank order: lower ranks own lower rows, i.e. lower columns of A^T
   std::vector<int32_t> cursor (B.rowptrF.begin (), B.rowptrF.end ());
   B.own_dst.assign ((size_t) B.m_loc + 1, 0);
   B.seg_dst.assign ((size_t) B.nseg + 1, 0);
   k = 0;
   for (int p = 0; p < B.P; p++) {
      if (p == B.me)
         for (int64_t c = 0; c < B.m_loc; c++) {
            B.own_dst[(size_t) c] = cursor[(size_t) c];
            cursor[(size_t) c] += B.h_rpT[(size_t) c + 1] - B.h_rpT[(size_t) c];
         }
      for (int q = 0; q < s->dist.x_halo.send_counts[(size_t) p]; q++, k++) {
         const int32_t c = rows[(size_t) k];
         B.seg_dst[(size_t) k] = cursor[(size_t) c];
         cursor[(size_t) c] += B.cnt_recv[(size_t) k];
      }
   }
   for (int64_t c = 0; c < B.m_loc; c++)
      if (cursor[(size_t) c] != B.rowptrF[(size_t) c + 1]) return fail (NKP_EINVAL, "%s: a row of this rank is sent twice to one peer (inconsistent halo plan)", who);
   return NKP_OK;
}

template <class T>
static int td_upload (mls::DBuf<T> &d, const std::vector<T> &h, size_t cnt, const char *who)
{
   TDHIP (d.alloc (cnt));
   if (cnt) TDHIP (hipMemcpy (d.p, h.data (), cnt * sizeof (T), hipMemcpyHostToDevice));
   return NKP_OK;
}

int td_place_entries (nkp_solver *s, TransDistBuild &B, bool values, int own_add, int recv_add, const char *who)
{
   hipStream_t st = s->stream;
   mls::DBuf<int> d_own_dst, d_seg_ptr, d_seg_dst, d_recv_col;
   int rc;
   if ((rc = td_upload (d_own_dst, B.own_dst, (size_t) B.m_loc, who))) return rc;
   if ((rc = td_upload (d_seg_ptr, B.seg_ptr, (size_t) B.nseg + 1, who))) return rc;
   if ((rc = td_upload (d_seg_dst, B.seg_dst, (size_t) B.nseg, who))) return rc;
   if (values && (rc = td_upload (d_recv_col, B.recv_col, (size_t) B.n_recv, who))) return rc;
   TDHIP (B.colF.alloc ((size_t) B.nnzF));
   if (values) TDHIP (B.valF.alloc ((size_t) B.nnzF));
   TDHIP (B.origin.alloc ((size_t) B.nnzF));
   if (B.n_own)
      hipLaunchKernelGGL (td_place_own_kernel, td_grid (B.n_own), dim3 (TD_T), 0, st, B.rowptrT.p, (int) B.m_loc, (int) B.n_own, d_own_dst.p, B.colindT.p, B.src.p,
                          values ? B.valT.p : nullptr, own_add, B.colF.p, B.valF.p, B.origin.p);
   if (B.n_recv)
      hipLaunchKernelGGL (td_place_recv_kernel, td_grid (B.n_recv), dim3 (TD_T), 0, st, d_seg_ptr.p, (int) B.nseg, (int) B.n_recv, d_seg_dst.p, d_recv_col.p,
                          B.recv_val.p, recv_add, B.colF.p, B.valF.p, B.origin.p);
   TDHIP (hipStreamSynchronize (st));      // the uploaded plan is freed on return
   TDHIP (hipGetLastError ());
   return NKP_OK;
}

// (after the source rows and the values arrived): the assembled block on the device, then on the host
static int td_place (nkp_solver *s, TransDistBuild &B, const char *who)
{
   struct timespec t0;
   clock_gettime (CLOCK_MONOTONIC, &t0);
   if (const int rc = td_place_entries (s, B, true, (int) s->dist.fst, 0, who)) return rc;
   TDHIP (B.ship.alloc ((size_t) B.n_ship));
   if (B.n_ship) TDHIP (hipMemcpy (B.ship.p, B.src.p + B.n_own, (size_t) B.n_ship * sizeof (int), hipMemcpyDeviceToDevice));
   B.kernel_seconds += td_since (t0);
   B.h_colF.assign ((size_t) B.nnzF + 1, 0);
   B.h_valF.assign ((size_t) B.nnzF + 1, 0.0);
   if (B.nnzF) {
      TDHIP (hipMemcpy (B.h_colF.data (), B.colF.p, (size_t) B.nnzF * sizeof (int32_t), hipMemcpyDeviceToHost));
      TDHIP (hipMemcpy (B.h_valF.data (), B.valF.p, (size_t) B.nnzF * sizeof (double), hipMemcpyDeviceToHost));
   }
   return NKP_OK;
}

// the global source rows of the entries to ship (nkp_transpose_dist alone: the index needs no columns)
static int td_ship_rows (nkp_solver *s, TransDistBuild &B, const char *who)
{
   B.ship_glob.assign ((size_t) B.n_ship + 1, 0);
   if (B.n_ship) TDHIP (hipMemcpy (B.ship_glob.data (), B.colindT.p + B.n_own, (size_t) B.n_ship * sizeof (int32_t), hipMemcpyDeviceToHost));
   for (int64_t k = 0; k < B.n_ship; k++) B.ship_glob[(size_t) k] += (int32_t) s->dist.fst;
   return NKP_OK;
}

// ---------------------------------------------------------------- the refactor of the source reaches the transposed solver
int trans_dist_follow (nkp_solver *s, int flags, const char *who, int (*refactor) (nkp_solver *t, const void *d_val, int flags, const char *who))
{
   nkp_solver *t = s->trans;
   const nkp_comm_ops &c = s->dist.ops;
   hipStream_t st = s->stream;
   int64_t n_ship = 0, n_recv = 0;
   for (int v : s->trans_send_counts) n_ship += v;
   for (int v : s->trans_recv_counts) n_recv += v;
   int rc = NKP_OK;
   if (!s->trans_val) {
      const size_t bytes = ((size_t) (s->trans_nnz ? s->trans_nnz : 1) + (size_t) (n_ship ? n_ship : 1) + (size_t) (n_recv ? n_recv : 1)) * sizeof (double);
      void *a = nullptr, *b = nullptr, *d = nullptr;
      if (hipMalloc (&a, (size_t) (s->trans_nnz ? s->trans_nnz : 1) * sizeof (double)) != hipSuccess || hipMalloc (&b, (size_t) (n_ship ? n_ship : 1) * sizeof (double)) != hipSuccess ||
          hipMalloc (&d, (size_t) (n_recv ? n_recv : 1) * sizeof (double)) != hipSuccess) {
         (void) hipGetLastError ();
         for (void *p : { a, b, d })
            if (p) (void) hipFree (p);
         rc = fail (NKP_ENOMEM, "%s: no device memory for the %zu bytes of the transposed solver's value buffers", who, bytes);
      } else {
         s->trans_val = (double *) a;
         s->trans_send = (double *) b;
         s->trans_recv = (double *) d;
         s->trans_map_bytes += bytes;
      }
   }
   if ((rc = dist_agree (s, rc, who, "value buffers of the transposed solver"))) return rc;
   if (n_ship) hipLaunchKernelGGL (td_pack_kernel, td_grid (n_ship), dim3 (TD_T), 0, st, n_ship, (const int *) s->trans_ship, (const double *) s->A.val, s->trans_send);
   if (c.alltoallv (c.ctx, s->trans_send, s->trans_send_counts.data (), s->trans_recv, s->trans_recv_counts.data (), (void *) st))
      rc = fail (NKP_ECOMM, "%s: the exchange of the transposed values failed", who);
   else {
      if (s->trans_nnz)
         hipLaunchKernelGGL (td_assemble_kernel, td_grid (s->trans_nnz), dim3 (TD_T), 0, st, s->trans_nnz, (const int *) s->trans_src, (const double *) s->A.val,
                             (const double *) s->trans_recv, s->trans_val);
      if (hipGetLastError () != hipSuccess) rc = fail (NKP_EDEVICE, "%s: the assembly of the transposed values failed", who);
   }
   if ((rc = dist_agree (s, rc, who, "values of the transposed solver"))) return rc;
   return refactor (t, s->trans_val, flags, who);
}

// ---------------------------------------------------------------- C ABI
extern "C" int nkp_transpose_dist (nkp_solver *s, nkp_solver **out)
{
   if (out) *out = nullptr;
   if (!s || !out) return fail (NKP_EINVAL, "nkp_transpose_dist: NULL argument");
   if (s->borrowed) return fail (NKP_EINVAL, "nkp_transpose_dist: a clone shares its matrix; transpose the solver it was cloned from");
   if (s->trans_of) return fail (NKP_EINVAL, "nkp_transpose_dist: this solver is itself a transposed handle; the solver it was transposed from holds A");
   if (!s->dist.on) return nkp_transpose (s, out);
   const nkp_comm_ops &c = s->dist.ops;
   const int P = c.nranks;
   static const char who[] = "nkp_transpose_dist";

   // ---- who holds a transposed handle: all (return it), none (build it), or some (a rank destroyed its handle alone)
   {
      std::vector<int64_t> all ((size_t) P + 1, 0);
      if (c.allgather_i64_host (c.ctx, s->trans ? 1 : 0, all.data ())) return fail (NKP_ECOMM, "nkp_transpose_dist: allgather failed (who holds a transposed solver)");
      int with = -1, without = -1;
      for (int p = P - 1; p >= 0; p--) {
         if (all[(size_t) p]) with = p;
         else without = p;
      }
      if (with >= 0 && without >= 0)
         return fail (NKP_EINVAL, "nkp_transpose_dist: rank %d holds no transposed solver while rank %d holds one (a rank destroyed its handle alone); destroy the handle on every rank, then call again",
                      without, with);
      if (with >= 0) { *out = s->trans; return NKP_OK; }
   }
   struct timespec t0;
   clock_gettime (CLOCK_MONOTONIC, &t0);
   TransDistBuild B (s);

   // ---- the local transpose
   int rc = s->shared->broken ? fail (NKP_ESINGULAR, "nkp_transpose_dist: %s", s->shared->why.c_str ()) : td_local_transpose (s, B, who);
   if (!rc) rc = td_ship_rows (s, B, who);
   if ((rc = dist_agree (s, rc, who, "local transpose"))) return rc;

   // ---- entry counts of the rows the peers hold as halo, then the plan of the assembled block
   if (!(rc = td_exchange_counts (s, B, who))) rc = td_plan_placement (s, B, who);
   if (!rc && B.recv_val.alloc ((size_t) B.n_recv) != hipSuccess) {      // a rank without its receive buffer must not enter the exchange
      (void) hipGetLastError ();
      rc = fail (NKP_ENOMEM, "nkp_transpose_dist: no device memory for the %lld received values", (long long) B.n_recv);
   }
   if ((rc = dist_agree (s, rc, who, "entry counts"))) return rc;

   // ---- global source rows and values, then the placement
   B.recv_col.assign ((size_t) B.n_recv + 1, 0);
   if (c.alltoallv_i32_host (c.ctx, B.ship_glob.data (), B.ent_send.data (), B.recv_col.data (), B.ent_recv.data ()))
      rc = fail (NKP_ECOMM, "nkp_transpose_dist: the exchange of the source rows failed");
   if (c.alltoallv (c.ctx, B.valT.p + B.n_own, B.ent_send.data (), B.recv_val.p, B.ent_recv.data (), (void *) s->stream) && !rc)
      rc = fail (NKP_ECOMM, "nkp_transpose_dist: the exchange of the values failed");
   if (!rc) {
      for (int64_t i = 0; i < B.n_recv && !rc; i++)
         if (B.recv_col[(size_t) i] < 0 || B.recv_col[(size_t) i] >= s->dist.n_global) rc = fail (NKP_ECOMM, "nkp_transpose_dist: a peer sent a source row outside the matrix");
   }
   if (!rc) rc = td_place (s, B, who);
   if (rc) { (void) hipStreamSynchronize (s->stream); (void) hipGetLastError (); }
   if ((rc = dist_agree (s, rc, who, "exchange and placement"))) return rc;

   // ---- the solver: nkp_create_dist on the assembled block with what the source resolved and kept (collective; it succeeds
   // or fails on all ranks together)
   nkp_options opt = s->opt;
   opt.device = s->device;
   opt.tuning = &s->tune;
   opt.col_i = s->dist.own_ci.empty () ? nullptr : s->dist.own_ci.data ();
   opt.col_j = s->dist.own_cj.empty () ? nullptr : s->dist.own_cj.data ();
   opt.col_t = s->dist.own_ct.empty () ? nullptr : s->dist.own_ct.data ();
   nkp_solver *t = nullptr;
   rc = nkp_create_dist (&t, &opt, s->dist.n_global, s->dist.fst, B.m_loc, B.nnzF, B.rowptrF.data (), B.h_colF.data (), B.h_valF.data (),
                         s->dist.own_has_blk ? s->dist.own_blk.data () : nullptr, s->dist.own_has_blk ? (int64_t) s->dist.own_blk.size () - 1 : 0, s->dist.own_tracer_cnt, &c);
   if (rc) {
      (void) hipGetLastError ();
      const std::string why = last_error_message ();
      return fail (rc, "nkp_transpose_dist: %s; the solver is unchanged", why.c_str ());
   }
   // same stream as the source
   if (t->own_stream && t->stream) { (void) hipStreamSynchronize (t->stream); (void) hipStreamDestroy (t->stream); }
   t->stream = s->stream;
   t->own_stream = false;
   t->trans_of = s;
   s->trans = t;
   s->trans_src = B.origin.release ();
   s->trans_ship = B.ship.release ();
   s->trans_map_bytes = ((size_t) (B.nnzF ? B.nnzF : 1) + (size_t) (B.n_ship ? B.n_ship : 1)) * sizeof (int);
   s->trans_send_counts = B.ent_send;
   s->trans_recv_counts = B.ent_recv;
   s->trans_nnz = B.nnzF;
   s->trans_sent = B.n_ship;
   s->trans_received = B.n_recv;
   s->trans_seconds = td_since (t0);
   s->trans_kernel_seconds = B.kernel_seconds;
   msg (s, 1, "nkp_transpose_dist: rows [%lld, %lld): %lld entries, %lld shipped, %lld received, %.1f MB on device %d; %.3f s device transpose and placement, %.3f s in all\n",
        (long long) s->dist.fst, (long long) (s->dist.fst + B.m_loc), (long long) B.nnzF, (long long) B.n_ship, (long long) B.n_recv, (double) trans_device_bytes (s) / 1.0e6, s->device,
        B.kernel_seconds, s->trans_seconds);
   *out = t;
   return NKP_OK;
}
