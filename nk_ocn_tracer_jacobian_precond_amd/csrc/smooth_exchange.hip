// Fine-level exchange of the row-distributed cycle (tuning dist_smooth_exchange; DESIGN.md section 7, "fine-level exchange").
//
// Level 0 of a rank's hierarchy holds [own rows | overlap rows].  Its Gauss-Seidel half sweeps treat the outer edge of the overlap
// as a wall, so the overlap rows -- and through them the own rows at the cut -- drift from what an undivided sweep computes.
// With the exchange on, every level-0 half sweep of colour c is followed by
//      pack     sendbuf[i] = x[send_idx[c][i]]        the own rows of colour c that other ranks hold as overlap rows
//      alltoallv                                      device doubles on the solver's stream, always made
//      unpack   x[recv_idx[c][i]] = recvbuf[i]        this rank's overlap rows of colour c, in their arrival order
// where x is the level-0 vector that holds the colour's new values (the cycle names it: MlSmoothHook) and the indices are level-0
// positions (colour-major behind perm0), rebuilt whenever the hierarchy is.  The own rows then see the global two-colour sweep.
// K interleaved vectors (K = 2, 4, 8) move as K-wide rows in the same number of exchanges.
#include "solver_impl.h"

#include <algorithm>

#define SX_T 256

// ---------------------------------------------------------------- kernels: one thread per row, no atomics, no LDS
__global__ __launch_bounds__ (SX_T)
void smooth_pack_kernel (int64_t nrows, const int *__restrict__ idx, const double *__restrict__ x, double *__restrict__ out)
{
   const int64_t i = (int64_t) blockIdx.x * SX_T + threadIdx.x;
   if (i < nrows) out[i] = x[idx[i]];
}

__global__ __launch_bounds__ (SX_T)
void smooth_unpack_kernel (int64_t nrows, const int *__restrict__ idx, const double *__restrict__ in, double *__restrict__ x)
{
   const int64_t i = (int64_t) blockIdx.x * SX_T + threadIdx.x;
   if (i < nrows) x[idx[i]] = in[i];
}

// K >= 2: a row is K doubles = K / 2 16-byte words on both sides (the vectors come from hipMalloc, rows start at multiples of K)
template <int K>
__global__ __launch_bounds__ (SX_T)
void smooth_pack_batch_kernel (int64_t nrows, const int *__restrict__ idx, const double2 *__restrict__ x, double2 *__restrict__ out)
{
   const int64_t i = (int64_t) blockIdx.x * SX_T + threadIdx.x;
   if (i >= nrows) return;
   const int64_t r = idx[i];
#pragma unroll
   for (int k = 0; k < K / 2; k++) out[i * (K / 2) + k] = x[r * (K / 2) + k];
}

template <int K>
__global__ __launch_bounds__ (SX_T)
void smooth_unpack_batch_kernel (int64_t nrows, const int *__restrict__ idx, const double2 *__restrict__ in, double2 *__restrict__ x)
{
   const int64_t i = (int64_t) blockIdx.x * SX_T + threadIdx.x;
   if (i >= nrows) return;
   const int64_t r = idx[i];
#pragma unroll
   for (int k = 0; k < K / 2; k++) x[r * (K / 2) + k] = in[i * (K / 2) + k];
}

static inline dim3 sx_grid (int64_t n) { return dim3 ((unsigned) ((n + SX_T - 1) / SX_T)); }

void launch_smooth_pack (int K, const int *idx, const double *x, double *out, int64_t nrows, hipStream_t st)
{
   if (nrows <= 0) return;
   const double2 *x2 = (const double2 *) x;
   double2 *o2 = (double2 *) out;
   if (K == 1) hipLaunchKernelGGL (smooth_pack_kernel, sx_grid (nrows), dim3 (SX_T), 0, st, nrows, idx, x, out);
   else if (K == 2) hipLaunchKernelGGL (smooth_pack_batch_kernel<2>, sx_grid (nrows), dim3 (SX_T), 0, st, nrows, idx, x2, o2);
   else if (K == 4) hipLaunchKernelGGL (smooth_pack_batch_kernel<4>, sx_grid (nrows), dim3 (SX_T), 0, st, nrows, idx, x2, o2);
   else hipLaunchKernelGGL (smooth_pack_batch_kernel<8>, sx_grid (nrows), dim3 (SX_T), 0, st, nrows, idx, x2, o2);
}

void launch_smooth_unpack (int K, const int *idx, const double *in, double *x, int64_t nrows, hipStream_t st)
{
   if (nrows <= 0) return;
   const double2 *i2 = (const double2 *) in;
   double2 *x2 = (double2 *) x;
   if (K == 1) hipLaunchKernelGGL (smooth_unpack_kernel, sx_grid (nrows), dim3 (SX_T), 0, st, nrows, idx, in, x);
   else if (K == 2) hipLaunchKernelGGL (smooth_unpack_batch_kernel<2>, sx_grid (nrows), dim3 (SX_T), 0, st, nrows, idx, i2, x2);
   else if (K == 4) hipLaunchKernelGGL (smooth_unpack_batch_kernel<4>, sx_grid (nrows), dim3 (SX_T), 0, st, nrows, idx, i2, x2);
   else hipLaunchKernelGGL (smooth_unpack_batch_kernel<8>, sx_grid (nrows), dim3 (SX_T), 0, st, nrows, idx, i2, x2);
}

// ---------------------------------------------------------------- the solver's side
// The hook of one cycle application: every rank comes here the same number of times in the same order (the level-0 sweep counts
// are the same everywhere: nkp_create_dist agreed on them), and always makes the call, whatever its lists hold.
static void smooth_refresh (void *ctx, int c, double *x, int K, hipStream_t st)
{
   nkp_solver *s = (nkp_solver *) ctx;
   // both colours pass through the buffers of colour 0 (K <= dist.bK: batch_prepare_exchange made the K-wide ones before the
   // group's first step)
   RowExchange &X = s->dist.x_smooth[c], &B = s->dist.x_smooth[0];
   launch_smooth_pack (K, X.send_idx, x, B.send_for (K), X.nsend, st);
   exchange_rows (s, X, K, B.send_for (K), B.recv_for (K), st);
   launch_smooth_unpack (K, X.recv_idx, B.recv_for (K), x, X.nrecv, st);
}

const MlSmoothHook *smooth_hook_of (nkp_solver *s)
{
   if (!s->dist.smooth) return nullptr;
   s->dist.smooth_hook = { smooth_refresh, s };      // (a batch member is a copy: its hook must name the member itself)
   return &s->dist.smooth_hook;
}

bool smooth_install (nkp_solver *s, const DistPlan &D)
{
   auto &S = s->dist;
   // one send and one receive buffer, and their K-wide twins, sized for the larger colour: colour 0 has them.  The index lists
   // are level-0 positions: smooth_build_lists fills them
   const int64_t cap_send = (int64_t) std::max (D.smooth_send_rows[0].size (), D.smooth_send_rows[1].size ());
   const int64_t cap_recv = (int64_t) std::max (D.smooth_recv_rows[0].size (), D.smooth_recv_rows[1].size ());
   bool ok = true;
   for (int c = 0; c < 2 && ok; c++) {
      S.h_smooth_send[c] = D.smooth_send_rows[c];
      S.h_smooth_recv[c] = D.smooth_recv_rows[c];
      ok = exchange_install (s, S.x_smooth[c], nullptr, D.smooth_give[c], D.smooth_need[c], true, c ? -1 : cap_send, c ? -1 : cap_recv, c ? -1 : cap_recv);
   }
   return ok;
}

int smooth_build_lists (nkp_solver *s)
{
   auto &S = s->dist;
   const MlHierarchy &H = s->ml;
   if (H.lev.empty () || !H.perm0 || H.lev[0].n != S.n_ext) return -3;
   const int64_t n = S.n_ext;
   // level-0 row i holds row perm0[i] of the hierarchy's matrix; the setup may still be copying it on the solver's stream
   std::vector<int> perm ((size_t) n + 1), pos ((size_t) n + 1, -1);
   if (hipStreamSynchronize (s->stream) != hipSuccess) return -3;
   if (n && hipMemcpy (perm.data (), H.perm0, (size_t) n * sizeof (int), hipMemcpyDeviceToHost) != hipSuccess) return -3;
   for (int64_t i = 0; i < n; i++) {
      if (perm[(size_t) i] < 0 || perm[(size_t) i] >= n) return -3;
      pos[(size_t) perm[(size_t) i]] = (int) i;
   }
   std::vector<int> idx;
   for (int c = 0; c < 2; c++)
      for (int side = 0; side < 2; side++) {
         const std::vector<int32_t> &rows = side ? S.h_smooth_recv[c] : S.h_smooth_send[c];
         int *dst = side ? S.x_smooth[c].recv_idx : S.x_smooth[c].send_idx;
         idx.resize (rows.size ());
         for (size_t k = 0; k < rows.size (); k++) {
            // own rows go out, overlap rows come in: an index outside its part would be a write outside the level's vectors
            const int32_t r = rows[k];
            if (side ? (r < s->n || r >= n) : (r < 0 || r >= s->n)) return -3;
            if ((idx[k] = pos[(size_t) r]) < 0) return -3;
         }
         if (!idx.empty () && hipMemcpy (dst, idx.data (), idx.size () * sizeof (int), hipMemcpyHostToDevice) != hipSuccess) return -3;
      }
   return 0;
}
